"""Validation metrics with device-side accumulators: L2metric and EvalAImetric of
/root/reference/src/models/hrnet/metrics.py:14-94, 142-229 -- same names, constructor arguments, methods
(reset / update(step_output) / compute / epoch_complete(state)) and dictionary keys.

AccMetric is the line model's (/root/reference/src/models/line/metrics.py:20-137): csrc/line_loss.hip counts, the host aggregates.

`state` is any object with `.phase` and `.metrics` (pytorch-argus is not a dependency).  update() queues device work only; the host
reads the accumulators once, in compute() / epoch_complete().  The per-class confusion matrices the reference also sums
(metrics.py:198-199) are never reported by it and are not kept here (CameraEvaluator.class_report gives them).  EvalAImetric sends the whole batch through the batched solve
(CameraCreator.solve_device) and the batched evaluation (CameraEvaluator.evaluate) instead of a 16-process pool over frames.

Mirrored, not fixed (the reference's behaviour is the definition):
  * L2metric.n_fp / n_fn are ASSIGNED by each update, not accumulated (metrics.py:67-68): precision and recall relate the
    matched points of the whole epoch to the false positives / negatives of the LAST batch;
  * pckhs counts count_nonzero(l2[l2 < t]) (metrics.py:70): a matched point at distance exactly 0 is not counted;
  * compute() is inf when no point matched.
"""
from typing import Callable, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .evaluate import CameraEvaluator


def _prefix(state) -> str:
    return f'{state.phase}_' if getattr(state, 'phase', None) else ''


class L2metric:
    name = 'l2'
    better = 'min'

    def __init__(self, num_keypoints: int = 30, conf_threshold: float = 0.5, pckhs_thres: Sequence[float] = (2.0, 5.0, 10.0, 50.0)):
        self.num_keypoints = num_keypoints
        self.conf_threshold = conf_threshold
        self.pckhs_thres = list(pckhs_thres)
        self.reset()

    def reset(self):
        self._acc = None            # fp64 device vector [sum, num_el, gt_points, pred_points, pckhs...]: exact for the counts
        self._last = None           # int64 device vector [n_fp, n_fn] of the last update

    def update(self, step_output: dict):
        preds = step_output['prediction']
        kpts = step_output['target'].to(preds.device).reshape(-1, self.num_keypoints, 3)
        l2 = torch.linalg.vector_norm(preds[:, :, :2] - kpts[:, :, :2], dim=-1)
        gt_valid = kpts[:, :, 0] != -1
        pred_valid = preds[:, :, 2] > self.conf_threshold
        mask = gt_valid & pred_valid
        # sums over l2[mask] without the host round trip of boolean indexing
        parts = [torch.where(mask, l2, torch.zeros_like(l2)).sum(dtype=torch.float64), mask.sum(), gt_valid.sum(), pred_valid.sum()]
        parts += [(mask & (l2 < t) & (l2 != 0)).sum() for t in self.pckhs_thres]
        acc = torch.stack([p.to(torch.float64) for p in parts])
        self._acc = acc if self._acc is None else self._acc + acc
        self._last = torch.stack([(~gt_valid & pred_valid).sum(), (~pred_valid & gt_valid).sum()])

    def _read(self):
        n = 4 + len(self.pckhs_thres)
        if self._acc is None:
            return [0.0] + [0] * (n - 1), [0, 0]
        acc = self._acc.cpu().numpy()
        return [float(acc[0])] + [int(round(v)) for v in acc[1:]], [int(v) for v in self._last.cpu().numpy()]

    def compute(self) -> float:
        acc, _ = self._read()
        return acc[0] / acc[1] if acc[1] > 0 else float('inf')

    def epoch_complete(self, state):
        acc, (n_fp, n_fn) = self._read()
        total, num_el, gt_points = acc[0], acc[1], acc[2]
        precision, recall = 0.0, 0.0
        if num_el > 0:
            precision = num_el / (num_el + n_fp)
            recall = num_el / (num_el + n_fn)
        p = _prefix(state)
        state.metrics[f'{p}precision'] = precision
        state.metrics[f'{p}recall'] = recall
        for i, t in enumerate(self.pckhs_thres):
            state.metrics[f'{p}pcks-{t}'] = acc[4 + i] / gt_points if gt_points > 0 else 0.0
        state.metrics[f'{p}{self.name}'] = total / num_el if num_el > 0 else float('inf')


class EvalAImetric:
    """pred2cam: a CameraCreator (its batched solve_device is what runs); threshold in pixels; img_size (W, H)."""
    name = 'evalai'
    better = 'max'

    def __init__(self, pred2cam: Callable, threshold: int = 5, img_size: Tuple[int, int] = (960, 540), max_workers: int = 16):
        self.pred2cam = pred2cam
        self.threshold = threshold
        self.img_size = tuple(int(v) for v in img_size)
        self._evaluator = None       # built on the first update, on the predictions' device (max_workers: no pool here, ignored)
        self.reset()

    def reset(self):
        self.total_frames = 0
        self._skipped = 0            # frames that never reached the network: missed without a solve
        self._acc = None             # fp64 [missed, accuracy, n_accuracy, tp, n_precision, n_recall, l2_proj_sum, n_l2_proj]

    def add_missed(self, n: int):
        """Frames without a prediction (e.g. images the decoder refused): counted in total_frames and as missed."""
        self.total_frames += int(n)
        self._skipped += int(n)

    def evaluator(self, device) -> CameraEvaluator:
        if self._evaluator is None or self._evaluator.device != torch.device(device):
            self._evaluator = CameraEvaluator(device, self.img_size[0], self.img_size[1], float(self.threshold))
        return self._evaluator

    def update(self, step_output: dict):
        preds = step_output['prediction']
        d_lp = None
        lp = self.pred2cam.line_points_array(step_output.get('img_name'))
        if lp is not None:
            d_lp = torch.from_numpy(lp).to(preds.device)
        records = self.pred2cam.solve_device(preds.contiguous().float(), d_lp)
        self.update_records(records, step_output['raw_annots'])

    def update_records(self, records: torch.Tensor, raw_annots: List[dict]):
        """The aggregation of metrics.py:185-207 for a batch whose cameras are already solved: records (B, sizeof(sncal_camera))
        uint8 on the device, status 0 = no camera."""
        B = records.shape[0]
        self.total_frames += B
        if B == 0:
            return
        out, err, cls = self.evaluator(records.device).evaluate(records, raw_annots, detail=True)
        done = out[:, 11] > 0
        plain = out[:, 10] == 1                                           # the kept pass: plain labels only when strictly better
        acc = torch.where(plain, out[:, 8], out[:, 9]).to(torch.float64)
        conf = torch.where(plain[:, None], out[:, 0:4], out[:, 4:8]).to(torch.float64)      # [0,0] [0,1] [1,0] [1,1]
        sel = torch.where(plain, 0, 1)
        idx = torch.arange(B, device=out.device)
        q = cls[idx, sel].to(torch.float64)                               # (B,C,4) [below, beyond, missed, fp_flag]
        e = err[idx, sel]                                                 # (B,C,max_gt)
        common = (q[..., 3] == 0) & (q[..., 2] == 0) & (q[..., 0] + q[..., 1] > 0) & done[:, None]
        n_pts = torch.where(common, q[..., 0] + q[..., 1], torch.zeros_like(q[..., 0]))
        k = torch.arange(e.shape[2], device=e.device)
        used = k[None, None, :] < n_pts[..., None]
        zero = torch.zeros((), dtype=torch.float64, device=out.device)
        d = done.to(torch.float64)
        parts = [(1.0 - d).sum(), torch.where(done, acc, zero).sum(), d.sum(),
                 torch.where(done, conf[:, 0], zero).sum(), torch.where(done, conf[:, 0] + conf[:, 1], zero).sum(),
                 torch.where(done, conf[:, 0] + conf[:, 2], zero).sum(),
                 torch.where(used, e, zero).sum(), n_pts.sum()]            # non-finite errors propagate, as sum() does in the reference
        a = torch.stack(parts)
        self._acc = a if self._acc is None else self._acc + a

    def _read(self):
        if self._acc is None:
            return np.zeros(8)
        return self._acc.cpu().numpy()

    def compute(self) -> float:
        missed = float(self._read()[0]) + self._skipped
        return (self.total_frames - missed) / self.total_frames if self.total_frames > 0 else 0.0

    def epoch_complete(self, state):
        _evalai_epoch(state, self.name, self._read(), self._skipped, self.total_frames)


def _evalai_epoch(state, name, a, skipped, total_frames):
    """metrics.py:209-229 on one accumulator row [missed, accuracy, n_accuracy, tp, n_precision, n_recall, l2_proj_sum, n_l2_proj]."""
    missed = float(a[0]) + skipped
    completeness = (total_frames - missed) / total_frames if total_frames > 0 else 0.0
    accuracy = a[1] / a[2] if a[2] > 0 else 0.0
    precision = a[3] / a[4] if a[4] > 0 else 0.0
    recall = a[3] / a[5] if a[5] > 0 else 0.0
    l2_reproj = a[6] / a[7] if a[7] > 0 else float('inf')
    p = _prefix(state)
    state.metrics[f'{p}l2_reprojection'] = float(l2_reproj)
    state.metrics[f'{p}completeness'] = float(completeness)
    state.metrics[f'{p}eval_precision'] = float(precision)
    state.metrics[f'{p}eval_recall'] = float(recall)
    state.metrics[f'{p}eval_accuracy'] = float(accuracy)
    state.metrics[f'{p}{name}'] = float(completeness * accuracy)


class EvalAISweep:
    """EvalAImetric for every (max_rmse, max_rmse_rel) of a grid at once (the search space of optimize_valid.yaml), from ONE solve and
    ONE evaluation per distinct camera: the two parameters only choose among the at most 1 + 5 T cameras a frame's solve produces
    (CameraCreator.sweep_device), and what a frame adds to the accumulators depends on its camera alone.  Per batch: the solve, the
    evaluation of every outcome slot (CameraEvaluator.evaluate_outcomes), and a gather-sum per grid point (sweep_fold).

    pred2cam: a CameraCreator with algorithm 'iterative_voter' or 'voter' (its own max_rmse / max_rmse_rel are not read); the grid
    is the cartesian product of the two lists, max_rmse outermost: .grid (n_grid,2), .params(g).  Same keys, same add_missed /
    total_frames handling as EvalAImetric, once per grid point g."""
    name = 'evalai'
    better = 'max'

    def __init__(self, pred2cam, max_rmse: Sequence[float], max_rmse_rel: Sequence[float], threshold: int = 5,
                 img_size: Tuple[int, int] = (960, 540)):
        from .prediction import sweep_grid
        self.pred2cam = pred2cam
        pred2cam.sweep_slots()                   # refuses the algorithms that have nothing to sweep
        self._values = (list(max_rmse), list(max_rmse_rel))
        self.grid = sweep_grid(*self._values)
        self.threshold = threshold
        self.img_size = tuple(int(v) for v in img_size)
        self._evaluator = None
        self.reset()

    def __len__(self):
        return len(self.grid)

    def params(self, g: int) -> dict:
        return {'max_rmse': float(self.grid[g, 0]), 'max_rmse_rel': float(self.grid[g, 1])}

    def reset(self):
        self.total_frames = 0
        self._skipped = 0
        self._acc = None             # fp64 (n_grid, 8) on the device: EvalAImetric's accumulator, one row per grid point

    def add_missed(self, n: int):
        self.total_frames += int(n)
        self._skipped += int(n)

    evaluator = EvalAImetric.evaluator

    def update(self, step_output: dict):
        preds = step_output['prediction']
        d_lp = None
        lp = self.pred2cam.line_points_array(step_output.get('img_name'))
        if lp is not None:
            d_lp = torch.from_numpy(lp).to(preds.device)
        outcomes, choice = self.pred2cam.sweep_device(preds.contiguous().float(), d_lp, *self._values)
        self.update_outcomes(outcomes, choice, step_output['raw_annots'])

    def update_outcomes(self, outcomes: torch.Tensor, choice: torch.Tensor, raw_annots: List[dict]):
        B = outcomes.shape[0]
        self.total_frames += B
        if B == 0:
            return
        ev = self.evaluator(outcomes.device)
        a = ev.sweep_fold(ev.evaluate_outcomes(outcomes, raw_annots), choice)
        self._acc = a if self._acc is None else self._acc + a

    def _read(self):
        if self._acc is None:
            return np.zeros((len(self.grid), 8))
        return self._acc.cpu().numpy()

    def compute(self) -> List[float]:
        """EvalAImetric.compute (completeness) per grid point."""
        a = self._read()
        return [(self.total_frames - (float(a[g, 0]) + self._skipped)) / self.total_frames if self.total_frames > 0 else 0.0
                for g in range(len(self.grid))]

    def epoch_complete(self, state, g: int):
        _evalai_epoch(state, self.name, self._read()[g], self._skipped, self.total_frames)


ACC_TS = (5.0, 10.0, 20.0)          # metrics.py:117-118
ACC_WS = (0.5, 0.35, 0.15)


def line_acc_counts(gt: torch.Tensor, pred: torch.Tensor, p_threshold: float, ts: Sequence[float] = ACC_TS) -> torch.Tensor:
    """sncal_line_acc_counts: gt, pred (B,C,2,3) fp32 on the GPU -> (len(ts),3) int64 [tp, fp, fn] on the device, all thresholds in
    one launch.  Asynchronous on the current stream."""
    import ctypes
    pred = _lib.require_device(pred, torch.float32, 'prediction')
    gt = _lib.require_device(gt, torch.float32, 'keypoints')
    if pred.dim() != 4 or tuple(pred.shape[2:]) != (2, 3) or gt.shape != pred.shape:
        raise _lib.SncalError(f'prediction {tuple(pred.shape)} and keypoints {tuple(gt.shape)} must both be (B,C,2,3)')
    out = torch.zeros((len(ts), 3), dtype=torch.int64, device=pred.device)
    c_ts = (ctypes.c_float * len(ts))(*[float(t) for t in ts])
    _lib.launch('sncal_line_acc_counts', pred.device, gt, pred, pred.shape[0], pred.shape[1], float(p_threshold), c_ts, len(ts), out)
    return out


def acc_from_counts(counts) -> float:
    """AccMetric.update + compute (metrics.py:105-137) on per-batch counts (n_batches, 3, 3) [threshold 5/10/20][tp, fp, fn].
    Mirrored, not fixed: the loop over the thresholds OVERWRITES acc each time and then adds acc * ws[i], so a batch is worth
    a@20 * 1.15 and the weights 0.5 / 0.35 never act; the epoch value is the plain mean over batches, whatever their sizes; a
    batch with tp + fp + fn == 0 raises ZeroDivisionError."""
    accs = []
    for batch in counts:
        acc = 0
        for i in range(len(ACC_TS)):
            tp, fp, fn = (int(v) for v in batch[i])
            acc = tp / (tp + fp + fn)
            acc += acc * ACC_WS[i]
        accs.append(acc)
    return float(np.mean(accs))


class AccMetric:
    """update() queues one kernel launch and keeps its (3,3) counts on the device; compute() reads them all at once."""
    name = 'acc'
    better = 'max'

    def __init__(self, num_keypoints: int = 23, conf_threshold: float = 0.2, device: str = 'cuda:0'):
        self.num_keypoints = num_keypoints
        self.conf_threshold = conf_threshold
        self.device = device
        self.reset()

    def reset(self):
        self._counts = []           # per update: (3,3) int64 on the device

    def update(self, step_output: dict):
        preds = step_output['prediction'].detach().to(torch.float32).contiguous()
        kpts = step_output['keypoints'].detach().to(preds.device, torch.float32).reshape(-1, self.num_keypoints, 2, 3).contiguous()
        self._counts.append(line_acc_counts(kpts, preds, self.conf_threshold))

    def _read(self) -> np.ndarray:
        if not self._counts:
            return np.zeros((0, len(ACC_TS), 3), dtype=np.int64)
        return torch.stack(self._counts).cpu().numpy()

    def compute(self) -> float:
        """nan (with numpy's warning) when nothing was added, as np.mean([]) is in the reference."""
        counts = self._read()
        return acc_from_counts(counts) if len(counts) else float(np.mean([]))

    def compute_detail(self) -> dict:
        """Not in the reference: a@5, a@10, a@20 over the POOLED counts of the epoch and the weighted score its docstring describes,
        0.5 a@5 + 0.35 a@10 + 0.15 a@20."""
        tot = self._read().sum(axis=0)
        out = {}
        for i, t in enumerate(ACC_TS):
            tp, fp, fn = (int(v) for v in tot[i])
            out[f'a@{int(t)}'] = tp / (tp + fp + fn)
        out['weighted'] = sum(w * out[f'a@{int(t)}'] for w, t in zip(ACC_WS, ACC_TS))
        return out

    def epoch_complete(self, state):
        state.metrics[f'{_prefix(state)}{self.name}'] = self.compute()


class ExtremityMetric:
    """The dev-kit's extremity metric (baseline/evaluate_extremities.py:156-261) with the counting on the device
    (sncal_extremity_counts, csrc/extremity.hip).  update() queues one launch for the batch, all thresholds at once, and keeps its
    three result tensors on the device, as AccMetric does; compute() reads everything once.

    thresholds      pixel thresholds (at most 8): each is scored as the reference's -t would score it
    conf_threshold  a decoded peak is a detection when p >= conf_threshold (get_line_data's prob_thre)
    scale           what turns the peaks' x, y into pixels: 4 for peaks in map cells (mask_heat_points_gauss), 1 for
                    EHMPredictionTransform's output, which carries its scale already
    img_size        (W, H) the annotations are scaled to, by (W - 1, H - 1) as scale_points does"""
    name = 'ext'
    better = 'max'

    def __init__(self, thresholds: Sequence[float] = (5, 10, 20), conf_threshold: float = 0.2, scale: float = 4,
                 img_size: Tuple[int, int] = (960, 540), device: str = 'cuda:0'):
        self.thresholds = tuple(thresholds)
        if not 1 <= len(self.thresholds) <= 8:
            raise _lib.SncalError(f'{len(self.thresholds)} thresholds (1..8)')
        self.conf_threshold = conf_threshold
        self.scale = scale
        self.img_size = tuple(int(v) for v in img_size)
        self.device = device
        self.reset()

    def reset(self):
        self._batches = []          # per update: (frame (T,B,4), cls (T,B,28,3), err (T,B,28,2)) on the device
        self._missing = []          # per missing frame: how many scored frames came before it
        self._scored = 0

    def update(self, step_output: dict):
        """step_output: {'prediction' (B,C,2,3) peaks, 'annot': the B raw annotations (normalised dicts) or their packed tuple}."""
        from .extremities import extremity_counts
        peaks = step_output['prediction'].detach().to(torch.float32).contiguous()
        self._keep(extremity_counts(step_output['annot'], peaks=peaks, img_size=self.img_size, ts=self.thresholds, scale=self.scale,
                                    p_threshold=self.conf_threshold))

    def update_annots(self, gt_annots, pred_annots):
        """The packed form: predictions as normalised dicts (the extremities_<id>.json files)."""
        from .extremities import extremity_counts
        self._keep(extremity_counts(gt_annots, pred_annots=pred_annots, img_size=self.img_size, ts=self.thresholds, device=self.device))

    def _keep(self, out):
        self._batches.append(out)
        self._scored += out[0].shape[1]

    def add_missing(self, n: int):
        """n frames without a prediction: accuracy, precision and recall 0 each (:175-179)."""
        self._missing += [self._scored] * int(n)

    @property
    def total_frames(self) -> int:
        return self._scored + len(self._missing)

    def _read(self):
        if not self._batches:
            T = len(self.thresholds)
            return np.zeros((T, 0, 4), np.int32), np.zeros((T, 0, 28, 3), np.int32), np.zeros((T, 0, 28, 2), np.float64)
        return tuple(torch.cat([b[i] for b in self._batches], dim=1).cpu().numpy() for i in range(3))

    def compute(self) -> dict:
        """{threshold: extremities.aggregate()'s dict}: mean / population std / median of the per-frame accuracy, precision and recall
        (precision over the frames with tp + fp > 0, recall over those with tp + fn > 0), the per-class table from the summed
        per-class confusion (numpy's nan for a zero denominator) and 'errors' {class: [distances, in frame order]}."""
        from .extremities import aggregate_counts
        frame, cls, err = self._read()
        return {t: aggregate_counts(frame[i], cls[i], err[i], self._missing) for i, t in enumerate(self.thresholds)}

    def epoch_complete(self, state, computed: dict = None):
        p = _prefix(state)
        for t, res in (computed if computed is not None else self.compute()).items():
            for key in ('acc', 'precision', 'recall'):
                state.metrics[f'{p}{self.name}_{key}@{t:g}'] = res['accuracy' if key == 'acc' else key]['mean']
