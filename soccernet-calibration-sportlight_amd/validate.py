"""Score a checkpoint: counterpart of /root/reference/src/models/hrnet/validate.py (val_config.yaml, optimize_valid.yaml) with
every stage on the GPU path.

    reference (argus Model.validate over get_loader)              here
    cv2.imread + ToTensor, get_intersections   dataset.py:52-87   JpegDecoder -> uint8 BGR frames; annotations.get_intersections
    model.val_step: forward, HRNetLoss, decode metamodel.py:59-86 HRNetMetaModel.val_step: one forward (heatmap + keypoints), fused loss
    L2metric                                   metrics.py:14-94   metrics.L2metric, accumulators on the device
    EvalAImetric: 16-process pool per frame    metrics.py:97-229  metrics.EvalAImetric: batched solve + batched evaluation
    Loss metric (argus)                                           mean of the step losses weighted by step size (see validate())

    python -m sncal_amd.validate --data DIR --model model.pth [--lines-file lines.pkl] [--batch-size 16] [--reduce 2]

The line model (line/train_config.yaml: val_loss and the monitored val_acc) is scored by validate_line():
    EHMDataset listing, sort_anno, extreme points  line/dataset.py:54-92   list_line_split, annotations.line_keypoints
    model.val_step: forward, EHMLoss, decode       line/metamodel.py:51-71 EHMMetaModel.val_step: one forward, fused loss, target rebuilt
    AccMetric                                      line/metrics.py:20-137  metrics.AccMetric: counts on the device

    python -m sncal_amd.validate --line --data DIR --model line.pth [--batch-size 8] [--reduce 2]

--reduce 2 / 4 / 8 decodes the split's frames at that fraction (libjpeg's scaled decode = cv2.imread's IMREAD_REDUCED_COLOR flags, not
cv2.resize): a 1920x1080 split scored by a 960x540 checkpoint.
--resize W H brings every frame to W x H after the decode with cv2.resize's bilinear shrink on the device (resize.resize_u8: the
cv2.resize of line/dataset.py:73): a 1280x720 split, or one of mixed sizes, scored by a 960x540 checkpoint.  It composes with --reduce.
"""
import argparse
import contextlib
import os
from typing import Callable, Dict, Iterable, List, Sequence, Union

import torch

from . import _lib
from .frames import (MAX_SOURCE_SIZES, _label_mode, annot_to_keypoints, decoded_batches, folder_batches,  # noqa: F401
                     labelled_batch, line_folder_batches, list_line_split, list_split, resize_plan,
                     train_batches)  # the loaders lived here until frames.py
from .lines import LINE_CLS
from .metrics import AccMetric, EvalAImetric, EvalAISweep, ExtremityMetric, L2metric
from .prediction import CameraCreator, parse_range
from .resize import add_resize_argument, parsed_resize


class _State:
    def __init__(self, phase='val'):
        self.phase = phase
        self.metrics = {}


class ValidationResult(dict):
    """The metrics dict; .frames = frames seen, .skipped = names of the frames that could not be decoded (counted as missed)."""
    frames = 0
    skipped: List[str] = []
    params: Dict[str, float] = {}           # validate(sweep=): the grid point this result belongs to
    extremities: Dict[float, dict] = None   # validate_line(extremities=): ExtremityMetric.compute()'s dict per threshold


class SweepResults(list):
    """validate(sweep=)'s ValidationResults in grid order (max_rmse outermost); .best = index of the first maximum of val_evalai."""
    best = 0


FOLDER_ONLY = {'transform': (None, 'labels'), 'labels': ('host', 'labels'), 'reduce': (1, 'frames'), 'resize': (None, 'frames')}


def _refuse_folder_keywords(data, **given):
    """The keywords of the folder form (FOLDER_ONLY: name -> (default, what a batch carries already)) are refused, in the order given,
    when one that is not at its default comes with batches handed in."""
    for name, value in given.items():
        default, carried = FOLDER_ONLY[name]
        if value != default and not isinstance(data, (str, os.PathLike)):
            raise _lib.SncalError(f'{name} applies to the folder form: batches handed in carry their {carried} already')


@contextlib.contextmanager
def _lent_loss(model, loss):
    """model.loss is `loss` for the block only (None: the model's own stays, built by the first val_step if need be)."""
    own_loss = model.loss
    if loss is not None:
        model.loss = loss
    try:
        yield
    finally:
        if loss is not None:
            model.loss = own_loss


def _epoch(model, data, open_folder: Callable, step: Callable):
    """One pass over data -- open_folder(path)'s batch dicts when it is a folder, else the iterable as it is: model.val_step per
    batch, then step(batch, out) for the metrics -> (val_loss, frames): the mean of the step losses weighted by step size (nan
    without a frame) and the frames that went through the network.  The host waits for the GPU once, at the end."""
    batches = open_folder(os.fspath(data)) if isinstance(data, (str, os.PathLike)) else None
    loss_sum = torch.zeros((), dtype=torch.float64, device=model.device)
    frames = 0
    try:
        for batch in (batches if batches is not None else data):
            out = model.val_step(batch)
            B = out['prediction'].shape[0]
            frames += B
            loss_sum = loss_sum + out['loss'].to(torch.float64) * B
            step(batch, out)
        model.check_range()
    finally:
        if batches is not None:
            batches.close()                    # ends the generator: its finally closes the decoders, also after an exception mid-epoch
    return (float(loss_sum.item()) / frames if frames else float('nan')), frames


def validate(model, data: Union[str, Iterable[dict]], camera: Union[CameraCreator, Sequence[CameraCreator]], batch_size: int = 16,
             loss=None, decoder_threads: int = 0, conf_threshold: float = 0.5, pckhs_thres: Sequence[float] = (2.0, 5.0, 10.0, 50.0),
             threshold: int = 5, img_size=(960, 540), transform=None, labels: str = 'host', reduce: int = 1, sweep: Dict[str, Sequence[float]] = None,
             resize=None):
    """-> {'val_loss', 'val_l2', 'val_precision', 'val_recall', 'val_pcks-2.0', ..., 'val_l2_reprojection', 'val_completeness',
    'val_eval_precision', 'val_eval_recall', 'val_eval_accuracy', 'val_evalai'} as floats (a ValidationResult).

    data    a SoccerNet split folder (NNNNN.jpg + NNNNN.json) or any iterable of the batch dicts the reference's loader yields
            ({'image', 'keypoints', 'mask', 'raw_annot', 'img_name'}; batch_size then is whatever the iterable delivers)
    camera  a CameraCreator, or a LIST of them: the network, the loss and L2metric run once per batch, only solve + evaluation run
            per calibrator, and a list of results comes back, one per calibrator -- the trials of optimize_valid.yaml without
            running the network once per trial
    loss    an HRNetLoss; default: the model's own (params['loss'] of the checkpoint)
    transform  folder form only.  None: the annotations as they are on disk.  augment.test_transform(): what the reference's
            validation loader applies (validate.py:33, train.py:34) -- FixLRAmbiguous mirrors the class names of a behind-the-goal
            frame annotated the other way round, so val_loss and the keypoint metrics of such frames are taken against the
            keypoints the reference takes them against
    labels  folder form only.  'host': annotations.get_intersections per frame; 'device': one launch of the label kernel per batch,
            the transform's FixLRAmbiguous included
    reduce  folder form only.  2 / 4 / 8: the frames are decoded at that fraction of their size (libjpeg's scaled decode, what
            cv2.imread returns with IMREAD_REDUCED_COLOR_2 / _4 / _8; not cv2.resize), so that a 1920x1080 split is scored by a
            network trained at 960x540.  img_size stays the size the metrics work in; the labels are normalised and do not change
    resize  folder form only.  (W, H): every frame is brought to that size after the decode (at 1 / reduce when given) by
            resize.resize_u8, cv2.resize's INTER_LINEAR on the device; frames of any size are taken, mixed sizes included
            (decoded_batches).  img_size is in the resized frame's units
    sweep   {'max_rmse': [...], 'max_rmse_rel': [...]}: the search space of optimize_valid.yaml in ONE pass.  camera then is one
            CameraCreator ('iterative_voter' or 'voter'; its own max_rmse / max_rmse_rel are not read): every batch is solved once
            and each distinct camera evaluated once (metrics.EvalAISweep), and a SweepResults comes back: one ValidationResult per
            point of the cartesian product, max_rmse outermost, each with .params, equal key by key to validate(..., [one
            calibrator per grid point]); .best is the first maximum of val_evalai.  val_loss and the keypoint metrics are computed
            once.  conf_thresh(s), min_points* and reliable_thresh change the solves themselves: they stay the caller's loop

    val_loss is the mean of the step losses weighted by step size.  This is the one definition here NOT taken from the reference:
    it is computed by pytorch-argus' Loss metric there, whose source is not part of the reference tree.
    A frame the decoder refuses (folder form) gets no prediction: it is left out of val_loss and the keypoint metrics and counted
    as a missed frame by the camera metrics, as a frame without a camera is.  The host waits for the GPU once, at the end."""
    _refuse_folder_keywords(data, transform=transform, labels=labels, reduce=reduce, resize=resize)
    if sweep is not None:
        if isinstance(camera, (list, tuple)):
            raise _lib.SncalError('sweep takes ONE CameraCreator: the grid replaces the list of calibrators')
        if set(sweep) != {'max_rmse', 'max_rmse_rel'}:
            raise _lib.SncalError(f"sweep={{'max_rmse': [...], 'max_rmse_rel': [...]}}, not keys {sorted(sweep)}")
    cams = list(camera) if isinstance(camera, (list, tuple)) else [camera]
    skipped: List[str] = []
    with _lent_loss(model, loss):
        loss_fn = model._loss()
        nk = loss_fn.num_keypoints
        l2 = L2metric(num_keypoints=nk, conf_threshold=conf_threshold, pckhs_thres=pckhs_thres)
        if sweep is not None:
            evals = [EvalAISweep(camera, sweep['max_rmse'], sweep['max_rmse_rel'], threshold=threshold, img_size=img_size)]
        else:
            evals = [EvalAImetric(c, threshold=threshold, img_size=img_size) for c in cams]

        def open_folder(folder):
            return folder_batches(folder, batch_size, model.device, nk, float(loss_fn.sigma), img_size, decoder_threads, skipped,
                                  transform=transform, labels=labels, reduce=reduce, resize=resize)

        def step(batch, out):
            l2.update(out)
            for ev in evals:
                ev.update(out)
        val_loss, _ = _epoch(model, data, open_folder, step)
    results = SweepResults() if sweep is not None else []
    for ev in evals:
        ev.add_missed(len(skipped))
        for g in (range(len(ev)) if sweep is not None else [None]):
            state = _State('val')
            state.metrics['val_loss'] = val_loss
            l2.epoch_complete(state)
            if g is None:
                ev.epoch_complete(state)
            else:
                ev.epoch_complete(state, g)
            res = ValidationResult({k: float(v) for k, v in state.metrics.items()})
            res.frames, res.skipped = ev.total_frames, list(skipped)          # the camera metric's own count: scored + skipped
            if g is not None:
                res.params = ev.params(g)
            results.append(res)
    if sweep is not None:
        scores = [r['val_evalai'] for r in results]
        results.best = scores.index(max(scores))
        return results
    return results if isinstance(camera, (list, tuple)) else results[0]


def validate_line(model, data: Union[str, Iterable[dict]], batch_size: int = 8, loss=None, conf_threshold: float = 0.2,
                  decoder_threads: int = 0, input_size=(960, 540), reduce: int = 1, extremities: Sequence[float] = None, resize=None):
    """Score a line-model checkpoint (EHMMetaModel) -> {'val_loss', 'val_acc'} as floats (a ValidationResult): the two numbers
    line/train_config.yaml logs and monitors.

    data    a SoccerNet split folder (NNNNN.jpg + NNNNN.json; frames whose annotation the reference's sort_anno rejects are
            dropped, as its dataset drops them) whose frames are input_size once decoded at 1 / reduce, or any iterable of the batch dicts the reference's loader
            yields ({'image', 'keypoints', 'line_para', ['keypoint_maps']}; batch_size then is whatever the iterable delivers)
    loss    an EHMLoss; default: the model's own (params['loss'] of the checkpoint)
    reduce  folder form only.  A 1920x1080 split is taken with reduce=2: libjpeg's scaled decode (cv2.imread with
            IMREAD_REDUCED_COLOR_2), which is NOT the cv2.resize of line/dataset.py:73 -- a declared deviation.
            The labels are normalised coordinates and do not change; a frame whose reduced size is not input_size is skipped
    resize  folder form only.  input_size again, as (W, H): every frame is brought to it after the decode (at 1 / reduce when given)
            by resize.resize_u8 -- the cv2.resize of line/dataset.py:73 -- so frames of any size are scored, mixed sizes included
    extremities  None (default): the two keys above, nothing else runs.  A tuple of pixel thresholds, e.g. (5, 10, 20): the
            dev-kit's extremity metric (baseline/evaluate_extremities.py; metrics.ExtremityMetric, one more launch per batch) on the
            decoded peaks with p >= conf_threshold, against each frame's RAW annotation scaled to input_size: the keys
            'val_ext_acc@t', 'val_ext_precision@t', 'val_ext_recall@t', the means over the frames, are added, and the per-class table and
            error lists are left in .extremities.  The folder form reads the annotations itself; in the iterable form every batch
            dict must carry 'annot', the B annotations {class: [{'x', 'y'}, ...]} in normalised coordinates (SncalError otherwise).
            The frames sort_anno drops are not scored here, as they are not in val_acc, and neither is a frame the decoder
            refuses: the dev-kit's scorer run over the folders (extremities.evaluate_extremities) scores every annotation file

    val_loss is the mean of the step losses weighted by step size, as in validate(); val_acc is AccMetric's value (the plain mean
    of the per-batch a@20 * 1.15, so it depends on batch_size, as in the reference).  A frame the decoder refuses (folder form) is
    left out and named in .skipped.  The host waits for the GPU once, at the end."""
    _refuse_folder_keywords(data, reduce=reduce, resize=resize)
    skipped: List[str] = []
    state = _State('val')
    with _lent_loss(model, loss):
        model._loss()
        acc = AccMetric(num_keypoints=len(LINE_CLS), conf_threshold=conf_threshold)
        # the prediction transform has applied its scale: the peaks are pixels already
        ext = None if extremities is None else ExtremityMetric(extremities, conf_threshold=conf_threshold, scale=1, img_size=input_size)

        def open_folder(folder):
            return line_folder_batches(folder, batch_size, model.device, acc.num_keypoints, input_size, decoder_threads, skipped,
                                       reduce=reduce, annots=ext is not None, resize=resize)

        def step(batch, out):
            if ext is not None and 'annot' not in batch:
                raise _lib.SncalError("validate_line(extremities=...): every batch dict must carry 'annot', the frames' raw annotations")
            acc.num_keypoints = out['prediction'].shape[1]          # the channel count is the network's
            acc.update(out)
            if ext is not None:
                ext.update({'prediction': out['prediction'], 'annot': batch['annot']})
        state.metrics['val_loss'], frames = _epoch(model, data, open_folder, step)
    acc.epoch_complete(state)
    detail = None
    if ext is not None:
        detail = ext.compute()
        ext.epoch_complete(state, detail)
    res = ValidationResult({k: float(v) for k, v in state.metrics.items()})
    if detail is not None:
        res.extremities = detail
    res.frames, res.skipped = frames + len(skipped), list(skipped)
    return res


def parser():
    ap = argparse.ArgumentParser(description='Validate a keypoint checkpoint on a SoccerNet split (validate.py counterpart)')
    ap.add_argument('--line', action='store_true', help='the checkpoint is the line model (EHMMetaModel): val_loss and val_acc')
    ap.add_argument('--data', required=True, help='split folder: NNNNN.jpg + NNNNN.json')
    ap.add_argument('--model', required=True, help='argus checkpoint of the keypoint model (model_name/params/nn_state_dict)')
    ap.add_argument('--lines-file', default=None, help='lines pickle of export_line_result.py (optional)')
    ap.add_argument('--batch-size', type=int, default=None, help='default 16, with --line 8')
    ap.add_argument('--reduce', type=int, default=1, choices=[1, 2, 4, 8],
                    help="decode the frames at 1/N of their size (libjpeg's scaled decode = cv2.IMREAD_REDUCED_COLOR_N)")
    add_resize_argument(ap)
    ap.add_argument('--sweep-max-rmse', default=None, metavar='START:STOP:STEP',
                    help="sweep camera.max_rmse over Hydra's range(start, stop, step), stop excluded (optimize_valid.yaml: 10:70:4); one solve per batch")
    ap.add_argument('--sweep-max-rmse-rel', default=None, metavar='START:STOP:STEP', help='the same for camera.max_rmse_rel (optimize_valid.yaml: 4:16:2)')
    ap.add_argument('--extremities', default=None, metavar='T[,T...]',
                    help="with --line: also the dev-kit's extremity metric at these pixel thresholds, e.g. 5,10,20")
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--dtype', default=None, choices=['fp16x3', 'bf16x3', 'fp32', 'bf16', 'fp8'])
    return ap


def main(argv=None):
    from .metamodel import load_model
    from .submit import default_calibrator
    ap = parser()
    a = ap.parse_args(argv)
    resize = parsed_resize(a)
    sweep = None
    if a.sweep_max_rmse is not None or a.sweep_max_rmse_rel is not None:
        if a.line:
            ap.error('--sweep-max-rmse / --sweep-max-rmse-rel are the keypoint model\'s: the line model has no calibrator')
        cal = default_calibrator(None)             # an axis that is not swept keeps the calibrator's value
        sweep = {'max_rmse': parse_range(a.sweep_max_rmse) if a.sweep_max_rmse is not None else [cal.max_rmse],
                 'max_rmse_rel': parse_range(a.sweep_max_rmse_rel) if a.sweep_max_rmse_rel is not None else [cal.max_rmse_rel]}
    ext = None
    if a.extremities is not None:
        if not a.line:
            ap.error("--extremities is the line model's metric: it goes with --line")
        ext = tuple(float(t) for t in a.extremities.split(','))
    if not torch.cuda.is_available():
        raise _lib.SncalError('no GPU visible: this package has no CPU path')
    model = load_model(a.model, device=a.device, dtype=a.dtype)
    if a.line:
        res = validate_line(model, a.data, batch_size=a.batch_size or 8, reduce=a.reduce, extremities=ext, resize=resize)
    else:
        res = validate(model, a.data, default_calibrator(a.lines_file), batch_size=a.batch_size or 16, reduce=a.reduce, sweep=sweep,
                       resize=resize)
    if sweep is not None:
        print(f"{'max_rmse':>10} {'max_rmse_rel':>12} {'completeness':>12} {'accuracy':>10} {'evalai':>10}")
        for r in res:
            print(f"{r.params['max_rmse']:>10g} {r.params['max_rmse_rel']:>12g} {r['val_completeness']:>12.6f} {r['val_eval_accuracy']:>10.6f} "
                  f"{r['val_evalai']:>10.6f}")
        best = res[res.best]
        print(f"best: max_rmse={best.params['max_rmse']:g} max_rmse_rel={best.params['max_rmse_rel']:g} val_evalai={best['val_evalai']:.6f}")
        res = best
    for k, v in res.items():
        print(f'{k}: {v:.6f}')
    if res.skipped:
        print(f'skipped: {len(res.skipped)} of {res.frames} frames')
    return res


if __name__ == '__main__':
    main()
