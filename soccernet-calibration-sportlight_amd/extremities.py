"""The dev-kit's extremity metric (/root/reference/baseline/evaluate_extremities.py): the published number of the line-detection task.

    reference                                                       here
    evaluate_detection_prediction                  :37-116          evaluate_detection_prediction (host restatement, numpy)
    mirror_labels, scale_points                    :24-34, 119-134  augment.mirror_labels, evaluate.scale_points
    __main__: both labellings per frame, the       :156-261         csrc/extremity.hip (sncal_extremity_counts) per batch,
      better kept, mean / std / median, per class                   aggregate() on the host; evaluate_extremities() over two folders
    get_line_data's `points` dict                  src/utils/export_line_result.py:115-124   the peaks form of extremity_counts
    extremities_<id>.json                          baseline/detect_extremities.py:116-117    export_extremities (see its docstring)

    python -m sncal_amd.extremities -s DATASET -p PREDICTIONS [-t 10] [--split test] [--resolution_width 960] [--resolution_height 540]

The histograms the reference draws from the per-class errors are not built (no matplotlib here); the lists they are drawn from are
returned as 'errors'.
"""
import argparse
import json
import os
import warnings
from typing import Dict, List, Sequence

import numpy as np

from . import _lib
from .annotations import ANNOT_CLASSES, pack_annotations
from .augment import mirror_labels
from .evaluate import scale_points  # noqa: F401  (the scorer's other half: re-exported beside evaluate_detection_prediction)
from .frames import decoded_batches
from .lines import LINE_CLS

IGNORED = 'Circle central'
FIRST_LINE = ANNOT_CLASSES.index(LINE_CLS[0])          # peak channel k is class FIRST_LINE + k


def distance(point1, point2):
    """:12-21."""
    diff = np.array([point1['x'], point1['y']]) - np.array([point2['x'], point2['y']])
    return np.sqrt(np.square(diff).sum())


def evaluate_detection_prediction(detected_lines, groundtruth_lines, threshold=2.):
    """:37-116, restated: {class: [{'x', 'y'} in pixels, ...]} twice -> (confusion (2,2) float32 [[tp, fp], [fn, 0]], {class: (2,2)
    float64}, {class: [dist1, dist2]}).  'Circle central' is ignored on both sides; a class on one side only counts all its points;
    a class on both sides compares first with first and last with last, or crossed when both crossed distances are <=; a distance
    below the threshold is a hit, anything else a false positive."""
    confusion_mat = np.zeros((2, 2), dtype=np.float32)
    per_class_confusion, errors_dict = {}, {}
    detected = [c for c in detected_lines if c != IGNORED]
    annotated = [c for c in groundtruth_lines if c != IGNORED]
    for cls in detected:
        if cls not in groundtruth_lines:
            n = len(detected_lines[cls])
            confusion_mat[0, 1] += n
            per_class_confusion[cls] = np.array([[0., n], [0., 0.]])
    for cls in annotated:
        if cls not in detected_lines:
            n = len(groundtruth_lines[cls])
            confusion_mat[1, 0] += n
            per_class_confusion[cls] = np.array([[0., 0.], [n, 0.]])
    for cls in detected:
        if cls not in groundtruth_lines:
            continue
        det, gt = detected_lines[cls], groundtruth_lines[cls]
        per_class_confusion[cls] = np.zeros((2, 2))
        dist1, dist1rev = distance(gt[0], det[0]), distance(gt[-1], det[0])
        dist2, dist2rev = distance(gt[-1], det[-1]), distance(gt[0], det[-1])
        if dist1rev <= dist1 and dist2rev <= dist2:
            dist1, dist2 = dist1rev, dist2rev
        errors_dict[cls] = [dist1, dist2]
        for d in (dist1, dist2):
            j = 0 if d < threshold else 1                    # too far: a false positive
            confusion_mat[0, j] += 1
            per_class_confusion[cls][0, j] += 1
    return confusion_mat, per_class_confusion, errors_dict


def evaluate_frame(prediction_px: dict, groundtruth_px: dict, threshold=2.):
    """:192-216: both labellings of one frame (pixels on both sides) -> (confusion, per_class, errors, labelling) of the kept one:
    the plain labelling (0) only when its accuracy is STRICTLY higher, else the annotation mirrored (1).  The accuracies are the
    reference's: a float32 quotient, or the Python float 0. for an empty matrix."""
    one = evaluate_detection_prediction(prediction_px, groundtruth_px, threshold)
    two = evaluate_detection_prediction(prediction_px, mirror_labels(groundtruth_px), threshold)
    acc = [0., 0.]
    for i, (conf, _, _) in enumerate((one, two)):
        if conf.sum() > 0:
            acc[i] = conf[0, 0] / conf.sum()
    return one + (0,) if acc[0] > acc[1] else two + (1,)


def host_counts(predictions_px: Sequence[dict], groundtruths_px: Sequence[dict], ts: Sequence[float]):
    """What sncal_extremity_counts writes, from evaluate_frame per frame and threshold: (frame (n_t,B,4) int32, cls (n_t,B,28,3)
    int32, err (n_t,B,28,2) float64) as numpy arrays."""
    B, T, N = len(predictions_px), len(ts), len(ANNOT_CLASSES)
    cid = {c: i for i, c in enumerate(ANNOT_CLASSES)}
    frame = np.zeros((T, B, 4), dtype=np.int32)
    cls = np.zeros((T, B, N, 3), dtype=np.int32)
    err = np.full((T, B, N, 2), np.nan, dtype=np.float64)
    for it, t in enumerate(ts):
        for b, (p, g) in enumerate(zip(predictions_px, groundtruths_px)):
            conf, per_class, errors, lab = evaluate_frame(p, g, t)
            frame[it, b] = (conf[0, 0], conf[0, 1], conf[1, 0], lab)
            for name, m in per_class.items():
                cls[it, b, cid[name]] = (m[0, 0], m[0, 1], m[1, 0])
            for name, d in errors.items():
                err[it, b, cid[name]] = d
    return frame, cls, err


def frame_rates(tp: int, fp: int, fn: int):
    """:200-224 for one frame's kept counts -> (accuracy, precision or None, recall or None), with the reference's types: float32
    quotients of the float32 confusion matrix; the accuracy of an empty matrix is the Python float 0."""
    tp, fp, fn = np.float32(tp), np.float32(fp), np.float32(fn)
    total = tp + fp + fn
    acc = tp / total if total > 0 else 0.
    return acc, (tp / (tp + fp) if tp + fp > 0 else None), (tp / (tp + fn) if tp + fn > 0 else None)


def aggregate(frames: List, cls_sum: np.ndarray, errors: Dict[str, list]) -> dict:
    """:218-259.  frames: per frame, in order, (tp, fp, fn) or None for a frame without a prediction file (accuracy, precision and
    recall 0., :175-179); cls_sum (28,3) the per-class counts summed over the frames -> {'accuracy' / 'precision' / 'recall': {'mean',
    'std', 'median'}, 'per_class': {class: {'accuracy', 'precision', 'recall'}}, 'errors', 'frames'}.  The lists hold what the
    reference's hold (float32 quotients, Python zeros), so numpy's mean / std / median give its bits; an empty list gives numpy's nan."""
    lists = {'accuracy': [], 'precision': [], 'recall': []}
    for f in frames:
        if f is None:
            for v in lists.values():
                v.append(0.)
            continue
        acc, prec, rec = frame_rates(*f)
        lists['accuracy'].append(acc)
        if prec is not None:
            lists['precision'].append(prec)
        if rec is not None:
            lists['recall'].append(rec)
    out = {'frames': len(frames)}
    with np.errstate(all='ignore'):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            for k, v in lists.items():
                out[k] = {'mean': float(np.mean(v)), 'std': float(np.std(v)), 'median': float(np.median(v))}
        per_class = {}
        for c, name in enumerate(ANNOT_CLASSES):
            tp, fp, fn = (np.float64(v) for v in cls_sum[c])
            if tp + fp + fn > 0:                             # the classes some frame's per_class_confusion carried
                per_class[name] = {'accuracy': float(tp / (tp + fp + fn)), 'precision': float(tp / (tp + fp)), 'recall': float(tp / (tp + fn))}
    out['per_class'] = per_class
    out['errors'] = errors
    return out


def aggregate_counts(frame: np.ndarray, cls: np.ndarray, err: np.ndarray, missing_after: Sequence[int] = ()) -> dict:
    """aggregate() on one threshold's rows of sncal_extremity_counts: frame (F,4), cls (F,28,3), err (F,28,2), frames in order;
    missing_after: for each frame without a prediction, how many scored frames came before it."""
    rows = [tuple(int(v) for v in f[:3]) for f in frame]
    for done, at in enumerate(sorted(missing_after)):
        rows.insert(at + done, None)
    errors: Dict[str, list] = {}
    for b in range(len(frame)):
        for c in np.nonzero(~np.isnan(err[b]).all(axis=1))[0]:
            errors.setdefault(ANNOT_CLASSES[c], []).extend(float(v) for v in err[b, c])
    return aggregate(rows, cls.sum(axis=0, dtype=np.int64) if len(cls) else np.zeros((len(ANNOT_CLASSES), 3), dtype=np.int64), errors)


def summary_lines(res: dict, split: str) -> List[str]:
    """The reference's three summary lines and its per-class lines (:241-261), in its format."""
    L = []
    for key in ('recall', 'precision', 'accuracy'):
        s = res[key]
        L.append(f" On SoccerNet {split} set, {key} mean value : {s['mean'] * 100:2.2f}% with standard deviation of {s['std'] * 100:2.2f}% "
                 f"and median of {s['median'] * 100:2.2f}%")
    for name, c in res['per_class'].items():
        L.append(f"For class {name}, accuracy of {c['accuracy'] * 100:2.2f}%, precision of {c['precision'] * 100:2.2f}%  and recall of "
                 f"{c['recall'] * 100:2.2f}%")
    return L


# ---- the device call ----------------------------------------------------------------------------------------------------

def _packed(side):
    return side if isinstance(side, tuple) else pack_annotations(side)


def extremity_counts(gt, peaks=None, pred_annots=None, img_size=(960, 540), ts: Sequence[float] = (5, 10, 20), scale: float = 4,
                     p_threshold: float = 0.2, device='cuda:0'):
    """sncal_extremity_counts for a batch -> (frame (n_t,B,4) int32 [tp, fp, fn, labelling], cls (n_t,B,28,3) int32, err
    (n_t,B,28,2) float64), on the device; asynchronous on the current stream.
    gt          B annotations {class: [{'x', 'y'} or (x, y), ...]} in NORMALISED coordinates, or pack_annotations' tuple of them
    peaks       (B,C,2,3) fp32 on the GPU, rows [x, y, p] in map cells (C <= 23 channels in LINE_CLS order): kept when p >= p_threshold,
                pixel = (x * scale, y * scale).  Rows that are pixels already (EHMPredictionTransform's output) take scale=1
    pred_annots the other form: predictions as normalised dicts (the extremities_<id>.json files) or their packed tuple
    A class outside ANNOT_CLASSES raises KeyError, as pack_annotations does."""
    import ctypes
    import torch
    if (peaks is None) == (pred_annots is None):
        raise _lib.SncalError('extremity_counts takes exactly one of peaks= and pred_annots=')
    g_pts, g_off, _ = _packed(gt)
    B, T = len(g_off), len(ts)
    if peaks is not None:
        peaks = _lib.require_device(peaks, torch.float32, 'peaks')
        if peaks.dim() != 4 or tuple(peaks.shape[2:]) != (2, 3) or peaks.shape[0] != B:
            raise _lib.SncalError(f'peaks {tuple(peaks.shape)} must be ({B},C,2,3)')
        dev = peaks.device
        parts = [g_pts, g_off]
    else:
        p_pts, p_off, _ = _packed(pred_annots)
        if len(p_off) != B:
            raise _lib.SncalError(f'{len(p_off)} predictions for {B} annotations')
        dev = torch.device(device)
        parts = [g_pts, g_off, p_pts, p_off]
    n_cls = len(ANNOT_CLASSES)
    c_ts = (ctypes.c_double * max(T, 1))(*[float(t) for t in ts])
    frame = torch.empty((T, B, 4), dtype=torch.int32, device=dev)
    cls = torch.empty((T, B, n_cls, 3), dtype=torch.int32, device=dev)
    err = torch.empty((T, B, n_cls, 2), dtype=torch.float64, device=dev)
    if B:
        # one upload, from pinned memory and without waiting: a copy from pageable memory would hold the host until the stream has
        # drained, i.e. until the forward queued in front of it has finished, and the next batch's JPEG stage would wait with it
        d_in, ptr = _lib.upload(parts, dev, pinned=True)
        if peaks is not None:
            args = (ptr[0], len(g_pts), ptr[1], peaks, peaks.shape[1], float(scale), float(p_threshold), None, 0, None)
        else:
            args = (ptr[0], len(g_pts), ptr[1], None, 0, float(scale), float(p_threshold), ptr[2], len(p_pts), ptr[3])
        _lib.launch('sncal_extremity_counts', dev, *args, B, n_cls, int(img_size[0]), int(img_size[1]), c_ts, T, frame, cls, err)
    elif not 1 <= T <= 8:
        raise _lib.SncalError(f'{T} thresholds (1..8)')
    return frame, cls, err


# ---- files -----------------------------------------------------------------------------------------------------------------

def peaks_to_points(peaks: np.ndarray, scale: float = 4, conf_threshold: float = 0.2) -> dict:
    """get_line_data's `points` (src/utils/export_line_result.py:115-124) for one frame's peaks (C,2,3) float32 rows [x, y, p], as
    the dict the scorer takes: per line class the slots with p >= conf_threshold, in slot order, as pixels (x * scale, y * scale)
    in float32; classes without a kept slot are left out (scale_points would drop them)."""
    peaks = np.asarray(peaks, dtype=np.float32)
    s, thr = np.float32(scale), np.float32(conf_threshold)
    out = {}
    for k in range(peaks.shape[0]):
        pts = [{'x': float(x * s), 'y': float(y * s)} for x, y, p in peaks[k] if p >= thr]
        if pts:
            out[LINE_CLS[k]] = pts
    return out


def peaks_to_extremities(peaks: np.ndarray, img_size=(960, 540), conf_threshold: float = 0.2, scale: float = 1) -> dict:
    """One frame's decoded peaks (C,2,3) rows [x, y, p] (pixels: EHMPredictionTransform's output; map cells with scale=4) -> the
    dev-kit's prediction dict {class: [{'x', 'y'}, ...]} in normalised coordinates: peaks_to_points' pixels divided by
    (W - 1, H - 1) -- the inverse of the scorer's scale_points.  Classes without a kept peak are left out."""
    w, h = img_size[0] - 1, img_size[1] - 1
    return {name: [{'x': p['x'] / w, 'y': p['y'] / h} for p in pts] for name, pts in peaks_to_points(peaks, scale, conf_threshold).items()}


def extremities_path(save_dir: str, img_name: str) -> str:
    return os.path.join(save_dir, f'extremities_{os.path.splitext(os.path.basename(img_name))[0]}.json')


def save_extremities(prediction: dict, path: str):
    """The dev-kit's writer (detect_extremities.py:283-285): json.dump(..., indent=4)."""
    with open(path, 'w') as f:
        json.dump(prediction, f, indent=4)


def export_extremities(img_dir: str, model, save_dir: str, batch_size: int = 64, conf_threshold: float = 0.2, decoder_threads: int = 0,
                       reduce: int = 1) -> int:
    """Run a line model (EHMMetaModel) over the .jpg files of img_dir and write extremities_<id>.json per frame in the dev-kit's
    schema -> files written.  The points are the kept peaks (p >= conf_threshold) as pixels divided by (W - 1, H - 1), so that the
    scorer's scale_points gives the pixels back; the dev-kit's own detector divides by (W, H) (detect_extremities.py:116-117) -- a
    declared choice.  A frame the decoder refuses gets no file: the scorer counts it as missing."""
    names = sorted(f for f in os.listdir(img_dir) if f.endswith('.jpg'))
    os.makedirs(save_dir, exist_ok=True)
    skipped: List[str] = []
    frames = decoded_batches(img_dir, names, batch_size, model.device, decoder_threads, skipped, reduce=reduce)
    written = 0
    try:
        for keep, image in frames:
            peaks = model.predict(image).cpu().numpy()
            size = (image.shape[2], image.shape[1])
            for j, p in zip(keep, peaks):
                save_extremities(peaks_to_extremities(p, size, conf_threshold), extremities_path(save_dir, names[j]))
                written += 1
    finally:
        frames.close()
    return written


def evaluate_extremities(soccernet_dir: str, prediction_dir: str, split: str = 'test', threshold=10, resolution=(960, 540),
                         batch_size: int = 256, device='cuda:0', verbose: bool = True) -> dict:
    """The dev-kit's folder-against-folder scorer (:156-261) over the device kernel: every .json of soccernet_dir/split (sorted; the
    reference takes os.listdir's order) against prediction_dir/split/extremities_<id>.json -> aggregate()'s dict.  Every annotation
    file is scored (none is dropped for what sort_anno would reject); a missing prediction file is a frame of accuracy, precision
    and recall 0.  Prints the reference's summary and per-class lines.  A class outside ANNOT_CLASSES raises KeyError."""
    from .metrics import ExtremityMetric
    dataset_dir = os.path.join(soccernet_dir, split)
    if not os.path.exists(dataset_dir):
        raise _lib.SncalError(f'{dataset_dir}: invalid dataset path')
    metric = ExtremityMetric(thresholds=(threshold,), img_size=resolution, device=device)
    gts, preds = [], []

    def flush():
        if gts:
            metric.update_annots(list(gts), list(preds))
            gts.clear(), preds.clear()
    for fname in sorted(f for f in os.listdir(dataset_dir) if '.json' in f):
        pred_file = os.path.join(prediction_dir, split, f"extremities_{fname.split('.')[0]}.json")
        if not os.path.exists(pred_file):
            flush()
            metric.add_missing(1)
            continue
        with open(os.path.join(dataset_dir, fname), 'r') as f:
            gts.append(json.load(f))
        with open(pred_file, 'r') as f:
            preds.append(json.load(f))
        if len(gts) == batch_size:
            flush()
    flush()
    res = metric.compute()[threshold]
    if verbose:
        for line in summary_lines(res, split):
            print(line)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description='Score extremity predictions against SoccerNet annotations (evaluate_extremities.py counterpart)')
    ap.add_argument('-s', '--soccernet', default='./annotations', type=str, help='Path to the SoccerNet-V3 dataset folder')
    ap.add_argument('-p', '--prediction', default='./results_bis', required=False, type=str, help='Path to the prediction folder')
    ap.add_argument('-t', '--threshold', default=10, required=False, type=int, help='Accuracy threshold in pixels')
    ap.add_argument('--split', required=False, type=str, default='test', help='Select the split of data')
    ap.add_argument('--resolution_width', required=False, type=int, default=960, help='width resolution of the images')
    ap.add_argument('--resolution_height', required=False, type=int, default=540, help='height resolution of the images')
    a = ap.parse_args(argv)
    return evaluate_extremities(a.soccernet, a.prediction, split=a.split, threshold=a.threshold,
                                resolution=(a.resolution_width, a.resolution_height))


if __name__ == '__main__':
    main()
