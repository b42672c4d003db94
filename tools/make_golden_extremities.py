"""Capture tests/golden/extremities.npz from the imported reference (CPU): the dev-kit's extremity metric
(/root/reference/baseline/evaluate_extremities.py) on two case sets.

    python tools/make_golden_extremities.py

The reference module is imported with empty stub modules for matplotlib, matplotlib.pyplot and tqdm (it is pure numpy); what is
stored comes from ITS evaluate_detection_prediction, mirror_labels and scale_points, composed as its __main__ composes them
(:187-236 per frame, :238-259 for the aggregates).  Its __main__ block itself cannot be imported, so that composition is restated
here, line for line, around the reference's functions.

Stored per set (A, B), data only:
    gt.points / gt.offsets                      the annotations, packed as annotations.pack_annotations packs them
    pred.points / pred.offsets                  the predictions as normalised dicts, packed (the extremities_<id>.json form)
    peaks, scale, p_threshold                   the predictions as decoded peaks (B,23,2,3) float32 where the class is a line class
    img_size, ts
    <form>.frame / .cls / .err                  what sncal_extremity_counts must write for form = packed, peaks
    <form>.agg (T,3,3)                          [accuracy, precision, recall] x [mean, std, median] over the frames
    <form>.per_class (T,28,3)                   accuracy, precision, recall per class from the summed confusion, NaN rows = class never seen
Set A also: <form>.agg_missing2 / packed.per_class unchanged (two missing frames appended), and the folder case: folder.removed (two
frame indices whose prediction file is absent), folder.threshold, folder.agg (3,3), folder.per_class (28,3), folder.lines (what the
reference prints).

Set A: the 24 annotated frames of tests/golden/annotations.json at 960 x 540, thresholds 5 / 10 / 20, predictions from a fixed seed
(see predictions_a).  Set B: hand-built frames at 513 x 257 with dyadic normalised coordinates, so pixels are exact (see set_b).
The tool asserts that every branch it was built for occurs, and that no compared distance of set A lies within 1e-9 of a threshold.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = '/root/reference'
sys.path.insert(0, ROOT)

for _name in ('matplotlib', 'matplotlib.pyplot', 'tqdm'):
    sys.modules[_name] = types.ModuleType(_name)
sys.modules['matplotlib'].pyplot = sys.modules['matplotlib.pyplot']
sys.modules['tqdm'].tqdm = None
sys.path.insert(0, REF)
from baseline import evaluate_extremities as ref  # noqa: E402

from sncal_amd.annotations import ANNOT_CLASSES, pack_annotations  # noqa: E402
from sncal_amd.lines import LINE_CLS  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
LINES = [LINE_CLS[i] for i in range(len(LINE_CLS))]
SYM = ref.SoccerPitch.symetric_classes
P_THRESHOLD = 0.2


# ---- the reference's composition ------------------------------------------------------------------------------------

def frame_eval(pred_px, gt_px, threshold):
    """:192-216 -> (accuracy, confusion, per_class_conf, reproj_errors, labelling, (accuracy1, accuracy2))."""
    confusion1, per_class_conf1, reproj_errors1 = ref.evaluate_detection_prediction(pred_px, gt_px, threshold)
    confusion2, per_class_conf2, reproj_errors2 = ref.evaluate_detection_prediction(pred_px, ref.mirror_labels(gt_px), threshold)
    accuracy1, accuracy2 = 0., 0.
    if confusion1.sum() > 0:
        accuracy1 = confusion1[0, 0] / confusion1.sum()
    if confusion2.sum() > 0:
        accuracy2 = confusion2[0, 0] / confusion2.sum()
    if accuracy1 > accuracy2:
        return accuracy1, confusion1, per_class_conf1, reproj_errors1, 0, (accuracy1, accuracy2)
    return accuracy2, confusion2, per_class_conf2, reproj_errors2, 1, (accuracy1, accuracy2)


def score(preds_px, gts_px, ts, missing=()):
    """The per-frame rows and the aggregates of :156-259 for every threshold; preds_px[i] None or i in `missing` = no prediction file."""
    cid = {c: i for i, c in enumerate(ANNOT_CLASSES)}
    B, T, N = len(gts_px), len(ts), len(ANNOT_CLASSES)
    frame = np.zeros((T, B, 4), np.int32)
    cls = np.zeros((T, B, N, 3), np.int32)
    err = np.full((T, B, N, 2), np.nan)
    agg = np.zeros((T, 3, 3))
    table = np.full((T, N, 3), np.nan)
    lines, stats = [], []
    for it, t in enumerate(ts):
        accuracies, precisions, recalls, per_class_confusion_dict = [], [], [], {}
        for b in range(B):
            if b in missing:
                accuracies.append(0.)
                precisions.append(0.)
                recalls.append(0.)
                continue
            accuracy, confusion, per_class_conf, reproj_errors, lab, both = frame_eval(preds_px[b], gts_px[b], t)
            stats.append((lab, both, confusion, reproj_errors, per_class_conf))
            accuracies.append(accuracy)
            if confusion[0, :].sum() > 0:
                precisions.append(confusion[0, 0] / (confusion[0, :].sum()))
            if (confusion[0, 0] + confusion[1, 0]) > 0:
                recalls.append(confusion[0, 0] / (confusion[0, 0] + confusion[1, 0]))
            for line_class, confusion_mat in per_class_conf.items():
                if line_class in per_class_confusion_dict.keys():
                    per_class_confusion_dict[line_class] = per_class_confusion_dict[line_class] + confusion_mat
                else:
                    per_class_confusion_dict[line_class] = confusion_mat
            assert confusion[1, 1] == 0
            frame[it, b] = (confusion[0, 0], confusion[0, 1], confusion[1, 0], lab)
            for name, m in per_class_conf.items():
                cls[it, b, cid[name]] = (m[0, 0], m[0, 1], m[1, 0])
            for name, d in reproj_errors.items():
                err[it, b, cid[name]] = d
        with np.errstate(all='ignore'):
            for k, v in enumerate((accuracies, precisions, recalls)):
                agg[it, k] = (np.mean(v), np.std(v), np.median(v)) if v else np.nan
            out = [f" On SoccerNet test set, {n} mean value : {agg[it, k, 0] * 100:2.2f}% with standard deviation of {agg[it, k, 1] * 100:2.2f}% "
                   f"and median of {agg[it, k, 2] * 100:2.2f}%" for n, k in (('recall', 2), ('precision', 1), ('accuracy', 0))]
            for c, name in enumerate(ANNOT_CLASSES):                   # the reference prints in its dict's order; here in class order
                if name not in per_class_confusion_dict:
                    continue
                confusion_mat = per_class_confusion_dict[name]
                class_accuracy = confusion_mat[0, 0] / confusion_mat.sum()
                class_recall = confusion_mat[0, 0] / (confusion_mat[0, 0] + confusion_mat[1, 0])
                class_precision = confusion_mat[0, 0] / (confusion_mat[0, 0] + confusion_mat[0, 1])
                table[it, c] = (class_accuracy, class_precision, class_recall)
                out.append(f"For class {name}, accuracy of {class_accuracy * 100:2.2f}%, precision of {class_precision * 100:2.2f}%  and recall of "
                           f"{class_recall * 100:2.2f}%")
        lines.append(out)
    return {'frame': frame, 'cls': cls, 'err': err, 'agg': agg, 'per_class': table}, lines, stats


# ---- predictions in both forms ------------------------------------------------------------------------------------------

def peaks_points(peaks, scale, prob_thre):
    """get_line_data's `points` (src/utils/export_line_result.py:115-124) for one frame's (C,2,3) float32 peaks, as the dict the
    scorer takes: classes without a kept point left out."""
    out = {}
    for k in range(peaks.shape[0]):
        valid_points = []
        for n in range(2):
            x, y, p = peaks[k, n]
            if p >= prob_thre:
                valid_points.append({'x': float(x * scale), 'y': float(y * scale)})
        if valid_points:
            out[LINES[k]] = valid_points
    return out


def to_dicts(frames):
    return [{c: [{'x': float(x), 'y': float(y)} for x, y in pts] for c, pts in f.items()} for f in frames]


def predictions_a(gts, W, H, seed=20240521):
    """Per frame {class: [(x_px, y_px), ...]} with pixels on multiples of 4 and the matching peaks (B,23,2,3) at scale 4: the
    annotation's first / last point of each line class, jittered with sigma in {0, 2, 6, 15} px (one sigma for the whole frame, nothing dropped, in half
    of the frames; per class otherwise); classes dropped; end points dropped (single-point predictions); pairs reversed; every third
    frame named by the mirrored classes; a few spurious classes; frame 7 without any prediction."""
    rng = np.random.Generator(np.random.PCG64(seed))
    B = len(gts)
    peaks = np.zeros((B, 23, 2, 3), np.float32)
    preds = []
    for b, gt in enumerate(gts):
        pred = {}
        frame_sigma = (0, 15, 6)[(b // 3) % 3] if b % 3 == 1 else 15 if b % 6 == 0 else None
        for k, name in enumerate(LINES):
            if b == 7:
                break
            if name in gt and len(gt[name]):
                if frame_sigma is None and rng.uniform() < 0.15:
                    continue                                            # class dropped
                sigma = frame_sigma if frame_sigma is not None else (0, 2, 6, 15)[int(rng.integers(4))]
                ends = np.array([gt[name][0], gt[name][-1]], np.float64) * (W - 1, H - 1)
                ends = 4.0 * np.rint((ends + rng.normal(0, 1, (2, 2)) * sigma) / 4.0)
                if rng.uniform() < 0.3:
                    ends = ends[::-1]                                   # pair reversed
                keep = [True, True]
                if frame_sigma is None and rng.uniform() < 0.2:
                    keep[int(rng.integers(2))] = False                  # one end dropped
            elif frame_sigma is None and rng.uniform() < 0.08:
                ends = 4.0 * np.rint(rng.uniform((0, 0), (W, H), (2, 2)) / 4.0)      # spurious class
                keep = [True, True]
            else:
                continue
            out = SYM[name] if b % 3 == 0 else name                     # named by the mirrored class
            ko = LINES.index(out)
            conf = rng.uniform(0.3, 0.95, 2)
            for i in range(2):
                peaks[b, ko, i] = (ends[i, 0] / 4.0, ends[i, 1] / 4.0, conf[i] if keep[i] else rng.uniform(0.0, 0.19))
            pred[out] = [tuple(ends[i]) for i in range(2) if keep[i]]
        preds.append(pred)
    return preds, peaks


def set_b():
    """Hand-built frames in PIXELS at 513 x 257 (normalised = pixel / 512, / 256: exact) -> (gts_px, preds_px) as {class: [(x, y)]}."""
    A = [(100, 100), (200, 100)]
    gts, preds = [], []

    def add(gt, pred):
        gts.append(gt)
        preds.append(pred)
    add({'Side line top': A}, {'Side line top': [(103, 104), (200, 100)]})                  # 0: a distance of exactly 5: not a hit at t = 5
    add({'Side line top': A}, {'Side line top': [(150, 60), (110, 100)]})                   # 1: dist1rev == dist1, dist2rev < dist2: reversed
    add({'Side line left': A, 'Big rect. left main': [(40, 40), (40, 80)]},                 # 2: equal accuracies 2 / 6: mirrored, seen in cls
        {'Side line left': A, 'Big rect. right main': [(40, 40), (40, 80)]})
    add({'Middle line': [(256, 10), (256, 120), (256, 250)]}, {'Middle line': [(256, 12), (257, 249)]})       # 3: maps to itself
    add({}, {'Side line top': A, 'Goal left crossbar': [(10, 10)]})                         # 4: empty ground truth, predictions
    add({}, {})                                                                             # 5: both empty: sum 0, labelling 1
    add({'Side line bottom': [(100, 200)]}, {'Side line bottom': [(101, 201), (300, 220)]})  # 6: a ground-truth class of one point
    add({'Side line right': [(400 + i, 20 + 5 * i) for i in range(40)], 'Side line top': A},  # 7: a 40-point polyline missed: fn += 40
        {'Side line top': A})
    add({'Circle central': [(250 + i, 120 + (i % 3)) for i in range(9)], 'Middle line': [(256, 10), (256, 250)]},       # 8: ignored on both sides
        {'Circle central': [(0, 0), (512, 256)], 'Middle line': [(256, 10), (256, 250)]})
    add({'Goal unknown': [(30, 30), (31, 60)], 'Line unknown': [(5, 5)], 'Side line top': A},   # 9: annotated, never detected: fn
        {'Side line top': [(200, 100), (100, 100)]})
    add({'Big rect. left top': [(60, 50), (120, 50)]}, {'Big rect. left top': [(60, 50), (120, 52)]})       # 10: a peak with p == p_threshold is kept
    add({'Circle left': [(60 + i, 100 + i * i % 7) for i in range(8)], 'Side line left': A},    # 11: circles other than the central one count
        {'Circle right': [(60, 100), (67, 100)], 'Side line right': A})
    return gts, preds


def peaks_b(preds_px):
    """Set B's predictions as peaks at scale 1 (pixels), line classes only; frame 10's second peak sits exactly on p_threshold."""
    peaks = np.zeros((len(preds_px), 23, 2, 3), np.float32)
    for b, pred in enumerate(preds_px):
        for name, pts in pred.items():
            if name not in LINES:
                continue
            k = LINES.index(name)
            for i, (x, y) in enumerate(pts):
                peaks[b, k, i] = (x, y, 0.75)
    peaks[10, LINES.index('Big rect. left top'), 1, 2] = np.float32(P_THRESHOLD)
    peaks[10, LINES.index('Big rect. left top'), 0, 2] = np.nextafter(np.float32(P_THRESHOLD), np.float32(1))
    peaks[6, LINES.index('Side line top'), 0] = (9, 9, np.nextafter(np.float32(P_THRESHOLD), np.float32(0)))       # just below: dropped
    return peaks


def normalised(frames_px, W, H):
    return [{c: [(x / (W - 1), y / (H - 1)) for x, y in pts] for c, pts in f.items()} for f in frames_px]


def store(out, key, gts_norm, preds_norm, peaks, scale, size, ts):
    W, H = size
    gts_d, preds_d = to_dicts(gts_norm), to_dicts(preds_norm)
    g_pts, g_off, _ = pack_annotations(gts_d)
    p_pts, p_off, _ = pack_annotations(preds_d)
    out.update({f'{key}.gt.points': g_pts, f'{key}.gt.offsets': g_off, f'{key}.pred.points': p_pts, f'{key}.pred.offsets': p_off,
                f'{key}.peaks': peaks, f'{key}.scale': np.float32(scale), f'{key}.p_threshold': np.float32(P_THRESHOLD),
                f'{key}.img_size': np.array(size, np.int32), f'{key}.ts': np.array(ts, np.float64)})
    gts_px = [ref.scale_points(g, W, H) for g in gts_d]
    forms = {'packed': [ref.scale_points(p, W, H) for p in preds_d],
             'peaks': [peaks_points(peaks[b], scale, P_THRESHOLD) for b in range(len(peaks))]}
    res = {}
    for form, preds_px in forms.items():
        got, lines, stats = score(preds_px, gts_px, ts)
        res[form] = (got, stats, preds_px, gts_px)
        for k, v in got.items():
            out[f'{key}.{form}.{k}'] = v
    return res


def main():
    out = {}
    # ---- set A ----
    with open(os.path.join(GOLD, 'annotations.json')) as f:
        gts = [{c: [tuple(p) for p in pts] for c, pts in case['points'].items()} for case in json.load(f)]
    assert len(gts) == 24
    W, H, ts = 960, 540, (5.0, 10.0, 20.0)
    preds_px, peaks = predictions_a(gts, W, H)
    res = store(out, 'A', gts, normalised(preds_px, W, H), peaks, 4, (W, H), ts)
    for form, (got, stats, p_px, g_px) in res.items():
        labs = [(lab, a1, a2) for lab, (a1, a2), _, _, _ in stats]
        n0, n1 = sum(lab == 0 for lab, _, _ in labs), sum(lab == 1 and a2 > a1 for lab, a1, a2 in labs)
        ties = sum(a1 == a2 for _, a1, a2 in labs)
        single = sum(len(v) == 1 for p in p_px for v in p.values())
        no_prec = int(((got['frame'][..., 0] + got['frame'][..., 1]) == 0).sum())
        no_rec = int(((got['frame'][..., 0] + got['frame'][..., 2]) == 0).sum())
        fp_only = int(((got['cls'][..., 0] == 0) & (got['cls'][..., 1] > 0) & np.isnan(got['err'][..., 0])).sum())
        fn_only = int((got['cls'][..., 2] > 0).sum())
        far = int(((got['cls'][..., 1] > 0) & ~np.isnan(got['err'][..., 0])).sum())
        print(f'A.{form}: labelling 0 in {n0} cells, labelling 1 strictly in {n1}, ties {ties}; single-point classes {single}; precision '
              f'undefined in {no_prec} cells, recall in {no_rec}; fp-only rows {fp_only}, fn rows {fn_only}, too-far rows {far}')
        assert n0 and n1 and ties and single and no_prec and no_rec and fp_only and fn_only and far
        assert n0 + n1 + ties == len(labs) == 72
        # reversed pairs occur: a stored pair differs from the straight one
        rev = 0
        for b in range(24):
            for name, d in stats[b][3].items():
                gt_cls = name if stats[b][0] == 0 else SYM[name]
                g, p = g_px[b][gt_cls], p_px[b][name]
                rev += ref.distance(g[0], p[0]) != d[0]
        assert rev, 'no reversed pair'
        # no compared distance near a threshold, under either labelling
        for b in range(24):
            for g in (g_px[b], ref.mirror_labels(g_px[b])):
                for d in ref.evaluate_detection_prediction(p_px[b], g, 5.0)[2].values():
                    assert all(abs(v - t) > 1e-9 for v in d for t in ts), (b, d)
    # two missing frames appended (ExtremityMetric.add_missing(2) after the updates)
    for form, (got, stats, p_px, g_px) in res.items():
        got2, _, _ = score(p_px + [None, None], g_px + [{}, {}], ts, missing=(24, 25))
        out[f'A.{form}.agg_missing2'] = got2['agg']
        assert np.array_equal(got2['per_class'], got['per_class'], equal_nan=True)
    # the folder case: two prediction files absent, threshold 10
    removed = (5, 17)
    _, _, p_px, g_px = res['packed']
    gotf, lines, _ = score(p_px, g_px, (10.0,), missing=removed)
    out.update({'A.folder.removed': np.array(removed, np.int32), 'A.folder.threshold': np.float64(10), 'A.folder.agg': gotf['agg'][0],
                'A.folder.per_class': gotf['per_class'][0], 'A.folder.lines': np.array(lines[0])})
    # ---- set B ----
    W, H = 513, 257
    g_b, p_b = set_b()
    res = store(out, 'B', normalised(g_b, W, H), normalised(p_b, W, H), peaks_b(p_b), 1, (W, H), ts)
    got, stats, p_px, g_px = res['packed']
    for b in range(len(g_b)):                                            # dyadic coordinates: the pixels come back exactly
        assert all(tuple(q.values()) == tuple(map(float, w)) for c in g_b[b] for q, w in zip(g_px[b][c], g_b[b][c]))
        assert all(tuple(q.values()) == tuple(map(float, w)) for c in p_b[b] for q, w in zip(p_px[b][c], p_b[b][c]))
    cid = {c: i for i, c in enumerate(ANNOT_CLASSES)}
    fr, cl, er = got['frame'], got['cls'], got['err']
    assert er[0, 0, cid['Side line top'], 0] == 5.0 and fr[0, 0].tolist() == [1, 1, 0, 0] and fr[1, 0].tolist() == [2, 0, 0, 0]
    assert er[2, 1, cid['Side line top']].tolist() == [np.sqrt(4100.0), 10.0] and fr[2, 1].tolist() == [1, 1, 0, 0]      # at t = 20; below, a tie
    assert fr[0, 2].tolist() == [2, 2, 2, 1] and cl[0, 2, cid['Side line left']].tolist() == [0, 2, 0] \
        and cl[0, 2, cid['Big rect. right main']].tolist() == [2, 0, 0] and stats[2][1][0] == stats[2][1][1] > 0
    assert fr[0, 3].tolist() == [2, 0, 0, 1] and fr[0, 4].tolist() == [0, 3, 0, 1] and fr[0, 5].tolist() == [0, 0, 0, 1]
    assert fr[0, 6, :3].tolist() == [1, 1, 0] and fr[0, 7, 2] == 40 and fr[0, 8].tolist() == [2, 0, 0, 1]
    assert fr[0, 9, :3].tolist() == [2, 0, 3] and cl[0, 9, cid['Goal unknown']].tolist() == [0, 0, 2]
    assert fr[0, 11].tolist() == [4, 0, 0, 1]
    pk = res['peaks'][0]
    assert pk['frame'][0, 10].tolist() == [2, 0, 0, 0] and np.array_equal(pk['frame'][:, 6], fr[:, 6])
    assert pk['frame'][0, 8].tolist() == fr[0, 8].tolist() and pk['frame'][0, 11].tolist() == [2, 0, 8, 1]       # no circle among the peaks
    path = os.path.join(GOLD, 'extremities.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
