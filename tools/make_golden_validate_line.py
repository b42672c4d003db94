"""Capture tests/golden/validate_line.npz from the imported reference (CPU): the line model's target maps
(EHMDataset._generate_keypoint_maps), EHMLoss.forward on reproducible predictions, AccMetric over three updates, and the labels
of sort_anno + get_extreme_points.

    python tools/make_golden_validate_line.py

The reference is imported with the stubs of tools/make_golden.py.  Predictions are NOT stored: tests/validate_line_ref.make_pred
regenerates them from the stored seed and endpoints; the reference's maps are stored for the small shapes only.  Stored per loss
case and weight set: the reference's fp32 result on its own fp32 maps, the fp64 evaluation of the same formula on those maps (v64)
and d_ref = |ref - v64| / |v64|, the reference's own distance from exact arithmetic, which the kernel tests scale their bound by.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import make_golden as mg  # noqa: E402

mg.install_stubs()
_m = types.ModuleType('argus.metrics')
_m.Metric = type('Metric', (), {'__init__': lambda self: None})
sys.modules['argus.metrics'] = _m
sys.modules['argus'].metrics = _m

import validate_line_ref as vr  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
STORE_MAPS = ('small', 'wide')


def endpoints(rng, B, C, h, w, stride, empty_frame=None):
    """(B,C,2,3) float32 in IMAGE pixels as the dataset yields them: a line is [x, y, 1] twice or [-1, -1, 0] twice."""
    kp = np.zeros((B, C, 2, 3), dtype=np.float32)
    kp[..., :2] = -1
    for b in range(B):
        for c in range(C):
            if b != empty_frame and rng.uniform() < 0.6:
                for p in range(2):
                    kp[b, c, p] = (rng.uniform(0, w * stride), rng.uniform(0, h * stride), 1.0)
    return kp


def edge_cases(kp, b, h, w, stride):
    """Into frame b, channels 0..4: a tie of x / stride on .5 (to even, both ways), a point beyond the right and bottom edge, a
    point with negative coordinates (mu < 0), two points 3 px apart, a channel with one flag 0."""
    s = stride
    kp[b, 0] = [(2.5 * s, 1.5 * s, 1), (3.5 * s, 6.5 * s, 1)]            # -> mu (2, 2) and (4, 6)
    kp[b, 1] = [(w * s + 20, h * s + 9, 1), (w * s - 1, 3.2 * s, 1)]     # clamped to (w-1, h-1); rint(w - 0.25) = w, clamped in x
    kp[b, 2] = [(-3.25 * s, -1.5 * s, 1), (1.0 * s, -2.6 * s, 1)]        # mu (-3, -2) and (1, -3): maximum below 1 before normalisation
    kp[b, 3] = [(5.0 * s, 4.0 * s, 1), (5.0 * s + 3, 4.0 * s, 1)]        # 3 px apart: the same or the next cell, sum near 2
    kp[b, 4] = [(7.3 * s, 2.2 * s, 0), (2.1 * s, 5.7 * s, 1)]            # first point not drawn


def gen_cases(out):
    from src.models.line.dataset import EHMDataset
    from src.models.line.loss import EHMLoss
    rng = np.random.Generator(np.random.PCG64(2323))
    cases = {'small': dict(shape=(2, 23, 16, 24), stride=4, sigma=1, gmse_sigma=4.0, seed=21),
             'wide': dict(shape=(1, 5, 33, 61), stride=4, sigma=7, gmse_sigma=4.0, seed=22),
             'mid': dict(shape=(3, 23, 34, 60), stride=4, sigma=2, gmse_sigma=0.7, seed=23)}
    out['case.names'] = np.array(list(cases))
    out['case.weights'] = np.array(list(vr.WEIGHTS))
    for name, c in cases.items():
        B, C, h, w = c['shape']
        stride = c['stride']
        kp = endpoints(rng, B, C, h, w, stride, empty_frame=1 if B > 1 else None)
        edge_cases(kp, 0, h, w, stride)
        ds = object.__new__(EHMDataset)
        ds._stride, ds._sigma, ds.num_keypoint_pairs = stride, c['sigma'], C
        image = np.zeros((h * stride, w * stride, 3), dtype=np.uint8)
        maps = np.stack([ds._generate_keypoint_maps({'image': image, 'keypoints': kp[b].reshape(-1)}).numpy() for b in range(B)])
        assert maps.shape == (B, C, h, w) and maps.dtype == np.float32
        mine = vr.keypoint_maps(kp, c['sigma'], stride, (h, w), as_dataset=True)
        assert np.array_equal(maps, mine), name                            # the restatement repeats the dataset bit for bit
        exact = vr.keypoint_maps(kp, c['sigma'], stride, (h, w))
        assert np.all(np.abs(maps - exact) <= 2.0 ** -23 * exact + 2.0 ** -149), name
        pred = vr.make_pred(c['seed'], c['shape'], kp, stride)
        for k, v in c.items():
            out[f'case.{name}.{k}'] = np.array(v)
        out[f'case.{name}.kp'] = kp
        out[f'case.{name}.max'] = np.array(maps.max())
        if name in STORE_MAPS:
            out[f'case.{name}.maps'] = maps
        sums = vr.loss_terms64(pred, maps, c['gmse_sigma'])
        out[f'case.{name}.sums64'] = sums
        tp, tm = torch.from_numpy(pred), torch.from_numpy(maps)
        for wname, wts in vr.WEIGHTS.items():
            ref_loss = EHMLoss(num_refinement_stages=0, gmse_w=wts[0], awing_w=wts[1], sigma=c['gmse_sigma'])
            ref = ref_loss([tp], tm)
            assert ref.dtype == torch.float32
            ref = float(ref)
            v64 = vr.combine(sums, wts, c['shape'])
            d_ref = abs(ref - v64) / abs(v64)
            key = f'case.{name}.{wname}'
            out[key + '.ref'] = np.array(ref, dtype=np.float32)
            out[key + '.v64'] = np.array(v64)
            out[key + '.d_ref'] = np.array(d_ref)
            d_tgt = abs(vr.combine(vr.loss_terms64(pred, exact, c['gmse_sigma']), wts, c['shape']) - v64) / abs(v64)
            print(f'{key:24s} ref {ref:.9g}  v64 {v64:.12g}  d_ref {d_ref:.3g}  (fp64 maps vs the reference\'s fp32 maps: {d_tgt:.2g})')
        print(f'{name}: largest map value {maps.max():.7g}')


def gen_acc(out):
    from src.models.line.metrics import AccMetric
    rng = np.random.Generator(np.random.PCG64(99))
    C, thr = 23, 0.2
    m = AccMetric(num_keypoints=C, conf_threshold=thr, device='cpu')
    counts, per_t = [], []
    sizes = [2, 3, 1]
    for i, B in enumerate(sizes):
        gt = np.zeros((B, C, 2, 3), dtype=np.float32)
        gt[..., :2] = -1
        has = rng.uniform(size=(B, C)) < 0.6
        pts = np.round(np.stack([rng.uniform(0, 960, (B, C, 2)), rng.uniform(0, 540, (B, C, 2))], -1))
        gt[..., :2] = np.where(has[..., None, None], pts, -1)
        gt[..., 2] = has[..., None]
        err = rng.normal(0, 1, (B, C, 2, 2)) * rng.choice([1.0, 4.0, 9.0, 30.0], size=(B, C, 2, 1))
        pred = np.zeros((B, C, 2, 3), dtype=np.float32)
        pred[..., :2] = np.where(has[..., None, None], pts + np.round(err * 4) / 4, np.round(rng.uniform(0, 500, (B, C, 2, 2))))
        pred[..., 2] = np.where(has[..., None], rng.uniform(0.05, 1.0, (B, C, 2)), rng.uniform(0.0, 0.4, (B, C, 2)))
        swap = rng.uniform(size=(B, C)) < 0.3                               # the prediction's slots in the other order
        pred[swap] = pred[swap][:, ::-1]
        if i == 0:
            gt[0, 0] = [(100, 100, 1), (400, 300, 1)]
            pred[0, 0] = [(101, 100, 0.1), (300, 300, 0.9)]                 # the LOW-confidence prediction is the nearest to gt slot 0
            gt[0, 1] = [(-1, -1, 0), (-1, -1, 0)]
            pred[0, 1] = [(50, 60, 0.95), (70, 80, 0.05)]                   # no ground truth, one confident prediction: fp
            gt[0, 2] = [(10, 10, 1), (13, 14, 1)]
            pred[0, 2] = [(10, 14, 0.5), (500, 14, 0.2)]                    # distance 4 and exactly 5 (== t counts); confidence == threshold
        d = np.linalg.norm(gt[..., :, None, :2].astype(np.float64) - pred[..., None, :, :2].astype(np.float64), axis=-1).min(-1)
        for t in vr.ACC_TS:
            assert np.all((np.abs(d - t) > 1e-3) | (d == t)), 'a distance too close to a threshold to be decided in fp32'
        out[f'acc.{i}.gt'], out[f'acc.{i}.pred'] = gt, pred
        tg, tp_ = torch.from_numpy(gt.reshape(B, -1)), torch.from_numpy(pred)
        c = vr.acc_counts(gt, pred, thr)
        a_t = [m.a_t_score(tg.reshape(-1, C, 2, 3), tp_, t=t, p_threshold=thr) for t in vr.ACC_TS]
        for k in range(3):
            assert a_t[k] == c[k, 0] / c[k].sum(), (i, k)
        m.update({'prediction': tp_, 'keypoints': tg})
        counts.append(c)
        per_t.append(a_t)
    value = float(m.compute())
    assert value == vr.acc_value(counts)
    out['acc.n'] = np.array(len(sizes))
    out['acc.conf_threshold'] = np.array(thr)
    out['acc.counts'] = np.stack(counts)
    out['acc.a_t'] = np.array(per_t, dtype=np.float64)
    out['acc.per_batch'] = np.array([float(v) for v in m.acc], dtype=np.float64)
    out['acc.value'] = np.array(value)
    print('acc', value, 'per batch', [float(v) for v in m.acc], 'counts', np.stack(counts).tolist())


def gen_labels(out):
    from src.datatools.line import get_extreme_points, sort_anno
    with open(os.path.join(GOLD, 'annotations.json')) as f:
        inputs = [{k: [tuple(p) for p in v] for k, v in c['points'].items()} for c in json.load(f)]
    nan = float('nan')
    inputs += [
        {'Side line top': [(0.1, 0.3), (0.5, 0.3), (0.9, 0.3)], 'Middle line': [(0.5, 0.1), (0.52, 0.9)]},          # horizontal: no fit
        {'Side line left': [(0.2, 0.2)], 'Middle line': [(0.5, 0.1), (0.52, 0.9)]},                                  # one point
        {'Middle line': [(0.5, 0.9), (nan, 0.5), (0.47, 0.1), (0.48, 0.4)], 'Circle central': [(0.4, 0.5), (0.6, 0.5)],
         'Line unknown': [(0.1, 0.1)]},                                                                              # NaN point, ignored classes
        {'Side line bottom': [(0.9, 0.8), (0.1, 0.7), (0.5, 0.75), (0.5, 0.75)], 'Big rect. left main': [(0.3, 0.2), (0.2, 0.6)]},
    ]
    cases = []
    for pts in inputs:
        res, usable = sort_anno(pts, img_size=(960, 540))
        ext = get_extreme_points(res, img_size=(960, 540))
        labels = {str(i): None if v is None else [[float(x) for x in v[0][0]], [float(x) for x in v[0][1]], [float(x) for x in v[1]]]
                  for i, v in ext.items()}
        cases.append({'points': {k: [list(p) for p in v] for k, v in pts.items()}, 'usable': bool(usable), 'labels': labels})
    out['labels.json'] = np.array(json.dumps(cases))
    print('labels:', len(cases), 'cases,', sum(c['usable'] for c in cases), 'usable,',
          sum(v is not None for c in cases for v in c['labels'].values()), 'lines')


def main():
    out = {}
    gen_cases(out)
    gen_acc(out)
    gen_labels(out)
    path = os.path.join(GOLD, 'validate_line.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
