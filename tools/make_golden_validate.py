"""Capture tests/golden/validate.npz from the imported reference (CPU): HRNetLoss.forward on reproducible predictions, L2metric
over three updates, and the EvalAImetric aggregation with `pred2cam` stubbed by stored cameras.

    python tools/make_golden_validate.py

The reference is imported with the stubs of tools/make_golden.py (cv2, argus, torchvision are not needed for these paths).
Predictions are NOT stored: tests/validate_ref.make_pred regenerates them from the stored seed and keypoints.  Stored per loss
case: the reference's fp32 result, the fp64 evaluation of the same formula on the reference's own fp32 target (v64), and
d_ref = |ref - v64| / |v64| -- the reference's own distance from exact arithmetic, which the kernel tests scale their bound by.
"""
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
for _name in ('matplotlib', 'matplotlib.pyplot', 'tqdm'):                  # plotting / progress bars of the baseline scripts
    try:
        __import__(_name)
    except ImportError:
        sys.modules[_name] = types.ModuleType(_name)
        if _name == 'tqdm':
            sys.modules[_name].tqdm = lambda it, *a, **k: it

import validate_ref as vr  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def keypoints(rng, B, N, h, w, stride, empty_frame=None):
    """(B,N,3) float32 in IMAGE pixels as the dataset yields them: [x, y, 1] or [-1, -1, 0]."""
    kp = np.zeros((B, N, 3), dtype=np.float32)
    for b in range(B):
        for n in range(N):
            if b != empty_frame and rng.uniform() < 0.8:
                kp[b, n] = (rng.uniform(-2.0, w * stride + 2.0), rng.uniform(-2.0, h * stride + 2.0), 1.0)
            else:
                kp[b, n] = (-1.0, -1.0, 0.0)
    return kp


def gen_loss(out):
    from src.models.hrnet.loss import HRNetLoss
    rng = np.random.Generator(np.random.PCG64(4242))
    cases = {'small': dict(shape=(3, 58, 68, 120), stride=8, sigma=1.0, seed=11),
             'train': dict(shape=(2, 58, 270, 480), stride=2, sigma=2.0, seed=12),
             'ragged': dict(shape=(1, 7, 33, 257), stride=1, sigma=1.5, seed=13)}
    out['loss.names'] = np.array(list(cases))
    out['loss.weights'] = np.array(list(vr.WEIGHTS))
    for name, c in cases.items():
        B, C, h, w = c['shape']
        N, stride = C - 1, c['stride']
        kp = keypoints(rng, B, N, h, w, stride, empty_frame=1 if B > 1 else None)
        b = B - 1
        kp[b, 0] = (1.0 * stride, 0.4 * h * stride, 0.0)      # x / stride == 1.0 exactly, flag 0: "visible" by loss.py:49
        kp[b, 1] = (0.5 * w * stride, 1.0 * stride, 0.0)      # the same through y
        if stride != 1:
            kp[b, 2] = (1.0, 0.6 * h * stride, 0.0)           # x == 1.0 BEFORE the division, flag 0: not visible
        kp[b, 3] = (np.float32(0.5 * w * stride), np.float32(0.5 * h * stride), 1.0)
        kp[b, 3, :2] = np.rint(kp[b, 3, :2] / stride) * stride  # on a cell centre: target exactly 1, background exactly 0
        mask = np.ones((B, C), dtype=np.int64)
        mask[:, [n for n in (2, 4, N - 1) if n < N]] = 0
        mask[0, 3 % N] = 0
        if name == 'ragged':
            mask[0, N] = 0                                    # the background channel too
        pred = vr.make_pred(c['seed'], c['shape'], kp, stride)
        out[f'loss.{name}.shape'] = np.array(c['shape'])
        out[f'loss.{name}.stride'] = np.array(stride)
        out[f'loss.{name}.sigma'] = np.array(c['sigma'])
        out[f'loss.{name}.seed'] = np.array(c['seed'])
        out[f'loss.{name}.kp'] = kp
        out[f'loss.{name}.mask'] = mask
        tp, tk = torch.from_numpy(pred), torch.from_numpy(kp.reshape(B, -1))
        for mname, m in (('none', None), ('zeros', mask)):
            ref_loss = HRNetLoss(num_refinement_stages=0, sigma=c['sigma'], stride=stride, pred_size=(h, w), num_keypoints=N)
            k2 = tk.detach().clone().reshape(-1, N, 3)
            k2[:, :, :2] /= stride
            target = ref_loss.create_target(k2).numpy()                                   # the reference's own fp32 target
            mine = vr.target32(kp, stride, c['sigma'], (h, w))
            # torch's vectorised exp vs the correctly rounded one: 4 ulp on the keypoint channels (two factors), 2 ulp of 1.0 on 1 - max
            big = mine > 1e-30
            big[:, N] = False
            assert (np.abs(target.astype(np.float64)[big] - mine[big]) / mine[big]).max() < 5e-7
            assert np.abs(target - mine)[~big].max() <= 2.4e-7
            sums = vr.loss_terms64(pred, target, m)
            sums_mine = vr.loss_terms64(pred, mine, m)
            out[f'loss.{name}.{mname}.sums64'] = sums
            for wname, wts in vr.WEIGHTS.items():
                ref_loss.l2_w, ref_loss.kldiv_w, ref_loss.awing_w = wts
                ref = ref_loss([tp], tk, None if m is None else torch.from_numpy(m))
                assert ref.dtype == torch.float32
                ref = float(ref)
                v64 = vr.combine(sums, wts, c['shape'])
                d_ref = abs(ref - v64) / abs(v64)
                key = f'loss.{name}.{mname}.{wname}'
                out[key + '.ref'] = np.array(ref, dtype=np.float32)
                out[key + '.v64'] = np.array(v64)
                out[key + '.d_ref'] = np.array(d_ref)
                d_tgt = abs(vr.combine(sums_mine, wts, c['shape']) - v64) / abs(v64)
                print(f'{key:32s} ref {ref:.9g}  v64 {v64:.12g}  d_ref {d_ref:.3g}  (helper target vs reference target: {d_tgt:.2g})')


def gen_l2(out):
    from src.models.hrnet.metrics import L2metric
    rng = np.random.Generator(np.random.PCG64(77))
    N, thres = 57, [2.0, 5.0, 10.0, 50.0]
    m = L2metric(num_keypoints=N, conf_threshold=0.5, pckhs_thres=thres)
    sizes = [4, 4, 2]
    for i, B in enumerate(sizes):
        target = np.zeros((B, N, 3), dtype=np.float32)
        vis = rng.uniform(size=(B, N)) < 0.7
        target[..., 0] = np.where(vis, np.round(rng.uniform(0, 960, (B, N))), -1)
        target[..., 1] = np.where(vis, np.round(rng.uniform(0, 540, (B, N))), -1)
        target[..., 2] = vis
        err = rng.normal(0, 1, (B, N, 2)) * rng.choice([0.5, 3.0, 8.0, 40.0], size=(B, N, 1))
        pred = np.zeros((B, N, 3), dtype=np.float32)
        pred[..., :2] = np.round((target[..., :2] + err) / 2) * 2
        pred[..., 2] = rng.uniform(0.2, 1.0, (B, N))
        exact = rng.uniform(size=(B, N)) < 0.1
        pred[..., :2] = np.where(exact[..., None], target[..., :2], pred[..., :2])        # distance exactly 0
        out[f'l2.{i}.pred'], out[f'l2.{i}.target'] = pred, target.reshape(B, -1)
        m.update({'prediction': torch.from_numpy(pred), 'target': torch.from_numpy(target.reshape(B, -1))})
    state = types.SimpleNamespace(phase='val', metrics={})
    m.epoch_complete(state)
    out['l2.n'] = np.array(len(sizes))
    out['l2.thres'] = np.array(thres)
    out['l2.keys'] = np.array(list(state.metrics))
    out['l2.values'] = np.array([float(v) for v in state.metrics.values()], dtype=np.float64)
    out['l2.num_el'] = np.array(int(m.num_el))
    print('l2', {k: float(v) for k, v in state.metrics.items()})


def gen_evalai(out):
    """Cameras and annotations: the ten frames of tests/golden/evaluator_batch.npz (captured by tools/make_golden.py); frames 2
    and 6 get no camera; three updates of 4, 4 and 2 frames."""
    import src.models.hrnet.metrics as rm
    from baseline.camera import Camera
    g = np.load(os.path.join(GOLD, 'evaluator_batch.npz'))
    n = int(g['n'])
    none = [2, 6]
    cams, annots, names = {}, [], []
    for i in range(n):
        name = f'{i:05d}.jpg'
        cam = Camera(960, 540)
        cam.position, cam.rotation = g[f'{i}.position'].astype(np.float64), g[f'{i}.rotation'].astype(np.float64)
        fx, fy = g[f'{i}.f']
        cam.xfocal_length, cam.yfocal_length = np.float64(fx), np.float64(fy)          # float64 fields: tools/make_golden.py, get_polylines
        cam.principal_point = (np.float64(g[f'{i}.pp'][0]), np.float64(g[f'{i}.pp'][1]))
        cam.calibration = np.array([[fx, 0, cam.principal_point[0]], [0, fy, cam.principal_point[1]], [0, 0, 1.0]])
        cams[name] = None if i in none else cam
        annots.append({str(c): [{'x': float(p[0]), 'y': float(p[1])} for p in g[f'{i}.gt.{c}']] for c in g[f'{i}.gt_classes']})
        names.append(name)

    class Pred2Cam:
        stat = {}

        def __call__(self, pred, name):
            return cams[name]
    m = rm.EvalAImetric(Pred2Cam(), threshold=5, img_size=(960, 540), max_workers=1)
    m.executor.shutdown()
    m.executor = types.SimpleNamespace(map=lambda fn, items: map(fn, items))
    for lo, hi in ((0, 4), (4, 8), (8, 10)):
        m.update({'prediction': torch.zeros((hi - lo, 57, 3)), 'raw_annots': annots[lo:hi], 'img_name': names[lo:hi]})
    state = types.SimpleNamespace(phase='val', metrics={})
    m.epoch_complete(state)
    out['evalai.none'] = np.array(none)
    out['evalai.batches'] = np.array([[0, 4], [4, 8], [8, 10]])
    out['evalai.keys'] = np.array(list(state.metrics))
    out['evalai.values'] = np.array([float(v) for v in state.metrics.values()], dtype=np.float64)
    out['evalai.n_l2_proj'] = np.array(int(m.n_l2_proj))
    print('evalai', {k: float(v) for k, v in state.metrics.items()}, 'n_l2_proj', m.n_l2_proj)


def main():
    out = {}
    gen_loss(out)
    gen_l2(out)
    gen_evalai(out)
    path = os.path.join(GOLD, 'validate.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
