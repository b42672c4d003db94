"""Capture tests/golden/loss_grad.npz from the imported reference (CPU): the gradient of HRNetLoss.forward and EHMLoss.forward with
respect to the prediction, by torch autograd in fp32, on the loss cases of validate.npz and validate_line.npz.

    python tools/make_golden_loss_grad.py

The reference is imported with the stubs of tools/make_golden.py, as tools/make_golden_validate.py does.  Predictions are NOT
stored (the two *_ref.make_pred regenerate them).  Whole gradients are not stored either; per combination:
    samples   the reference gradient at the 4096 positions of loss_grad_ref.seeded_positions(case seed)
    top_idx   the 64 flat positions of largest |gradient|, and `top`, the reference gradient there
    gmax      max |g64|, g64 the fp64 evaluation of the same formula (tests/loss_grad_ref.py) on the reference's own fp32 target
    E_ref     max |g_ref32 - g64| / gmax: the reference's own distance from exact arithmetic, which the kernel tests scale their bound by
    E_tgt     max |g64 - g64'| / gmax, g64' on the helper's target (validate_ref.target32; the fp64 recipe of validate_line_ref)
    corner    how many elements lie in the wing term's ill-conditioned corner (0 < delta < 2^-14, t > 0.25), `wing_zero` how many
              have delta exactly 0
Keypoint combinations: small and ragged with every mask x every validate_ref.WEIGHTS; train with mask zeros x all.
Line combinations: small, wide, mid x validate_line_ref.WEIGHTS.
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

import loss_grad_ref as lg  # noqa: E402
import validate_line_ref as vl  # noqa: E402
import validate_ref as vr  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def store(out, key, ref, g64, g64_helper, seed, extra):
    gmax = float(np.abs(g64).max())
    top = lg.top_positions(ref)
    flat = ref.reshape(-1)
    out[key + '.samples'] = flat[lg.seeded_positions(seed, flat.size)].astype(np.float32)
    out[key + '.top_idx'] = top
    out[key + '.top'] = flat[top].astype(np.float32)
    out[key + '.gmax'] = np.array(gmax)
    out[key + '.E_ref'] = np.array(float(np.abs(ref.astype(np.float64) - g64).max()) / gmax)
    out[key + '.E_tgt'] = np.array(float(np.abs(g64 - g64_helper).max()) / gmax)
    for k, v in extra.items():
        out[f'{key}.{k}'] = np.array(v)
    print(f"{key:34s} gmax {gmax:.6g}  E_ref {float(out[key + '.E_ref']):.3g}  E_tgt {float(out[key + '.E_tgt']):.3g}  {extra}")


def gen_keypoint(out):
    from src.models.hrnet.loss import HRNetLoss
    g = np.load(os.path.join(GOLD, 'validate.npz'))
    cases = vr.loss_cases(g)
    combos = lg.kp_combinations(cases)
    out['kp.combinations'] = np.array(['.'.join(c) for c in combos])
    for name, c in cases.items():
        B, C, h, w = c['shape']
        N, stride = C - 1, c['stride']
        pred = vr.make_pred(c['seed'], c['shape'], c['kp'], stride)
        ref_loss = HRNetLoss(num_refinement_stages=0, sigma=c['sigma'], stride=stride, pred_size=(h, w), num_keypoints=N)
        k2 = torch.from_numpy(c['kp']).clone().reshape(-1, N, 3)
        k2[:, :, :2] /= stride
        target = ref_loss.create_target(k2).numpy()                                   # the reference's own fp32 target
        helper = vr.target32(c['kp'], stride, c['sigma'], (h, w))
        tk = torch.from_numpy(c['kp'].reshape(B, -1))
        for cname, mname, wname in combos:
            if cname != name:
                continue
            m, wts = c['masks'][mname], vr.WEIGHTS[wname]
            ref_loss.l2_w, ref_loss.kldiv_w, ref_loss.awing_w = wts
            tp = torch.from_numpy(pred).clone().requires_grad_()
            ref_loss([tp], tk, None if m is None else torch.from_numpy(m)).backward()
            ref = tp.grad.numpy()
            assert ref.dtype == np.float32 and np.isfinite(ref).all()
            coef, terms = lg.kp_coef(wts, c['shape']), lg.KP_TERMS[wname]
            extra = {}
            if terms & 4:
                extra = {'corner': int(lg.kp_corner(pred, helper, m).sum()), 'wing_zero': int(lg.kp_wing_zero(pred, helper, m).sum())}
            store(out, f'kp.{name}.{mname}.{wname}', ref, lg.kp_grad64(pred, target, m, coef, terms),
                  lg.kp_grad64(pred, helper, m, coef, terms), c['seed'], extra)


def gen_line(out):
    from src.models.line.loss import EHMLoss
    g = np.load(os.path.join(GOLD, 'validate_line.npz'))
    for name, c in vl.cases(g).items():
        hw = c['shape'][2:]
        pred = vl.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        maps = c['maps'] if c['maps'] is not None else vl.keypoint_maps(c['kp'], c['sigma'], c['stride'], hw, as_dataset=True)
        exact = vl.keypoint_maps(c['kp'], c['sigma'], c['stride'], hw)
        for wname, wts in vl.WEIGHTS.items():
            ref_loss = EHMLoss(num_refinement_stages=0, gmse_w=wts[0], awing_w=wts[1], sigma=c['gmse_sigma'])
            tp = torch.from_numpy(pred).clone().requires_grad_()
            ref_loss([tp], torch.from_numpy(maps)).backward()
            ref = tp.grad.numpy()
            assert ref.dtype == np.float32 and np.isfinite(ref).all()
            coef, terms = lg.line_coef(wts, c['shape']), lg.LINE_TERMS[wname]
            extra = {}
            if terms & 2:
                extra = {'corner': int(lg.line_corner(pred, maps).sum()), 'wing_zero': int((pred.astype(np.float64) == maps.astype(np.float64)).sum())}
            store(out, f'line.{name}.{wname}', ref, lg.line_grad64(pred, maps, c['gmse_sigma'], coef, terms),
                  lg.line_grad64(pred, exact, c['gmse_sigma'], coef, terms), c['seed'], extra)


def main():
    out = {}
    gen_keypoint(out)
    gen_line(out)
    path = os.path.join(GOLD, 'loss_grad.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
