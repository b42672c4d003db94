"""CPU: tests/loss_grad_ref.py (closed-form fp64 gradients of HRNetLoss and EHMLoss) against the reference's autograd gradients
captured in tests/golden/loss_grad.npz (tools/make_golden_loss_grad.py), and the fixture's own invariants.

Bound per combination (set by the issue): |g64 - g_ref32| <= (E_ref + E_tgt + 2^-23) * max|g64| at every stored position, where
E_ref is the reference's own distance from the fp64 evaluation on its own fp32 target, E_tgt the distance between the fp64
evaluations on the reference's target and on the helper's, and 2^-23 covers the rounding of the stored fp32 value."""
import os

import numpy as np
import pytest

import loss_grad_ref as lg
import validate_line_ref as vl
import validate_ref as vr


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'loss_grad.npz'))


@pytest.fixture(scope='module')
def kp_cases(gold_dir):
    return vr.loss_cases(np.load(os.path.join(gold_dir, 'validate.npz')))


@pytest.fixture(scope='module')
def line_cases(gold_dir):
    return vl.cases(np.load(os.path.join(gold_dir, 'validate_line.npz')))


def _check(gold, key, g64, seed):
    flat = g64.reshape(-1)
    gmax = float(np.abs(flat).max())
    bound = (float(gold[key + '.E_ref']) + float(gold[key + '.E_tgt']) + lg.EPS32) * gmax
    pos = lg.seeded_positions(seed, flat.size)
    d_s = float(np.abs(flat[pos] - gold[key + '.samples'].astype(np.float64)).max())
    d_t = float(np.abs(flat[gold[key + '.top_idx']] - gold[key + '.top'].astype(np.float64)).max())
    print(f'{key:34s} max|g64| {gmax:.6g}  samples {d_s / gmax:.3g}  top {d_t / gmax:.3g}  bound {bound / gmax:.3g}')
    assert abs(gmax - float(gold[key + '.gmax'])) <= (float(gold[key + '.E_tgt']) + 1e-12) * gmax, key
    assert d_s <= bound and d_t <= bound, (key, d_s / gmax, d_t / gmax, bound / gmax)


def test_keypoint_closed_form_matches_the_captured_autograd(gold, kp_cases):
    for name, c in kp_cases.items():
        pred = vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        target = vr.target32(c['kp'], c['stride'], c['sigma'], c['shape'][2:])
        for cname, mname, wname in lg.kp_combinations(kp_cases):
            if cname == name:
                g64 = lg.kp_grad64(pred, target, c['masks'][mname], lg.kp_coef(vr.WEIGHTS[wname], c['shape']), lg.KP_TERMS[wname])
                _check(gold, f'kp.{name}.{mname}.{wname}', g64, c['seed'])


def test_line_closed_form_matches_the_captured_autograd(gold, line_cases):
    for name, c in line_cases.items():
        pred = vl.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        exact = vl.keypoint_maps(c['kp'], c['sigma'], c['stride'], c['shape'][2:])          # the fp64 recipe: E_tgt covers the distance
        for wname, wts in vl.WEIGHTS.items():
            g64 = lg.line_grad64(pred, exact, c['gmse_sigma'], lg.line_coef(wts, c['shape']), lg.LINE_TERMS[wname])
            _check(gold, f'line.{name}.{wname}', g64, c['seed'])


def test_fixture_invariants(gold, kp_cases, line_cases):
    combos = ['kp.' + '.'.join(c) for c in lg.kp_combinations(kp_cases)]
    assert combos == ['kp.' + str(s) for s in gold['kp.combinations']]
    assert len(combos) == 2 * 2 * len(vr.WEIGHTS) + 1 and 'kp.train.zeros.all' in combos
    sizes = {'kp.' + '.'.join(c): int(np.prod(kp_cases[c[0]]['shape'])) for c in lg.kp_combinations(kp_cases)}
    for name, c in line_cases.items():
        for wname in vl.WEIGHTS:
            combos.append(f'line.{name}.{wname}')
            sizes[combos[-1]] = int(np.prod(c['shape']))
    assert sorted(line_cases) == ['mid', 'small', 'wide']
    for key in combos:
        s, top, idx = gold[key + '.samples'], gold[key + '.top'], gold[key + '.top_idx']
        assert s.shape == (lg.N_SEEDED,) and s.dtype == np.float32 and np.isfinite(s).all(), key
        assert top.shape == (lg.N_TOP,) and top.dtype == np.float32 and np.isfinite(top).all(), key
        assert idx.shape == (lg.N_TOP,) and len(set(idx.tolist())) == lg.N_TOP and idx.min() >= 0 and idx.max() < sizes[key], key
        assert np.all(np.diff(np.abs(top)) <= 0), key                                          # largest first
        assert np.abs(s).max() <= np.abs(top[0]), key                                          # no sample beats the largest of the top
        assert 0 <= float(gold[key + '.E_ref']) < 1e-5 and 0 <= float(gold[key + '.E_tgt']) < 1e-5 and float(gold[key + '.gmax']) > 0, key
        if key + '.corner' in gold.files:
            assert int(gold[key + '.corner']) <= 16, key                                       # the issue's cap on the ill-conditioned corner
    assert int(gold['kp.train.zeros.all.wing_zero']) >= 1 and int(gold['kp.small.none.awing.wing_zero']) >= 1
