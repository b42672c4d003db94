"""GPU: csrc/line_loss.hip -- sncal_line_target, sncal_line_loss (both forms) and sncal_line_acc_counts -- against the reference
capture (tests/golden/validate_line.npz) and its fp64 restatement (tests/validate_line_ref.py).

Tolerances (set by the issue, not tuned):
  target  |got - ref| <= 2^-22 * ref + 2^-126 per element against the fp64 recipe: two factor roundings, one product, one sum,
          plus the smallest normal for flushed denormals;
  loss    the kernel and the reference are both fp32 evaluations of one formula with different summation orders, so the kernel's
          relative distance from the fp64 evaluation (on the reference's own fp32 maps) may be at most 4 * max(d_ref, 2^-23) per
          case and weight set, d_ref being the reference's own distance stored in the fixture; against the captured fp32 value the
          triangle inequality adds d_ref + 2^-24;
  counts  integers: exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

import validate_line_ref as vr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'validate_line.npz'))


@pytest.fixture(scope='module')
def big():
    """One frame at the line head's real size, (1,23,135,240): no capture exists for it, d_ref counts as 0."""
    rng = np.random.Generator(np.random.PCG64(7))
    shape, stride = (1, 23, 135, 240), 4
    kp = np.zeros((1, 23, 2, 3), dtype=np.float32)
    kp[..., :2] = -1
    for c in range(23):
        if c % 4 != 3:
            kp[0, c] = [(rng.uniform(-8, 968), rng.uniform(-8, 548), 1), (rng.uniform(-8, 968), rng.uniform(-8, 548), 1)]
    kp[0, 0, 1, 2] = 0
    maps = vr.keypoint_maps(kp, 1.0, stride, shape[2:], as_dataset=True)
    return dict(shape=shape, stride=stride, sigma=1.0, gmse_sigma=4.0, seed=31, kp=kp, maps=maps)


def _all_cases(gold, big):
    out = dict(vr.cases(gold))
    out['big'] = big
    return out


def test_target_matches_the_fp64_recipe(sncal, cuda, gold):
    worst = 0.0
    for name, c in vr.cases(gold).items():
        hw = c['shape'][2:]
        ref = vr.keypoint_maps(c['kp'], c['sigma'], c['stride'], hw)
        d_kp = torch.from_numpy(c['kp']).to(cuda)
        got = sncal.loss.create_keypoint_maps(d_kp, c['sigma'], c['stride'], hw)
        assert got.shape == c['shape'] and got.dtype == torch.float32 and got.is_cuda
        assert torch.equal(got, sncal.loss.create_keypoint_maps(d_kp.reshape(c['shape'][0], -1), c['sigma'], c['stride'], hw))    # (B, C*6)
        got = got.cpu().numpy().astype(np.float64)
        bound = 2.0 ** -22 * ref + 2.0 ** -126
        ratio = float((np.abs(got - ref) / bound).max())
        print(f'{name}: largest |got - ref| / bound = {ratio:.3g}; largest value {got.max():.7g}')
        worst = max(worst, ratio)
        assert np.all(np.abs(got - ref) <= bound), name
        assert not got[c['kp'][..., 2].sum(axis=2) == 0].any()                      # channels without a drawn point are exactly 0
    print('target: largest distance / bound:', worst)


def _rebuild(sncal, cuda, c, pred, terms=3):
    return sncal.loss.line_loss_sums(pred, keypoints=torch.from_numpy(c['kp']).to(cuda), target_sigma=c['sigma'], stride=c['stride'],
                                     gmse_sigma=c['gmse_sigma'], terms=terms)


def _check_against_fp64(name, c, gold, got_by_weights, exact):
    worst = 0.0
    for wname, wts in vr.WEIGHTS.items():
        key = f'case.{name}.{wname}'
        d_ref = float(gold[key + '.d_ref']) if name != 'big' else 0.0
        bound = 4.0 * max(d_ref, vr.EPS32)
        v, v64 = vr.combine(got_by_weights[wname], wts, c['shape']), vr.combine(exact, wts, c['shape'])
        dist = abs(v - v64) / abs(v64)
        line = f'{key:22s} kernel {v:.12g} fp64 {v64:.12g} dist {dist:.3g} (bound {bound:.3g})'
        if name != 'big':
            ref = float(gold[key + '.ref'])
            assert abs(v64 - float(gold[key + '.v64'])) <= 1e-12 * abs(v64), key
            dist_ref = abs(v - ref) / abs(ref)
            line += f'  ref {ref:.9g} vs capture {dist_ref:.3g}'
        print(line)
        worst = max(worst, dist / bound)
        assert dist <= bound, (key, dist, bound)
        if name != 'big':
            assert dist_ref <= bound + d_ref + 2.0 ** -24, (key, dist_ref)
    return worst


def test_loss_matches_capture_and_fp64(sncal, cuda, gold, big):
    worst = 0.0
    for name, c in _all_cases(gold, big).items():
        pred = vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        maps = c['maps'] if c['maps'] is not None else vr.keypoint_maps(c['kp'], c['sigma'], c['stride'], c['shape'][2:], as_dataset=True)
        exact = vr.loss_terms64(pred, maps, c['gmse_sigma'])                        # fp64 on the reference's own fp32 maps
        d_pred, d_maps = torch.from_numpy(pred).to(cuda), torch.from_numpy(maps).to(cuda)
        for form in ('rebuild', 'maps'):
            got = {}
            for wname in vr.WEIGHTS:
                if form == 'rebuild':
                    got[wname] = _rebuild(sncal, cuda, c, d_pred, vr.TERMS[wname]).cpu().numpy()
                else:
                    got[wname] = sncal.loss.line_loss_sums(d_pred, target=d_maps, gmse_sigma=c['gmse_sigma'], terms=vr.TERMS[wname]).cpu().numpy()
                for k in range(2):
                    if not (vr.TERMS[wname] >> k) & 1:
                        assert not got[wname][:, k].any()                           # a cleared bit: exact zeros, the term is not computed
            print(f'--- {name}, {form} form')
            worst = max(worst, _check_against_fp64(name, c, gold, got, exact))
    print('loss: largest distance / bound:', worst)


def test_the_two_forms_give_the_same_bits_and_so_do_two_runs(sncal, cuda, gold, big):
    for name, c in _all_cases(gold, big).items():
        pred = torch.from_numpy(vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])).to(cuda)
        own = sncal.loss.create_keypoint_maps(torch.from_numpy(c['kp']).to(cuda), c['sigma'], c['stride'], c['shape'][2:])
        for terms in (1, 2, 3):
            a = _rebuild(sncal, cuda, c, pred, terms)
            b = sncal.loss.line_loss_sums(pred, target=own, gmse_sigma=c['gmse_sigma'], terms=terms)
            assert a.shape == (c['shape'][0], 2) and a.dtype == torch.float64
            assert torch.equal(a, b), (name, terms)                                 # per frame and per term
            assert torch.equal(a, _rebuild(sncal, cuda, c, pred, terms)), (name, terms)
            assert torch.equal(b, sncal.loss.line_loss_sums(pred, target=own, gmse_sigma=c['gmse_sigma'], terms=terms)), (name, terms)
        assert not _rebuild(sncal, cuda, c, pred, 0).any()


def test_scalar_path_on_an_unaligned_base_and_an_odd_width(sncal, cuda, gold):
    """'small' has w = 24 (16-byte path when aligned): moved one float off alignment it takes the scalar path.  'wide' has w = 61:
    scalar path whatever the pointer.  Both must meet the bound of the aligned run."""
    for name in ('small', 'wide'):
        c = vr.cases(gold)[name]
        pred = vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        maps = c['maps']
        exact = vr.loss_terms64(pred, maps, c['gmse_sigma'])
        flat_p = torch.empty(pred.size + 4, dtype=torch.float32, device=cuda)
        flat_t = torch.empty(pred.size + 4, dtype=torch.float32, device=cuda)
        for off_p, off_t in ((1, 0), (0, 1), (1, 1)):
            d_pred = flat_p[off_p:off_p + pred.size].view(c['shape'])
            d_maps = flat_t[off_t:off_t + pred.size].view(c['shape'])
            d_pred.copy_(torch.from_numpy(pred))
            d_maps.copy_(torch.from_numpy(maps))
            assert d_pred.data_ptr() % 16 == 4 * off_p and d_maps.data_ptr() % 16 == 4 * off_t
            forms = {'maps': {w: sncal.loss.line_loss_sums(d_pred, target=d_maps, gmse_sigma=c['gmse_sigma'], terms=vr.TERMS[w]).cpu().numpy()
                              for w in vr.WEIGHTS}}
            if off_p:
                forms['rebuild'] = {w: _rebuild(sncal, cuda, c, d_pred, vr.TERMS[w]).cpu().numpy() for w in vr.WEIGHTS}
            for form, got in forms.items():
                print(f'--- {name}, {form} form, pred + {off_p} floats, maps + {off_t} floats')
                _check_against_fp64(name, c, gold, got, exact)


@pytest.mark.parametrize('B,C,h,w', [(2, 1, 1, 1), (1, 2, 5, 6), (1, 2, 17, 8), (1, 64, 9, 66), (1, 64, 9, 68)])
def test_sums_on_more_shapes(sncal, cuda, B, C, h, w):
    """What the capture's cases leave out of the sums kernel: one channel on a 1 x 1 map, maps smaller than a tile on a width that
    cannot take the 16-byte path and on one that does (waves without rows, lanes past the width), and 64 channels -- all that the
    row tables in LDS hold -- on both kinds of width.  Both forms, each term alone and both: per frame and per term against the fp64
    evaluation on the device's own maps, and the two forms with the same bits.
    Bound: the floor of the bound above, 4 * 2^-23, for every shape (no capture exists, d_ref counts as 0, as for `big`), as the
    keypoint loss's test of more shapes holds its own 1 x 1 case."""
    rng = np.random.default_rng(60 + C + w)
    stride, t_sigma, g_sigma = 4.0, 1.5, 4.0
    kp = np.zeros((B, C, 2, 3), dtype=np.float32)
    kp[..., :2] = -1
    for b in range(B):
        for ch in range(C):
            if ch % 3 != 2:
                kp[b, ch] = [(rng.uniform(-4, w * stride + 4), rng.uniform(-4, h * stride + 4), 1), (rng.uniform(0, w * stride), rng.uniform(0, h * stride), ch % 5 != 0)]
    d_kp = torch.from_numpy(kp).to(cuda)
    own = sncal.loss.create_keypoint_maps(d_kp, t_sigma, stride, (h, w))
    p_np = rng.uniform(0, 1, (B, C, h, w)).astype(np.float32) ** 4 + np.float32(2.0 ** -10)
    pred = torch.from_numpy(p_np).to(cuda)
    exact = vr.loss_terms64(p_np, own.cpu().numpy(), g_sigma)
    bound = 4 * vr.EPS32
    for terms in (1, 2, 3):
        a = sncal.loss.line_loss_sums(pred, keypoints=d_kp, target_sigma=t_sigma, stride=stride, gmse_sigma=g_sigma, terms=terms)
        b = sncal.loss.line_loss_sums(pred, target=own, gmse_sigma=g_sigma, terms=terms)
        assert torch.equal(a, b), terms
        got = a.cpu().numpy()
        for k in range(2):
            if (terms >> k) & 1:
                rel = np.abs(got[:, k] - exact[:, k]) / np.abs(exact[:, k])
                print((B, C, h, w), 'terms', terms, 'term', k, 'largest relative distance', rel.max(), 'bound', bound)
                assert (rel <= bound).all(), ((B, C, h, w), terms, k, rel)
            else:
                assert not got[:, k].any()


def test_short_workspace_and_bad_arguments(sncal, cuda):
    E = sncal._lib.SncalError
    L = sncal._lib.lib()
    pred = torch.full((1, 5, 8, 8), 0.2, device=cuda)
    maps = torch.zeros((1, 5, 8, 8), device=cuda)
    kp = torch.zeros((1, 5, 2, 3), device=cuda)
    n = ctypes.c_size_t()
    assert L.sncal_line_loss_workspace(1, 5, 8, 8, ctypes.byref(n)) == 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=cuda)
    out = torch.zeros((1, 2), dtype=torch.float64, device=cuda)
    for target, kpts in ((maps.data_ptr(), None), (None, kp.data_ptr())):
        args = (pred.data_ptr(), target, kpts, 1, 5, 8, 8, 1.0, 4.0, 4.0, 3, out.data_ptr(), ws.data_ptr())
        assert L.sncal_line_loss(*args, n.value - 1, None) == -4                    # SNCAL_ERR_WORKSPACE
        assert b'workspace' in L.sncal_last_error()
        assert L.sncal_line_loss(*args, n.value, None) == 0
        torch.cuda.synchronize()
        assert out[0, 0] > 0 and out[0, 1] > 0
    with pytest.raises(E, match='exactly one'):
        sncal.loss.line_loss_sums(pred, target=maps, keypoints=kp)
    with pytest.raises(E, match='exactly one'):
        sncal.loss.line_loss_sums(pred)
    with pytest.raises(E, match='shape of pred'):
        sncal.loss.line_loss_sums(pred, target=maps[:, :4].contiguous())
    with pytest.raises(E, match='keypoints'):
        sncal.loss.line_loss_sums(pred, keypoints=kp[:, :4].contiguous())
    with pytest.raises(E, match='float32'):
        sncal.loss.line_loss_sums(pred.double(), target=maps)
    with pytest.raises(E, match='C=65'):
        sncal.loss.line_loss_sums(torch.zeros((1, 65, 8, 8), device=cuda), target=torch.zeros((1, 65, 8, 8), device=cuda))
    with pytest.raises(E, match='sigma'):
        sncal.loss.create_keypoint_maps(kp, 0.0, 4.0, (8, 8))
    with pytest.raises(E, match='GPU'):
        sncal.loss.create_keypoint_maps(kp.cpu(), 1.0, 4.0, (8, 8))
    with pytest.raises(E, match='C\\*6'):
        sncal.loss.create_keypoint_maps(torch.zeros((1, 7), device=cuda), 1.0, 4.0, (8, 8))
    assert sncal.loss.create_keypoint_maps(torch.zeros((0, 5, 2, 3), device=cuda), 1.0, 4.0, (8, 8)).shape == (0, 5, 8, 8)


def test_ehmloss_surface(sncal, cuda, gold):
    c = vr.cases(gold)['small']
    pred = torch.from_numpy(vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])).to(cuda)
    maps, kp = torch.from_numpy(c['maps']), torch.from_numpy(c['kp'])
    B = c['shape'][0]
    for wname, wts in vr.WEIGHTS.items():
        loss = sncal.EHMLoss(num_refinement_stages=0, gmse_w=wts[0], awing_w=wts[1], sigma=c['gmse_sigma'], target_sigma=c['sigma'],
                             stride=c['stride'])
        v = loss([pred], maps)                                                      # maps on the host, as a loader yields them
        assert v.is_cuda and v.dim() == 0 and v.dtype == torch.float32
        assert torch.equal(v, loss.forward(pred, maps.to(cuda)))                    # a bare tensor is taken as the list's entry
        key = f'case.small.{wname}'
        d_ref, ref = float(gold[key + '.d_ref']), float(gold[key + '.ref'])
        assert abs(float(v) - ref) <= (4 * max(d_ref, vr.EPS32) + d_ref + 2.0 ** -23) * abs(ref), key
        by_kp = loss([pred], kp.reshape(B, -1))                                     # (B, C*6): the rebuild form
        assert torch.equal(by_kp, loss([pred], kp.to(cuda))) and torch.equal(by_kp, loss([pred], loss.create_keypoint_maps(kp.to(cuda), c['shape'][2:])))
        assert abs(float(by_kp) - ref) <= (4 * max(d_ref, vr.EPS32) + d_ref + 2.0 ** -23) * abs(ref), key
        s = loss.components([pred], kp)
        assert s.shape == (B, 2) and s.dtype == torch.float64
        assert abs(vr.combine(s.cpu().numpy(), wts, c['shape']) - float(by_kp)) <= 2.0 ** -23 * abs(float(by_kp))
    none = sncal.EHMLoss(gmse_w=0.0, awing_w=0.0)
    assert float(none([pred], maps)) == 0.0                                         # no term at all: the reference returns 0
    empty = sncal.EHMLoss()([torch.zeros((0, 23, 16, 24), device=cuda)], torch.zeros((0, 138)))
    assert empty.dim() == 0 and torch.isnan(empty)


def test_acc_counts_equal_the_restatement(sncal, cuda, gold):
    thr = float(gold['acc.conf_threshold'])
    batches = vr.acc_batches(gold)
    rng = np.random.Generator(np.random.PCG64(5))
    gt = np.zeros((5, 23, 2, 3), dtype=np.float32)                                  # integer coordinates: d^2 is exact, no tie is in doubt
    gt[..., :2] = rng.integers(0, 40, (5, 23, 2, 2))
    gt[..., 2] = rng.uniform(size=(5, 23, 2)) < 0.7                                 # flags per point, not per line
    pred = np.zeros_like(gt)
    pred[..., :2] = gt[..., ::-1, :2] + rng.integers(-12, 13, (5, 23, 2, 2))
    pred[..., 2] = rng.choice([0.0, 0.1, 0.2, 0.5, 0.9], size=(5, 23, 2)).astype(np.float32)
    for i, (g, p) in enumerate(batches + [(gt, pred)]):
        got = sncal.metrics.line_acc_counts(torch.from_numpy(g).to(cuda), torch.from_numpy(p).to(cuda), thr, (5.0, 10.0, 20.0))
        assert got.shape == (3, 3) and got.dtype == torch.int64 and got.is_cuda
        want = vr.acc_counts(g, p, thr)
        assert np.array_equal(got.cpu().numpy(), want), (i, got, want)
        if i < len(batches):
            assert np.array_equal(want, gold['acc.counts'][i])
    ts8 = (1.0, 2.0, 3.0, 5.0, 8.0, 13.0, 21.0, 34.0)
    got = sncal.metrics.line_acc_counts(torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda), 0.2, ts8).cpu().numpy()
    assert np.array_equal(got, vr.acc_counts(gt, pred, 0.2, ts8))
    with pytest.raises(sncal._lib.SncalError, match='n_t'):
        sncal.metrics.line_acc_counts(torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda), 0.2, ts8 + (55.0,))


def test_accmetric_matches_the_capture(sncal, cuda, gold):
    m = sncal.AccMetric(num_keypoints=23, conf_threshold=float(gold['acc.conf_threshold']))
    for g, p in vr.acc_batches(gold):
        m.update({'prediction': torch.from_numpy(p).to(cuda), 'keypoints': torch.from_numpy(g.reshape(len(g), -1))})   # (B,138) on the host
    assert all(c.is_cuda for c in m._counts)                                        # counts stay on the device until compute()
    assert abs(m.compute() - float(gold['acc.value'])) <= 1e-12
    state = type('S', (), {'phase': 'val', 'metrics': {}})()
    m.epoch_complete(state)
    assert state.metrics == {'val_acc': m.compute()}
    d = m.compute_detail()
    tot = gold['acc.counts'].sum(axis=0)
    a = tot[:, 0] / tot.sum(axis=1)
    assert [d['a@5'], d['a@10'], d['a@20']] == a.tolist() and abs(d['weighted'] - (0.5 * a[0] + 0.35 * a[1] + 0.15 * a[2])) <= 1e-15
    m.reset()
    empty = np.zeros((2, 23, 2, 3), dtype=np.float32)
    m.update({'prediction': torch.from_numpy(empty).to(cuda), 'keypoints': torch.from_numpy(empty)})
    with pytest.raises(ZeroDivisionError):
        m.compute()
