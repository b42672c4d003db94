"""GPU: sncal_ehm_loss_grad (csrc/line_loss.hip), loss.line_loss_grad and the autograd path of EHMLoss against the reference's
autograd gradients (tests/golden/loss_grad.npz), the fp64 closed form (tests/loss_grad_ref.py) and torch autograd through the
composed path (sncal_line_target + torch ops) in fp64.

Tolerance (set by the issue, not tuned): max over elements of |g - g64| <= 4 * max(E_ref, 2^-23) * max|g64| per case and weight
set, g64 evaluated on the very target the kernel sees (the reference's fp32 maps for the maps form, sncal_line_target's output for
the rebuild form) and E_ref the reference's own distance stored in the fixture; against the captured fp32 samples (maps form, the
reference's maps) the triangle inequality adds E_ref.  Shapes without a capture take the floor.  Elements in the wing term's
ill-conditioned corner (0 < delta64 < 2^-14, t > 0.25; at most 16 per case, the fixture counts 0) are left out where the wing bit
is set; elements with delta64 exactly 0 stay in and must get exactly 0."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loss_grad_ref as lg
import validate_line_ref as vl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'loss_grad.npz'))


@pytest.fixture(scope='module')
def cases(gold_dir):
    out = vl.cases(np.load(os.path.join(gold_dir, 'validate_line.npz')))
    for c in out.values():
        c['pred'] = vl.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        if c['maps'] is None:
            c['maps'] = vl.keypoint_maps(c['kp'], c['sigma'], c['stride'], c['shape'][2:], as_dataset=True)     # the capture's maps, bit for bit
    return out


def _rebuild(sncal, cuda, c, pred, coef, terms, **kw):
    return sncal.loss.line_loss_grad(pred, keypoints=torch.from_numpy(c['kp']).to(cuda), target_sigma=c['sigma'], stride=c['stride'],
                                     gmse_sigma=c['gmse_sigma'], coef=coef, terms=terms, **kw)


def _dist(g, g64, pred, target, terms):
    err = np.abs(g.astype(np.float64) - g64)
    corner = lg.line_corner(pred, target) if terms & 2 else np.zeros(pred.shape, dtype=bool)
    assert int(corner.sum()) <= 16
    err[corner] = 0.0
    return err, corner


@pytest.mark.parametrize('name', ['small', 'wide', 'mid'])
def test_kernel_matches_fp64_and_capture(sncal, cuda, gold, cases, name):
    c = cases[name]
    pred, maps = c['pred'], c['maps']
    d_pred, d_maps = torch.from_numpy(pred).to(cuda), torch.from_numpy(maps).to(cuda)
    own = sncal.loss.create_keypoint_maps(torch.from_numpy(c['kp']).to(cuda), c['sigma'], c['stride'], c['shape'][2:])
    own_np = own.cpu().numpy()
    pos = lg.seeded_positions(c['seed'], pred.size)
    worst = 0.0
    for wname, wts in vl.WEIGHTS.items():
        key = f'line.{name}.{wname}'
        coef, terms = lg.line_coef(wts, c['shape']), lg.LINE_TERMS[wname]
        e_ref = float(gold[key + '.E_ref'])
        bound = 4.0 * max(e_ref, lg.EPS32)
        # the maps form on the reference's maps
        got = sncal.loss.line_loss_grad(d_pred, target=d_maps, gmse_sigma=c['gmse_sigma'], coef=coef, terms=terms)
        assert got.shape == d_pred.shape and got.dtype == torch.float32
        assert torch.equal(got, sncal.loss.line_loss_grad(d_pred, target=d_maps, gmse_sigma=c['gmse_sigma'], coef=coef, terms=terms)), key
        g = got.cpu().numpy()
        g64 = lg.line_grad64(pred, maps, c['gmse_sigma'], coef, terms)
        gmax = float(np.abs(g64).max())
        assert abs(gmax - float(gold[key + '.gmax'])) <= 1e-12 * gmax
        err, corner = _dist(g, g64, pred, maps, terms)
        if terms & 2:
            assert int(corner.sum()) == int(gold[key + '.corner'])
        gf, cf, top = g.reshape(-1).astype(np.float64), corner.reshape(-1), gold[key + '.top_idx']
        d_cap = float((np.abs(gf[pos] - gold[key + '.samples'].astype(np.float64)) * ~cf[pos]).max()) / gmax
        d_top = float((np.abs(gf[top] - gold[key + '.top'].astype(np.float64)) * ~cf[top]).max()) / gmax
        # the rebuild form on the target it rebuilds
        reb = _rebuild(sncal, cuda, c, d_pred, coef, terms)
        assert torch.equal(reb, _rebuild(sncal, cuda, c, d_pred, coef, terms)), key
        assert torch.equal(reb, sncal.loss.line_loss_grad(d_pred, target=own, gmse_sigma=c['gmse_sigma'], coef=coef, terms=terms)), key   # the two forms: the same bits
        g64_own = lg.line_grad64(pred, own_np, c['gmse_sigma'], coef, terms)
        err_own, _ = _dist(reb.cpu().numpy(), g64_own, pred, own_np, terms)
        dist, dist_own = float(err.max()) / gmax, float(err_own.max()) / float(np.abs(g64_own).max())
        print(f'{key:20s} max|g64| {gmax:.6g}  maps form {dist:.3g}  rebuild form {dist_own:.3g} (bound {bound:.3g})  vs samples {d_cap:.3g}  vs top {d_top:.3g}')
        worst = max(worst, dist / bound, dist_own / bound)
        assert dist <= bound and dist_own <= bound, (key, dist, dist_own, bound)
        assert d_cap <= bound + e_ref and d_top <= bound + e_ref, (key, d_cap, d_top)
        if terms & 2:                                                          # delta exactly 0: exactly 0 from the wing term
            zero = pred.astype(np.float64) == maps.astype(np.float64)
            assert int(zero.sum()) == int(gold[key + '.wing_zero'])
            w_only = sncal.loss.line_loss_grad(d_pred, target=d_maps, gmse_sigma=c['gmse_sigma'], coef=(0.0, 1.0), terms=2).cpu().numpy()
            assert np.isfinite(w_only).all() and not w_only[zero].any()
    # a cleared bit contributes nothing
    cf2 = lg.line_coef((1.0, 1.0), c['shape'])
    for bit in range(2):
        only = tuple(v if k == bit else 0.0 for k, v in enumerate(cf2))
        assert torch.equal(_rebuild(sncal, cuda, c, d_pred, cf2, 1 << bit), _rebuild(sncal, cuda, c, d_pred, only, 3)), bit
    assert not _rebuild(sncal, cuda, c, d_pred, cf2, 0).any()
    print('largest distance / bound:', worst)


def _raw_grad(sncal, pred, target, kp, c_sigma, stride, gmse_sigma, coef, terms, gout, grad, ws_bytes=None):
    L = sncal._lib.lib()
    B, C, h, w = pred.shape
    n = ctypes.c_size_t()
    assert L.sncal_line_loss_workspace(B, C, h, w, ctypes.byref(n)) == 0
    ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=pred.device)
    st = L.sncal_ehm_loss_grad(pred.data_ptr(), None if target is None else target.data_ptr(), None if kp is None else kp.data_ptr(), B, C, h, w,
                                c_sigma, stride, gmse_sigma, terms, (ctypes.c_double * 2)(*coef), None if gout is None else gout.data_ptr(),
                                grad.data_ptr(), ws.data_ptr(), n.value if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return st


SHAPES = [(1, 1, 1, 1, 0), (2, 23, 16, 24, 0), (1, 5, 33, 61, 0), (1, 64, 9, 66, 1), (1, 64, 9, 68, 1)]


@pytest.mark.parametrize('B,C,h,w,off', SHAPES)
def test_more_shapes_against_the_closed_form(sncal, cuda, B, C, h, w, off):
    """One element, the line head's channel count, odd sizes, 64 channels on a width that is no multiple of 4, and on one that is
    with every base one float off alignment (all, and each alone).  Softmax-like predictions with exact zeros (target 0 there gives
    gradient 0) and exact hits of the target.  Both forms, each term alone and both, at the floor bound."""
    rng = np.random.default_rng(40 + C + w)
    stride, t_sigma, g_sigma = 4.0, 1.5, 0.8
    kp = np.zeros((B, C, 2, 3), dtype=np.float32)
    kp[..., :2] = -1
    for b in range(B):
        for ch in range(C):
            if ch % 3 != 2:
                kp[b, ch] = [(rng.uniform(-4, w * stride + 4), rng.uniform(-4, h * stride + 4), 1), (rng.uniform(0, w * stride), rng.uniform(0, h * stride), ch % 5 != 0)]
    d_kp = torch.from_numpy(kp).to(cuda)
    own = sncal.loss.create_keypoint_maps(d_kp, t_sigma, stride, (h, w))
    own_np = own.cpu().numpy()
    p_np = rng.uniform(0, 1, (B, C, h, w)).astype(np.float32) ** 4
    p_np[rng.uniform(size=p_np.shape) < 0.2] = 0.0                                    # exact zeros
    hit = rng.uniform(size=p_np.shape) < 0.05
    p_np[hit] = own_np[hit]                                                           # delta exactly 0
    numel = p_np.size
    bufs = [torch.full((numel + 8,), 7.0, dtype=torch.float32, device=cuda) for _ in range(3)]

    def view(i, o):
        return bufs[i][o:o + numel].view(B, C, h, w)
    offsets = [(off, off, off)] + ([(1, 0, 0), (0, 1, 0), (0, 0, 1)] if off else [])
    for terms, coef in ((3, lg.line_coef((0.5, 2.0), p_np.shape)), (1, (1.0, 0.0)), (2, (0.0, 1.0))):
        g64 = lg.line_grad64(p_np, own_np, g_sigma, coef, terms)
        gmax = float(np.abs(g64).max())
        zero_t = (p_np == 0) & (own_np == 0)
        assert not g64[zero_t].any()
        results = []
        for o_p, o_t, o_g in offsets:
            pred, tgt = view(0, o_p), view(1, o_t)
            pred.copy_(torch.from_numpy(p_np))
            tgt.copy_(own)
            for form in ('maps', 'rebuild'):
                bufs[2].fill_(7.0)
                grad = view(2, o_g)
                st = _raw_grad(sncal, pred, tgt if form == 'maps' else None, None if form == 'maps' else d_kp, t_sigma, stride, g_sigma, coef, terms, None, grad)
                assert st == 0
                assert (bufs[2][:o_g] == 7.0).all() and (bufs[2][o_g + numel:] == 7.0).all()             # nothing written outside the gradient
                g = grad.cpu().numpy()
                err, corner = _dist(g, g64, p_np, own_np, terms)
                print((B, C, h, w), (o_p, o_t, o_g), form, terms, 'max|g64|', gmax, 'dist', float(err.max()) / gmax if gmax > 0 else 0.0, 'corner', int(corner.sum()))
                assert err.max() <= 4 * lg.EPS32 * gmax, ((B, C, h, w), form, terms)
                assert not g[zero_t].any()                                            # prediction 0 against target 0: gradient 0
                if terms & 2:
                    assert not sncal.loss.line_loss_grad(pred.clone(), target=own, gmse_sigma=g_sigma, coef=(0.0, 1.0), terms=2).cpu().numpy()[hit].any()
                results.append(grad.clone())
        assert all(torch.equal(results[0], r) for r in results[1:])                   # forms and alignments: the same bits
    coef = lg.line_coef((1.0, 1.0), p_np.shape)
    pred = torch.from_numpy(p_np).to(cuda)
    one = _rebuild_plain(sncal, pred, d_kp, t_sigma, stride, g_sigma, coef, None)
    k = _rebuild_plain(sncal, pred, d_kp, t_sigma, stride, g_sigma, coef, torch.tensor([1024.0], device=cuda))
    assert torch.equal(k, one * 1024.0)


def _rebuild_plain(sncal, pred, d_kp, t_sigma, stride, g_sigma, coef, gout):
    return sncal.loss.line_loss_grad(pred, keypoints=d_kp, target_sigma=t_sigma, stride=stride, gmse_sigma=g_sigma, coef=coef, terms=3, grad_output=gout)


def test_autograd_surface(sncal, cuda, cases):
    c = cases['small']
    B = c['shape'][0]
    pred = torch.from_numpy(c['pred']).to(cuda)
    maps, kp = torch.from_numpy(c['maps']), torch.from_numpy(c['kp'])
    for wname, wts in vl.WEIGHTS.items():
        loss = sncal.EHMLoss(num_refinement_stages=0, gmse_w=wts[0], awing_w=wts[1], sigma=c['gmse_sigma'], target_sigma=c['sigma'], stride=c['stride'])
        coef = lg.line_coef(wts, c['shape'])
        for target, where in ((maps, dict(target=maps.to(cuda))), (kp.reshape(B, -1), dict(keypoints=kp.to(cuda), target_sigma=c['sigma'], stride=c['stride']))):
            plain = loss([pred], target)                                        # maps / endpoints on the host, as a loader yields them
            assert plain.grad_fn is None and not plain.requires_grad
            p = pred.clone().requires_grad_()
            v = loss([p], target)
            assert v.grad_fn is not None and v.dtype == torch.float32 and v.dim() == 0 and torch.equal(v.detach(), plain)
            v.backward()
            want = sncal.loss.line_loss_grad(pred, gmse_sigma=c['gmse_sigma'], coef=coef, terms=loss.terms, **where)
            assert p.grad.shape == pred.shape and p.grad.device == pred.device and torch.equal(p.grad, want) and want.abs().max() > 0
            loss([p], target).backward()                                        # accumulates into the existing .grad
            assert torch.equal(p.grad, want + want)
            q = pred.clone().requires_grad_()
            (loss(q, target) * 1024).backward()
            assert torch.equal(q.grad, want * 1024.0)
            with torch.no_grad():
                quiet = loss([p], target)
            assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, plain)
    loss = sncal.EHMLoss(sigma=c['gmse_sigma'], target_sigma=c['sigma'], stride=c['stride'])
    want = sncal.loss.line_loss_grad(pred, target=maps.to(cuda), gmse_sigma=c['gmse_sigma'], coef=lg.line_coef((1.0, 1.0), c['shape']), terms=3)
    nc = pred.to(memory_format=torch.channels_last).requires_grad_()           # made contiguous inside
    assert not nc.is_contiguous()
    loss([nc], maps).backward()
    assert nc.grad.shape == pred.shape and torch.equal(nc.grad, want)
    p = pred.clone().requires_grad_()
    v = loss([p], maps)
    g, = torch.autograd.grad(v * v, p, create_graph=True)                    # an upstream gradient that is itself on the tape
    assert torch.equal(g.detach(), want * (v.detach() * 2))
    with pytest.raises(RuntimeError, match='once_differentiable'):
        g.sum().backward()
    g, = torch.autograd.grad(loss([p], maps), p, create_graph=True)  # a constant upstream gradient: no second-order graph at all
    assert torch.equal(g, want) and not g.requires_grad
    with pytest.raises(RuntimeError):
        g.sum().backward()
    assert loss.components([pred.clone().requires_grad_()], maps).grad_fn is None
    with pytest.raises(sncal._lib.SncalError, match='num_refinement_stages'):
        sncal.EHMLoss(num_refinement_stages=1)
    e = torch.zeros((0, 23, 16, 24), device=cuda, requires_grad=True)
    v = loss([e], torch.zeros((0, 138)))
    assert torch.isnan(v)
    v.backward()
    assert e.grad.shape == e.shape


def test_short_workspace_and_bad_arguments(sncal, cuda):
    E = sncal._lib.SncalError
    G = sncal.loss.line_loss_grad
    pred = torch.full((1, 5, 8, 8), 0.2, device=cuda)
    maps = torch.zeros((1, 5, 8, 8), device=cuda)
    kp = torch.zeros((1, 5, 2, 3), device=cuda)
    grad = torch.zeros_like(pred)
    cf = (1.0, 1.0)
    assert _raw_grad(sncal, pred, None, kp, 1.0, 4.0, 4.0, cf, 3, None, grad, ws_bytes=64) == -4         # SNCAL_ERR_WORKSPACE: the tables do not fit
    assert b'workspace' in sncal._lib.lib().sncal_last_error()
    assert _raw_grad(sncal, pred, None, kp, 1.0, 4.0, 4.0, cf, 3, None, grad) == 0 and grad.abs().max() > 0
    assert _raw_grad(sncal, pred, maps, None, 1.0, 4.0, 4.0, cf, 3, None, grad.zero_()) == 0 and grad.abs().max() > 0
    assert _raw_grad(sncal, pred, maps, kp, 1.0, 4.0, 4.0, cf, 3, None, grad) == -1                      # both given
    with pytest.raises(E, match='exactly one'):
        G(pred, target=maps, keypoints=kp, coef=cf)
    with pytest.raises(E, match='exactly one'):
        G(pred, coef=cf)
    with pytest.raises(E, match='shape of pred'):
        G(pred, target=maps[:, :4].contiguous(), coef=cf)
    with pytest.raises(E, match='keypoints'):
        G(pred, keypoints=kp[:, :4].contiguous(), coef=cf)
    with pytest.raises(E, match='float32'):
        G(pred.double(), target=maps, coef=cf)
    with pytest.raises(E, match='C=65'):
        G(torch.zeros((1, 65, 8, 8), device=cuda), target=torch.zeros((1, 65, 8, 8), device=cuda), coef=cf)
    with pytest.raises(E, match='gmse_sigma'):
        G(pred, target=maps, gmse_sigma=0.0, coef=cf)
    with pytest.raises(E, match='coef'):
        G(pred, target=maps, coef=(1.0, 1.0, 1.0))
    with pytest.raises(E, match='grad_output'):
        G(pred, target=maps, coef=cf, grad_output=torch.ones(2, device=cuda))


def test_matches_torch_autograd_through_the_composed_path_in_fp64(sncal, cuda, cases):
    c = cases['mid']
    pred = torch.from_numpy(c['pred']).to(cuda)
    d_kp = torch.from_numpy(c['kp']).to(cuda)
    loss = sncal.EHMLoss(gmse_w=0.5, awing_w=2.0, sigma=c['gmse_sigma'], target_sigma=c['sigma'], stride=c['stride'])
    p = pred.clone().requires_grad_()
    loss([p], d_kp).backward()
    t32 = sncal.loss.create_keypoint_maps(d_kp, c['sigma'], c['stride'], c['shape'][2:])
    t = t32.double()
    x = pred.double().requires_grad_()
    sq = (x - t) ** 2
    gm = (sq * torch.exp(-sq / (2 * c['gmse_sigma'] ** 2))).mean()
    half = torch.tensor(0.5, dtype=torch.float64, device=cuda)
    delta, a = (t - x).abs(), vl.ALPHA - t
    A = vl.OMEGA * (1 / (1 + torch.pow(half, a))) * a * torch.pow(half, a - 1)
    Cc = vl.THETA * A - vl.OMEGA * torch.log(1 + torch.pow(half, a))
    aw = torch.where(delta < vl.THETA, vl.OMEGA * torch.log(1 + torch.pow(delta, a)), A * delta - Cc).mean()
    (0.5 * gm + 2.0 * aw).backward()
    g64 = x.grad
    corner = torch.from_numpy(lg.line_corner(c['pred'], t32.cpu().numpy())).to(cuda)
    assert int(corner.sum()) <= 16
    # torch differentiates |.| and pow at delta == 0 to nan where a < 1 (0 * inf); the kernel's sign(0) = 0 rule gives 0 there
    zero = delta.detach() == 0
    assert not p.grad[zero].any()                                              # the GMSE term is 0 there too
    err = (p.grad.double() - g64).abs().masked_fill(corner | (zero & ~torch.isfinite(g64)), 0.0)
    gmax = float(g64[torch.isfinite(g64)].abs().max())
    print('max|g64|', gmax, 'dist', float(err.max()) / gmax, 'corner', int(corner.sum()), 'delta 0:', int(zero.sum()))
    assert float(err.max()) <= 4 * lg.EPS32 * gmax
