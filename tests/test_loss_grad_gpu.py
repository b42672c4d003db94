"""GPU: sncal_heatmap_loss_grad (csrc/loss.hip), loss.heatmap_loss_grad and the autograd path of HRNetLoss against the reference's
autograd gradients (tests/golden/loss_grad.npz), the fp64 closed form (tests/loss_grad_ref.py) and torch autograd through the
composed path (create_target + torch ops) in fp64.

Tolerance of the kernel (set by the issue, not tuned): max over elements of |g - g64| <= 4 * max(E_ref, 2^-23) * max|g64| per
combination, E_ref being the reference's own distance from the fp64 evaluation (stored in the fixture): the rule of the forward
test, for a different evaluation order.  Against the captured fp32 samples the triangle inequality adds E_ref + E_tgt.  Shapes
without a capture take the floor, 4 * 2^-23 * max|g64|.
The wing term is ill-conditioned in one corner: at t near 1, w' goes as delta^0.1, so an element with 0 < delta64 < 2^-14 and
t > 0.25 is decided by the rounding of exp.  Such elements are left out where the wing bit is set (at most 16 per case; the
fixture counts 0-2); elements with delta64 exactly 0 stay in and must get exactly 0 from the wing term."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loss_grad_ref as lg
import validate_ref as vr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'loss_grad.npz'))


@pytest.fixture(scope='module')
def cases(gold_dir):
    """The loss cases of validate.npz with their prediction and the helper's fp32 target, computed once."""
    out = vr.loss_cases(np.load(os.path.join(gold_dir, 'validate.npz')))
    for c in out.values():
        c['pred'] = vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        c['target'] = vr.target32(c['kp'], c['stride'], c['sigma'], c['shape'][2:])
    return out


def _dev_mask(m, cuda):
    return None if m is None else torch.from_numpy(np.asarray(m)).to(cuda, torch.float32)


@pytest.mark.parametrize('name', ['small', 'train', 'ragged'])
def test_kernel_matches_fp64_and_capture(sncal, cuda, gold, cases, name):
    c = cases[name]
    pred, target = c['pred'], c['target']
    d_pred, d_kp = torch.from_numpy(pred).to(cuda), torch.from_numpy(c['kp']).to(cuda)
    pos = lg.seeded_positions(c['seed'], pred.size)
    worst = 0.0
    for cname, mname, wname in lg.kp_combinations(cases):
        if cname != name:
            continue
        key = f'kp.{name}.{mname}.{wname}'
        m, terms, coef = c['masks'][mname], lg.KP_TERMS[wname], lg.kp_coef(vr.WEIGHTS[wname], c['shape'])
        got = sncal.loss.heatmap_loss_grad(d_pred, d_kp, _dev_mask(m, cuda), c['sigma'], c['stride'], coef, terms)
        again = sncal.loss.heatmap_loss_grad(d_pred, d_kp, _dev_mask(m, cuda), c['sigma'], c['stride'], coef, terms)
        assert got.shape == d_pred.shape and got.dtype == torch.float32 and torch.equal(got, again), key      # the same bits twice
        g = got.cpu().numpy().astype(np.float64)
        g64 = lg.kp_grad64(pred, target, m, coef, terms)
        gmax = float(np.abs(g64).max())
        corner = lg.kp_corner(pred, target, m) if terms & 4 else np.zeros(pred.shape, dtype=bool)
        n_corner = int(corner.sum())
        if terms & 4:
            assert n_corner <= 16 and n_corner == int(gold[key + '.corner']), (key, n_corner)
        gf, cf = g.reshape(-1), corner.reshape(-1)
        e_ref, e_tgt = float(gold[key + '.E_ref']), float(gold[key + '.E_tgt'])
        bound = 4.0 * max(e_ref, lg.EPS32)
        dist = float(np.abs(g - g64)[~corner].max()) / gmax
        top = gold[key + '.top_idx']
        d_cap = float((np.abs(gf[pos] - gold[key + '.samples'].astype(np.float64)) * ~cf[pos]).max()) / gmax
        d_top = float((np.abs(gf[top] - gold[key + '.top'].astype(np.float64)) * ~cf[top]).max()) / gmax
        print(f'{key:28s} max|g64| {gmax:.6g}  dist {dist:.3g} (bound {bound:.3g})  vs samples {d_cap:.3g}  vs top {d_top:.3g}  corner {n_corner}')
        worst = max(worst, dist / bound)
        assert dist <= bound, (key, dist, bound)
        assert d_cap <= bound + e_ref + e_tgt and d_top <= bound + e_ref + e_tgt, (key, d_cap, d_top)
    print('largest distance / bound:', worst)


@pytest.mark.parametrize('name', ['small', 'train', 'ragged'])
def test_wing_term_is_exactly_zero_where_delta_is(sncal, cuda, gold, cases, name):
    c = cases[name]
    d_pred, d_kp = torch.from_numpy(c['pred']).to(cuda), torch.from_numpy(c['kp']).to(cuda)
    m = c['masks']['zeros']
    zero = lg.kp_wing_zero(c['pred'], c['target'], m)
    n = int(zero.sum())
    print(name, 'elements with delta exactly 0:', n)
    assert 1 <= n <= 53 or (name == 'ragged' and n == 0)                      # the on-cell-centre keypoint, saturated background cells
    assert n == int(gold[f'kp.{name}.zeros.all.wing_zero'])
    g = sncal.loss.heatmap_loss_grad(d_pred, d_kp, _dev_mask(m, cuda), c['sigma'], c['stride'], (0.0, 0.0, 1.0), 4).cpu().numpy()
    assert np.isfinite(g).all() and not g[zero].any()
    if name == 'ragged':                                                       # its unmasked run has one such element
        zero = lg.kp_wing_zero(c['pred'], c['target'], None)
        assert int(zero.sum()) == 1
        g = sncal.loss.heatmap_loss_grad(d_pred, d_kp, None, c['sigma'], c['stride'], (0.0, 0.0, 1.0), 4).cpu().numpy()
        assert not g[zero].any()


def test_a_cleared_bit_contributes_nothing(sncal, cuda, cases):
    c = cases['small']
    d_pred, d_kp = torch.from_numpy(c['pred']).to(cuda), torch.from_numpy(c['kp']).to(cuda)
    m = _dev_mask(c['masks']['zeros'], cuda)
    coef = lg.kp_coef((1.0, 1.0, 1.0), c['shape'])
    for bit in range(3):
        only = tuple(v if k == bit else 0.0 for k, v in enumerate(coef))
        a = sncal.loss.heatmap_loss_grad(d_pred, d_kp, m, c['sigma'], c['stride'], coef, 1 << bit)       # the other coefficients are not read
        b = sncal.loss.heatmap_loss_grad(d_pred, d_kp, m, c['sigma'], c['stride'], only, 7)
        assert torch.equal(a, b) and a.abs().max() > 0, bit
    assert not sncal.loss.heatmap_loss_grad(d_pred, d_kp, m, c['sigma'], c['stride'], coef, 0).any()


def _raw_grad(sncal, pred, kp, mask, sigma, stride, coef, terms, gout, grad, ws_bytes=None):
    """The C entry point on tensors as they lie (any base alignment); returns the status."""
    L = sncal._lib.lib()
    B, C, h, w = pred.shape
    n = ctypes.c_size_t()
    assert L.sncal_heatmap_loss_workspace(B, C - 1, h, w, ctypes.byref(n)) == 0
    ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=pred.device)
    st = L.sncal_heatmap_loss_grad(pred.data_ptr(), kp.data_ptr(), None if mask is None else mask.data_ptr(), B, C - 1, h, w, sigma, stride,
                                   terms, (ctypes.c_double * 3)(*coef), None if gout is None else gout.data_ptr(), grad.data_ptr(),
                                   ws.data_ptr(), n.value if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return st


SHAPES = [(2, 57, 68, 120, 8.0, 1.0, 0), (1, 64, 33, 257, 1.0, 1.5, 0), (3, 5, 70, 300, 2.0, 3.0, 0), (2, 57, 19, 64, 4.0, 2.0, 1),
          (1, 1, 1, 1, 1.0, 1.0, 0)]


@pytest.mark.parametrize('B,N,h,w,stride,sigma,off', SHAPES)
def test_more_shapes_against_the_closed_form(sncal, cuda, B, N, h, w, stride, sigma, off):
    """Widths that take 16-byte accesses and widths that cannot, a base one float off alignment (prediction, gradient, and each
    alone), heights that leave waves without rows, 64 keypoints, a mask with a 0 and a 0.5 entry, predictions that are real
    log-probabilities.  Target: create_target's own output, which the kernel must rebuild.  All terms with the class's
    coefficients, and each term alone with coefficient 1, at the floor bound 4 * 2^-23 * max|g64|.  The wing term alone gets, per
    element, what one ulp of exp(p) moves it by through delta (loss_grad_ref.kp_wing_exp_rounding) on top: at t near 1 and e near t
    that exceeds the floor well outside the corner, for any fp32 evaluation (w' ~ delta^0.1: an element with delta = 2^-8 moves by
    0.1 * 2^-23 / 2^-8 of w' ~ 8, which is 2.6e-6 against a floor of 5.3e-6 at max|g64| = 11.1)."""
    rng = np.random.default_rng(3 + N + h)
    kp = np.stack([rng.uniform(-3, w * stride + 3, (B, N)), rng.uniform(-3, h * stride + 3, (B, N)), rng.uniform(size=(B, N)) < 0.8],
                  -1).astype(np.float32)
    kp[0, 0] = (np.rint(0.5 * w) * stride, np.rint(0.5 * h) * stride, 1.0)           # on a cell centre: target exactly 1
    logits = torch.from_numpy(rng.normal(0, 3, (B, N + 1, h, w)).astype(np.float32)).to(cuda)
    numel = logits.numel()
    flat_p = torch.empty(numel + 8, dtype=torch.float32, device=cuda)
    pred = flat_p[off:off + numel].view(B, N + 1, h, w)
    pred.copy_(torch.log_softmax(logits, dim=1))
    d_kp = torch.from_numpy(kp).to(cuda)
    k2 = d_kp.clone()
    k2[:, :, :2] /= stride
    target = sncal.loss.create_target(k2, sigma, (h, w)).cpu().numpy()
    mask = torch.ones((B, N + 1), dtype=torch.float32, device=cuda)
    mask[0, 0] = 0
    if N > 2:
        mask[B - 1, 2] = 0.5
    p_np = pred.cpu().numpy()
    shape = (B, N + 1, h, w)
    runs = [(7, lg.kp_coef((1.0, 1.0, 1.0), shape)), (1, (1.0, 0.0, 0.0)), (2, (0.0, 1.0, 0.0)), (4, (0.0, 0.0, 1.0))]
    for m in (None, mask):
        m_np = None if m is None else m.cpu().numpy()
        corner = lg.kp_corner(p_np, target, m_np)
        assert int(corner.sum()) <= 16
        for terms, coef in runs:
            flat_g = torch.full((numel + 8,), 7.0, dtype=torch.float32, device=cuda)
            grad = flat_g[off:off + numel].view(shape)
            assert _raw_grad(sncal, pred, d_kp, m, sigma, stride, coef, terms, None, grad) == 0
            assert (flat_g[:off] == 7.0).all() and (flat_g[off + numel:] == 7.0).all()       # nothing written outside the gradient
            g64 = lg.kp_grad64(p_np, target, m_np, coef, terms)
            err = np.abs(grad.cpu().numpy().astype(np.float64) - g64)
            if terms & 4:
                err[corner] = 0.0
            gmax = float(np.abs(g64).max())
            print((B, N, h, w, off, m is not None, terms), 'max|g64|', gmax, 'dist', float(err.max()) / gmax if gmax > 0 else 0.0, 'corner', int(corner.sum()))
            bound = 4 * lg.EPS32 * gmax
            if terms == 4:                                                        # the wing term alone: nothing larger hides its conditioning
                bound = bound + lg.kp_wing_exp_rounding(p_np, target, m_np, coef[2])
            assert (err <= bound).all(), ((B, N, h, w), terms, float(err.max()) / gmax, float((err / np.maximum(bound, 1e-300)).max()))
            if off == 0:
                assert torch.equal(grad, sncal.loss.heatmap_loss_grad(pred, d_kp, m, sigma, stride, coef, terms))
    if off:                                                                           # each of the two bases alone off alignment
        want = grad.clone()                                                           # terms 4, mask: the last run above
        aligned_p = pred.clone()
        assert aligned_p.data_ptr() % 16 == 0 and pred.data_ptr() % 16 == 4 and grad.data_ptr() % 16 == 4
        assert _raw_grad(sncal, aligned_p, d_kp, mask, sigma, stride, runs[-1][1], 4, None, grad.zero_()) == 0
        assert torch.equal(grad, want)
        aligned_g = torch.zeros_like(aligned_p)
        assert _raw_grad(sncal, pred, d_kp, mask, sigma, stride, runs[-1][1], 4, None, aligned_g) == 0
        assert torch.equal(aligned_g, want)
        assert _raw_grad(sncal, aligned_p, d_kp, mask, sigma, stride, runs[-1][1], 4, None, aligned_g.zero_()) == 0      # both aligned: 16-byte accesses
        d = np.abs(aligned_g.cpu().numpy().astype(np.float64) - g64)
        d[corner] = 0.0
        assert (d <= bound).all()
    # the upstream gradient: a device scalar; 1024 scales every element exactly
    coef = runs[0][1]
    one = sncal.loss.heatmap_loss_grad(pred.contiguous().clone(), d_kp, mask, sigma, stride, coef, 7)
    k = sncal.loss.heatmap_loss_grad(pred.contiguous().clone(), d_kp, mask, sigma, stride, coef, 7, grad_output=torch.tensor(1024.0, device=cuda))
    assert torch.equal(k, one * 1024.0)


def _loss_and_inputs(sncal, cuda, c, wts=(1.0, 1.0, 1.0)):
    B, C, h, w = c['shape']
    loss = sncal.HRNetLoss(num_refinement_stages=0, sigma=c['sigma'], stride=int(c['stride']), pred_size=(h, w), num_keypoints=C - 1,
                           l2_w=wts[0], kldiv_w=wts[1], awing_w=wts[2])
    return loss, torch.from_numpy(c['pred']).to(cuda), torch.from_numpy(c['kp']), torch.from_numpy(c['masks']['zeros'])


def test_autograd_surface(sncal, cuda, cases):
    c = cases['small']
    B = c['shape'][0]
    for wts in ((1.0, 1.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.5)):
        loss, pred, kp, mask = _loss_and_inputs(sncal, cuda, c, wts)
        for m in (None, mask):                                                # int64, on the host: as the loader yields it
            plain = loss([pred], kp.reshape(B, -1), m)
            assert plain.grad_fn is None and not plain.requires_grad
            p = pred.clone().requires_grad_()
            v = loss([p], kp.reshape(B, -1), m)
            assert v.grad_fn is not None and v.dtype == torch.float32 and v.dim() == 0 and torch.equal(v.detach(), plain)
            v.backward()
            want = sncal.loss.heatmap_loss_grad(pred, kp.to(cuda), _dev_mask(m, cuda), c['sigma'], c['stride'], loss.coef(pred), loss.terms)
            assert p.grad.shape == pred.shape and p.grad.device == pred.device and torch.equal(p.grad, want)
            assert want.abs().max() > 0
            loss([p], kp, m).backward()                                        # accumulates into the existing .grad
            assert torch.equal(p.grad, want + want)
            q = pred.clone().requires_grad_()
            (loss(q, kp.to(cuda), m) * 1024).backward()                        # a bare tensor; the scale arrives as grad_output
            assert torch.equal(q.grad, want * 1024.0)
            with torch.no_grad():
                quiet = loss([p], kp, m)
            assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, plain)
    # a non-contiguous prediction is made contiguous inside; the gradient has the shape of the prediction as passed
    loss, pred, kp, mask = _loss_and_inputs(sncal, cuda, c)
    want = sncal.loss.heatmap_loss_grad(pred, kp.to(cuda), _dev_mask(mask, cuda), c['sigma'], c['stride'], loss.coef(pred), loss.terms)
    nc = pred.to(memory_format=torch.channels_last).requires_grad_()
    assert not nc.is_contiguous()
    v = loss([nc], kp, mask)
    v.backward()
    assert nc.grad.shape == pred.shape and torch.equal(nc.grad, want) and torch.equal(v.detach(), loss([pred], kp, mask))
    # through an op in front of the loss: the chain rule reaches the leaf
    leaf = (pred * 2).requires_grad_()
    loss([leaf * 0.5], kp, mask).backward()
    assert torch.equal(leaf.grad, want * 0.5)
    # a double backward raises
    p = pred.clone().requires_grad_()
    v = loss([p], kp, mask)
    g, = torch.autograd.grad(v * v, p, create_graph=True)                    # an upstream gradient that is itself on the tape
    assert torch.equal(g.detach(), want * (v.detach() * 2))
    with pytest.raises(RuntimeError, match='once_differentiable'):
        g.sum().backward()
    g, = torch.autograd.grad(loss([p], kp, mask), p, create_graph=True)  # a constant upstream gradient: no second-order graph at all
    assert torch.equal(g, want) and not g.requires_grad
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # components() stays off the tape; refinement stages are still refused
    assert loss.components([pred.clone().requires_grad_()], kp, mask).grad_fn is None
    with pytest.raises(sncal._lib.SncalError, match='num_refinement_stages'):
        sncal.HRNetLoss(num_refinement_stages=1)
    # B == 0: nan forward as before, an empty gradient
    e = torch.zeros((0,) + tuple(c['shape'][1:]), device=cuda, requires_grad=True)
    v = loss([e], torch.zeros((0, 3 * (c['shape'][1] - 1))))
    assert torch.isnan(v)
    v.backward()
    assert e.grad.shape == e.shape


def test_bad_arguments_fail_loudly(sncal, cuda):
    E = sncal._lib.SncalError
    good = torch.zeros((1, 6, 8, 8), device=cuda)
    kp = torch.zeros((1, 5, 3), device=cuda)
    cf = (1.0, 1.0, 0.0)
    G = sncal.loss.heatmap_loss_grad
    with pytest.raises(E, match='N=65'):
        G(torch.zeros((1, 66, 8, 8), device=cuda), torch.zeros((1, 65, 3), device=cuda), None, 1.0, 1.0, cf)
    with pytest.raises(E, match='sigma'):
        G(good, kp, None, 0.0, 1.0, cf)
    with pytest.raises(E, match='stride'):
        G(good, kp, None, 1.0, -2.0, cf)
    with pytest.raises(E, match='must be'):
        G(torch.zeros((1, 7, 8, 8), device=cuda), kp, None, 1.0, 1.0, cf)
    with pytest.raises(E, match='mask'):
        G(good, kp, torch.ones((1, 5), device=cuda), 1.0, 1.0, cf)
    with pytest.raises(E, match='float32'):
        G(good.double(), kp, None, 1.0, 1.0, cf)
    with pytest.raises(E, match='terms'):
        G(good, kp, None, 1.0, 1.0, cf, 8)
    with pytest.raises(E, match='coef'):
        G(good, kp, None, 1.0, 1.0, (1.0, 1.0))
    with pytest.raises(E, match='grad_output'):
        G(good, kp, None, 1.0, 1.0, cf, 3, torch.ones(2, device=cuda))
    with pytest.raises(E, match='GPU'):
        G(good.cpu(), kp, None, 1.0, 1.0, cf)
    grad = torch.zeros_like(good)
    assert _raw_grad(sncal, good, kp, None, 1.0, 1.0, cf, 3, None, grad, ws_bytes=64) == -4             # SNCAL_ERR_WORKSPACE
    assert b'workspace' in sncal._lib.lib().sncal_last_error()
    assert _raw_grad(sncal, good, kp, None, 1.0, 1.0, cf, 3, None, grad) == 0
    assert grad.abs().max() > 0
    with pytest.raises(E, match='pred_size'):
        sncal.HRNetLoss(pred_size=(8, 9), num_keypoints=5)([good.clone().requires_grad_()], kp)


def test_matches_torch_autograd_through_the_composed_path_in_fp64(sncal, cuda):
    B, N, h, w, stride, sigma = 2, 57, 68, 120, 8.0, 1.0
    rng = np.random.default_rng(17)
    kp = torch.from_numpy(np.stack([rng.uniform(-3, w * stride + 3, (B, N)), rng.uniform(-3, h * stride + 3, (B, N)),
                                    rng.uniform(size=(B, N)) < 0.8], -1).astype(np.float32)).to(cuda)
    pred = torch.log_softmax(torch.from_numpy(rng.normal(0, 3, (B, N + 1, h, w)).astype(np.float32)).to(cuda), dim=1)
    mask = torch.ones((B, N + 1), dtype=torch.float32, device=cuda)
    mask[0, 1] = 0
    mask[1, 2] = 0.5
    loss = sncal.HRNetLoss(sigma=sigma, stride=int(stride), pred_size=(h, w), num_keypoints=N, l2_w=1.0, kldiv_w=1.0, awing_w=1.0)
    p = pred.clone().requires_grad_()
    loss([p], kp, mask).backward()
    # the composed path: create_target's own output, then the reference's torch ops, in fp64
    k2 = kp.clone()
    k2[:, :, :2] /= stride
    mm = mask.double()[:, :, None, None]
    t0 = sncal.loss.create_target(k2, sigma, (h, w))
    t = t0.double() * mm
    x = pred.double().requires_grad_()
    z = x * mm
    e = torch.exp(z)
    half = torch.tensor(0.5, dtype=torch.float64, device=cuda)
    delta, a = (t - e).abs(), vr.ALPHA - t
    A = vr.OMEGA * (1 / (1 + torch.pow(half, a))) * a * torch.pow(half, a - 1)
    Cc = vr.THETA * A - vr.OMEGA * torch.log(1 + torch.pow(half, a))
    aw = torch.where(delta < vr.THETA, vr.OMEGA * torch.log(1 + torch.pow(delta, a)), A * delta - Cc).mean()
    total = torch.nn.functional.mse_loss(e, t) + torch.nn.functional.kl_div(z, t, reduction='batchmean') + aw
    total.backward()
    g64 = x.grad
    corner = torch.from_numpy(lg.kp_corner(pred.cpu().numpy(), t0.cpu().numpy(), mask.cpu().numpy())).to(cuda)
    assert int(corner.sum()) <= 16
    err = (p.grad.double() - g64).abs().masked_fill(corner, 0.0)
    gmax = float(g64.abs().max())
    print('max|g64|', gmax, 'dist', float(err.max()) / gmax, 'corner', int(corner.sum()))
    assert float(err.max()) <= 4 * lg.EPS32 * gmax
