"""GPU: sncal_heatmap_loss (csrc/loss.hip), HRNetLoss and HRNetMetaModel.val_step against the reference capture
(tests/golden/validate.npz), the fp64 restatement (tests/validate_ref.py) and the composed path (create_target + torch ops).

Tolerance of the kernel (set by the issue, not tuned): the reference and the kernel are both fp32 evaluations of one formula
with different summation orders, so the kernel's relative distance from the fp64 evaluation may be at most
4 * max(d_ref, 2^-23) per case, d_ref being the reference's own distance stored in the fixture.  Against the captured fp32 value the
triangle inequality adds the capture's own d_ref."""
import os

import numpy as np
import pytest
import torch

import validate_ref as vr
from oracle import hrnet_ref as hr

pytestmark = pytest.mark.gpu

TERMS = {'mse': 1, 'kl': 2, 'awing': 4, 'default': 3, 'all': 7}


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'validate.npz'))


def _sums(sncal, pred, kp, mask, sigma, stride, terms):
    m = None if mask is None else mask.to(torch.float32)
    return sncal.loss.heatmap_loss_sums(pred, kp, m, sigma, stride, terms)


def test_kernel_matches_capture_and_fp64_helper(sncal, cuda, gold):
    worst = 0.0
    for name, c in vr.loss_cases(gold).items():
        B, C, h, w = c['shape']
        pred = vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        target = vr.target32(c['kp'], c['stride'], c['sigma'], (h, w))
        d_pred, d_kp = torch.from_numpy(pred).to(cuda), torch.from_numpy(c['kp']).to(cuda)
        for mname, m in c['masks'].items():
            exact = vr.loss_terms64(pred, target, m)
            d_m = None if m is None else torch.from_numpy(m).to(cuda)
            for wname, wts in vr.WEIGHTS.items():
                got = _sums(sncal, d_pred, d_kp, d_m, c['sigma'], c['stride'], TERMS[wname])
                again = _sums(sncal, d_pred, d_kp, d_m, c['sigma'], c['stride'], TERMS[wname])
                assert torch.equal(got, again), (name, mname, wname)                   # no atomics: the same bits twice
                got = got.cpu().numpy()
                for k in range(3):
                    if not (TERMS[wname] >> k) & 1:
                        assert not got[:, k].any()                                     # a term that was not asked for is not computed
                key = f'loss.{name}.{mname}.{wname}'
                d_ref, ref = float(gold[key + '.d_ref']), float(gold[key + '.ref'])
                bound = 4.0 * max(d_ref, vr.EPS32)
                v, v64 = vr.combine(got, wts, c['shape']), vr.combine(exact, wts, c['shape'])
                dist, dist_ref = abs(v - v64) / abs(v64), abs(v - ref) / abs(ref)
                print(f'{key:30s} kernel {v:.12g} fp64 {v64:.12g} ref {ref:.9g}  dist {dist:.3g} (bound {bound:.3g})  vs capture {dist_ref:.3g}')
                worst = max(worst, dist / bound)
                assert dist <= bound, (key, dist, bound)
                assert dist_ref <= bound + d_ref + 2.0 ** -24, (key, dist_ref)
    print('largest distance / bound:', worst)


def _composed64(sncal, pred, kp_img, mask, sigma, stride, hw):
    """The composed path in fp64 on the device: create_target's own output (the kernel must rebuild exactly these values), then
    torch ops -> (B,3) sums."""
    kp = kp_img.clone()
    kp[:, :, :2] /= stride
    t = sncal.loss.create_target(kp, sigma, hw).double()
    p = pred.double()
    if mask is not None:
        mm = mask.double()[:, :, None, None]
        t, p = t * mm, p * mm
    e = torch.exp(p)
    mse = ((e - t) ** 2).sum(dim=(1, 2, 3))
    kl = (torch.special.xlogy(t, t) - t * p).sum(dim=(1, 2, 3))
    delta, a = (t - e).abs(), vr.ALPHA - t
    P = torch.pow(torch.tensor(0.5, dtype=torch.float64, device=pred.device), a)
    A = vr.OMEGA * (1 / (1 + P)) * a * torch.pow(torch.tensor(0.5, dtype=torch.float64, device=pred.device), a - 1)
    Cc = vr.THETA * A - vr.OMEGA * torch.log(1 + P)
    aw = torch.where(delta < vr.THETA, vr.OMEGA * torch.log(1 + torch.pow(delta, a)), A * delta - Cc).sum(dim=(1, 2, 3))
    return torch.stack([mse, kl, aw], dim=1)


def test_kernel_matches_composed_path_on_more_shapes(sncal, cuda):
    """Widths that take the 16-byte path and widths that cannot, an unaligned base pointer, heights that leave waves without
    rows, 64 keypoints, a mask with a fractional entry, predictions that are real log-probabilities.  Per-frame, per-term sums
    against the fp64 composed path within 4 * 2^-23 (the bound above at its floor: no reference capture exists for these)."""
    rng = np.random.default_rng(3)
    for (B, N, h, w, stride, sigma, off) in [(2, 57, 68, 120, 8.0, 1.0, 0), (1, 64, 33, 257, 1.0, 1.5, 0), (3, 5, 70, 300, 2.0, 3.0, 0),
                                             (2, 57, 19, 64, 4.0, 2.0, 1), (1, 1, 1, 1, 1.0, 1.0, 0), (5, 57, 135, 240, 4.0, 2.0, 0)]:
        kp = np.stack([rng.uniform(-3, w * stride + 3, (B, N)), rng.uniform(-3, h * stride + 3, (B, N)), rng.uniform(size=(B, N)) < 0.8],
                      -1).astype(np.float32)
        logits = torch.from_numpy(rng.normal(0, 3, (B, N + 1, h, w)).astype(np.float32)).to(cuda)
        flat = torch.empty(logits.numel() + 4, dtype=torch.float32, device=cuda)
        pred = flat[off:off + logits.numel()].view(B, N + 1, h, w)
        pred.copy_(torch.log_softmax(logits, dim=1))
        d_kp = torch.from_numpy(kp).to(cuda)
        mask = torch.ones((B, N + 1), dtype=torch.float32, device=cuda)
        mask[0, 0] = 0
        if N > 2:
            mask[B - 1, 2] = 0.5
        for m in (None, mask):
            want = _composed64(sncal, pred, d_kp, m, sigma, stride, (h, w)).cpu().numpy()
            got = sncal.loss.heatmap_loss_sums(pred, d_kp, m, sigma, stride, 7).cpu().numpy()
            rel = np.abs(got - want) / np.abs(want)
            print((B, N, h, w, off, m is not None), 'largest relative distance per term', rel.max(axis=0))
            assert (rel <= 4 * vr.EPS32).all(), ((B, N, h, w), rel)


def test_hrnetloss_surface(sncal, cuda, gold):
    c = vr.loss_cases(gold)['small']
    B, C, h, w = c['shape']
    pred = torch.from_numpy(vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])).to(cuda)
    kp = torch.from_numpy(c['kp'])
    loss = sncal.HRNetLoss(num_refinement_stages=0, sigma=c['sigma'], stride=int(c['stride']), pred_size=(h, w), num_keypoints=C - 1)
    for mname, m in c['masks'].items():
        tm = None if m is None else torch.from_numpy(m)                    # int64, on the host: as the loader yields it
        for wname, wts in vr.WEIGHTS.items():
            loss.l2_w, loss.kldiv_w, loss.awing_w = wts
            v = loss([pred], kp.reshape(B, -1), tm)                        # (B, 3N) on the host
            assert v.is_cuda and v.dim() == 0 and v.dtype == torch.float32
            assert torch.equal(v, loss.forward(pred, kp.to(cuda), tm))     # bare tensor, (B,N,3) on the device
            key = f'loss.small.{mname}.{wname}'
            d_ref, ref = float(gold[key + '.d_ref']), float(gold[key + '.ref'])
            assert abs(float(v) - ref) <= (4 * max(d_ref, vr.EPS32) + d_ref + 2.0 ** -23) * abs(ref), key
            s = loss.components([pred], kp, tm)
            assert s.shape == (B, 3) and s.dtype == torch.float64
            assert abs(vr.combine(s.cpu().numpy(), wts, c['shape']) - float(v)) <= 2.0 ** -23 * abs(float(v))
    # the target the loss object writes is create_target's
    k2 = kp.clone().to(cuda)
    k2[:, :, :2] /= c['stride']
    assert torch.equal(loss.create_target(k2), sncal.loss.create_target(k2, c['sigma'], (h, w)))
    # B == 0: nan, as torch's means over nothing
    loss.l2_w, loss.kldiv_w, loss.awing_w = 1.0, 1.0, 0.0
    empty = loss([torch.zeros((0, C, h, w), device=cuda)], torch.zeros((0, 3 * (C - 1))))
    assert empty.dim() == 0 and torch.isnan(empty)
    loss.l2_w = loss.kldiv_w = 0.0                                         # no term at all: the reference returns 0
    assert float(loss([pred], kp)) == 0.0


def test_bad_arguments_fail_loudly(sncal, cuda):
    E = sncal._lib.SncalError
    good = torch.zeros((1, 6, 8, 8), device=cuda)
    kp = torch.zeros((1, 5, 3), device=cuda)
    with pytest.raises(E, match='N=65'):
        sncal.loss.heatmap_loss_sums(torch.zeros((1, 66, 8, 8), device=cuda), torch.zeros((1, 65, 3), device=cuda), None, 1.0, 1.0)
    with pytest.raises(E, match='sigma'):
        sncal.loss.heatmap_loss_sums(good, kp, None, 0.0, 1.0)
    with pytest.raises(E, match='stride'):
        sncal.loss.heatmap_loss_sums(good, kp, None, 1.0, -2.0)
    with pytest.raises(E, match='must be'):                                 # size mismatch: 5 keypoints need 6 channels
        sncal.loss.heatmap_loss_sums(torch.zeros((1, 7, 8, 8), device=cuda), kp, None, 1.0, 1.0)
    with pytest.raises(E, match='mask'):
        sncal.loss.heatmap_loss_sums(good, kp, torch.ones((1, 5), device=cuda), 1.0, 1.0)
    with pytest.raises(E, match='float32'):
        sncal.loss.heatmap_loss_sums(good.double(), kp, None, 1.0, 1.0)
    # a short workspace, through the C ABI
    import ctypes
    L = sncal._lib.lib()
    n = ctypes.c_size_t()
    assert L.sncal_heatmap_loss_workspace(1, 5, 8, 8, ctypes.byref(n)) == 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=cuda)
    out = torch.zeros((1, 3), dtype=torch.float64, device=cuda)
    args = (good.data_ptr(), kp.data_ptr(), None, 1, 5, 8, 8, 1.0, 1.0, 3, out.data_ptr(), ws.data_ptr())
    assert L.sncal_heatmap_loss(*args, n.value - 1, None) == -4
    assert L.sncal_heatmap_loss(*args, n.value, None) == 0
    torch.cuda.synchronize()
    assert out[0, 0] > 0
    with pytest.raises(E, match='pred_size'):
        sncal.HRNetLoss(pred_size=(8, 9), num_keypoints=5)([good], kp)


def test_val_step_on_a_real_forward(sncal, cuda, tmp_path):
    """HRNet-W18 forward: val_step's loss is HRNetLoss on that forward's heatmap, its prediction is predict()'s, the batch dict
    is left alone, and sync=True hands the loss out as a float."""
    cfg = hr.load_config('hrnet_w18')
    sd = hr.seeded_state_dict(cfg, 5, 4.0)
    lp = {'num_refinement_stages': 0, 'stride': 8, 'sigma': 1.0, 'pred_size': [68, 120], 'num_keypoints': 57}
    ck = {'model_name': 'HRNetMetaModel',
          'params': {'nn_module': {'hrnet_config': cfg, 'num_refinement_stages': 0, 'num_heatmaps': 58}, 'loss': lp,
                     'prediction_transform': {'size': [540, 960]}, 'device': 'cuda:0'},
          'nn_state_dict': sd}
    path = str(tmp_path / 'model.pth')
    torch.save(ck, path)
    x = hr.seeded_input(3, 135, 240, 6)
    kps = torch.from_numpy(sncal.synth.synthetic_keypoints(3, seed=9))
    kps[..., 2] = (kps[..., 2] > 0.5).float()
    mask = torch.ones((3, 58), dtype=torch.int64)
    mask[1, 31] = 0
    for dtype in ('fp32', None):
        model = sncal.load_model(path, loss=None, optimizer=None, device='cuda:0', dtype=dtype)
        batch = {'image': x, 'keypoints': kps.reshape(3, -1), 'mask': mask, 'raw_annot': [{}, {}, {}], 'img_name': ['a', 'b', 'c']}
        out = model.val_step(batch)
        assert sorted(out) == ['img_name', 'loss', 'prediction', 'raw_annots', 'target'] and sorted(batch) == ['image', 'img_name', 'keypoints', 'mask', 'raw_annot']
        assert out['loss'].is_cuda and out['loss'].dim() == 0
        heat = model.nn_module(x.to(cuda))[-1]
        want = sncal.HRNetLoss(**lp)([heat], kps, mask)
        assert torch.equal(out['loss'], want) and torch.isfinite(want) and float(want) > 0
        assert torch.equal(out['prediction'], model.predict(x))
        assert torch.equal(out['target'].cpu(), kps.reshape(3, -1)) and out['raw_annots'] == [{}, {}, {}] and out['img_name'] == ['a', 'b', 'c']
        assert model.val_step(batch, sync=True)['loss'] == float(want)
    # a loss handed in replaces the checkpoint's; a checkpoint without a loss section says what to do
    other = sncal.load_model(path, loss={'sigma': 2.0, 'stride': 8, 'pred_size': [68, 120], 'kldiv_w': 0.0}, device='cuda:0', dtype='fp32')
    assert other.loss.sigma == 2.0 and other.loss.terms == 1
    del ck['params']['loss']
    torch.save(ck, path)
    bare = sncal.load_model(path, device='cuda:0', dtype='fp32')
    with pytest.raises(sncal._lib.SncalError, match='loss'):
        bare.val_step(batch)
