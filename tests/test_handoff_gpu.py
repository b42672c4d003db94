"""GPU: what stands in front of the reduced-precision launches and is an INPUT of the per-launch references of tests/test_kernels_gpu.py.

    fp8 calibration (hrnet.cpp sncal_hrnet_calibrate_fp8, quant.hip absmax_bf16_kernel): tw['scale'] enters the e4m3 convolution's
    reference as a given, so a scale from a wrong maximum gives consistent launches on saturated or wasted codes.  Here every scale is
    held to float32(max |x|) / 448.0f of the dense bf16 tensor, bit for bit -- over the sub-batches of one calibration, and after a second
    calibration that has to forget the first.
    uint8 frames (ops.hip u8hwc_to_nhwc_kernel): the input tensor of forward(uint8 HWC) equals that of forward(x / 255), bit for bit.

W48 at 270x480 (the size of test_fp8_gpu.py::test_fp8_plumbing_small; W18 has no two-team layers, hence no e4m3 twins), seeded peaked
weights and stamped frames as the other fp8 tests use."""
import numpy as np
import pytest
import torch

from test_kernels_gpu import verify_plan

pytestmark = pytest.mark.gpu

SIZE = (270, 480)


@pytest.fixture(scope='module')
def w48(sncal):
    import bench
    return sncal.synth.peaked_state_dict(bench.seeded_weights('hrnet_w48', seed=1))


def _frames(sncal, cuda, n, seed):
    frames, _ = sncal.synth.stamped_frames(n, seed=seed, size=SIZE)
    return torch.from_numpy(frames).to(cuda)


def _fp8_net(sncal, cuda, sd):
    net = sncal.HRNetHeatmap('hrnet_w48', dtype='fp8', device=cuda)
    net.load_state_dict(sd)
    return net


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _plan(net, spec, x):
    net.set_fp8_layers(spec)
    net.workspace_bytes(x.shape[0], x.shape[2], x.shape[3])              # lays the plan out: no device work
    return [o for o in net.plan_ops() if o['active']]


def _candidates(net, x):
    """{tensor id: index of an op that reads it} for every tensor with an (allocated) e4m3 twin under 'all': the inputs of the e4m3
    convolutions.  Needs a calibrated network (no layer runs in fp8 before)."""
    cands = {}
    for o in _plan(net, 'all', x):
        if o['type'] == 'conv' and o['fp8']:
            tw = net.plan_tensor(o['in'])['twin']
            assert tw >= 0 and net.plan_tensor(tw)['alive']
            cands.setdefault(o['in'], o['idx'])
    assert len(cands) >= 20, len(cands)
    return cands


def _scales(net, x):
    _plan(net, 'all', x)
    n = net._L.sncal_hrnet_plan_num_tensors(net._h)
    return {t: net.plan_tensor(t)['scale'] for t in range(n) if net.plan_tensor(t)['dtype'] != 'e4m3'}


def _amax_none(net, x, cands):
    """{tensor id: float32 max |x|} of the dense bf16 candidates in one 'none' forward of x (the bf16 engine bit for bit:
    test_fp8_gpu.py::test_fp8_plumbing_small), each tapped at an op that reads it."""
    ops = _plan(net, 'none', x)
    assert x.shape[0] <= net.plan_tensor(0)['sub_batch'], 'taps hold the first sub-batch only'
    assert not any(o['fp8'] for o in ops)
    reads = {o['idx']: o for o in ops}
    taps = {}
    for t, idx in cands.items():
        assert reads[idx]['in'] == t and net.plan_tensor(t)['dtype'] == 'bf16' and net.plan_tensor(t)['alive']
        taps[t] = net.tap(idx, t)
    net.forward(x, want_heat=False, decode_size=SIZE)
    torch.cuda.synchronize()
    net.clear_taps()
    out = {}
    for t, v in taps.items():
        assert v.shape[0] == x.shape[0]
        out[t] = np.float32(float(v.to(torch.float32).abs().max()))
        assert np.isfinite(out[t]) and out[t] > 0, (t, out[t])
    return out


def _check_scales(net, x, cands, amax, what):
    """scale == float32(amax) / 448.0f as fp32 bits for every candidate; 1.0 for every tensor no e4m3 convolution reads."""
    scales = _scales(net, x)
    bad = []
    for t in sorted(cands):
        want = np.float32(amax[t]) / np.float32(448.0)
        if _bits(scales[t]) != _bits(want):
            bad.append(f'tensor {t}: scale {scales[t]!r} (0x{_bits(scales[t]):08x}), max |x| {float(amax[t])!r} / 448 = {float(want)!r} (0x{_bits(want):08x})')
    assert not bad, f'{what}: {len(bad)} of {len(cands)} calibrated scales are not amax / 448: ' + '; '.join(bad[:4])
    stray = [f'tensor {t}: {s!r}' for t, s in sorted(scales.items()) if t not in cands and s != 1.0]
    assert not stray, f'{what}: tensors no e4m3 convolution reads carry a scale: ' + '; '.join(stray[:6])
    return scales


def test_calibrated_scales_are_amax_over_448(sncal, cuda, w48):
    x = _frames(sncal, cuda, 3, 5)
    net = _fp8_net(sncal, cuda, w48)
    net.calibrate_fp8(x)
    cands = _candidates(net, x)
    amax = _amax_none(net, x, cands)
    scales = _check_scales(net, x, cands, amax, 'one calibration of 3 frames')
    assert len({_bits(scales[t]) for t in cands}) > len(cands) // 2          # per-tensor scales, not one value


def test_calibration_accumulates_over_sub_batches(sncal, cuda, w48, monkeypatch):
    """5 frames in sub-batches of 2, 2 and 1 (SNCAL_SUBBATCH is read when the network is created): the maximum is taken over all three
    launches of absmax_bf16_kernel.  The last, ragged sub-batch holds the one bright frame, so a calibration that keeps the first
    launch's maximum (or the first two) comes out too small."""
    monkeypatch.setenv('SNCAL_SUBBATCH', '2')
    x = _frames(sncal, cuda, 5, 6)
    x[:4] *= 0.35
    net = _fp8_net(sncal, cuda, w48)
    net.calibrate_fp8(x)
    cands = _candidates(net, x[:2])
    assert net.plan_tensor(0)['sub_batch'] == 2
    parts = [_amax_none(net, x[a:b], cands) for a, b in ((0, 2), (2, 4), (4, 5))]
    amax = {t: max(p[t] for p in parts) for t in cands}
    last_only = sum(parts[2][t] > max(parts[0][t], parts[1][t]) for t in cands)
    print(f'HANDOFF sub-batches: {last_only} of {len(cands)} maxima come from the last sub-batch alone')
    assert last_only >= 1, (last_only, len(cands))              # (deep tensors are led by the weights' peaks, not by the frame's brightness)
    _check_scales(net, x[:2], cands, amax, 'one calibration of 5 frames in sub-batches of 2, 2, 1')


def test_recalibration_forgets_and_the_output_scales_follow(sncal, cuda, w48):
    """Calibrate on a bright batch, then on a dim one: every scale is the dim batch's alone (the maxima are cleared before the second
    forward accumulates into them), and the per-channel output scales of the e4m3 convolutions were rebuilt from them: every launch of an
    'all' forward still matches its torch reference, which multiplies by tw['scale'] (test_kernels_gpu.verify_plan)."""
    bright = _frames(sncal, cuda, 3, 7)
    dim = bright * 0.3
    net = _fp8_net(sncal, cuda, w48)
    net.calibrate_fp8(bright)
    cands = _candidates(net, bright)
    first = _scales(net, bright)
    net.calibrate_fp8(dim)
    amax = _amax_none(net, dim, cands)
    second = _check_scales(net, dim, cands, amax, 'second calibration, on the dim batch')
    smaller = sum(second[t] < first[t] for t in cands)
    print(f'HANDOFF re-calibration: {smaller} of {len(cands)} scales shrank')
    assert smaller >= 1, (smaller, len(cands))                  # maxima that survived the first calibration would show here
    stats = verify_plan(sncal, cuda, 'hrnet_w48', w48, dim, 'fp8', fp8_layers='all', tag='w48 270x480 fp8 after re-calibration', net=net)
    k = 'conv_tt<fp8,k3,s1,8x32x96>'
    assert stats[k]['ops'] + stats[k + ' e4m3 out']['ops'] >= 144
    assert stats['quantize_fp8 in front']['ops'] >= 1 and stats['e4m3 twin = q(dense)']['ops'] >= 1
    assert stats['_case']['twin_pairs_compared'] == stats['_case']['twin_pairs_expected']


@pytest.mark.parametrize('dtype', ['bf16', 'fp16x3'])
def test_uint8_frames_give_the_input_tensor_of_their_float_form(sncal, cuda, dtype):
    """Two 64x96 frames that hold all 256 byte values in each of the three channels (6144 pixels = 24 x 256, shuffled): the NHWC input
    tensor under forward(uint8 HWC) is, bit for bit, the one under forward(x.float() / 255) -- and that one is float32(v) / 255.0f
    (rounded to bf16 in the bf16 engine), the padded channels zero."""
    from oracle import hrnet_ref as hr
    if dtype == 'fp16x3':
        dtype = sncal._lib.lib().sncal_x3_name().decode()
    B, H, W = 2, 64, 96
    g = torch.Generator().manual_seed(31)
    u8 = torch.stack([torch.stack([(torch.arange(H * W) % 256)[torch.randperm(H * W, generator=g)] for _ in range(3)], dim=-1)
                      for _ in range(B)]).reshape(B, H, W, 3).to(torch.uint8)
    for b in range(B):
        for c in range(3):
            assert torch.equal(torch.bincount(u8[b, :, :, c].reshape(-1).long(), minlength=256), torch.full((256,), 24))
    xf_np = (u8.numpy().astype(np.float32) / np.float32(255.0)).astype(np.float32)               # IEEE division, as x.float().div(255)
    xf = torch.from_numpy(xf_np).permute(0, 3, 1, 2).contiguous()
    cfg = hr.load_config('hrnet_w18')
    net = sncal.HRNetHeatmap('hrnet_w18', dtype=dtype, device=cuda)
    net.load_state_dict(hr.seeded_state_dict(cfg, 3, 4.0))
    net.workspace_bytes(B, H, W)
    op = [o for o in net.plan_ops() if o['active'] and o['type'] == 'input']
    assert len(op) == 1
    dst = net.tap(op[0]['idx'], op[0]['out'])
    k8 = net.forward(u8.to(cuda), want_heat=False, decode_size=(H, W))[1]
    torch.cuda.synchronize()
    t8 = dst.clone()
    dst.zero_()
    kf = net.forward(xf.to(cuda), want_heat=False, decode_size=(H, W))[1]
    torch.cuda.synchronize()
    tf = dst.clone()
    net.clear_taps()
    assert t8.shape == tf.shape == (B, H, W, t8.shape[-1]) and t8.shape[-1] >= 4
    want = torch.zeros(tf.shape, dtype=torch.float32)
    want[..., :3] = torch.from_numpy(xf_np)
    want = want.to(tf.dtype)
    as_int = lambda t: t.cpu().view(torch.int16 if t.element_size() == 2 else torch.int32)
    assert torch.equal(as_int(tf), as_int(want)), 'float frames: the input tensor is not x (rounded to the engine type), padded with zeros'
    bad = as_int(t8) != as_int(want)
    if bad.any():
        i = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f'uint8 frames: {int(bad.sum())} of {bad.numel()} elements of the input tensor differ from the float path; first at '
                             f'{list(i)}: {float(t8[i])!r} for byte {int(u8[i[0], i[1], i[2], i[3]]) if i[3] < 3 else "(padding)"}, float path {float(tf[i])!r}')
    assert torch.equal(as_int(t8), as_int(tf)) and torch.equal(k8, kf)
