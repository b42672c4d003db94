"""GPU: the keypoint network at `upscale: 4` (hrnet_w48x4) -- the head runs at four times branch 0's size, every source interpolated.

The fp16x3 engine serves the head with headx4.hip (stem and branches 0 / 1 blended into stage 1's K, branches 2 / 3 gathered); the
exact-fp32, bf16 and fp8 engines, and fp16x3 with SNCAL_FUSED_HEAD=0, run the reference formulation (upsample + concat + two 1x1
convolutions) with the frames per sub-batch capped.  Bounds are tests/test_hrnet_gpu.py's: fp32-class engines 2e-4 on the
log-probabilities, bf16 0.6; decoded keypoints = the oracle decode of the engine's own heat.

Networks are reduced-depth (tests/width_cases.py, W48 widths, upscale 4) unless a test says full depth.  Sizes: 72x104 (head 72x104 =
2 x stem: three full 32-column tiles and one of 8), 70x102 (stem 35x51, head 72x104: not twice the stem), 270x480 (head 272x480, taller
than the frame).
"""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import decode as od
from oracle import hrnet_ref as hr
from test_kernels_gpu import Weights, bilinear_up, check, folded, run_case
import width_cases as wc

pytestmark = pytest.mark.gpu

SIZES = {'72x104': (2, 72, 104), '70x102': (2, 70, 102), '270x480': (1, 270, 480)}
HEADS = {'72x104': (72, 104), '70x102': (72, 104), '270x480': (272, 480)}
SEED = 31
LM_SEED = 75
_ORACLE = {}


def x4_config():
    cfg = copy.deepcopy(wc.width_config((48, 96, 192, 384)))
    cfg['upscale'] = 4
    return cfg


def _case(size):
    """(cfg, state dict, frames, oracle log-probabilities) of one size; the oracle runs once per session and is not modified."""
    if size not in _ORACLE:
        cfg = x4_config()
        sd = hr.seeded_state_dict(cfg, SEED, 4.0)
        B, H, W = SIZES[size]
        x = hr.seeded_input(B, H, W, SEED + 1)
        ref = hr.forward(sd, x, cfg).numpy()
        assert ref.shape == (B, 58) + HEADS[size] and np.isfinite(ref).all()
        ref.setflags(write=False)
        _ORACLE[size] = (cfg, sd, x, ref)
    return _ORACLE[size]


def _net(sncal, cuda, cfg, sd, dtype):
    net = sncal.HRNetHeatmap(cfg, dtype=dtype, device=cuda)
    net.load_state_dict(sd)
    return net


def _head_launches(net):
    """(profile kernel names, active head-side ops) of the last profiled forward: the ops behind the trunk that belong to a head
    formulation -- concat parts (upsample_add without base), last_layer.* convolutions, head-internal slices, the fused head op."""
    ops = [o for o in net.plan_ops() if o['active']]
    head = [o for o in ops if o['type'] == 'head' or (o['type'] == 'upsample_add' and o['base'] < 0) or
            (o['type'] == 'conv' and (o['name'].startswith('model.last_layer') or o['name'].startswith('head')))]
    return [r['kernel'] for r in net.get_profile()], head


def test_create_accepts_upscale_4_and_refuses_3_and_8(sncal, cuda):
    cfg = x4_config()
    net = sncal.HRNetHeatmap(cfg, dtype='fp32', device=cuda)
    assert net.output_size(540, 960) == (540, 960) and net.output_size(70, 102) == (72, 104)
    for bad in (3, 8):
        c = dict(cfg, upscale=bad)
        with pytest.raises(sncal._lib.SncalError, match='upscale must be 1, 2 or 4'):
            sncal.HRNetHeatmap(c, dtype='fp32', device=cuda)


@pytest.mark.parametrize('size', list(SIZES))
def test_whole_network_matches_the_oracle(sncal, cuda, size):
    """Every engine against hr.forward on the CPU.  Measured max |logp - oracle| (MI355X):
        72x104   fp32 9.5e-06   fp16x3 1.1e-05   bf16 5.4e-02
        70x102   fp32 8.8e-06   fp16x3 1.2e-05   bf16 4.6e-02
        270x480  fp32 1.0e-05   fp16x3 1.6e-05   bf16 6.5e-02
    (log-probabilities between -11.5 and -0.8).  Full depth against the reference capture: fp32 2.8e-05, fp16x3 6.5e-05
    (test_full_depth_w48x4_matches_the_reference_capture); fused head against the reference formulation 8.6e-06; the head alone against
    torch on its own operands 7.4e-06, 0.9 % of the tolerance."""
    cfg, sd, x, ref = _case(size)
    x3 = sncal._lib.lib().sncal_x3_name().decode()
    for dtype, tol in (('fp32', 2e-4), (x3, 2e-4), ('bf16', 0.6)):
        net = _net(sncal, cuda, cfg, sd, dtype)
        heat, kp = net.forward(x.to(cuda), want_heat=True, decode_size=(540, 960))
        heat, kp = heat.cpu().numpy(), kp.cpu().numpy()
        err = float(np.abs(heat - ref).max())
        print(f'UPSCALE4-ORACLE {size} {dtype}: max |logp - oracle| {err:.3e} (bound {tol:g}), oracle range {ref.min():.2f} .. {ref.max():.2f}')
        assert heat.shape == ref.shape
        assert err <= tol, (size, dtype, err)
        assert np.array_equal(kp, od.keypoint_decode(heat, (540, 960))), (size, dtype)
        del net


@pytest.mark.parametrize('dtype', ['fp32', 'fp16x3'])
@pytest.mark.parametrize('hw', ['64x96', '70x102'])
def test_full_depth_w48x4_matches_the_reference_capture(sncal, cuda, gold_dir, hw, dtype):
    """Full-depth hrnet_w48x4 against the capture of the reference's own HRNetHeatmap (tools/make_golden_upscale4.py): stored samples
    within 2e-4, indices identical to the reference's decode, confidences within 1e-5 (fp32) / 1.5e-5 (fp16x3)."""
    tight = sncal._lib.lib().sncal_x3_name() == b'fp16x3' or dtype == 'fp32'      # (a build on bf16 splits: test_hrnet_gpu.py's wider bounds)
    g = np.load(os.path.join(gold_dir, 'hrnet_w48x4.npz'))
    H, W = (int(v) for v in hw.split('x'))
    cfg = hr.load_config('hrnet_w48x4')
    sd = hr.seeded_state_dict(cfg, int(g['seed']), float(g['head_gain']))
    x = hr.seeded_input(1, H, W, int(g['seed']) + 1)
    net = _net(sncal, cuda, 'hrnet_w48x4', sd, dtype)
    heat, kp = net.forward(x.to(cuda), want_heat=True, decode_size=(540, 960))
    heat, kp = heat.cpu().numpy(), kp.cpu().numpy()
    e_s = float(np.abs(heat[:, :, ::4, ::4] - g[hw + '.out_strided']).max())
    e_f = float(np.abs(heat[:, g[hw + '.full_channels']] - g[hw + '.full']).max())
    e_c = float(np.abs(kp[..., 2] - g[hw + '.decode'][..., 2]).max())
    print(f'UPSCALE4-GOLDEN {hw} {dtype}: strided {e_s:.3e} full maps {e_f:.3e} confidences {e_c:.3e}')
    assert e_s <= (2e-4 if tight else 6e-4) and e_f <= (2e-4 if tight else 6e-4)
    assert np.array_equal(kp[..., :2], g[hw + '.decode'][..., :2])
    assert e_c <= (1e-5 if dtype == 'fp32' else 1.5e-5 if tight else 3e-5)
    if dtype == 'fp16x3':
        net.set_profiling(1)
        net.forward(x.to(cuda), want_heat=False, decode_size=(540, 960))
        assert 'headx4_fused' in [r['kernel'] for r in net.get_profile()]


@pytest.mark.parametrize('size', list(SIZES))
def test_fp16x3_head_is_served_by_headx4_and_the_fallback_agrees(sncal, cuda, monkeypatch, size):
    """The profile and plan_ops() name headx4_fused and no concat part or last_layer convolution runs; with SNCAL_FUSED_HEAD=0 (read when
    the net is created) the reference formulation runs instead and agrees within 2e-4."""
    cfg, sd, x, ref = _case(size)
    x3 = sncal._lib.lib().sncal_x3_name().decode()
    net = _net(sncal, cuda, cfg, sd, x3)
    net.set_profiling(1)
    heat, kp = net.forward(x.to(cuda), want_heat=True, decode_size=(540, 960))
    kernels, head = _head_launches(net)
    assert 'headx4_fused' in kernels, kernels
    assert [o['type'] for o in head].count('head') == 1, head
    hop = [o for o in head if o['type'] == 'head'][0]
    assert hop['kernel'] == 'headx4_fused' and hop['head_direct'] == -1 and len(hop['head_fold']) == 3 and len(hop['head_src']) == 2
    assert all(o['type'] != 'upsample_add' and not o['name'].startswith('model.last_layer') for o in head), [o['name'] or o['type'] for o in head]
    assert sorted(o['name'] for o in head if o['type'] == 'conv') == ['head.t0', 'head.t1']      # the two gathered products only
    monkeypatch.setenv('SNCAL_FUSED_HEAD', '0')
    net0 = _net(sncal, cuda, cfg, sd, x3)
    net0.set_profiling(1)
    heat0, kp0 = net0.forward(x.to(cuda), want_heat=True, decode_size=(540, 960))
    kernels0, head0 = _head_launches(net0)
    assert 'headx4_fused' not in kernels0, kernels0
    assert [o['type'] for o in head0].count('upsample_add') == 5 and not any(o['type'] == 'head' for o in head0)
    d = float((heat - heat0).abs().max())
    print(f'UPSCALE4-FALLBACK {size}: max |fused - fallback| {d:.3e}')
    assert d <= 2e-4


def test_headx4_alone_against_torch_on_its_own_operands(sncal, cuda):
    """3 frames of 72x104 (frame boundaries fall inside the tile walk): hidden = ReLU(b0 + W0 . concat(up(sources))), logits = W1 . hidden
    + b1 in torch fp32 from the tapped stem, branch 0 / 1 tensors and the two gathered products; head_reference's split-fp16 tolerances."""
    cfg = x4_config()
    sd = hr.seeded_state_dict(cfg, SEED, 4.0)
    x = hr.seeded_input(3, 72, 104, SEED + 2).to(cuda)
    x3 = sncal._lib.lib().sncal_x3_name().decode()
    ops, taps, net = run_case(sncal, cuda, cfg, sd, x, x3)
    op = [o for o in ops if o['active'] and o['type'] == 'head'][0]
    assert op['kernel'] == 'headx4_fused' and op['head_direct'] == -1

    def T(tid):
        return taps[(op['idx'], tid)].to(torch.float32)
    to = net.plan_tensor(op['out'])
    H, Wd = to['H'], to['W']
    assert (H, Wd) == (72, 104)
    kin = torch.cat([bilinear_up(T(f), H, Wd, lambda t: t) for f in op['head_fold']], dim=-1)      # (N,H,W,208): stem | branch 0 | branch 1
    K1 = kin.shape[-1]
    assert K1 == 208
    W = Weights(net, sd, cuda)
    _, bn0, _, cout0, _, _, hb0 = W.units['model.last_layer.0']
    w0, sc0, sh0 = folded(sd, 'model.last_layer.0', bn0, hb0)
    w0s = (w0 * sc0[:, None, None, None])[:, :K1, 0, 0].to(cuda)
    hid = (kin.reshape(-1, K1) @ w0s.t() + sh0.to(cuda)[None]).reshape(kin.shape[0], H, Wd, cout0)
    for s in op['head_src']:
        hid = hid + bilinear_up(T(s)[..., :cout0], H, Wd, lambda t: t)
    hid = torch.relu(hid)
    _, _, _, cout1, _, _, hb1 = W.units['model.last_layer.3']
    w1, _, sh1 = folded(sd, 'model.last_layer.3', '', hb1)
    ref = (hid.reshape(-1, cout0) @ w1[:, :, 0, 0].to(cuda).t() + sh1.to(cuda)[None]).reshape(kin.shape[0], H, Wd, cout1)
    got = T(op['out'])[..., :cout1]
    stats = {}
    check(f'head -> logits {H}x{Wd} (split-fp16, upscale 4)', got, ref, 1e-4, 5e-4, stats, 'headx4_fused')
    print('UPSCALE4-HEAD', stats)


@pytest.mark.parametrize('size', ['72x104', '70x102'])
def test_keypoints_only_forward_is_bit_identical(sncal, cuda, size):
    """predict()'s path (decode fused into the head: neither logits nor heatmap written) == the keypoints of the want_heat forward."""
    cfg, sd, x, _ = _case(size)
    net = _net(sncal, cuda, cfg, sd, sncal._lib.lib().sncal_x3_name().decode())
    _, kp = net.forward(x.to(cuda), want_heat=True, decode_size=(540, 960))
    net.set_profiling(1)
    heat2, kp2 = net.forward(x.to(cuda), want_heat=False, decode_size=(540, 960))
    kernels = [r['kernel'] for r in net.get_profile()]
    assert heat2 is None and torch.equal(kp, kp2)
    assert 'kp_finish' in kernels and 'softmax_nchw' not in kernels and 'kp_decode' not in kernels, kernels      # DEC_HEAD


def test_uint8_frames_equal_totensor_frames(sncal, cuda):
    cfg, sd, _, _ = _case('72x104')
    net = _net(sncal, cuda, cfg, sd, sncal._lib.lib().sncal_x3_name().decode())
    frames = torch.randint(0, 256, (2, 70, 102, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    as_totensor = frames.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    h8, k8 = net.forward(frames.to(cuda), want_heat=True, decode_size=(540, 960))
    hf, kf = net.forward(as_totensor.to(cuda), want_heat=True, decode_size=(540, 960))
    assert torch.equal(h8, hf) and torch.equal(k8, kf)


def test_batch_of_5_in_sub_batches_of_2_equals_per_frame_results(sncal, cuda, monkeypatch):
    cfg, sd, _, _ = _case('72x104')
    monkeypatch.setenv('SNCAL_SUBBATCH', '2')
    net = _net(sncal, cuda, cfg, sd, sncal._lib.lib().sncal_x3_name().decode())
    x = hr.seeded_input(5, 72, 104, SEED + 3).to(cuda)
    heat, kp = net.forward(x, want_heat=True, decode_size=(540, 960))
    _, kpo = net.forward(x, want_heat=False, decode_size=(540, 960))
    assert torch.equal(kp, kpo)
    for i in range(5):
        h1, k1 = net.forward(x[i:i + 1].contiguous(), want_heat=True, decode_size=(540, 960))
        assert torch.equal(h1[0], heat[i]) and torch.equal(k1[0], kp[i]), i


def test_load_model_predict_surface_takes_an_x4_checkpoint(sncal, cuda, tmp_path):
    """argus-style checkpoint dict carrying the x4 config -> load_model(...).predict(x), default engine: keypoints in 960x540 units,
    indices = the oracle decode.  Seed 75 at gain 4.0: the oracle's decode gap (top two of the column / row maxima) on these frames is
    1.48e-3, beyond twice the engines' 2e-4 bound, so an engine inside the bound cannot move an index (of seeds 70..89 at gains 1.5 and 4.0
    the only one above 1e-3)."""
    cfg = x4_config()
    sd = hr.seeded_state_dict(cfg, LM_SEED, 4.0)
    ck = {'model_name': 'HRNetMetaModel',
          'params': {'nn_module': {'hrnet_config': cfg, 'num_refinement_stages': 0, 'num_heatmaps': 58},
                     'prediction_transform': {'size': [540, 960]}, 'device': 'cuda:0'},
          'nn_state_dict': sd}
    path = str(tmp_path / 'model_x4.pth')
    torch.save(ck, path)
    model = sncal.load_model(path, loss=None, optimizer=None, device='cuda:0')
    assert model.nn_module.cfg['upscale'] == 4
    x = hr.seeded_input(2, 72, 104, LM_SEED + 1)
    pred = model.predict(x)
    assert pred.shape == (2, 57, 3) and pred.is_cuda
    logp = hr.forward(sd, x, cfg).numpy()
    assert _decode_gap(logp) >= 1e-3
    ref = od.keypoint_decode(logp, (540, 960))
    assert np.array_equal(pred.cpu().numpy()[..., :2], ref[..., :2])
    assert model.nn_module(x.to(cuda))[-1].shape == (2, 58, 72, 104)


def _decode_gap(logp):
    kp = logp[:, :-1]
    gap = np.inf
    for v in (kp.max(axis=2), kp.max(axis=3)):
        s = np.sort(v, axis=-1)
        gap = min(gap, float((s[..., -1] - s[..., -2]).min()))
    return gap


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp8'])
def test_workspace_of_64_frames_stays_within_c5s(sncal, cuda, dtype):
    """Query only.  The engines without a fused x4 head hold a concat and a hidden tensor of 784 channels at 540x960 per frame, so their
    frames per sub-batch are capped: 64 frames of 960x540 through hrnet_w48x4 must not ask for more workspace than the same engine asks
    for 64 frames of 1920x1080 through hrnet_w48 (config C5, which the suite runs)."""
    sizes = {}
    for name, H, W in (('hrnet_w48x4', 540, 960), ('hrnet_w48', 1080, 1920)):
        cfg = hr.load_config(name)
        net = _net(sncal, cuda, name, hr.seeded_state_dict(cfg, 2, 1.5), dtype)
        sizes[name] = net.workspace_bytes(64, H, W)
        sb = net.plan_tensor(0)['sub_batch']
        print(f'UPSCALE4-WORKSPACE {dtype} {name} 64 x {H}x{W}: {sizes[name] / 2 ** 30:.2f} GiB, sub-batch {sb}')
        assert net.output_size(H, W) == (540, 960)
        del net
    assert sizes['hrnet_w48x4'] <= sizes['hrnet_w48'], sizes


def test_workspace_query_of_64_frames_on_the_default_engine(sncal, cuda):
    """The fused head needs no cap: 64 frames of 960x540 stay one sub-batch, and neither a concat nor a hidden tensor is laid out."""
    cfg = hr.load_config('hrnet_w48x4')
    net = _net(sncal, cuda, 'hrnet_w48x4', hr.seeded_state_dict(cfg, 2, 1.5), sncal._lib.lib().sncal_x3_name().decode())
    n = net.workspace_bytes(64, 540, 960)
    print(f'UPSCALE4-WORKSPACE default engine 64 x 540x960: {n / 2 ** 30:.2f} GiB')
    assert n > 0 and net.plan_tensor(0)['sub_batch'] == 64
    hop = [o for o in net.plan_ops() if o['type'] == 'head'][0]
    assert hop['active']
    alive = [net.plan_tensor(t) for t in range(net._L.sncal_hrnet_plan_num_tensors(net._h))]
    assert not any(t['alive'] and t['C'] >= 784 and (t['H'], t['W']) == (540, 960) for t in alive)
