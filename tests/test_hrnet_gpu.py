"""GPU: the HIP HRNet engine (through sncal_hrnet_* in libsncal.so) vs goldens captured from the reference.

Tolerances (stated per the north star: fp32 tolerance, bit-identical indices):
  fp32 path : |logp - ref| <= 2e-4 absolute on log-probabilities of magnitude <= ~50 (accumulation order
              and BN folding differ from the reference's conv->BN sequence); keypoint indices identical.
  bf16 path : |logp - ref| <= 0.6, index agreement >= 85 % on these random-weight (weakly peaked) heatmaps
              -- reported, not bit-exact: bf16 rounding (2^-8 relative) exceeds the top-1/top-2 gaps.
"""
import os

import numpy as np
import pytest
import torch

from oracle import decode as od
from oracle import hrnet_ref as hr

pytestmark = pytest.mark.gpu


def _run(sncal, cuda, gold_dir, name, cfgn, dtype, line=False):
    g = np.load(os.path.join(gold_dir, name + '.npz'))
    cfg = hr.load_config(cfgn)
    sd = hr.seeded_state_dict(cfg, int(g['seed']), float(g['head_gain']))
    x = hr.seeded_input(int(g['batch']), int(g['hw'][0]), int(g['hw'][1]), int(g['seed']) + 1)
    net = sncal.HRNetHeatmap(cfgn, dtype=dtype, device=cuda)
    net.load_state_dict(sd)
    heat, kp = net.forward(x.to(cuda), want_heat=True, decode_size=None if line else (540, 960))
    return g, heat.cpu().numpy(), None if kp is None else kp.cpu().numpy()


def _err(g, heat):
    if 'out' in g:
        return np.abs(heat - g['out']).max()
    return np.abs(heat[:, :, ::16, ::16] - g['out_strided']).max()


@pytest.mark.parametrize('name,cfgn', [('hrnet_w18_64x96', 'hrnet_w18'), ('hrnet_w18_135x240', 'hrnet_w18'),
                                       ('hrnet_w48_540x960', 'hrnet_w48')])
def test_keypoint_net_fp32_matches_reference(sncal, cuda, gold_dir, name, cfgn):
    g, heat, kp = _run(sncal, cuda, gold_dir, name, cfgn, 'fp32')
    assert np.isfinite(heat[np.isfinite(heat)]).all()
    assert _err(g, heat) <= 2e-4
    assert np.array_equal(kp[..., :2], g['decode'][..., :2])              # bit-identical keypoint indices
    assert np.abs(kp[..., 2] - g['decode'][..., 2]).max() <= 1e-5
    assert np.array_equal(kp, od.keypoint_decode(heat, (540, 960)))       # fused decode == oracle decode


def test_keypoint_net_fp16x3_matches_reference_at_the_fp32_tolerance(sncal, cuda, gold_dir):
    """The fp32-class engine (fp32 tensors, every product as hi.hi + hi.lo + lo.hi of fp16 splits on the matrix pipe) against the SAME
    reference capture as the exact-fp32 engine AT ITS TOLERANCE: bit-identical indices, log-probabilities (down to -52) to 2e-4 (confidences to 1.5e-5).
    Measured on this golden: exact-fp32 engine 4.6e-5 max / 8.7e-6 mean (confidences 3.4e-6); fp16x3 1.3e-4 / 2.6e-5 (confidences
    6.3e-6); the same engine built on bf16 splits (round 3's bf16x3, -DSNCAL_X3_F16=0): 4.3e-4 / 9.0e-5 (1.0e-5) -- tools/dev/golden_err.py."""
    g, heat, kp = _run(sncal, cuda, gold_dir, 'hrnet_w48_540x960', 'hrnet_w48', 'fp16x3')
    tight = sncal._lib.lib().sncal_x3_name() == b'fp16x3'
    assert _err(g, heat) <= (2e-4 if tight else 6e-4)                     # 2e-4 = test_keypoint_net_fp32_matches_reference's bound
    assert np.array_equal(kp[..., :2], g['decode'][..., :2])
    assert np.abs(kp[..., 2] - g['decode'][..., 2]).max() <= (1.5e-5 if tight else 3e-5)
    assert np.array_equal(kp, od.keypoint_decode(heat, (540, 960)))


def test_line_net_fp16x3_matches_reference_at_the_fp32_tolerance(sncal, cuda, gold_dir):
    """Line net on the fp32-class engine: heatmaps to the exact-fp32 engine's 2e-5 of the reference capture (measured 1.5e-5; exact-fp32 engine 4.9e-6;
    bf16 splits 3.8e-5), EHM decode indices identical."""
    g, heat, _ = _run(sncal, cuda, gold_dir, 'line_w48_540x960', 'line_hrnet_w48', 'fp16x3', line=True)
    assert _err(g, heat) <= (2e-5 if sncal._lib.lib().sncal_x3_name() == b'fp16x3' else 1e-4)        # 2e-5 = test_line_net_matches_reference[fp32]
    dec = sncal.EHMPredictionTransform(scale=4, sigma=3)(torch.from_numpy(heat).to(cuda)).cpu().numpy()
    assert np.array_equal(dec[..., :2], g['decode'][..., :2])


@pytest.mark.parametrize('name,cfgn', [('hrnet_w18_64x96', 'hrnet_w18'), ('hrnet_w48_540x960', 'hrnet_w48')])
def test_keypoint_net_bf16_close_to_reference(sncal, cuda, gold_dir, name, cfgn):
    g, heat, kp = _run(sncal, cuda, gold_dir, name, cfgn, 'bf16')
    assert _err(g, heat) <= 0.6
    agree = (kp[..., :2] == g['decode'][..., :2]).all(-1).mean()
    assert agree >= 0.85, agree
    assert np.array_equal(kp, od.keypoint_decode(heat, (540, 960)))


@pytest.mark.parametrize('name,cfgn', [('line_w18_64x96', 'line_hrnet_w18'), ('line_w48_540x960', 'line_hrnet_w48')])
@pytest.mark.parametrize('dtype,tol', [('fp32', 2e-5), ('bf16', 6e-2)])
def test_line_net_matches_reference(sncal, cuda, gold_dir, name, cfgn, dtype, tol):
    g, heat, _ = _run(sncal, cuda, gold_dir, name, cfgn, dtype, line=True)
    assert _err(g, heat) <= tol
    assert np.abs(heat.sum(1) - 1).max() < 1e-4                          # softmax head
    if dtype == 'fp32':
        dec = sncal.EHMPredictionTransform(scale=4, sigma=3)(torch.from_numpy(heat).to(cuda)).cpu().numpy()
        assert np.array_equal(dec[..., :2], g['decode'][..., :2])


@pytest.mark.parametrize('dtype', ['bf16', 'fp16x3'])
def test_batch_and_subbatch_consistency(sncal, cuda, dtype):
    """Frames are independent: a batch of 11 (sub-batches 8 + 3) equals per-frame results bit-for-bit."""
    cfg = hr.load_config('hrnet_w18')
    sd = hr.seeded_state_dict(cfg, 9, 4.0)
    net = sncal.HRNetHeatmap('hrnet_w18', dtype=dtype, device=cuda)
    net.load_state_dict(sd)
    x = hr.seeded_input(11, 64, 96, 10).to(cuda)
    heat, kp = net.forward(x, want_heat=True, decode_size=(540, 960))
    for i in (0, 7, 8, 10):
        h1, k1 = net.forward(x[i:i + 1].contiguous(), want_heat=True, decode_size=(540, 960))
        assert torch.equal(h1[0], heat[i]) and torch.equal(k1[0], kp[i])


def test_odd_input_size_stem_interpolation(sncal, cuda):
    """480x270 input: branch-0 is 68x120 -> head 136x240 while the stem is 135x240, so the stem is
    bilinearly resized (hrnet.py:495-498).  Compared with the torch oracle run on the GPU box's CPU."""
    cfg = hr.load_config('hrnet_w18')
    sd = hr.seeded_state_dict(cfg, 21, 4.0)
    x = hr.seeded_input(1, 270, 480, 22)
    ref = hr.forward(sd, x, cfg).numpy()
    net = sncal.HRNetHeatmap('hrnet_w18', dtype='fp32', device=cuda)
    net.load_state_dict(sd)
    heat, _ = net.forward(x.to(cuda))
    assert heat.shape == (1, 58, 136, 240)
    assert np.abs(heat.cpu().numpy() - ref).max() <= 2e-4


def _width_family_against_the_oracle(sncal, cuda, name, cfg, seed):
    """One width family of tests/width_cases.py, 2 frames of 72x104 (head 36x52), every engine against hr.forward on the CPU: the bounds of
    this file (fp32-class engines 2e-4 on the log-probabilities, bf16 0.6) and the decoded keypoints = the oracle decode of the engine's own
    heat.  Returns {engine: max |logp - ref|}."""
    sd = hr.seeded_state_dict(cfg, seed, 4.0)
    x = hr.seeded_input(2, 72, 104, seed + 1)
    ref = hr.forward(sd, x, cfg).numpy()
    assert ref.shape == (2, 58, 36, 52) and np.isfinite(ref).all()
    errs = {}
    for dtype, tol in (('fp32', 2e-4), ('fp16x3', 2e-4), ('bf16', 0.6)):
        net = sncal.HRNetHeatmap(cfg, dtype=dtype, device=cuda)
        net.load_state_dict(sd)
        heat, kp = net.forward(x.to(cuda), want_heat=True, decode_size=(540, 960))
        heat, kp = heat.cpu().numpy(), kp.cpu().numpy()
        errs[dtype] = float(np.abs(heat - ref).max())
        print(f'WIDTH-ORACLE {name} {dtype}: max |logp - oracle| {errs[dtype]:.3e} (bound {tol:g}), oracle range {ref.min():.2f} .. {ref.max():.2f}')
        assert errs[dtype] <= tol, (name, dtype, errs[dtype])
        assert np.array_equal(kp, od.keypoint_decode(heat, (540, 960))), (name, dtype)
        del net
    return errs


@pytest.mark.parametrize('name', ['W64', 'P64', 'Q64', 'M96'])
def test_width_families_match_the_oracle(sncal, cuda, name):
    """Branch widths beyond W18 / W32 / W48 at reduced depth (one module per stage, one BasicBlock per branch; tests/width_cases.py), whole
    network against the CPU oracle.  tests/test_width_kernels_gpu.py checks the same networks launch by launch; here the launches are chained.
    Measured max |logp - oracle| on an MI355X (fp32 / fp16x3 / bf16), log-probabilities of about -12 .. -0.5:
        W64  7.6e-6 / 8.6e-6 / 0.033
        P64  7.6e-6 / 1.0e-5 / 0.050
        Q64  1.1e-5 / 1.9e-5 / 0.048
        M96  1.4e-5 / 2.1e-5 / 0.064"""
    import width_cases as wc
    _width_family_against_the_oracle(sncal, cuda, name, wc.reduced(name), {'W64': 41, 'P64': 43, 'Q64': 45, 'M96': 47}[name])


def test_w64_at_the_reference_depth_matches_the_oracle(sncal, cuda):
    """64 / 128 / 256 / 512 at the depth of the reference's own families (stage1 of 4 blocks, modules 1 / 4 / 3, 4 blocks per branch: 117 M
    weights, three engines loaded one after the other -- the time of this test is its weight packing and upload).
    Measured max |logp - oracle| on an MI355X (fp32 / fp16x3 / bf16): 7.2e-5 / 1.98e-4 / 0.43 on log-probabilities down to -48 (the fp16x3 figure is the
    engine's drift over 300 layers against a bound of 2e-4: deterministic inputs, no margin to give away; the CPU oracle's own fp32 run is 4.0e-5
    from a float64 run of the same oracle, and does not move with the thread count)"""
    import width_cases as wc
    _width_family_against_the_oracle(sncal, cuda, 'W64 full depth', wc.reference_depth('W64'), 51)


@pytest.mark.parametrize('name,dtype', [('P64', 'fp16x3'), ('M96', 'bf16')])
def test_width_families_frames_are_independent(sncal, cuda, name, dtype):
    """A batch of 5 frames equals each frame run alone, bit for bit (as test_batch_and_subbatch_consistency): the partial last 64-channel
    blocks of P64 on the split engine, the 3- and 5-block launches of M96 on bf16 -- stacked frames share tiles, never values."""
    import width_cases as wc
    cfg = wc.reduced(name)
    net = sncal.HRNetHeatmap(cfg, dtype=dtype, device=cuda)
    net.load_state_dict(hr.seeded_state_dict(cfg, 61, 4.0))
    x = hr.seeded_input(5, 72, 104, 62).to(cuda)
    heat, kp = net.forward(x, want_heat=True, decode_size=(540, 960))
    heat, kp = heat.clone(), kp.clone()
    assert torch.isfinite(heat).all()
    for i in range(5):
        h1, k1 = net.forward(x[i:i + 1].contiguous(), want_heat=True, decode_size=(540, 960))
        assert torch.equal(h1[0], heat[i]) and torch.equal(k1[0], kp[i]), i


def test_load_model_predict_surface(sncal, cuda, tmp_path):
    """argus-style checkpoint dict -> load_model(...).predict(x) -> (B,57,3) on the device (D2)."""
    cfg = hr.load_config('hrnet_w18')
    sd = hr.seeded_state_dict(cfg, 5, 4.0)
    ck = {'model_name': 'HRNetMetaModel',
          'params': {'nn_module': {'hrnet_config': cfg, 'num_refinement_stages': 0, 'num_heatmaps': 58},
                     'prediction_transform': {'size': [540, 960]}, 'device': 'cuda:0'},
          'nn_state_dict': sd}
    path = str(tmp_path / 'model.pth')
    torch.save(ck, path)
    model = sncal.load_model(path, loss=None, optimizer=None, device='cuda:0', dtype='fp32')
    x = hr.seeded_input(2, 135, 240, 6)
    pred = model.predict(x)
    assert pred.shape == (2, 57, 3) and pred.is_cuda
    ref = od.keypoint_decode(hr.forward(sd, x, cfg).numpy(), (540, 960))
    assert np.array_equal(pred.cpu().numpy()[..., :2], ref[..., :2])
    assert np.array_equal(model.nn_module(x.to(cuda))[-1].shape, (2, 58, 68, 120))
    # the drop-in default (no dtype): the fp32-class engine of the build, the one bench.py measures -- same indices, same surface
    model_d = sncal.load_model(path, loss=None, optimizer=None, device='cuda:0')
    assert model_d.nn_module.dtype_name == sncal._lib.lib().sncal_x3_name().decode()
    pred_d = model_d.predict(x)
    assert np.array_equal(pred_d.cpu().numpy()[..., :2], ref[..., :2])
    assert np.abs(pred_d.cpu().numpy()[..., 2] - ref[..., 2]).max() <= 2e-5


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_uint8_frames_equal_totensor_frames(sncal, cuda, dtype):
    """sncal_hrnet_forward_u8 on cv2-style (B,H,W,3) uint8 frames == sncal_hrnet_forward on torchvision ToTensor's
    output of the same frames (make_submit.py:62-66: permute to CHW, float32, divide by 255): bit-identical."""
    cfg = hr.load_config('hrnet_w18')
    net = sncal.HRNetHeatmap('hrnet_w18', dtype=dtype, device=cuda)
    net.load_state_dict(hr.seeded_state_dict(cfg, 3, 4.0))
    gen = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (3, 64, 96, 3), dtype=torch.uint8, generator=gen)
    as_totensor = frames.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    h8, k8 = net.forward(frames.to(cuda), want_heat=True, decode_size=(540, 960))
    hf, kf = net.forward(as_totensor.to(cuda), want_heat=True, decode_size=(540, 960))
    assert torch.equal(h8, hf) and torch.equal(k8, kf)


def test_fused_basicblock_is_bit_identical_to_two_convs(sncal, cuda, monkeypatch):
    """bblock.hip (conv1+BN+ReLU+conv2+BN+residual+ReLU of the 48-channel branch in one kernel) keeps the MFMA
    order and the bf16 rounding of the intermediate, so the whole bf16 network output must not change by one bit
    (odd sizes: tiles are 12x14, the image is 135x240 at the branch)."""
    cfg = hr.load_config('hrnet_w48')
    sd = hr.seeded_state_dict(cfg, 2, 1.5)
    x = hr.seeded_input(2, 540, 960, 9).to(cuda)
    outs = []
    for flag in ('1', '0'):
        monkeypatch.setenv('SNCAL_FUSE_BBLOCK', flag)
        net = sncal.HRNetHeatmap('hrnet_w48', dtype='bf16', device=cuda)
        net.load_state_dict(sd)
        net.set_profiling(True)
        heat, _ = net.forward(x, want_heat=True)
        kernels = {p['kernel'] for p in net.get_profile()}
        assert ('bblock48_fused' in kernels) == (flag == '1')
        outs.append(heat.clone())
    assert torch.equal(outs[0], outs[1])


def _fused_decode_case(sncal, cuda, cfg_name, hw, dtype):
    cfg = hr.load_config(cfg_name)
    net = sncal.HRNetHeatmap(cfg_name, dtype=dtype, device=cuda)
    net.load_state_dict(hr.seeded_state_dict(cfg, 7, 3.0))
    x = hr.seeded_input(3, hw[0], hw[1], 11).to(cuda)
    net.set_profiling(True)
    _, k_fused = net.forward(x, want_heat=False, decode_size=(540, 960))
    kernels = {p['kernel'] for p in net.get_profile()}
    assert ('logsoftmax_decode_fused' in kernels or 'kp_finish' in kernels) and 'softmax_nchw' not in kernels
    if cfg_name == 'hrnet_w48' and (hw[0] >= 540 or hw == (140, 240)):
        assert 'kp_finish' in kernels and 'logsoftmax_decode_fused' not in kernels      # the head kernel did the first half
    net.set_profiling(False)
    heat, k_heat = net.forward(x, want_heat=True, decode_size=(540, 960))
    assert torch.equal(k_fused, k_heat)
    ref = od.keypoint_decode(heat.cpu().numpy(), (540, 960))
    assert np.array_equal(k_fused.cpu().numpy()[..., :2], ref[..., :2])


@pytest.mark.parametrize('cfg_name,hw', [('hrnet_w18', (64, 96)), ('hrnet_w18', (135, 240)), ('hrnet_w48', (540, 960)), ('hrnet_w48', (1080, 1920)),
                                         ('hrnet_w48', (270, 500)), ('hrnet_w48', (140, 240))])
def test_fused_logsoftmax_decode_is_bit_identical(sncal, cuda, cfg_name, hw):
    """predict() without the heatmap runs log-softmax + keypoint decode fused: inside the head kernel where head32.hip applies
    (W48 at 540x960: neither logits nor the (B,58,h,w) tensor are written, `kp_finish` reduces the tiles' maxima), as
    logsoftmax_rowcol + kp_finish on the logits otherwise (decode.hip).  Same per-pixel arithmetic (softmax_px.hpp) and exact
    maxima, so the keypoints must equal, bit for bit, those decoded from the heatmap the unfused path writes -- including
    sizes that are not multiples of the tiles or the 18-row strip (140x240: a 70x120 head, partial 4 x 32 tiles in both directions)."""
    _fused_decode_case(sncal, cuda, cfg_name, hw, 'bf16')


@pytest.mark.parametrize('hw', [(540, 960), (1080, 1920), (270, 500), (140, 240)])
def test_fused_logsoftmax_decode_is_bit_identical_fp16x3(sncal, cuda, hw):
    """The same on the fp16x3 engine: headx3.hip includes the same decode-fused epilogue (head_frame.hpp) as head32.hip."""
    _fused_decode_case(sncal, cuda, 'hrnet_w48', hw, 'fp16x3')


def test_grouped_branch_convs_are_bit_identical(sncal, cuda, monkeypatch):
    """The same-depth 3x3 convs of branches 1..3 share one grouped launch (conv.hpp conv_group_kernel; plan emitted
    depth-major, workspace lifetimes widened to the group).  Same code per work item: the bf16 network output must not
    change by one bit against the one-launch-per-conv plan, and the launch count of the dominant variant drops."""
    cfg = hr.load_config('hrnet_w48')
    sd = hr.seeded_state_dict(cfg, 2, 1.5)
    x = hr.seeded_input(2, 540, 960, 9).to(cuda)
    outs, launches = [], []
    monkeypatch.setenv('SNCAL_CONV_TT', '0')       # the generic kernel's grouping (the two-team kernel has its own test below)
    for flag in ('1', '0'):
        monkeypatch.setenv('SNCAL_GROUP_CONVS', flag)
        net = sncal.HRNetHeatmap('hrnet_w48', dtype='bf16', device=cuda)
        net.load_state_dict(sd)
        net.set_profiling(True)
        heat, _ = net.forward(x, want_heat=True)
        prof = {p['kernel']: p for p in net.get_profile()}
        launches.append(prof['conv<bf16,k3,s1,NI3,MI6,G4>']['launches'])
        outs.append(heat.clone())
        flops = sum(p['flops'] for p in prof.values())
        assert abs(flops / (2 * 2 * 253910384640) - 1) < 0.3          # accounting still covers every conv (2 frames; fused head counts fewer)
    assert torch.equal(outs[0], outs[1])
    assert launches[0] < launches[1], launches


@pytest.mark.parametrize('hw,batch', [((540, 960), 3), ((270, 480), 5), ((1080, 1920), 1)])
def test_two_team_conv_kernel_matches_the_generic_kernel(sncal, cuda, monkeypatch, hw, batch):
    """conv_tt.hip (wide 3x3 stride-1 convolutions: two teams of four waves alternate LDS-DMA and MFMA phases, frames
    stacked with a shared zero row, swizzled halo image, v_mfma_f32_32x32x16_bf16) against the generic kernel
    (v_mfma_f32_16x16x32_bf16) on the whole bf16 network.  Same operands, same fp32 accumulation, but the matrix unit sums
    the products of one output in a different order: outputs agree to accumulator rounding, which the ~300 bf16 layers
    turn into occasional one-ulp flips -- a few 1e-2 in log-probability at worst, far inside the bf16 engine's distance
    from the fp32 engine (tests/test_parity_gpu.py).  [The first version of the kernel used the 16x16x32 shape and was
    bit-identical to the generic kernel on these very cases: tiling, stacking and swizzle are exact.]
    Batches > 1 put frame boundaries inside tiles; the odd sizes (135/68/34/17 rows, 9x15 at 270x480) exercise partial tiles."""
    cfg = hr.load_config('hrnet_w48')
    sd = hr.seeded_state_dict(cfg, 2, 1.5)
    x = hr.seeded_input(batch, hw[0], hw[1], 9).to(cuda)
    outs, kps = [], []
    for flag in ('1', '0'):
        monkeypatch.setenv('SNCAL_CONV_TT', flag)
        net = sncal.HRNetHeatmap('hrnet_w48', dtype='bf16', device=cuda)
        net.load_state_dict(sd)
        net.set_profiling(True)
        heat, kp = net.forward(x, want_heat=True, decode_size=(540, 960))
        prof = {p['kernel']: p for p in net.get_profile()}
        assert ('conv_tt<bf16,k3,s1,8x32x96>' in prof) == (flag == '1'), sorted(prof)
        assert ('conv<bf16,k3,s1,NI3,MI6,G4>' in prof) == (flag == '0'), sorted(prof)
        outs.append(heat.clone())
        kps.append(kp.clone())
    assert torch.isfinite(outs[0]).all()
    d = (outs[0] - outs[1]).abs()
    assert float(d.max()) <= 0.25 and float(d.mean()) <= 0.01, (float(d.max()), float(d.mean()))
    assert float((kps[0][..., :2] == kps[1][..., :2]).all(-1).float().mean()) >= 0.9


@pytest.mark.parametrize('dtype', ['bf16', 'fp16x3'])
def test_frames_are_independent_of_batch_size_and_position(sncal, cuda, dtype):
    """Size-independent property at the bench configuration (W48, 960x540, both fast engines): a frame's keypoints and heatmap do not
    depend on the batch it travels in -- different batch sizes pick different tile shapes, grid orders and grouped
    launches, and a 67-frame batch crosses the 64-frame sub-batch boundary -- because every output element is accumulated
    in a fixed order."""
    cfg = hr.load_config('hrnet_w48')
    net = sncal.HRNetHeatmap('hrnet_w48', dtype=dtype, device=cuda)
    net.load_state_dict(hr.seeded_state_dict(cfg, 1, 1.5))
    x = torch.rand((67, 3, 540, 960), device=cuda, generator=torch.Generator(device=cuda).manual_seed(3))
    _, k_all = net.forward(x, want_heat=False, decode_size=(540, 960))
    k_all = k_all.clone()
    for lo, hi in ((0, 1), (1, 4), (60, 67), (10, 41)):
        _, k = net.forward(x[lo:hi].contiguous(), want_heat=False, decode_size=(540, 960))
        assert torch.equal(k, k_all[lo:hi]), (lo, hi)
    h3, _ = net.forward(x[:3].contiguous(), want_heat=True)
    h2, _ = net.forward(x[:2].contiguous(), want_heat=True)
    assert torch.equal(h3[:2], h2)


def test_load_model_ehm_checkpoint_without_head_key(sncal, cuda, tmp_path, gold_dir):
    """A genuine EHMMetaModel checkpoint: params.nn_module.hrnet_config is the line yaml, which has NO 'head' and NO
    'upscale' key (src/models/line/model_config/hrnet_w48.yaml) -- the Softmax head is hard-coded in the model class
    (src/models/line/hrnet.py:101).  load_model must build the softmax / stride-4 network from the class, not from the
    yaml; checked against the reference-captured line golden and through predict()'s two-peak decode."""
    g = np.load(os.path.join(gold_dir, 'line_w18_64x96.npz'))
    cfg = hr.load_config('line_hrnet_w18')
    bare = {k: v for k, v in cfg.items() if k not in ('head', 'upscale')}
    sd = hr.seeded_state_dict(cfg, int(g['seed']), float(g['head_gain']))
    x = hr.seeded_input(int(g['batch']), int(g['hw'][0]), int(g['hw'][1]), int(g['seed']) + 1)
    ck = {'model_name': 'EHMMetaModel',
          'params': {'nn_module': {'hrnet_config': bare, 'num_refinement_stages': 0, 'num_heatmaps': 23},
                     'prediction_transform': {'scale': 4, 'sigma': 6}, 'device': 'cuda:0'},
          'nn_state_dict': sd}
    path = str(tmp_path / 'line.pth')
    torch.save(ck, path)
    model = sncal.load_model(path, loss=None, optimizer=None, device='cuda:0', dtype='fp32')
    assert type(model).__name__ == 'EHMMetaModel'
    assert model.nn_module.cfg['head'] == 'softmax' and model.nn_module.cfg['upscale'] == 1
    heat = model.nn_module(x.to(cuda))[-1]
    assert np.abs(heat.cpu().numpy() - g['out']).max() <= 2e-5
    s = heat.sum(dim=1)
    assert torch.allclose(s, torch.ones_like(s), atol=1e-5)           # a softmax head, not log-softmax
    pred = model.predict(x)
    assert pred.shape == (x.shape[0], 23, 2, 3)
    assert np.array_equal(pred.cpu().numpy()[..., :2], od.line_decode(g['out'], 6.0, 4.0)[..., :2])
    assert float(pred[..., 2].max()) > 0.0                            # the bug this pins returned p = 0 everywhere


def test_ticket_dealt_kernels_give_the_same_bytes_beside_a_busy_side_stream(sncal, cuda):
    """The layer1 seam kernel and the fused 48-channel block take their work from ticket counters (bneckx3.hip, bblockx3.hip): a
    workgroup whose CU another stream holds starts late and takes fewer tickets.  Which workgroup computes a tile must not show in
    the result: the same forward alone and beside a side stream that keeps CUs busy (large workgroups with all of a CU's LDS, as the
    camera solves hold whole CUs in production), byte for byte, several times (the counters re-arm themselves between launches)."""
    cfg = hr.load_config('hrnet_w48')
    net = sncal.HRNetHeatmap('hrnet_w48', dtype='fp16x3', device=cuda)
    net.load_state_dict(hr.seeded_state_dict(cfg, 21, 4.0))
    x = hr.seeded_input(6, 270, 480, 22).to(cuda)
    heat0, kp0 = net.forward(x, want_heat=True, decode_size=(540, 960))
    heat0, kp0 = heat0.clone(), kp0.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    a = torch.randn((6144, 6144), device=cuda)
    for rep in range(3):
        with torch.cuda.stream(side):
            for _ in range(6 + 4 * rep):
                a = torch.tanh(a @ a * 1e-4)             # ~ms-long GEMMs with CU-filling workgroups, back to back
        heat, kp = net.forward(x, want_heat=True, decode_size=(540, 960))
        torch.cuda.synchronize()
        assert torch.equal(heat, heat0) and torch.equal(kp, kp0), rep


def test_fused_block_in_several_launches_gives_the_same_bytes(sncal, cuda, monkeypatch):
    """bblockx3 addresses one launch's tensors with 32-bit buffer offsets; a sub-batch whose tensors exceed them goes out as several launches
    over frame ranges (launch_bblockx3).  No shipped configuration reaches the limit (64 frames of 1920x1080 are 1.6 GB per tensor), so the
    path is driven here through the launcher's test hook: with the limit at three frames' worth of bytes a 7-frame forward runs every fused
    block as 3 + 3 + 1 frames, and must return the one-launch result byte for byte (tiles of the stacked frames differ between the two)."""
    cfg = hr.load_config('hrnet_w48')
    net = sncal.HRNetHeatmap('hrnet_w48', dtype='fp16x3', device=cuda)
    net.load_state_dict(hr.seeded_state_dict(cfg, 31, 4.0))
    x = hr.seeded_input(7, 270, 480, 32).to(cuda)
    heat0, kp0 = net.forward(x, want_heat=True, decode_size=(540, 960))
    heat0, kp0 = heat0.clone(), kp0.clone()
    monkeypatch.setenv('SNCAL_BBX_MAX_BYTES', str(3 * 68 * 120 * 192 + 1000))      # (the 48-channel branch of a 270x480 input: 68 x 120 x 192 B per frame)
    heat, kp = net.forward(x, want_heat=True, decode_size=(540, 960))
    assert torch.equal(heat, heat0) and torch.equal(kp, kp0)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16x3'])
def test_persistent_kernels_rearm_between_forwards(sncal, cuda, dtype):
    """The persistent kernels draw their work from ticket words that the last workgroup (wave, for the layer1 seam) to leave zeroes for
    the next launch on the stream (ticket_leave, persist.hpp; conv_tt's per-XCD form).  A re-arm that fails shows only in the SECOND
    launch, which then starts from used tickets and skips or repeats tiles: three forwards of one batch on one handle and stream must
    give the same bytes, and so must a fourth with profiling on, whose rows show that the fused BasicBlock, the two-team convolution
    and (split engine) the seam kernel did run, not a fallback path.  Three frames of 64x96: the 48-channel branch is 16x24, 2x2 tiles
    of 16x14 with partial columns per frame in the bf16 kernel, and in the split engine's stack of 3 x 17 rows tiles that straddle
    frames."""
    cfg = hr.load_config('hrnet_w48')
    net = sncal.HRNetHeatmap('hrnet_w48', dtype=dtype, device=cuda)
    net.load_state_dict(hr.seeded_state_dict(cfg, 41, 4.0))
    x = hr.seeded_input(3, 64, 96, 42).to(cuda)
    outs = []
    for rep in range(4):
        if rep == 3:
            net.set_profiling(True)
        heat, kp = net.forward(x, want_heat=True, decode_size=(540, 960))
        outs.append((heat.clone(), kp.clone()))
    for rep in (1, 2, 3):
        assert torch.equal(outs[rep][0], outs[0][0]) and torch.equal(outs[rep][1], outs[0][1]), rep
    assert float(outs[0][0].abs().max()) > 0.0
    kernels = {p['kernel'] for p in net.get_profile()}
    assert ('bblock48_fused' if dtype == 'bf16' else 'bblockx3_fused') in kernels, kernels
    assert any(k.startswith('conv_tt<' + dtype + ',') for k in kernels), kernels
    if dtype != 'bf16':
        assert 'bneck_seam_x3' in kernels, kernels
