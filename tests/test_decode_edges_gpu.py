"""GPU: the heatmap decodes (csrc/decode.hip) on the inputs of tests/decode_cases.py -- every kp_decode_kernel<VEC, NQ> the dispatch can
launch, the tie rule where exp collapses distinct log-probabilities, the LDS size limit, the line decode around its exp shortcut, on
plateaus and on planes smaller than a workgroup, and all-tie planes through the fused decodes of the network.  Every comparison is bit for
bit against oracle/decode.py; tests/test_decode_cases_host.py shows on the CPU that each input tells a wrong kernel from a right one."""
import numpy as np
import pytest
import torch

import decode_cases as dc
from oracle import decode as od
from oracle import hrnet_ref as hr

pytestmark = pytest.mark.gpu


def _place(lp, cuda, aligned):
    """lp on the device: at an allocation's start (16-byte aligned), or as a contiguous view one float into a larger buffer."""
    if aligned:
        t = torch.from_numpy(lp).to(cuda)
    else:
        flat = torch.empty(lp.size + 4, dtype=torch.float32, device=cuda)
        t = flat[1:1 + lp.size].view(lp.shape)
        t.copy_(torch.from_numpy(lp))
    assert t.is_contiguous() and (t.data_ptr() % 16 == 0) == aligned
    return t


@pytest.mark.parametrize('w,aligned', dc.VARIANT_CASES)
def test_every_launch_variant(sncal, cuda, w, aligned):
    """Widths that reach all ten kp_decode_kernel instantiations (test_decode_cases_host.py checks the list against the dispatch rule),
    heights that leave waves without a row, two decode sizes: the maximum in the last / first row and column, an exact tie and an
    exp collision between lane group 0 and the last lane group in rows of different waves, an all -inf plane."""
    for h in dc.HEIGHTS:
        lp, _ = dc.variant_case(h, w, aligned)
        t = _place(lp, cuda, aligned)
        for size in dc.DECODE_SIZES:
            out = sncal.HRNetPredictionTransform(size)(t).cpu().numpy()
            ref = od.keypoint_decode(lp, size)
            assert np.array_equal(out, ref), (h, w, size, np.argwhere(out != ref)[:4], out[out != ref][:4], ref[out != ref][:4])


@pytest.mark.parametrize('hw', dc.BIG_OK)
def test_largest_admitted_shapes(sncal, cuda, hw):
    """(h + 5 w + 4) * 4 bytes of LDS per workgroup at its limit of 64 KiB: 6140 x 2048 (16-byte path, NQ 8) uses all of it, 8192 x 1637
    (scalar path, NQ 32) is the last width at the largest height.  Then the same plane with its only maximum in the last row and column."""
    h, w = hw
    lp = dc.big_case(h, w)
    t = torch.from_numpy(lp).to(cuda)
    dec = sncal.HRNetPredictionTransform((540, 960))
    out = dec(t).cpu().numpy()
    assert np.array_equal(out, od.keypoint_decode(lp, (540, 960)))
    assert out[0, 0, 2] == 1.0 and out[0, 0, 0] == np.float32(dc.BIG_FIRST[1] * 960) / np.float32(w)
    lp[0, 0, h - 1, w - 1] = dc.BIG_LAST
    t[0, 0, h - 1, w - 1] = dc.BIG_LAST
    out = dec(t).cpu().numpy()
    assert np.array_equal(out, od.keypoint_decode(lp, (540, 960)))
    assert out[0, 0, 0] == np.float32((w - 1) * 960) / np.float32(w) and out[0, 0, 1] == np.float32((h - 1) * 540) / np.float32(h)


@pytest.mark.parametrize('hw', dc.BIG_REFUSED)
def test_shapes_over_the_lds_limit_are_refused(sncal, cuda, hw):
    """One row / one column more: refused by the argument check (status -1 = SNCAL_ERR_ARG, the message names the shape and the bound),
    not sent to a launch that cannot be configured (that would be status -2, a HIP error string)."""
    h, w = hw
    t = torch.empty((1, 2, h, w), dtype=torch.float32, device=cuda)
    with pytest.raises(sncal._lib.SncalError) as e:
        sncal.HRNetPredictionTransform((540, 960))(t)
    msg = str(e.value)
    assert 'status -1:' in msg and f'{h}x{w}' in msg and str(dc.decode_lds_bytes(h, w)) in msg and '65536' in msg and 'LDS' in msg, msg
    assert 'hip' not in msg.lower()
    torch.cuda.synchronize()                                                    # nothing was launched: no error is pending either


def _line(sncal, cuda, heat, sigma, scale):
    out = sncal.EHMPredictionTransform(scale=scale, sigma=sigma)(torch.from_numpy(heat).to(cuda)).cpu().numpy()
    ref = od.line_decode(heat, float(sigma), float(scale))
    assert np.array_equal(out, ref), (heat.shape, sigma, scale, np.argwhere(out != ref)[:4], out[out != ref][:4], ref[out != ref][:4])
    return out


@pytest.mark.parametrize('which', ['below', 'above'])
def test_line_decode_around_the_exp_shortcut(sncal, cuda, which):
    """Three equal values per plane, sigma 3: at t = 16.06 the neighbour of the first peak is suppressed in its last bit and the far
    pixel wins; at t = 17.39 -- still below the kernel's cut at 17.5, where it computes the exp -- the keep factor is exactly 1.0f and the
    neighbour wins by its index."""
    heat, want = dc.line_shortcut_case(which)
    out = _line(sncal, cuda, heat, 3, 1).reshape(6, 2, 3)
    assert [(int(p[1, 1]), int(p[1, 0])) for p in out] == want
    _line(sncal, cuda, heat, 3, 4)


@pytest.mark.parametrize('sigma', [0.5, 3, 6, 50])
def test_line_decode_plateau(sncal, cuda, sigma):
    """About 2000 equal maxima per 135 x 240 plane: the first by flat index wins both times (better() / block_peak), at every sigma."""
    heat = dc.line_plateau()
    for scale in (1, 8):
        _line(sncal, cuda, heat, sigma, scale)


@pytest.mark.parametrize('hw', dc.LINE_SMALL_SHAPES)
def test_line_decode_small_planes(sncal, cuda, hw):
    """Planes below one workgroup (most threads see no pixel), w = 1, n = 256 and n % 256 != 0, quantised like the plateau case."""
    heat = dc.line_plateau((2, 3) + hw, seed=hw[0] * 100 + hw[1])
    for sigma in (0.5, 3):
        for scale in (1, 8):
            _line(sncal, cuda, heat, sigma, scale)


def test_line_decode_degenerate_planes(sncal, cuda):
    """All negative: both peaks are pixel 0 with value 0.  One positive pixel, first or last: the second peak is pixel 0 with value 0."""
    for heat in (dc.line_all_negative(), dc.line_single_pixel(False), dc.line_single_pixel(True)):
        for scale in (1, 8):
            _line(sncal, cuda, heat, 3, scale)


@pytest.mark.parametrize('cfg_name,hw,dtype', [('hrnet_w18', (64, 96), 'bf16'), ('hrnet_w18', (64, 96), 'fp16x3'), ('hrnet_w18', (64, 96), 'fp32'),
                                               ('hrnet_w48', (140, 240), 'bf16'), ('hrnet_w48', (140, 240), 'fp16x3')])
def test_ties_through_the_fused_decodes(sncal, cuda, cfg_name, hw, dtype):
    """A network whose logit planes are constant (decode_cases.tie_state_dict): every pixel of every channel ties, so the strips, tiles
    and partial maxima of the fused decodes (logsoftmax_rowcol + kp_finish; the decode-fused head epilogue + kp_finish) must all hand the
    first row and column through.  Fused and heatmap decode agree bit for bit, with each other and with the oracle on the heatmap."""
    cfg = hr.load_config(cfg_name)
    net = sncal.HRNetHeatmap(cfg_name, dtype=dtype, device=cuda)
    net.load_state_dict(dc.tie_state_dict(hr.seeded_state_dict(cfg, 7, 3.0)))
    x = hr.seeded_input(2, hw[0], hw[1], 11).to(cuda)
    net.set_profiling(True)
    _, k_fused = net.forward(x, want_heat=False, decode_size=(540, 960))
    kernels = {p['kernel'] for p in net.get_profile()}
    assert 'softmax_nchw' not in kernels
    if cfg_name == 'hrnet_w48':
        assert 'kp_finish' in kernels and 'logsoftmax_decode_fused' not in kernels      # the head kernel did the first half
    else:
        assert 'logsoftmax_decode_fused' in kernels
    net.set_profiling(False)
    heat, k_fwd = net.forward(x, want_heat=True, decode_size=(540, 960))
    k_heat = sncal.HRNetPredictionTransform((540, 960))(heat)
    assert torch.equal(k_fwd, k_heat)
    heat_np = heat.cpu().numpy()
    assert all(np.unique(heat_np[b, c]).size == 1 for b in range(heat_np.shape[0]) for c in range(heat_np.shape[1])), 'a logit plane is not constant'
    for k in (k_fused, k_heat):
        assert k.shape == (2, heat_np.shape[1] - 1, 3) and not k[..., :2].any(), k[..., :2].nonzero()[:4]
    assert torch.equal(k_fused.view(torch.int32), k_heat.view(torch.int32))
    ref = od.keypoint_decode(heat_np, (540, 960))
    assert np.array_equal(k_fused.cpu().numpy(), ref) and np.array_equal(k_heat.cpu().numpy(), ref)
    assert np.unique(ref[..., 2]).size > 2                                       # the channels differ: conf is not one constant
