"""CPU: the inputs of tests/test_decode_edges_gpu.py (tests/decode_cases.py) discriminate -- shown with the oracle alone (oracle/decode.py,
pinned to the reference by the goldens): the width list reaches every kp_decode_kernel instantiation, the collision planes separate
"first occurrence after exp" from the argmax of the log-probabilities, the two shortcut cases lie on either side of the point from which
the line decode's keep factor is exactly 1.0f, and the plateau planes hold enough equal maxima."""
import numpy as np
import pytest

import decode_cases as dc
from oracle import decode as od
from oracle import hrnet_ref as hr


def test_width_list_reaches_all_ten_instantiations():
    got = {dc.plan(w, aligned) for (w, aligned) in dc.VARIANT_CASES}
    assert got == dc.ALL_VARIANTS and len(got) == 10
    # the buckets by hand: nvec = w / 4 or w, NQ = ceil(nvec / 64) rounded up to 1, 2, 4, 8, 16, 32
    assert [dc.plan(w, True) for w in dc.VEC4_WIDTHS] == [(4, 1), (4, 2), (4, 2), (4, 4), (4, 4), (4, 8), (4, 8)]
    assert [dc.plan(w, True) for w in dc.SCALAR_WIDTHS] == [(1, 2), (1, 2), (1, 4), (1, 4), (1, 8), (1, 8), (1, 16), (1, 16), (1, 32), (1, 32)]
    assert [dc.plan(w, False) for w in dc.OFFSET_WIDTHS] == [(1, 1), (1, 2), (1, 16), (1, 32)]
    assert all(w % 4 == 0 for w in dc.VEC4_WIDTHS + dc.OFFSET_WIDTHS) and all(w % 4 for w in dc.SCALAR_WIDTHS)
    # the widths the older tests use (tests/test_decode_gpu.py and the goldens) reach four
    assert {dc.plan(w, True) for w in (480, 240, 30, 960, 61, 3, 120, 60)} == {(4, 1), (4, 2), (4, 4), (1, 1)}
    with pytest.raises(ValueError):
        dc.plan(2052, True)


def test_size_limit_cases_sit_on_the_bound():
    assert [dc.decode_lds_bytes(h, w) for (h, w) in dc.BIG_OK] == [65536, 65524]
    assert all(dc.decode_lds_bytes(h, w) <= dc.LDS_MAX for (h, w) in dc.BIG_OK)
    assert all(dc.decode_lds_bytes(h, w) > dc.LDS_MAX and h <= 8192 and w <= 2048 for (h, w) in dc.BIG_REFUSED)
    assert dc.decode_lds_bytes(8192, 1636) <= dc.LDS_MAX                      # 1637 is the last width at h = 8192, 6140 the last height at 2048
    assert [dc.plan(w, True) for (_, w) in dc.BIG_OK] == [(4, 8), (1, 32)]
    assert dc.decode_lds_bytes(8192, 2048) == 73744                           # what the old check admitted


def test_collision_case_separates_exp_order_from_logp_order():
    assert od.exp_ref(np.float32([-1e-9, -3e-9])).tolist() == [1.0, 1.0]
    p = dc.collision_plane(5, 300, (1, 10), (3, 290))
    lp = np.stack([p, np.full_like(p, -1.0)])[None]
    x, y = od.keypoint_decode_indices(lp)
    assert (int(x[0, 0]), int(y[0, 0])) == (10, 1)
    assert dc.raw_argmax_xy(p) == (290, 3)
    out = od.keypoint_decode(lp, (540, 960))
    assert out[0, 0].tolist() == [np.float32(10 * 960) / np.float32(300), np.float32(540) / np.float32(5), 1.0]


@pytest.mark.parametrize('w,aligned', dc.VARIANT_CASES)
def test_variant_planes_hold_what_they_claim(w, aligned):
    vec, _ = dc.plan(w, aligned)
    for h in dc.HEIGHTS:
        lp, where = dc.variant_case(h, w, aligned)
        assert lp.shape == (3, 3, h, w) and lp.dtype == np.float32
        x, y = od.keypoint_decode_indices(lp)
        assert (x[0, 0], y[0, 0]) == (w - 1, h - 1) and (x[0, 1], y[0, 1]) == (0, 0)
        (r_a, c_early), (r_b, c_late) = where['tie']
        assert c_early < 64 * vec and c_late >= dc.last_group_start(w, aligned) and lp[1, 0, r_a, c_early] == lp[1, 0, r_b, c_late] == lp[1, 0].max()
        assert (x[1, 0], y[1, 0]) == (c_early, min(r_a, r_b))               # column of one pixel, row of the other
        (r_e, c_e), (r_l, c_l) = where['collision']
        assert (x[1, 1], y[1, 1]) == (c_e, r_e) and c_e < 64 * vec and c_l >= dc.last_group_start(w, aligned)
        assert dc.raw_argmax_xy(lp[1, 1]) == (c_l, r_l) and c_l != c_e
        if h > 1:
            assert r_l != r_e and r_l % 4 != r_e % 4 and r_a % 4 != r_b % 4   # rows of different waves (row y belongs to wave y % 4)
        out = od.keypoint_decode(lp, (537, 955))
        assert np.isneginf(lp[2, 0]).all() and out[2, 0].tolist() == [0.0, 0.0, 0.0] and np.isfinite(out).all()


def test_big_case_collides_outside_wave_zero():
    h, w = 700, 600                                                            # the builder at a size the CPU test can afford
    lp = dc.big_case(h, w)
    x, y = od.keypoint_decode_indices(lp)
    assert (int(y[0, 0]), int(x[0, 0])) == dc.BIG_FIRST and dc.raw_argmax_xy(lp[0, 0])[::-1] == dc.BIG_RAW
    assert all(64 <= i % 256 for i in dc.BIG_FIRST) and all(i % 256 < 64 for i in dc.BIG_RAW)
    assert all(r < 6140 and c < 1637 for (r, c) in (dc.BIG_FIRST, dc.BIG_RAW))
    lp[0, 0, h - 1, w - 1] = dc.BIG_LAST
    x, y = od.keypoint_decode_indices(lp)
    assert (int(y[0, 0]), int(x[0, 0])) == (h - 1, w - 1)


def test_keep_factor_is_one_from_17_33_on():
    keep = lambda t: np.float32(1) - od.exp_ref(np.float32([-t]))[0]
    # exp(-16.06) = 1.06e-7 = 1.78 * 2^-24: the keep factor at A is two steps below 1 (the spacing there is 2^-24)
    assert keep(17.0) == np.float32(1) - np.float32(2.0 ** -24) and keep(np.float32(289) / np.float32(18)) == np.float32(1) - np.float32(2.0 ** -23)
    assert keep(17.33) == 1 and keep(np.float32(313) / np.float32(18)) == 1 and keep(17.5) == 1
    assert np.float32(289) / np.float32(18) > 16.0                             # a cut lowered to 16 would skip the exp at A


@pytest.mark.parametrize('which', ['below', 'above'])
def test_line_shortcut_cases(which):
    heat, want = dc.line_shortcut_case(which)
    out = od.line_decode(heat, 3.0, 1.0).reshape(6, 2, 3)
    for k, (y1, x1) in enumerate(dc.LINE_PEAKS):
        assert out[k, 0].tolist() == [x1, y1, 0.75]
        assert (int(out[k, 1, 1]), int(out[k, 1, 0])) == want[k], (k, out[k])
        assert out[k, 1, 2] == 0.75
        plane = np.maximum(heat[k // 3, k % 3], 0)
        assert (plane == 0.75).sum() == 3
        ys, xs = np.nonzero(plane == 0.75)
        if which == 'below':                                                    # B is the last of the three, A (suppressed in its last bit) the second
            assert want[k] == (ys[2], xs[2]) and (ys[1], xs[1]) == (y1, x1 + 17)
        else:                                                                   # A' is kept whole and comes before B
            assert want[k] == (ys[1], xs[1]) == (y1 + 12, x1 + 13)
    assert {(y * 240 + x) % 256 // 64 for (y, x) in dc.LINE_PEAKS} == {0, 1, 2, 3}    # every wave finds a first peak


def test_plateau_case_has_many_equal_maxima():
    heat = dc.line_plateau()
    assert heat.shape == (2, 3, 135, 240) and heat.max() == 0.75 and heat.min() == -0.25
    counts = (heat == 0.75).reshape(6, -1).sum(axis=1)
    print('equal maxima per plane', counts.tolist())
    assert (counts >= 100).all()
    out = od.line_decode(heat, 3.0, 1.0).reshape(6, 2, 3)
    flat = heat.reshape(6, -1)
    for k in range(6):
        i1 = int(np.flatnonzero(flat[k] == 0.75)[0])
        assert out[k, 0].tolist() == [i1 % 240, i1 // 240, 0.75]
        assert out[k, 1, 2] == 0.75 and (out[k, 1, 0], out[k, 1, 1]) != (out[k, 0, 0], out[k, 0, 1])
    for hw in dc.LINE_SMALL_SHAPES:                                             # the small planes are built the same way
        small = dc.line_plateau((2, 3) + hw, seed=hw[0] * 100 + hw[1])
        assert small.shape == (2, 3) + hw and od.line_decode(small, 3.0, 1.0).shape == (2, 3, 2, 3)


def test_degenerate_line_planes():
    neg = dc.line_all_negative()
    assert (neg < 0).all()
    assert np.array_equal(od.line_decode(neg, 3.0, 8.0), np.zeros((2, 3, 2, 3), dtype=np.float32))
    for at_last in (False, True):
        heat = dc.line_single_pixel(at_last)
        out = od.line_decode(heat, 3.0, 1.0)
        first = [30.0, 16.0, np.float32(0.6)] if at_last else [0.0, 0.0, np.float32(0.6)]
        assert (heat > 0).reshape(6, -1).sum(axis=1).tolist() == [1] * 6
        assert all(out[b, c, 0].tolist() == first and out[b, c, 1].tolist() == [0.0, 0.0, 0.0] for b in range(2) for c in range(3))


@pytest.mark.parametrize('cfg_name', ['hrnet_w18', 'hrnet_w48'])
def test_tie_network_has_constant_logit_planes(cfg_name):
    cfg = hr.load_config(cfg_name)
    sd = dc.tie_state_dict(hr.seeded_state_dict(cfg, 7, 3.0))
    b = sd['model.last_layer.1.bias'].numpy()
    assert not sd['model.last_layer.1.weight'].any() and b[5] == 30 and b[7] == b[11] and np.abs(np.delete(b, 5)).max() == 2
    if cfg_name == 'hrnet_w18':                                                 # the oracle forward of the small net: every plane is one value
        heat = hr.forward(sd, hr.seeded_input(1, 64, 96, 11), cfg).numpy()
        assert all(np.unique(heat[0, c]).size == 1 for c in range(heat.shape[1]))
        out = od.keypoint_decode(heat, (540, 960))
        assert not out[..., :2].any() and np.unique(out[..., 2]).size > 1
