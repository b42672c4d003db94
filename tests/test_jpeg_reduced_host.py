"""CPU: libjpeg's scaled decode (JpegDecoder(reduce=2 / 4 / 8) = cv2.imread's IMREAD_REDUCED_COLOR_2 / _4 / _8).  The numpy
restatement (tests/jpeg_reduced_ref.py) equals libjpeg-turbo's frames (tests/golden/jpeg_reduced.npz, tools/make_golden_jpeg_reduced.py)
bit for bit, and the library's plan -- the function the decoder fills its frame descriptors with -- equals the restatement's."""
import ctypes

import numpy as np
import pytest

import jpeg_reduced_ref as rr


def test_restatement_equals_libjpeg_turbo_on_every_golden_frame(sncal, gold_dir):
    g, names, denoms = rr.cases(gold_dir)
    n = 0
    for name in names:
        data = g['jpg.' + name].tobytes()
        for d in denoms[name]:
            want = g[f'bgr.{name}.d{d}']
            got = rr.decode_bgr(data, d)
            assert got.shape == want.shape and np.array_equal(got, want), (name, d)
            n += 1
    assert n == 184                                              # 9 sizes x 4 layouts x 2 restart settings x the denominators that fit


def test_hd_stream_restatement_matches_the_stored_row_sums(sncal, gold_dir):
    g, _, _ = rr.cases(gold_dir)
    data = g['jpg.hd'].tobytes()
    for d in (2, 4, 8):
        got = rr.decode_bgr(data, d)
        assert got.shape == (-(-1080 // d), 1920 // d, 3)
        assert np.array_equal(got.astype(np.int64).sum(axis=(1, 2)), g[f'bgr.hd.d{d}.rowsum']), d


def test_library_plan_equals_the_restatement_and_the_golden_shapes(sncal, gold_dir):
    g, names, denoms = rr.cases(gold_dir)
    seen = set()
    for name in names + ['hd']:
        info = sncal.jpeg.probe(g['jpg.' + name].tobytes())
        samp = [(info['h_samp'], info['v_samp']), (1, 1), (1, 1)][:info['components']]
        for d in (1, 2, 4, 8):
            got = sncal.jpeg.scaled_layout(info, d)
            assert got == rr.plan(info['height'], info['width'], samp, d), (name, d)
            assert got['out_hw'] == sncal.jpeg.reduced_size(info['height'], info['width'], d)
            if d in denoms.get(name, ()):
                assert g[f'bgr.{name}.d{d}'].shape == got['out_hw'] + (3,)
            seen.add((info['h_samp'], info['v_samp'], info['components'], d, tuple(got['comp_block']), tuple(got['comp_up'])))
    # the plans the kernel has a path for: 4:2:0 chroma one size larger and never upsampled below full size, 4:2:2 upsampled h2v1
    assert (2, 2, 3, 2, (4, 8, 8), ((1, 1), (1, 1), (1, 1))) in seen
    assert (2, 2, 3, 8, (1, 2, 2), ((1, 1), (1, 1), (1, 1))) in seen
    assert (2, 1, 3, 4, (2, 2, 2), ((1, 1), (1, 2), (1, 2))) in seen
    assert (2, 2, 3, 1, (8, 8, 8), ((1, 1), (2, 2), (2, 2))) in seen
    assert (1, 1, 1, 4, (2,), ((1, 1),)) in seen


def test_reduced_size_rounds_up():
    import sncal_amd
    assert sncal_amd.jpeg.reduced_size(1080, 1920, 2) == (540, 960)
    assert sncal_amd.jpeg.reduced_size(1080, 1920, 8) == (135, 240)
    assert sncal_amd.jpeg.reduced_size(17, 23, 4) == (5, 6)
    assert sncal_amd.jpeg.reduced_size(1, 1, 8) == (1, 1)
    assert sncal_amd.jpeg.reduced_size(540, 960, 1) == (540, 960)


def test_bad_denominators_are_refused(sncal):
    L = sncal._lib
    info = dict(width=64, height=48, components=3, h_samp=2, v_samp=2)
    for bad in (0, 3, 5, 16, -2, 2.0, None):
        with pytest.raises(L.SncalError):
            sncal.jpeg.reduced_size(48, 64, bad)
        with pytest.raises(L.SncalError):
            sncal.jpeg.scaled_layout(info, bad)
    ci = L.JpegInfo(width=64, height=48, components=3, h_samp=2, v_samp=2)
    out_hw, block, hw, up = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 6)()
    assert L.lib().sncal_jpeg_scaled_layout(ctypes.byref(ci), 3, out_hw, block, hw, up) == -1 and b'scale_denom 3' in L.lib().sncal_last_error()
    assert L.lib().sncal_jpeg_scaled_layout(None, 2, out_hw, block, hw, up) == -1
    ci.h_samp = 4                                                   # not a header the decoder accepts
    assert L.lib().sncal_jpeg_scaled_layout(ctypes.byref(ci), 2, out_hw, block, hw, up) == -1
    # the argument check of the constructor comes before any device call
    assert L.lib().sncal_jpeg_create_scaled(4, 48, 64, 3, 1, ctypes.byref(ctypes.c_void_p())) == -1 and b'scale_denom 3' in L.lib().sncal_last_error()
    assert L.lib().sncal_jpeg_create_scaled(0, 48, 64, 2, 1, ctypes.byref(ctypes.c_void_p())) == -1
    assert L.lib().sncal_jpeg_output_size(None, None, None) == -1
