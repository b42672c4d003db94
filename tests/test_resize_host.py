"""CPU: the host side of the resize stage (cv2.resize's INTER_LINEAR on uint8 frames, csrc/resize.hip).
    sncal_resize_tables -- the function the kernel forms its taps with -- against the numpy restatement's tables (tests/resize_ref.py);
    the restatement itself against float64 bilinear (strictly less than one level) and on its area-path rule;
    the reduce-then-resize size bookkeeping of decoded_batches and the --resize argument of the three command lines.
No cv2 here: tests/test_resize_cv2_optional.py is what holds the restatement to OpenCV's own bytes, where a cv2 is installed."""
import numpy as np
import pytest

import resize_ref as ref

PAIRS = ref.AXES + [(a, b) for a in range(1, 41) for b in range(1, 41)]


def test_tables_equal_the_restatement_for_both_edge_rules(sncal):
    for n_src, n_dst in PAIRS:
        for zero_edges in (True, False):
            ofs, coef = sncal.resize.tables(n_src, n_dst, zero_edges)
            want_ofs, want_coef = ref.tables(n_src, n_dst, zero_edges)
            assert ofs.dtype == np.int32 and coef.dtype == np.int16 and coef.shape == (n_dst, 2)
            assert np.array_equal(ofs, want_ofs) and np.array_equal(coef, want_coef), (n_src, n_dst, zero_edges)


def test_tables_edge_rules_and_arguments(sncal):
    # 360 -> 540: the first row sits at -1/6, s = -1 under the y rule (both weights kept), pinned to 0 with (2048, 0) under the x rule
    yo, yc = sncal.resize.tables(360, 540, False)
    xo, xc = sncal.resize.tables(360, 540, True)
    assert yo[0] == -1 and yc[0].tolist() == [341, 1707] and xo[0] == 0 and xc[0].tolist() == [2048, 0]
    assert xo[-1] == 359 and xc[-1].tolist() == [2048, 0] and yo[-1] == 359 and yc[-1, 1] != 0
    # the weights need not sum to 2048 (two roundings), but never miss it by more than one
    s = sncal.resize.tables(53, 52, False)[1].astype(int).sum(1)
    assert set(s.tolist()) <= {2047, 2048, 2049}
    for bad in ((0, 4), (4, 0), (-1, 3)):
        with pytest.raises(sncal._lib.SncalError):
            sncal.resize.tables(bad[0], bad[1], True)


@pytest.mark.parametrize('case', ref.CASES, ids=lambda c: '%dx%d-%dx%d' % c[:4])
def test_restatement_is_within_one_level_of_float_bilinear(case):
    h, w, H, W, B = case
    for kind, src in ref.inputs(h, w, B).items():
        out = ref.resize(src, (W, H))
        assert out.shape == (B, H, W, 3) and out.dtype == np.uint8
        worst = ref.worst_level(out, src, (W, H))
        print(case, kind, worst)
        assert worst < 1.0, (kind, worst)


def test_restatement_takes_the_area_path_at_exactly_half_both_ways_only():
    assert ref.takes_area_path(64, 96, 32, 48) and not ref.takes_area_path(64, 96, 32, 96) and not ref.takes_area_path(64, 96, 64, 48)
    src = ref.inputs(64, 96)['noise'][0]
    S = src.astype(np.int32)
    area = ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    assert np.array_equal(ref.resize(src, (48, 32)), area)
    # ratio 2 along y only: the general path; its rows carry weights (1024, 1024), its columns (2048, 0)
    half = ref.resize(src, (96, 32))
    yo, yc = ref.tables(64, 32, False)
    assert yo.tolist() == list(range(0, 64, 2)) and (yc == 1024).all()
    want = (((1024 * ((S[0::2] * 2048) >> 4)) >> 16) + ((1024 * ((S[1::2] * 2048) >> 4)) >> 16) + 2) >> 2
    assert np.array_equal(half, want.astype(np.uint8))


def test_reduce_then_resize_size_bookkeeping(sncal):
    plan = sncal.frames.resize_plan
    assert plan(1080, 1920, 1, None) == ((1080, 1920), (1080, 1920))
    assert plan(1080, 1920, 2, None) == ((540, 960), (540, 960))
    assert plan(720, 1280, 1, (960, 540)) == ((720, 1280), (540, 960))           # resize is (W, H), sizes are (H, W)
    assert plan(1081, 1921, 2, (960, 540)) == ((541, 961), (540, 960))           # libjpeg rounds up, then cv2.resize
    assert plan(97, 129, 8, (72, 54)) == ((13, 17), (54, 72))
    for bad in ((960,), (960, 0), (960.5, 540), 'ab', 960):
        with pytest.raises(sncal._lib.SncalError):
            plan(720, 1280, 1, bad)
    with pytest.raises(sncal._lib.SncalError):
        plan(720, 1280, 3, (960, 540))
    assert sncal.frames.MAX_SOURCE_SIZES == 4
    # frame_size stays the size of the frames yielded: one that contradicts resize is refused before a file is opened
    with pytest.raises(sncal._lib.SncalError, match='frame_size'):
        next(sncal.frames.decoded_batches('/nonexistent', ['a.jpg'], 1, 'cpu', 0, [], frame_size=(540, 960), resize=(72, 54)))


def test_resize_argument_of_the_three_command_lines(sncal):
    v, s, b = sncal.validate, sncal.submit, sncal.baseline_cameras
    lines = [(v, ['--data', 'd', '--model', 'm']), (s, ['--img-dir', 'd', '--model', 'm', '--save-dir', 'o']),
             (b, ['--line-model', 'm', '--img-dir', 'd', '--save-dir', 'o'])]
    for mod, argv in lines:
        a = mod.parser().parse_args(argv)
        assert a.resize is None and sncal.resize.parsed_resize(a) is None and a.reduce == 1
        a = mod.parser().parse_args(argv + ['--resize', '960', '540', '--reduce', '2'])
        assert sncal.resize.parsed_resize(a) == (960, 540) and a.reduce == 2
        for bad in (['--resize', '960'], ['--resize', '960', 'x'], ['--resize', '960', '540', '3']):
            with pytest.raises(SystemExit):
                mod.parser().parse_args(argv + bad)
        with pytest.raises(sncal._lib.SncalError):
            sncal.resize.parsed_resize(mod.parser().parse_args(argv + ['--resize', '960', '0']))


MOVED_TO_FRAMES = ['list_split', 'list_line_split', 'annot_to_keypoints', 'resize_plan', 'MAX_SOURCE_SIZES', 'decoded_batches', '_label_mode',
                   'labelled_batch', 'folder_batches', 'train_batches', 'line_folder_batches']


def test_the_old_addresses_in_validate_are_the_same_objects(sncal):
    """The loaders lived in validate.py until frames.py: README, DESIGN, INTEGRATION and code outside this tree still say
    validate.train_batches.  The old address is the object itself, not a wrapper."""
    for n in MOVED_TO_FRAMES:
        assert getattr(sncal.validate, n) is getattr(sncal.frames, n), n
    for n in ('add_resize_argument', 'parsed_resize'):
        assert getattr(sncal.validate, n) is getattr(sncal.resize, n), n
    assert not hasattr(sncal.validate, '_resized_batches') and not hasattr(sncal.frames, '_resized_batches')


def test_resize_u8_refuses_what_is_not_on_the_gpu(sncal):
    import torch
    with pytest.raises(sncal._lib.SncalError):
        sncal.resize.resize_u8(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), (2, 2))
    with pytest.raises(sncal._lib.SncalError):
        sncal.resize.resize_u8(np.zeros((1, 4, 4, 3), np.uint8), (2, 2))
