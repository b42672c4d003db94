"""CPU: the (max_rmse, max_rmse_rel) sweep's inputs are worth testing on, and its host side is in place.

tests/golden/sweep_cases.npz is the ORACLE's table of candidate cameras for the frames of tests/sweep_cases.py
(tools/make_golden_sweep.py).  The selection restated in sweep_cases.voter_choice (python's max() over the reference's list) is run
over the test grid on it: enough frames must change outcome across the grid, and every outcome must occur, for the byte identity of
tests/test_sweep_gpu.py to say anything.  The bounds leave a margin below what the oracle shows (59 frames with more than one outcome,
21 with three or more, 17 reaching the voter): the device's cameras agree with the oracle's to the solve's tolerance, not bit for bit,
so a frame at a threshold may fall the other way there.  The GPU test asserts the same bounds on the device's own choices.
"""
import ctypes
import os

import numpy as np
import pytest

import sweep_cases as SC


@pytest.fixture(scope='module')
def table(gold_dir):
    g = np.load(os.path.join(gold_dir, 'sweep_cases.npz'))
    return {k: g[k] for k in g.files}


def outcomes_per_frame(table, n_thr, use_first):
    grid = SC.grid_points()
    return [[SC.frame_choice(table, b, n_thr, a, r, first_ok=use_first and bool(table['first_ok'][b]))[0] for a, r in grid]
            for b in range(int(table['n_synth']))]


def test_the_table_belongs_to_the_frames(table):
    kp, lp = SC.frames()
    assert table['good'].shape == (len(kp), len(SC.THRESHS), 4) and table['rmse'].shape == table['good'].shape
    assert list(table['threshs']) == SC.THRESHS and int(table['n_synth']) == SC.N_SYNTH
    assert kp.shape == (SC.N_SYNTH + len(SC.dc.CASES), 57, 3) and lp.shape == (len(kp), 30, 3)
    assert (lp[SC.N_SYNTH:, :, 2] > 0.5).any() and not lp[:SC.N_SYNTH].any()


def test_voter_outcomes_change_across_the_test_grid(table):
    """The voter algorithm (one threshold, no first pass) on the 64 synthetic frames."""
    per_frame = outcomes_per_frame(table, 1, False)
    distinct = [len(set(o)) for o in per_frame]
    assert sum(d >= 3 for d in distinct) >= 12, distinct
    seen = set().union(*map(set, per_frame))
    assert {None, 'rel', 'acc', 'all', 'hom'} <= seen, seen


def test_iterative_voter_reaches_the_voter(table):
    reach = [b for b in range(SC.N_SYNTH) if not table['first_ok'][b]]
    assert len(reach) >= 10, reach
    per_frame = outcomes_per_frame(table, len(SC.THRESHS), True)
    assert all(set(per_frame[b]) == {'first'} for b in range(SC.N_SYNTH) if table['first_ok'][b])


def test_nan_and_infinite_grid_points(table):
    """Every comparison with NaN is false: no camera anywhere.  (inf, -inf): everything is accepted, the rel flag never holds."""
    for b in range(SC.N_SYNTH):
        row = [table[k][b, 0] for k in ('good', 'rmse', 'hom_ok', 'hom_rmse', 'raises')]
        if row[4]:
            continue
        assert SC.voter_choice(*row, float('nan'), float('nan')) is None
        c = SC.voter_choice(*row, float('inf'), float('-inf'))
        if row[0].any():
            best = int(np.argmin(np.where(row[0], row[1], np.inf)))           # no flag: the smallest rmse, first on ties
            assert c == SC.OUTCOMES[1 + best]
        else:
            assert c == ('hom' if row[2] else None)


def test_grid_order_and_range_parser():
    from sncal_amd.prediction import parse_range, sweep_grid
    g = sweep_grid([10, 14], [4, 6, 8])
    assert g.dtype == np.float64 and g.tolist() == [[10, 4], [10, 6], [10, 8], [14, 4], [14, 6], [14, 8]]           # max_rmse outermost
    assert np.array_equal(sweep_grid(SC.MAX_RMSE, SC.MAX_RMSE_REL), SC.grid_points()[:-2])
    assert parse_range('10:70:4') == list(range(10, 70, 4)) and len(parse_range('10:70:4')) == 15
    assert parse_range('4:16:2') == [4, 6, 8, 10, 12, 14]
    assert parse_range('0:3') == [0, 1, 2] and parse_range('5:5:1') == [] and parse_range('3:0:-1') == [3, 2, 1]
    assert parse_range('1.5:3:0.5') == [1.5, 2.0, 2.5]
    for bad in ('10', '10:70:0', 'a:b:c', '1:2:3:4', '1::2', '0:inf:1'):
        with pytest.raises(ValueError):
            parse_range(bad)
    import sncal_amd
    with pytest.raises(sncal_amd._lib.SncalError):
        sweep_grid([], [1.0])
    with pytest.raises(sncal_amd._lib.SncalError):
        sweep_grid(range(65), range(64))                                      # 4160 > 4096
    assert len(sweep_grid(range(64), range(64))) == 4096


def test_signatures_and_host_side_refusals():
    """The new entry points are bound, and refuse before they touch the device: the algorithms that have nothing to sweep, n_grid out
    of range, null pointers (no kernel is launched here; an empty batch is fine)."""
    import sncal_amd
    L = sncal_amd._lib
    lib = L.lib()
    for name in ('sncal_calibrate_sweep_workspace', 'sncal_calibrate_sweep', 'sncal_evaluate_outcomes', 'sncal_sweep_fold'):
        assert name in L.SIGNATURES and name not in L.MISSING
    assert lib.sncal_version() == 100
    cfg = L.VoterCfg()
    cfg.algorithm, cfg.n_conf_threshs, cfg.img_w, cfg.img_h = 0, 3, 960, 540
    n = ctypes.c_size_t()
    one = ctypes.c_void_p(16)
    assert lib.sncal_calibrate_sweep_workspace(64, ctypes.byref(cfg), 90, ctypes.byref(n)) == 0
    plain = ctypes.c_size_t()
    assert lib.sncal_calibrate_workspace(64, ctypes.byref(cfg), ctypes.byref(plain)) == 0
    assert plain.value < n.value <= plain.value + 64 * (144 + 3 * 48) + 1024          # + the first pass's records and the selection's table
    for alg in (1, 3, 4):
        cfg.algorithm = alg
        assert lib.sncal_calibrate_sweep_workspace(64, ctypes.byref(cfg), 90, ctypes.byref(n)) == -1
        assert b'never reads max_rmse' in lib.sncal_last_error()
        assert lib.sncal_calibrate_sweep(one, None, 1, ctypes.byref(cfg), one, 1, one, one, one, 1 << 20, None) == -1
        assert b'never reads max_rmse' in lib.sncal_last_error()
        with pytest.raises(L.SncalError):
            sncal_amd.CameraCreator(sncal_amd.PITCH_POINTS, algorithm={1: 'original_voter', 3: 'opencv_calibration',
                                                                       4: 'opencv_calibration_multiplane'}[alg]).sweep_slots()
    for alg, slots in ((0, 16), (2, 6)):
        cfg.algorithm = alg
        assert sncal_amd.CameraCreator(sncal_amd.PITCH_POINTS, algorithm='voter' if alg else 'iterative_voter').sweep_slots() == slots
        for bad in (0, -1, 4097):
            assert lib.sncal_calibrate_sweep_workspace(64, ctypes.byref(cfg), bad, ctypes.byref(n)) == -1 and b'n_grid' in lib.sncal_last_error()
            assert lib.sncal_calibrate_sweep(one, None, 1, ctypes.byref(cfg), one, bad, one, one, one, 1 << 20, None) == -1
        assert lib.sncal_calibrate_sweep_workspace(64, ctypes.byref(cfg), 4096, ctypes.byref(n)) == 0
        assert lib.sncal_calibrate_sweep_workspace(64, None, 1, ctypes.byref(n)) == -1
        assert lib.sncal_calibrate_sweep_workspace(64, ctypes.byref(cfg), 1, None) == -1
        assert lib.sncal_calibrate_sweep(None, None, 0, ctypes.byref(cfg), None, 1, None, None, None, 0, None) == 0           # B == 0
        for hole in range(4):                                                  # d_kpts, d_grid, d_outcomes, d_choice
            ptrs = [one, one, one, one]
            ptrs[hole] = None
            assert lib.sncal_calibrate_sweep(ptrs[0], None, 1, ctypes.byref(cfg), ptrs[1], 1, ptrs[2], ptrs[3], one, 1 << 20, None) == -1
            assert b'null' in lib.sncal_last_error()
        assert lib.sncal_calibrate_sweep(one, None, 1, ctypes.byref(cfg), one, 1, one, one, None, 1 << 20, None) == -1
        assert lib.sncal_calibrate_sweep(one, None, 1, ctypes.byref(cfg), one, 1, one, one, ctypes.c_void_p(24), 1 << 20, None) == -1      # not 16-byte aligned
        assert lib.sncal_calibrate_sweep(one, None, 1, ctypes.byref(cfg), one, 1, one, one, one, 64, None) == -4              # SNCAL_ERR_WORKSPACE
        assert b'sncal_calibrate_sweep_workspace' in lib.sncal_last_error()
    assert lib.sncal_evaluate_outcomes(None, 0, 16, None, None, None, 26, None, None, None, 4, 5.0, 960, 540, None, None) == 0
    assert lib.sncal_evaluate_outcomes(one, 1, 0, one, one, one, 26, one, one, one, 4, 5.0, 960, 540, one, None) == -1        # S < 1
    assert lib.sncal_evaluate_outcomes(one, 1, 16, one, one, one, 26, one, one, one, 4, 5.0, 960, 540, None, None) == -1
    assert lib.sncal_sweep_fold(None, None, 1, 16, 1, one, None) == -1
    assert lib.sncal_sweep_fold(one, one, 1, 16, 0, one, None) == -1
    assert lib.sncal_sweep_fold(one, one, 1, 16, 4097, one, None) == -1


def test_validate_refuses_a_sweep_over_a_list_before_any_work():
    import sncal_amd
    from sncal_amd import validate as V
    cc = sncal_amd.CameraCreator(sncal_amd.PITCH_POINTS, algorithm='voter')
    with pytest.raises(sncal_amd._lib.SncalError, match='ONE CameraCreator'):
        V.validate(None, [], [cc, cc], sweep={'max_rmse': [10.0], 'max_rmse_rel': [4.0]})
    with pytest.raises(sncal_amd._lib.SncalError, match='max_rmse'):
        V.validate(None, [], cc, sweep={'max_rmse': [10.0]})
