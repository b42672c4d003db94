"""GPU: one solve answers a whole grid of (max_rmse, max_rmse_rel) -- sncal_calibrate_sweep, sncal_evaluate_outcomes, sncal_sweep_fold,
metrics.EvalAISweep and validate(sweep=).

The contract is an identity with what exists: for every grid point g and frame b, outcomes[b, choice[g, b]] IS the record
sncal_calibrate_ws writes for frame b with grid point g's values (all 144 bytes), and the accumulators of EvalAISweep are those of one
EvalAImetric per grid point (counts exactly; the error sum within n_pts * 2^-52 relative: two fp64 summation orders of n_pts positive
terms).  The frames and the grid are tests/sweep_cases.py's: the coverage statements of tests/test_sweep_host.py are asserted here on
the device's own choices, so that an identity over constant outcomes cannot pass.  refine_max_iters = 200 on both sides.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import sweep_cases as SC
from oracle import camera_math as cm
from oracle import synth

pytestmark = pytest.mark.gpu

REC = 144                                               # sizeof(sncal_camera)
GRID = SC.grid_points()
ALGS = ['voter', 'iterative_voter']
_RUNS = {}


def creator(sncal, algorithm, lines, max_rmse=55.0, max_rmse_rel=5.0):
    cc = sncal.CameraCreator(sncal.PITCH_POINTS, algorithm=algorithm, **dict(SC.KW, max_rmse=max_rmse, max_rmse_rel=max_rmse_rel))
    if lines:
        cc.lines_data = SC.lines_data(SC.frames()[1])
    return cc


def device_frames(cuda, lines, sel=slice(None)):
    kp, lp = SC.frames()
    return torch.from_numpy(kp[sel]).to(cuda), (torch.from_numpy(np.ascontiguousarray(lp[sel])).to(cuda) if lines else None)


def raw_sweep(sncal, cc, d_kp, d_lp, grid):
    """sncal_calibrate_sweep on an arbitrary (n,2) grid (CameraCreator.sweep_device takes the two axes of a product)."""
    L = sncal._lib
    B, S = d_kp.shape[0], cc.sweep_slots()
    cfg = cc._cfg()
    n = ctypes.c_size_t()
    L.check(L.lib().sncal_calibrate_sweep_workspace(B, ctypes.byref(cfg), len(grid), ctypes.byref(n)))
    d_grid = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.float64)).to(d_kp.device)
    outcomes = torch.full((B, S, REC), 0xA5, dtype=torch.uint8, device=d_kp.device)
    choice = torch.full((len(grid), B), -7, dtype=torch.int32, device=d_kp.device)
    ws = torch.empty(n.value, dtype=torch.uint8, device=d_kp.device)
    L.check(L.lib().sncal_calibrate_sweep(d_kp.data_ptr(), d_lp.data_ptr() if d_lp is not None else None, B, ctypes.byref(cfg),
                                          d_grid.data_ptr(), len(grid), outcomes.data_ptr(), choice.data_ptr(), ws.data_ptr(), ws.numel(),
                                          L.current_stream_ptr()), 'sncal_calibrate_sweep')
    return outcomes.cpu().numpy(), choice.cpu().numpy()


def full_run(sncal, cuda, algorithm, lines):
    """The sweep of all frames over the test grid: computed once per (algorithm, lines) and shared, never modified."""
    key = (algorithm, lines)
    if key not in _RUNS:
        d_kp, d_lp = device_frames(cuda, lines)
        _RUNS[key] = raw_sweep(sncal, creator(sncal, algorithm, lines), d_kp, d_lp, GRID)
    return _RUNS[key]


def taken(outcomes, choice_g):
    """(B,144) the records grid point g takes: outcomes[b, choice[b]], the zero record for -1."""
    rec = outcomes[np.arange(len(choice_g)), np.maximum(choice_g, 0)].copy()
    rec[choice_g < 0] = 0
    return rec


def kinds(choice, S):
    """slot indices -> outcome names."""
    names = np.array(['none', 'first'] + ['rel', 'acc', 'all', 'ground', 'hom'] * ((S - 1) // 5), dtype=object)
    return names[choice + 1]


@pytest.mark.parametrize('lines', [False, True], ids=['no_lines', 'lines'])
@pytest.mark.parametrize('algorithm', ALGS)
def test_every_grid_point_is_the_plain_solve_byte_for_byte(sncal, cuda, algorithm, lines):
    outcomes, choice = full_run(sncal, cuda, algorithm, lines)
    d_kp, d_lp = device_frames(cuda, lines)
    B, S = outcomes.shape[:2]
    assert S == (6 if algorithm == 'voter' else 16) and choice.shape == (len(GRID), B)
    assert choice.min() >= -1 and choice.max() < S
    for g, (a, r) in enumerate(GRID):
        want = creator(sncal, algorithm, lines, a, r).solve_device(d_kp, d_lp).cpu().numpy()
        got = taken(outcomes, choice[g])
        bad = np.nonzero((want != got).any(axis=1))[0]
        assert bad.size == 0, (algorithm, lines, (a, r), bad[:8], choice[g, bad[:8]])
    # the outcome table itself: tags by slot, empty slots all zero, slot 0 only where the first pass has a camera
    status = outcomes[:, :, 136:140].copy().view(np.int32)[:, :, 0]
    tags = np.array([0] + [3, 4, 5, 6, 7] * ((S - 1) // 5))
    assert ((status == 0) | (status == tags[None, :]) | ((np.arange(S) == 0)[None, :] & np.isin(status, (1, 2)))).all()
    assert not outcomes[status == 0].any()
    if algorithm == 'voter':
        assert (status[:, 0] == 0).all()
    # coverage, on the device's own choices over the synthetic frames (tests/test_sweep_host.py states the same on the oracle's table)
    k = kinds(choice[:, :SC.N_SYNTH], S)
    if algorithm == 'voter':
        distinct = [len(set(k[:, b])) for b in range(SC.N_SYNTH)]
        assert sum(d >= 3 for d in distinct) >= 12, distinct
        assert {'none', 'rel', 'acc', 'all', 'hom'} <= set(k.ravel()), set(k.ravel())
    else:
        reach = status[:SC.N_SYNTH, 0] == 0
        assert reach.sum() >= 10, reach.sum()
        assert (k[:, ~reach] == 'first').all() and (k[:, reach] != 'first').all()
    assert (choice[len(GRID) - 2] == (-1 if algorithm == 'voter' else np.where(status[:, 0] > 0, 0, -1))).all()          # the NaN point


@pytest.mark.parametrize('algorithm', ALGS)
def test_frames_and_grid_points_are_independent(sncal, cuda, algorithm):
    """A frame's bytes do not depend on the batch around it (B = 1, 3, 64, 65: one wavefront of the selection, and one thread past it),
    a grid point's choices not on the grid around it (alone; duplicated and permuted), and a second run gives the same bytes."""
    outcomes, choice = full_run(sncal, cuda, algorithm, True)
    cc = creator(sncal, algorithm, True)
    for B in (1, 3, 64, 65):
        d_kp, d_lp = device_frames(cuda, True, slice(0, B))
        o, c = raw_sweep(sncal, cc, d_kp, d_lp, GRID)
        assert np.array_equal(o, outcomes[:B]) and np.array_equal(c, choice[:, :B]), B
    lo = SC.N_SYNTH - 8                                                       # frames of both kinds, their line points included
    d_kp, d_lp = device_frames(cuda, True, slice(lo, lo + 20))
    for g in (0, 9, 17, len(GRID) - 2, len(GRID) - 1):
        o, c = raw_sweep(sncal, cc, d_kp, d_lp, GRID[g:g + 1])
        assert np.array_equal(o, outcomes[lo:lo + 20]) and np.array_equal(c[0], choice[g, lo:lo + 20]), g
    order = np.random.Generator(np.random.PCG64(5)).permutation(np.concatenate([np.arange(len(GRID)), [3, 3, 11, len(GRID) - 2]]))
    o, c = raw_sweep(sncal, cc, d_kp, d_lp, GRID[order])
    assert np.array_equal(o, outcomes[lo:lo + 20]) and np.array_equal(c, choice[order][:, lo:lo + 20])
    o2, c2 = raw_sweep(sncal, cc, d_kp, d_lp, GRID[order])
    assert np.array_equal(o, o2) and np.array_equal(c, c2)


_ANNOTS = {}


def annotations(sncal):
    """Per frame {class: [{'x', 'y'}]} in pixels: the pitch model projected through the frame's TRUE camera, every 7th in-image
    sample of a class (at most 6), each moved by up to 3 px so that distances sit on both sides of the 5 px threshold."""
    if not _ANNOTS:
        from sncal_amd.evaluate import CLASSES, field_table
        pts, start = field_table(0.9)
        cams = [synth.synth_keypoints(s, **SC.SYNTH_KW)[1] for s in range(SC.N_SYNTH)] + [SC.dc.base_camera()] * len(SC.dc.CASES)
        rng = np.random.Generator(np.random.PCG64(77))
        out = []
        for cam in cams:
            ann = {}
            for c, name in enumerate(CLASSES):
                q = np.array([cm.project_point(cam['position'], cam['rotation'], cam['f'], cam['f'], cam['pp'], p) for p in pts[start[c]:start[c + 1]:7]])
                q = q[(q[:, 2] > 0) & (q[:, 0] >= 0) & (q[:, 0] < 960) & (q[:, 1] >= 0) & (q[:, 1] < 540)][:6]
                if len(q):
                    ann[name] = [{'x': float(x + dx), 'y': float(y + dy)} for (x, y, _), (dx, dy) in zip(q, rng.uniform(-3, 3, (len(q), 2)))]
            out.append(ann)
        _ANNOTS['a'] = out
    return _ANNOTS['a']


def check_rows(got, want, where):
    """EvalAImetric's accumulator rows: [missed, accuracy, n, tp, tp+fp, tp+fn] and n_pts exactly, the error sum within n_pts * 2^-52."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(got[..., :6], want[..., :6]) and np.array_equal(got[..., 7], want[..., 7]), where
    tol = want[..., 7] * 2.0 ** -52 * np.abs(want[..., 6])
    same = (np.abs(got[..., 6] - want[..., 6]) <= tol) | (np.isnan(got[..., 6]) & np.isnan(want[..., 6]))      # a NaN distance propagates on both sides
    assert same.all(), (where, got[..., 6], want[..., 6])


@pytest.mark.parametrize('algorithm', ALGS)
def test_evalai_sweep_is_one_evalai_metric_per_grid_point(sncal, cuda, algorithm):
    """Two updates (40 and 51 frames, line points included) and three frames that never reached the network."""
    axes = ([3.0, 20.0, float('nan'), 1e9], [0.0, 20.0])
    ann = annotations(sncal)
    kp, _ = SC.frames()
    cc = creator(sncal, algorithm, True)
    sweep = sncal.metrics.EvalAISweep(cc, *axes, threshold=5)
    assert len(sweep) == 8 and sweep.params(3) == {'max_rmse': 20.0, 'max_rmse_rel': 20.0}
    singles = [sncal.EvalAImetric(creator(sncal, algorithm, True, a, r), threshold=5) for a, r in sweep.grid]
    assert sweep.compute() == [0.0] * 8
    for lo, hi in ((0, 40), (40, len(kp))):
        out = {'prediction': torch.from_numpy(kp[lo:hi]).to(cuda), 'raw_annots': ann[lo:hi], 'img_name': [SC.frame_name(b) for b in range(lo, hi)]}
        sweep.update(out)
        for m in singles:
            m.update(out)
    for m in singles + [sweep]:
        m.add_missed(3)
    assert sweep._acc.is_cuda and sweep.total_frames == singles[0].total_frames == len(kp) + 3
    rows = sweep._read()
    want = np.stack([m._read() for m in singles])
    check_rows(rows, want, algorithm)
    assert len({tuple(r[:6]) for r in want}) >= 2 and want[:, 7].max() > 0     # the grid points do differ in what they score
    assert sweep.compute() == [m.compute() for m in singles]
    for g, m in enumerate(singles):
        a, b = types.SimpleNamespace(phase='val', metrics={}), types.SimpleNamespace(phase='val', metrics={})
        sweep.epoch_complete(a, g)
        m.epoch_complete(b)
        assert list(a.metrics) == list(b.metrics)
        for k in b.metrics:
            if k == 'val_l2_reprojection':
                assert a.metrics[k] == b.metrics[k] or abs(a.metrics[k] - b.metrics[k]) <= want[g, 7] * 2.0 ** -52 * abs(b.metrics[k]), (g, k)
            else:
                assert a.metrics[k] == b.metrics[k], (g, k)
    # the fold alone: the same bits on a second run, -1 counts as a missed frame
    ev = sweep.evaluator(cuda)
    outcomes, choice = cc.sweep_device(torch.from_numpy(kp[:33]).to(cuda), None, *axes)
    contrib = ev.evaluate_outcomes(outcomes, ann[:33])
    acc = ev.sweep_fold(contrib, choice)
    assert torch.equal(acc, ev.sweep_fold(ev.evaluate_outcomes(outcomes, ann[:33]), choice))
    c, ch = contrib.cpu().numpy(), choice.cpu().numpy()
    empty = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
    ref = np.stack([sum((c[b, ch[g, b]] if ch[g, b] >= 0 else empty) for b in range(33)) for g in range(8)])
    assert np.array_equal(acc.cpu().numpy(), ref)                              # frame order, fp64: numpy's sequential sum is the same sum
    status = outcomes.cpu().numpy()[:, :, 136:140].copy().view(np.int32)[:, :, 0]
    assert (c[status == 0] == empty).all() and (c[status != 0][:, [0, 2]] == [0.0, 1.0]).all()


def test_validate_sweep_equals_validate_over_a_list_of_calibrators(sncal, cuda, tmp_path):
    from test_validate_gpu import KW, _batches, _dataset, _model
    images, annots = _dataset(sncal, 7)
    names = [f'{i:05d}.jpg' for i in range(len(images))]
    model = _model(sncal, tmp_path)
    kw = dict(KW, algorithm='voter', refine_max_iters=200)
    axes = {'max_rmse': [0.05, 4.0, 55.0], 'max_rmse_rel': [0.0, 5.0]}
    n_pts_max = len(images) * sum(len(v) for a in annots for v in a.values())       # more points than any error sum can hold
    one = sncal.CameraCreator(sncal.PITCH_POINTS, **kw)
    cams = [sncal.CameraCreator(sncal.PITCH_POINTS, **dict(kw, max_rmse=a, max_rmse_rel=r)) for a in axes['max_rmse'] for r in axes['max_rmse_rel']]
    want = sncal.validate.validate(model, _batches(sncal, images, annots, names, 3), cams)
    got = sncal.validate.validate(model, _batches(sncal, images, annots, names, 3), one, sweep=axes)
    assert len(got) == len(want) == 6 and isinstance(got, list)
    for g, (a, b) in enumerate(zip(got, want)):
        assert a.params == {'max_rmse': cams[g].max_rmse, 'max_rmse_rel': cams[g].max_rmse_rel}
        assert list(a) == list(b) and a.frames == b.frames == 7 and a.skipped == b.skipped
        for k in b:
            if k == 'val_l2_reprojection':
                assert a[k] == b[k] or abs(a[k] - b[k]) <= n_pts_max * 2.0 ** -52 * abs(b[k]), (g, k)
            else:
                assert a[k] == b[k], (g, k, a[k], b[k])
    scores = [r['val_evalai'] for r in want]
    assert got.best == scores.index(max(scores))
    assert len({r['val_completeness'] for r in want}) >= 2                     # 0.05 px refuses cameras that 55 px takes
    with pytest.raises(sncal._lib.SncalError):
        sncal.validate.validate(model, _batches(sncal, images, annots, names, 3), cams, sweep=axes)
    with pytest.raises(sncal._lib.SncalError):
        sncal.validate.validate(model, _batches(sncal, images, annots, names, 3),
                                sncal.CameraCreator(sncal.PITCH_POINTS, **dict(kw, algorithm='original_voter')), sweep=axes)


def test_refused_calls_launch_nothing(sncal, cuda):
    """Algorithms without the two parameters, n_grid out of range, a short workspace, null pointers: the status, and outcomes / choice
    keep the pattern they were filled with."""
    L = sncal._lib
    lib = L.lib()
    d_kp, _ = device_frames(cuda, False, slice(0, 4))
    d_grid = torch.from_numpy(GRID).to(cuda)
    outcomes = torch.full((4, 16, REC), 0x5A, dtype=torch.uint8, device=cuda)
    choice = torch.full((len(GRID), 4), -9, dtype=torch.int32, device=cuda)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=cuda)

    def call(cfg, n_grid=len(GRID), kp=d_kp, grid=d_grid, out=outcomes, ch=choice, wsp=ws, ws_bytes=1 << 20):
        return lib.sncal_calibrate_sweep(kp.data_ptr() if kp is not None else None, None, 4, ctypes.byref(cfg), grid.data_ptr() if grid is not None else None,
                                         n_grid, out.data_ptr() if out is not None else None, ch.data_ptr() if ch is not None else None,
                                         wsp.data_ptr() if wsp is not None else None, ws_bytes, L.current_stream_ptr())
    for alg in (1, 3, 4):
        cfg = creator(sncal, 'voter', False)._cfg()
        cfg.algorithm = alg
        assert call(cfg) == -1 and b'never reads max_rmse' in lib.sncal_last_error()
    cfg = creator(sncal, 'iterative_voter', False)._cfg()
    assert call(cfg, n_grid=0) == -1 and call(cfg, n_grid=4097) == -1
    need = ctypes.c_size_t()
    assert lib.sncal_calibrate_sweep_workspace(4, ctypes.byref(cfg), len(GRID), ctypes.byref(need)) == 0
    assert call(cfg, ws_bytes=need.value - 1) == -4 and b'sncal_calibrate_sweep_workspace' in lib.sncal_last_error()
    assert call(cfg, kp=None) == -1 and call(cfg, grid=None) == -1 and call(cfg, out=None) == -1 and call(cfg, ch=None) == -1
    assert call(cfg, wsp=None) == -1
    torch.cuda.synchronize()
    assert (outcomes == 0x5A).all() and (choice == -9).all()
    assert call(cfg, ws_bytes=need.value) == 0                                 # the exact size is enough
    torch.cuda.synchronize()
    assert not (outcomes == 0x5A).all() and (choice >= -1).all()
    with pytest.raises(L.SncalError):
        creator(sncal, 'opencv_calibration', False).sweep_device(d_kp, None, [10.0], [4.0])
    with pytest.raises(L.SncalError):
        sncal.metrics.EvalAISweep(creator(sncal, 'original_voter', False), [10.0], [4.0])
