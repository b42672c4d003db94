"""Inputs of the (max_rmse, max_rmse_rel) sweep tests: the frames, the test grid, and the voter's final choice restated on a table of
candidate cameras (prediction.py:293-329 of the reference, :250-256 for the walk over the thresholds).

Frames: 64 noisy synthetic ones (4 px of noise, 12 % gross outliers: the candidate cameras of a frame then differ by tens of pixels of
rmse, so the two thresholds decide between them) and the frames of tests/solve_decision_cases.py with their line points.

The grid is NOT the reference's search space (optimize_valid.yaml: max_rmse 10..66, max_rmse_rel 4..14): on frames like these the
RANSAC-consistent camera sits at 1-5 px and wins at every point of that grid, so an identity over it would compare constants.  The
test grid spans 1.5 px .. 1e9 on one axis and 0 .. 1e9 on the other, plus a NaN point (every comparison false: no camera) and an
(inf, -inf) point.

tests/golden/sweep_cases.npz (tools/make_golden_sweep.py) holds oracle/solve.py's candidate table for these frames.
"""
import numpy as np

from oracle import synth

import solve_decision_cases as dc

N_SYNTH = 64
SYNTH_KW = dict(sigma_px=4.0, outlier_frac=0.12, min_visible=8)
THRESHS = [0.5, 0.35, 0.2]                                   # make_submit.py:45-50; the voter algorithm runs at THRESHS[0]
KW = dict(dc.KW, refine_max_iters=200)                       # 200: both sides of every comparison, to keep the runs short
MAX_RMSE = [1.5, 3.0, 5.0, 20.0, 60.0, 100.0, 1e9]
MAX_RMSE_REL = [0.0, 3.5, 20.0, 1e9]
EXTRA_POINTS = [(float('nan'), float('nan')), (float('inf'), float('-inf'))]
CAND_TAGS = ['camera_rel', 'camera_acc', 'cam_all', 'cam_ground']      # the order of the reference's list (prediction.py:293-310)
OUTCOMES = ['none', 'rel', 'acc', 'all', 'ground', 'hom']


def grid_points():
    """(n,2) [max_rmse, max_rmse_rel]: the cartesian product, max_rmse outermost, then the two extra points."""
    return np.array([(a, r) for a in MAX_RMSE for r in MAX_RMSE_REL] + EXTRA_POINTS, dtype=np.float64)


_FRAMES = {}


def frames():
    """(kpts (N,57,3) float32, line_pts (N,30,3) float32 [x, y, valid]): synthetic frames first (no line points), then the decision
    table's.  Built once per process."""
    if not _FRAMES:
        kp = [synth.synth_keypoints(s, **SYNTH_KW)[0] for s in range(N_SYNTH)] + [c['kp'] for c in dc.CASES]
        lp = [np.zeros((30, 3), np.float32)] * N_SYNTH + [c['line_pts'] if c['line_pts'] is not None else np.zeros((30, 3), np.float32)
                                                          for c in dc.CASES]
        _FRAMES['kp'] = np.ascontiguousarray(np.stack(kp), dtype=np.float32)
        _FRAMES['lp'] = np.ascontiguousarray(np.stack(lp), dtype=np.float32)
    return _FRAMES['kp'], _FRAMES['lp']


def lines_data(lp):
    """(N,30,3) line points -> CameraCreator.lines_data / the oracle's, keyed by frame name."""
    return {frame_name(b): {i: (float(lp[b, i, 0]), float(lp[b, i, 1])) for i in range(30) if lp[b, i, 2] > 0.5}
            for b in range(len(lp)) if (lp[b, :, 2] > 0.5).any()}


def frame_name(b):
    return f'{b:05d}.jpg'


def voter_choice(good, rmse, hom_ok, hom_rmse, raises, max_rmse, max_rmse_rel):
    """CameraCreator.voter's final choice (prediction.py:293-329) on ONE threshold's candidates, as the reference writes it: python's
    max() over the list of good cameras with key (rel and rmse < max_rmse_rel, 1 / rmse), accepted below max_rmse, else the
    homography camera below max_rmse.  -> 'rel' / 'acc' / 'all' / 'ground' / 'hom', None (no camera) or 'raise'."""
    if raises:
        return 'raise'
    cams = [(OUTCOMES[1 + i], float(rmse[i])) for i in range(4) if good[i]]
    if cams:
        if any(r == 0.0 for _, r in cams):
            return 'raise'                                    # 1 / 0: ZeroDivisionError
        best = max(cams, key=lambda x: (x[0] == 'rel' and x[1] < max_rmse_rel, 1 / x[1]))
        if best[1] < max_rmse:
            return best[0]
    if hom_ok and float(hom_rmse) < max_rmse:
        return 'hom'
    return None


def frame_choice(table, b, n_thr, max_rmse, max_rmse_rel, first_ok=False):
    """iterative_voter's walk (prediction.py:245-257) over the first n_thr thresholds of the table for frame b: 'first' when the
    original_voter pass has a camera, else the first threshold whose voter returns one -> (outcome, threshold index); an exception
    ends the walk without a camera."""
    if first_ok:
        return 'first', None
    for t in range(n_thr):
        c = voter_choice(table['good'][b, t], table['rmse'][b, t], table['hom_ok'][b, t], table['hom_rmse'][b, t], table['raises'][b, t],
                         max_rmse, max_rmse_rel)
        if c == 'raise':
            return None, t
        if c is not None:
            return c, t
    return None, None
