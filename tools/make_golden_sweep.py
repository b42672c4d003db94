"""Writes tests/golden/sweep_cases.npz: oracle/solve.py's table of candidate cameras for the frames of tests/sweep_cases.py -- what the
voter's final choice (prediction.py:293-329) reads, for every frame and every threshold of make_submit.py's conf_threshs:

    good      (N,T,4) bool     camera_rel / camera_acc / cam_all / cam_ground was solved and is a good_camera
    rmse      (N,T,4) float64  its projection_rmse (0 where not good)
    hom_ok    (N,T)   bool     the homography camera exists;  hom_rmse (N,T) float64
    raises    (N,T)   bool     the voter raises at this threshold whatever max_rmse / max_rmse_rel are (get_camera_from_homography's
                               solve_pnp failure)
    first_ok  (N,)    bool     iterative_voter's original_voter pass has a camera: the frame never reaches the voter
    n_synth, threshs

The table does not depend on max_rmse / max_rmse_rel -- that is the point of the sweep.  It is the ORACLE's: the device's cameras
agree with it to the solve's tolerance, not bit for bit, so tests/test_sweep_host.py uses it for coverage statements (with margin)
and tests/test_sweep_gpu.py asserts the same statements on the device's own choices.

    python tools/make_golden_sweep.py        (CPU, a few minutes)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import solve  # noqa: E402
from oracle.pitch import GROUND, KEEP_POINTS  # noqa: E402
import sweep_cases as SC  # noqa: E402


def voter_candidates(oc, pred, name, thr, cache):
    """CameraCreatorOracle.voter up to its selection: the same calls in the same order (oracle/solve.py)."""
    oc.conf_thresh = thr
    ids, uv = oc._select(pred, False)
    for i, p in sorted(oc.lines_data.get(name, {}).items()):
        if i not in ids and sum(1 for k in ids if k in GROUND) < oc.min_points_per_plane:
            ids.append(i)
            uv.append((float(p[0]), float(p[1])))
    uv = np.array(uv, dtype=np.float64).reshape(-1, 2)
    key = (tuple(ids), uv.tobytes())
    if key in cache:                                   # the thresholds of a frame often select the same points
        return cache[key]
    row = dict(good=np.zeros(4, bool), rmse=np.zeros(4), hom_ok=False, hom_rmse=0.0, raises=False)
    try:
        hom = solve.camera_from_homography(ids, uv, oc.img_size)
    except Exception:
        row['raises'] = True
        cache[key] = row
        return row

    def sub(keep):
        k = [j for j, i in enumerate(ids) if keep(i)]
        return solve.camera_all_points([ids[j] for j in k], uv[k], oc.img_size)
    c_all = solve.camera_all_points(ids, uv, oc.img_size)
    c_rel = sub(lambda i: i in KEEP_POINTS)
    c_acc = oc._accurate(ids, uv, 5.0)
    c_gnd = sub(lambda i: i in GROUND)
    for k, c in enumerate((c_rel, c_acc, c_all, c_gnd)):
        if c is not None and solve.good_cam(c[0]):
            row['good'][k], row['rmse'][k] = True, c[1]
    if hom is not None:
        row['hom_ok'], row['hom_rmse'] = True, hom[1]
    cache[key] = row
    return row


def main():
    solve.opencv_stops(SC.KW['refine_max_iters'])
    kp, lp = SC.frames()
    N, T = len(kp), len(SC.THRESHS)
    kw = {k: v for k, v in SC.KW.items() if k != 'refine_max_iters'}
    oc = solve.CameraCreatorOracle(algorithm='voter', lines_data=SC.lines_data(lp), **kw)
    out = dict(good=np.zeros((N, T, 4), bool), rmse=np.zeros((N, T, 4)), hom_ok=np.zeros((N, T), bool), hom_rmse=np.zeros((N, T)),
               raises=np.zeros((N, T), bool), first_ok=np.zeros(N, bool))
    for b in range(N):
        name, cache = SC.frame_name(b), {}
        for t, thr in enumerate(SC.THRESHS):
            row = voter_candidates(oc, kp[b], name, thr, cache)
            for k in ('good', 'rmse', 'hom_ok', 'hom_rmse', 'raises'):
                out[k][b, t] = row[k]
        oc.conf_thresh = 0.5
        try:
            out['first_ok'][b] = oc.original_voter(kp[b], name) is not None
        except Exception:
            out['first_ok'][b] = False
        print(b, out['first_ok'][b], out['raises'][b], np.round(out['rmse'][b, 0], 2), np.round(out['hom_rmse'][b, 0], 2), flush=True)
    path = os.path.join(ROOT, 'tests', 'golden', 'sweep_cases.npz')
    np.savez_compressed(path, n_synth=SC.N_SYNTH, threshs=np.array(SC.THRESHS), **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
