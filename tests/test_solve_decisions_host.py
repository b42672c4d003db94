"""CPU: the decision table of tests/solve_decision_cases.py against oracle/solve.py.

The table states the reference's selection rules (prediction.py:138-437) in python sets; this file shows that the oracle has the same
rules -- None-ness, branch and the ids the camera's rmse was measured on -- and that the cases discriminate: every neighbour set (what
a wrong rule would have used) moves the rmse by more than 1e-3 px, and in every voter case either camera_rel's flag decides or the
winner's rmse lies at least 10 % below the runner-up's, so that no winner hangs on the last bits of a minimiser.  The GPU half is
tests/test_solve_decisions_gpu.py.  min_points_for_refinement is left out on purpose (the table's docstring says why)."""
import numpy as np
import pytest

import solve_decision_cases as T

NAMES = [c['name'] for c in T.CASES]
BY_NAME = {c['name']: c for c in T.CASES}


oracle_camera = T.oracle_camera


def rmse_over(cam, obs):
    ids = sorted(obs)
    return cam.projection_rmse(ids, np.array([obs[i] for i in ids], dtype=np.float64))


def test_the_table_covers_every_rule():
    assert len(T.CASES) >= 22 and len(set(NAMES)) == len(NAMES)
    for prefix in ('gt_', 'rel_', 'm0_', 'm1_', 'm2_', 'oc_', 'min7_', 'plane_', 'ground_3', 'it_'):
        assert any(n.startswith(prefix) for n in NAMES), prefix
    voter_stage = {c['status'] for c in T.CASES if c['algorithm'] in ('voter', 'iterative_voter')}
    assert {0, 3, 6, 7} <= voter_stage                                          # camera_rel, cam_ground, voter_hom and no camera
    assert {c['thr'] for c in T.CASES if c['algorithm'] == 'iterative_voter' and c['status']} == {0.5, 0.35, 0.2}
    # numpy compares a float32 scalar with a python float in double under the reference's numpy: the table's threshold cases rest on this
    assert float(T.F02) > 0.2 and not float(T.F035) > 0.35 and not float(np.float32(0.5)) > 0.5 and float(T.ABOVE_05) > 0.5
    for i, d in T.OFF.items():
        assert 2.0 <= np.hypot(*d) <= 4.0, i
    for c in T.CASES:                                                           # a case with a camera has an offset point inside its set
        moved = {i for i in range(57) if not np.array_equal(c['kp'][i, :2], T.BASE[i])}
        cand = set() if c['line_pts'] is None else {i for i in range(30) if c['line_pts'][i, 2] > 0.5}
        assert c['status'] == 0 or (moved | cand) & set(c['ids']), c['name']
        assert c['kp'].dtype == np.float32 and c['kp'].shape == (57, 3)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_agrees_with_the_table(name):
    c, o = BY_NAME[name], oracle_camera(name)
    assert (o is None) == (c['status'] == 0)
    if o is None:
        assert c['ids'] == []
        return
    assert T.STATUS_OF_TAG[o.tag] == c['status'], o.tag
    assert sorted(o.ids) == c['ids']
    assert abs(rmse_over(o, c['obs']) - o.rmse) <= 1e-9 * max(1.0, o.rmse)      # ... and on the coordinates the table says were used


@pytest.mark.parametrize('name', NAMES)
def test_cases_discriminate(name):
    c, o = BY_NAME[name], oracle_camera(name)
    if o is None:
        return
    assert c['near_obs'], 'a case with a camera names what a wrong rule would have used'
    for n in c['near_obs']:
        assert abs(rmse_over(o, n) - o.rmse) > 1e-3, (sorted(n), rmse_over(o, n), o.rmse)
    if name == 'm0_present':                                                    # the candidate's coordinates in the keypoint's place
        lp = c['line_pts']
        assert abs(rmse_over(o, {**c['obs'], 9: (float(lp[9, 0]), float(lp[9, 1]))}) - o.rmse) > 1e-3
    if c['status'] >= 3:                                                        # voter stage: the candidates are separated
        cands = sorted(o.candidates, key=lambda x: (x[2], 1 / x[1]), reverse=True)
        if c['status'] == 7:
            assert all(r >= dict(T.KW, **c['kw'])['max_rmse'] for _, r, _ in cands), cands      # nobody to beat the homography camera
        else:
            assert cands[0][0] == o.tag
            if name == 'it_0.35_rel':                                          # the flag decides against the rmse here, not with it
                assert min(r for _, r, _ in cands) < 0.9 * o.rmse, cands
            assert len(cands) == 1 or cands[0][2] != cands[1][2] or cands[0][1] <= 0.9 * cands[1][1], cands
