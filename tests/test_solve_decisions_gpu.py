"""GPU: the camera solve's decisions (csrc/solve_flow.hpp) against the table of tests/solve_decision_cases.py.

Per case, through sncal_calibrate_ws: the branch (`status`), the size of the point set (`n_points`), and the set itself -- the
record's rmse is Camera.projection_rmse (host mirror) of the returned camera over the table's set to 1e-9, and is NOT that over any of
the neighbour sets a wrong rule would have used (> 1e-4 px apart).  Against oracle/solve.py only the rmse, at the suite's 1e-4
relative; the frames are noise-free, the rmse is the contribution of the table's 2-4 px offsets.  Line points go in both as a device
array and as lines_data + names; batches of every size against single frames, byte for byte.
min_points_for_refinement is not observable on clean frames (the pose is at its minimum already) and is left out on purpose.
The host half, which holds the oracle to the same table: tests/test_solve_decisions_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import solve_decision_cases as T

pytestmark = pytest.mark.gpu
NAMES = [c['name'] for c in T.CASES]
BY_NAME = {c['name']: c for c in T.CASES}
CONFIGS = []                                     # the distinct (algorithm, keywords) of the table
for _c in T.CASES:
    if (_c['algorithm'], _c['kw']) not in CONFIGS:
        CONFIGS.append((_c['algorithm'], _c['kw']))
ALL_KP = np.stack([c['kp'] for c in T.CASES])
ALL_LP = np.stack([c['line_pts'] if c['line_pts'] is not None else np.zeros((30, 3), np.float32) for c in T.CASES])


def creator(sncal, algorithm, kw):
    return sncal.CameraCreator(sncal.PITCH_POINTS, algorithm=algorithm, **dict(T.KW, **kw))


def solve_bytes(cc, cuda, kp, lp):
    """(B, sizeof(sncal_camera)) uint8: the records of one sncal_calibrate_ws call."""
    d_lp = torch.from_numpy(np.ascontiguousarray(lp)).to(cuda) if lp is not None else None
    return cc.solve_device(torch.from_numpy(np.ascontiguousarray(kp)).to(cuda), d_lp).cpu().numpy()


def records(sncal, raw):
    return (sncal._lib.Camera * raw.shape[0]).from_buffer_copy(raw.tobytes())


def host_rmse(sncal, cam, obs):
    return cam.projection_rmse([(sncal.PITCH_POINTS[sncal.pitch.INTERSECTON_TO_PITCH_POINTS[i]], obs[i]) for i in sorted(obs)])


def check_record(sncal, c, rec, raw):
    assert rec.status == c['status'], (c['name'], c['rule'])
    assert rec.n_points == len(c['ids']), (c['name'], c['rule'])
    if c['status'] == 0:
        assert not raw.any(), 'a frame without a camera leaves a record of zero bytes'
        return None
    cam = sncal.prediction.camera_from_record(rec)
    assert cam.n_points == len(c['ids']) and cam.source == sncal.prediction.STATUS_NAMES[c['status']]
    assert abs(host_rmse(sncal, cam, c['obs']) - rec.rmse) <= 1e-9 * max(1.0, rec.rmse), (c['name'], c['rule'])
    for n in c['near_obs']:
        assert abs(host_rmse(sncal, cam, n) - rec.rmse) > 1e-4, (c['name'], sorted(n))
    return cam


@pytest.mark.parametrize('name', NAMES)
def test_case(sncal, cuda, name):
    c = BY_NAME[name]
    cc = creator(sncal, c['algorithm'], c['kw'])
    lp = c['line_pts'][None] if c['line_pts'] is not None else None
    raw = solve_bytes(cc, cuda, c['kp'][None], lp)
    rec = records(sncal, raw)[0]
    cam = check_record(sncal, c, rec, raw)
    o = T.oracle_camera(name)
    assert (o is None) == (cam is None)
    if o is not None:
        print(f'{name}: status {rec.status} n_points {rec.n_points} rmse {rec.rmse:.6f} oracle {o.rmse:.6f} '
              f'rel {abs(rec.rmse - o.rmse) / o.rmse:.2e}')
        assert abs(rec.rmse - o.rmse) <= 1e-4 * o.rmse
    if name == 'm0_present':                     # the candidate's coordinates in the detected keypoint's place would show
        xy = (float(c['line_pts'][9, 0]), float(c['line_pts'][9, 1]))
        assert abs(host_rmse(sncal, cam, {**c['obs'], 9: xy}) - rec.rmse) > 1e-4
    if lp is None:                               # no candidates at all == a row of invalid ones
        assert np.array_equal(raw, solve_bytes(cc, cuda, c['kp'][None], np.zeros((1, 30, 3), np.float32)))
        return
    # the other way in: lines_data + frame names (what a lines file becomes), through line_points_array and through solve_batch
    cc.lines_data = T.lines_data(c, 'frame.jpg')
    arr = cc.line_points_array(['frame.jpg'])
    assert np.array_equal(arr[0][arr[0, :, 2] > 0.5], c['line_pts'][c['line_pts'][:, 2] > 0.5])
    assert np.array_equal(raw, solve_bytes(cc, cuda, c['kp'][None], arr))
    by_name = cc.solve_batch(c['kp'][None], ['frame.jpg'])[0]
    assert by_name.rmse == rec.rmse and by_name.n_points == rec.n_points and by_name.source == cam.source
    assert np.array_equal(by_name.rotation, cam.rotation) and np.array_equal(by_name.position, cam.position)


@pytest.mark.parametrize('cfg', range(len(CONFIGS)), ids=[f"{a}-{'-'.join(f'{k}{v}' for k, v in kw.items()) or 'default'}" for a, kw in CONFIGS])
def test_batches_equal_single_frames(sncal, cuda, cfg):
    """Every frame of the table under one configuration: as one batch, reversed, as batches of 1, 2 and 3 (the partly empty last
    workgroup of every launch form) and frame by frame -- the same bytes per frame; the cases that belong to this configuration meet
    their expectations inside the batch too."""
    algorithm, kw = CONFIGS[cfg]
    cc = creator(sncal, algorithm, kw)
    B = len(T.CASES)
    full = solve_bytes(cc, cuda, ALL_KP, ALL_LP)
    assert full.shape == (B, ctypes.sizeof(sncal._lib.Camera))
    assert np.array_equal(solve_bytes(cc, cuda, ALL_KP[::-1], ALL_LP[::-1])[::-1], full)
    for n in (1, 2, 3):
        assert np.array_equal(solve_bytes(cc, cuda, ALL_KP[B - n:], ALL_LP[B - n:]), full[B - n:]), n
        assert np.array_equal(solve_bytes(cc, cuda, ALL_KP[:n], ALL_LP[:n]), full[:n]), n
    for i in range(B):
        assert np.array_equal(solve_bytes(cc, cuda, ALL_KP[i:i + 1], ALL_LP[i:i + 1]), full[i:i + 1]), T.CASES[i]['name']
    recs = records(sncal, full)
    own = [i for i, c in enumerate(T.CASES) if (c['algorithm'], c['kw']) == (algorithm, kw)]
    assert own
    for i in own:
        check_record(sncal, T.CASES[i], recs[i], full[i])
    for r, raw in zip(recs, full):                                    # whatever the configuration makes of a frame: a camera counts its points
        assert (r.n_points > 0) == (r.status != 0) and (r.status != 0 or not raw.any())
