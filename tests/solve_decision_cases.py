"""The camera solve's DECISIONS as a table: which points a frame is solved on, which line intersections are let in, which branch
produced the camera and in which threshold pass (CameraCreator, prediction.py:138-437 of the reference).

Every case is one noise-free frame: the float32 projections of the 57 template points under one broadcast camera (all 57 in front of
it; a projection outside the image is still a valid correspondence -- the confidences alone decide what is "detected").  Every point
whose membership a case decides carries a deliberate offset of 2-4 px, and so does at least one point inside the expected set: the
minimum the solve reaches is then the offsets' contribution, well away from 0, and a point more or less shows in the rmse.

The expected point sets come from `expected()` below, a restatement of the reference's selection rules in python sets that cites its
lines -- neither from oracle/solve.py nor from the kernel.  tests/test_solve_decisions_host.py holds the oracle to this table,
tests/test_solve_decisions_gpu.py the kernel.

Not in the table: min_points_for_refinement.  On clean frames the pose calibrateCamera leaves is already at refine_camera's minimum,
so whether the refinement ran is not observable; noise would make it so, and noisy frames are what this table avoids.
"""
import numpy as np

from oracle import camera_math as cm
from oracle import synth
from oracle.pitch import GOAL_LEFT, GOAL_RIGHT, GROUND, KEEP_POINTS, pitch_points

P = pitch_points()
IMG_W, IMG_H = 960, 540
# make_submit.py:45-50
KW = dict(conf_thresh=0.5, conf_threshs=[0.5, 0.35, 0.2], max_rmse=55.0, max_rmse_rel=5.0, min_points=5, min_focal_length=10.0,
          min_points_per_plane=6, min_points_for_refinement=6, reliable_thresh=57)
STATUS_OF_TAG = {'original': 1, 'original_hom': 2, 'camera_rel': 3, 'camera_acc': 4, 'cam_all': 5, 'cam_ground': 6, 'voter_hom': 7,
                 'opencv_calibration': 1, 'multiplane': 1}      # oracle/solve.py's tags -> sncal_camera.status
F02, F035 = np.float32(0.2), np.float32(0.35)                  # as doubles: 0.2000000030 > 0.2, 0.3499999940 < 0.35
ABOVE_05 = np.nextafter(np.float32(0.5), np.float32(1))


def base_camera():
    """oracle.synth.sample_camera of seed 2 (sees the left half, both posts of the left goal and the centre circle's left side), turned
    about its own centre by two fixed angles so that template point 15 projects 2.6 px inside the right image border and point 13
    2.6 px below the top one: the border clauses of prediction.py:361-362 can then be put to candidates that are 2-4 px off."""
    cam = synth.sample_camera(np.random.Generator(np.random.PCG64(2)))
    a, b = 0.03006, 0.16713
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return dict(cam, rotation=rx @ ry @ cam['rotation'])


def base_frame():
    cam = base_camera()
    assert ((P - cam['position']) @ cam['rotation'].T)[:, 2].min() > 30          # all 57 points in front of the camera
    return np.array([cm.project_point(cam['position'], cam['rotation'], cam['f'], cam['f'], cam['pp'], P[i])[:2] for i in range(57)],
                    dtype=np.float32)


BASE = base_frame()
# offsets of the contested points, by id (2-4 px each); the top-gate "spoilers" of the cam_ground case are the one exception
OFF = {0: (2.0, 2.5), 1: (-2.5, 2.0), 2: (2.0, -2.5), 3: (-2.0, 2.5), 4: (2.5, 2.0), 5: (-3.0, 1.0), 6: (2.0, 3.0), 7: (-2.0, -2.0),
       9: (3.0, -2.0), 13: (1.5, -2.6), 15: (2.6, 1.5), 31: (2.0, 2.0), 33: (-2.0, 2.5), 35: (3.0, 0.0), 39: (0.0, -3.0),
       44: (-2.0, 3.0), 45: (2.0, -2.0), 48: (0.0, 3.0)}


def _case(name, algorithm, conf, status, off=(), lines=None, thr=None, kw=None, near=(), rule=''):
    """conf {id: confidence} (0.01 elsewhere); off: ids that carry their OFF offset as keypoints; lines {id: (dx, dy, valid)}: a
    candidate at the id's projection + (dx, dy), or {id: (x, y, valid, 'abs')} at (x, y); thr: the threshold pass that yields the camera
    (iterative_voter's voter stage: one of conf_threshs); near: neighbour sets, each {'add': ids, 'drop': ids} relative to the
    expected set."""
    kp = np.zeros((57, 3), dtype=np.float32)
    kp[:, :2] = BASE
    kp[:, 2] = 0.01
    for i in off:
        kp[i, :2] = BASE[i] + np.float32(OFF[i])
    for i, c in conf.items():
        kp[i, 2] = c
    line_pts = None
    if lines is not None:
        line_pts = np.zeros((30, 3), dtype=np.float32)
        for i, v in lines.items():
            xy = v[:2] if len(v) == 4 else BASE[i] + np.float32(v[:2])
            line_pts[i] = (xy[0], xy[1], v[2])
    return dict(name=name, algorithm=algorithm, kw=dict(kw or {}), kp=kp, line_pts=line_pts, status=status, thr=thr, near=list(near),
                rule=rule)


# ---- the reference's selection rules, restated ---------------------------------------------------------------------------------------
def select(kp, thr, reliable_thresh=None):
    """prediction.py:263-268 (voter), :178-185 / :345-354 with the reliable rule.  `conf > self.conf_thresh` on a float32 SCALAR is a
    double comparison under the reference's numpy (1.24); n_det_points (:178, :345) compares the float32 COLUMN: a float32 comparison."""
    det = {i for i in range(57) if float(kp[i, 2]) > float(thr)}
    if reliable_thresh is None:
        return det
    n_det = sum(1 for i in range(57) if np.float32(kp[i, 2]) > np.float32(thr))
    return {i for i in det if n_det < reliable_thresh or i in KEEP_POINTS}


def admit(ids, line_pts, mode, cfg):
    """The three ingestion rules for line intersections, candidates in ascending id order: mode 0 prediction.py:356-364
    (original_voter: the ground count is the keypoints', fixed), mode 1 :270-278 (voter: the ground count is re-evaluated after every
    addition, top gates do not count), mode 2 :186-192 (multiplane: the point count, re-evaluated)."""
    ids = set(ids)
    if line_pts is None:
        return ids
    n_ground_kp = len(ids & set(GROUND))
    for i in range(30):
        x, y, valid = (float(v) for v in line_pts[i])
        if valid <= 0.5 or i in ids:
            continue
        if mode == 0:
            take = n_ground_kp < cfg['min_points_per_plane'] or (0 <= x <= IMG_W and 0 <= y <= IMG_H)
        elif mode == 1:
            take = len(ids & set(GROUND)) < cfg['min_points_per_plane']
        else:
            take = len(ids) <= cfg['min_points']
        if take:
            ids.add(i)
    return ids


def has_view(ids, cfg):      # prediction.py:207-212, 389-394: a plane is a view from min_points_per_plane points on
    return any(len(ids & set(plane)) >= cfg['min_points_per_plane'] for plane in (GROUND, GOAL_LEFT, GOAL_RIGHT))


def expected(case):
    """(status, ids, thr) the reference's rules give the case.  For the voter stages the winner among the candidate cameras is the
    table's statement (`status`, `thr`); everything else, the point set included, follows from the rules.  On these clean frames a
    calibrated camera is a good camera and the homography camera's rmse is far below 26 px unless the case says otherwise."""
    cfg = dict(KW, **case['kw'])
    kp, lp, alg = case['kp'], case['line_pts'], case['algorithm']
    if alg == 'opencv_calibration':                              # :143-151
        ids = select(kp, cfg['conf_thresh']) & set(GROUND)
        return (1, ids, cfg['conf_thresh']) if len(ids) > 5 else (0, set(), None)
    if alg == 'opencv_calibration_multiplane':                   # :178-215
        ids = admit(select(kp, cfg['conf_thresh'], cfg['reliable_thresh']), lp, 2, cfg)
        return (1, ids, cfg['conf_thresh']) if has_view(ids, cfg) and len(ids) > cfg['min_points'] else (0, set(), None)
    if alg in ('original_voter', 'iterative_voter'):             # :345-437 (iterative_voter runs it at 0.5, :246)
        thr = 0.5 if alg == 'iterative_voter' else cfg['conf_thresh']
        ids = admit(select(kp, thr, cfg['reliable_thresh']), lp, 0, cfg)
        if has_view(ids, cfg) and len(ids) > cfg['min_points']:                  # :396-397
            return 1, ids, thr
        if len(ids & set(GROUND)) >= 4 and not case.get('hom_spoiled'):          # :434, get_camera_from_homography :497
            return 2, ids, thr
        if alg == 'original_voter':
            return 0, set(), None
    # voter (:259-330), for iterative_voter at each threshold in turn (:253-257): a pass with four ground points has a homography camera
    # and so, on a clean frame, ends with some camera
    for thr in ([cfg['conf_thresh']] if alg == 'voter' else cfg['conf_threshs']):
        m = admit(select(kp, thr), lp, 1, cfg)
        if len(m & set(GROUND)) >= 4:
            break
    else:
        return 0, set(), None
    assert alg == 'voter' or thr == case['thr'], (case['name'], thr)
    cut = {3: set(KEEP_POINTS), 5: set(range(57)), 6: set(GROUND), 7: set(range(57))}[case['status']]     # :558-570; 4 (:572-606) is not in the table
    return case['status'], m & cut, thr


def observations(case, thr):
    """{id: (x, y)} the frame offers at the pass `thr`: the keypoint's coordinates for a detected id, the candidate's for an
    undetected id that has one (prediction.py:189, 273, 359: a candidate never replaces a keypoint)."""
    kp, lp = case['kp'], case['line_pts']
    obs = {i: (float(kp[i, 0]), float(kp[i, 1])) for i in range(57)}
    if lp is not None and thr is not None:
        for i in range(30):
            if (lp[i, 0] != 0 or lp[i, 1] != 0) and not float(kp[i, 2]) > float(thr):
                obs[i] = (float(lp[i, 0]), float(lp[i, 1]))
    return obs


HI = 0.9
G8 = [3, 4, 5, 8, 11, 44, 45, 48]                    # eight ground points, all in keep_points
NONKEEP = [31, 33, 35, 39]


def _c(ids, c=HI):
    return {i: c for i in ids}


CASES = [
    # strict `>` in double
    _case('gt_f32_0.2', 'iterative_voter', {**_c([4, 8, 45]), **_c([3, 5, 9, 11, 13, 44, 48], F02)}, 3, off=[9, 44], thr=0.2,
          near=[dict(drop=[9]), dict(drop=[44]), dict(drop=[3, 5, 9, 11, 13, 44, 48])], rule='float32(0.2) > 0.2: no camera at 0.5 / 0.35, all points at 0.2'),
    _case('gt_f32_0.35', 'iterative_voter', {**_c([4, 8, 45]), **_c([3, 5, 9, 11, 13, 44, 48], F035), 6: 0.3}, 3, off=[9, 6], thr=0.2,
          near=[dict(drop=[6]), dict(drop=[9])], rule='float32(0.35) > 0.35 is false: the pass at 0.35 has three points, the one at 0.2 also the point at 0.3'),
    _case('gt_above_0.5', 'original_voter', {**_c([4, 5, 8, 9, 11, 44]), **_c([13, 48], 0.5), **_c([3, 45], ABOVE_05)}, 1, off=[9, 13, 48, 3, 45],
          near=[dict(add=[13, 48]), dict(drop=[3, 45]), dict(add=[13]), dict(drop=[3])], rule='0.5 is out, nextafter(0.5) is in'),
    # reliable rule
    _case('rel_14_original', 'original_voter', _c(G8 + [9, 13] + NONKEEP), 1, off=[9] + NONKEEP, kw=dict(reliable_thresh=12),
          near=[dict(add=NONKEEP), dict(add=[31])], rule='14 detected >= reliable_thresh: keep_points only'),
    _case('rel_11_original', 'original_voter', _c(G8[:6] + [9] + NONKEEP), 1, off=[9] + NONKEEP, kw=dict(reliable_thresh=12),
          near=[dict(drop=NONKEEP), dict(drop=[31])], rule='11 detected < reliable_thresh: all of them'),
    _case('rel_14_multiplane', 'opencv_calibration_multiplane', _c(G8 + [9, 13] + NONKEEP), 1, off=[9] + NONKEEP, kw=dict(reliable_thresh=12),
          near=[dict(add=NONKEEP), dict(add=[39])], rule='14 detected >= reliable_thresh: keep_points only'),
    _case('rel_11_multiplane', 'opencv_calibration_multiplane', _c(G8[:6] + [9] + NONKEEP), 1, off=[9] + NONKEEP, kw=dict(reliable_thresh=12),
          near=[dict(drop=NONKEEP), dict(drop=[39])], rule='11 detected < reliable_thresh: all of them'),
    _case('rel_count_f32', 'opencv_calibration_multiplane', {**_c(G8[:6] + [9] + NONKEEP[:3]), **_c([13, 48], F02)}, 1, off=[9] + NONKEEP[:3],
          kw=dict(reliable_thresh=12, conf_thresh=0.2), near=[dict(drop=NONKEEP[:3]), dict(drop=[13, 48])],
          rule='n_det_points compares the float32 column: two points at float32(0.2) are points but do not count, 10 < 12'),
    # line points, mode 0 (original_voter)
    _case('m0_in_image', 'original_voter', _c(G8), 1, off=[4], lines={9: (*OFF[9], 1)}, near=[dict(drop=[9])], rule='in-image candidate, 8 ground keypoints: taken'),
    _case('m0_border_in', 'original_voter', _c(G8), 1, off=[4], lines={15: (960.0, BASE[15, 1] + 1.5, 1, 'abs'), 13: (BASE[13, 0] + 1.5, 0.0, 1, 'abs')},
          near=[dict(drop=[15]), dict(drop=[13]), dict(drop=[13, 15])], rule='x = 960.0 and y = 0.0 are inside (<=)'),
    _case('m0_border_out', 'original_voter', _c(G8), 1, off=[4], lines={15: (960.5, BASE[15, 1] + 1.5, 1, 'abs'), 13: (BASE[13, 0] + 1.5, -0.5, 1, 'abs')},
          near=[dict(add=[15]), dict(add=[13]), dict(add=[13, 15])], rule='x = 960.5 and y = -0.5 are outside, 8 ground keypoints: not taken'),
    _case('m0_out_5_ground', 'original_voter', _c([4, 5, 8, 44, 48, 0, 1]), 1, off=[4], lines={15: (960.5, BASE[15, 1] + 1.5, 1, 'abs'), 13: (BASE[13, 0] + 1.5, -0.5, 1, 'abs')},
          near=[dict(drop=[15]), dict(drop=[13]), dict(drop=[13, 15])], rule='the same candidates with 5 ground keypoints (top gates do not count): taken'),
    _case('m0_present', 'original_voter', _c(G8 + [9]), 1, off=[4], lines={9: (30.0, 20.0, 1)}, near=[dict(drop=[9])],
          rule='candidate for a detected id: ignored, the keypoint counts'),
    _case('m0_invalid', 'original_voter', _c(G8), 1, off=[4], lines={9: (*OFF[9], 0)}, near=[dict(add=[9])], rule='valid = 0: ignored'),
    # line points, mode 1 (voter)
    _case('m1_order', 'voter', _c([8, 9, 44, 48]), 3, off=[9], lines={i: (*OFF[i], 1) for i in (0, 2, 3, 4, 5, 6)},
          near=[dict(add=[4]), dict(drop=[0], add=[4]), dict(drop=[0]), dict(add=[4, 5, 6]), dict(drop=[3])],
          rule='4 ground keypoints: 0, 2, 3 are added -- ascending, count re-evaluated, the top gate does not count'),
    _case('m1_6_ground', 'voter', _c([8, 9, 11, 44, 45, 48]), 3, off=[9], lines={i: (*OFF[i], 1) for i in (0, 2, 3, 4, 5, 6)},
          near=[dict(add=[0]), dict(add=[2]), dict(add=[0, 2, 3])], rule='6 ground keypoints: nothing is added'),
    # line points, mode 2 (multiplane)
    _case('m2_stop', 'opencv_calibration_multiplane', _c([8, 9, 44, 48]), 1, off=[9], lines={i: (*OFF[i], 1) for i in (2, 3, 4, 5, 6, 7)},
          near=[dict(add=[4]), dict(drop=[3]), dict(add=[4, 5, 6, 7])], rule='4 keypoints + 6 candidates: additions stop at 6 points'),
    # gates
    _case('oc_5_ground', 'opencv_calibration', _c([4, 5, 8, 44, 48, 0, 1]), 0, off=[4, 0, 1], rule='5 ground + 2 top-gate points: len > 5 fails'),
    _case('oc_6_ground', 'opencv_calibration', _c([4, 5, 8, 9, 44, 48, 0, 1]), 1, off=[4, 0, 1], near=[dict(add=[0, 1]), dict(add=[0])],
          rule='6 ground points: a camera on those 6'),
    _case('min7_7', 'original_voter', _c([4, 5, 8, 9, 11, 44, 48]), 2, off=[9], kw=dict(min_points=7), near=[dict(drop=[9])],
          rule='7 points, min_points 7: > fails, homography fallback'),
    _case('min7_8', 'original_voter', _c([4, 5, 8, 9, 11, 44, 45, 48]), 1, off=[9], kw=dict(min_points=7), near=[dict(drop=[9])],
          rule='8 points, min_points 7: calibrated'),
    _case('plane_5', 'original_voter', _c([4, 5, 8, 9, 44, 0, 1]), 2, off=[9, 0, 1], near=[dict(drop=[0, 1]), dict(drop=[0])],
          rule='5 ground points are no view (7 points > min_points): homography fallback on all 7'),
    _case('plane_6', 'original_voter', _c([4, 5, 8, 9, 44, 45, 0, 1]), 1, off=[9, 0, 1], near=[dict(drop=[0, 1]), dict(drop=[0])],
          rule='6 ground points are a view: calibrated'),
    _case('ground_3', 'iterative_voter', _c([4, 8, 48]), 0, rule='3 ground points: no camera at any threshold, the record stays zero'),
    # threshold order and voter selection (iterative_voter)
    _case('it_0.35_hom', 'iterative_voter', {**_c([4, 8, 48]), **_c([9, 44], 0.4)}, 7, off=[9], thr=0.35, near=[dict(drop=[9]), dict(drop=[9, 44])],
          rule='3 points at 0.5, 5 at 0.35: no plane is a view, voter_hom'),
    _case('it_0.35_rel', 'iterative_voter', {**_c([4, 8, 48]), **_c([0, 1, 3, 5, 9, 11, 44, 45] + NONKEEP, 0.4), **_c([13, 6], 0.3)}, 3, off=[0, 1, 9, 13, 6], thr=0.35,
          near=[dict(add=[13]), dict(add=[6]), dict(add=[6, 13]), dict(drop=[9]), dict(add=NONKEEP), dict(add=[31]), dict(drop=[0, 1]), dict(drop=[0, 1], add=NONKEEP)],
          rule='camera at 0.35: the points at 0.3 stay out; camera_rel by its flag, on keep_points only, though cam_ground (without the two offset top gates) has the lower rmse'),
]
# the cam_ground case: both posts' tops 200 px off spoil every camera that uses them -- the homography camera of the first pass (rmse >= 26)
# and the voter's rel / acc / all candidates -- so that the ground-plane camera wins by rmse
_g = _case('it_0.5_ground', 'iterative_voter', _c([3, 4, 5, 8, 9, 11, 13, 44, 45, 48, 0, 1]), 6, off=[9, 44], thr=0.5, kw=dict(min_points=20),
           near=[dict(drop=[9]), dict(drop=[44]), dict(add=[0])], rule='original_voter fails (min_points 20, homography rmse >= 26); voter at 0.5: cam_ground by rmse')
_g['kp'][0, :2] += np.float32((200.0, 150.0))
_g['kp'][1, :2] += np.float32((-200.0, 150.0))
_g['hom_spoiled'] = True
CASES.append(_g)

for _case_ in CASES:
    _st, _ids, _thr = expected(_case_)
    assert _st == _case_['status'], (_case_['name'], _st)
    _obs = observations(_case_, _thr)
    _case_['ids'] = sorted(_ids)
    _case_['obs'] = {i: _obs[i] for i in sorted(_ids)}
    _case_['near_obs'] = [{i: _obs[i] for i in sorted((_ids - set(n.get('drop', []))) | set(n.get('add', [])))} for n in _case_['near']]
    assert all(set(n) != _ids for n in _case_['near_obs']), _case_['name']


def lines_data(case, name):
    """The case's candidates as CameraCreator.lines_data: {name: {id: (x, y)}} -- the valid ones (a lines file holds no others)."""
    lp = case['line_pts']
    if lp is None:
        return {}
    return {name: {i: (float(lp[i, 0]), float(lp[i, 1])) for i in range(30) if lp[i, 2] > 0.5}}


_ORACLE = {}


def oracle_camera(name):
    """oracle/solve.py's camera for the case (None = no camera), computed once per process and shared by the tests that need it."""
    if name not in _ORACLE:
        from oracle import solve
        c = next(c for c in CASES if c['name'] == name)
        oc = solve.CameraCreatorOracle(algorithm=c['algorithm'], lines_data=lines_data(c, 'frame.jpg'), **dict(KW, **c['kw']))
        _ORACLE[name] = oc(c['kp'].copy(), 'frame.jpg')
    return _ORACLE[name]
