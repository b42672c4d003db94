"""Frames and the host reference for tests/test_labels_gpu.py (and tools/bench_labels.py): annotations in the SoccerNet form
{class: [{'x', 'y'}, ...]} (normalised), and what annotations.get_intersections / frames.annot_to_keypoints /
augment.FixLRAmbiguous make of them.  The reference of a set of frames is computed once per process and handed out unchanged."""
import json
import os
from unittest import mock

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
W, H = 960.0, 540.0


def to_annot(points: dict) -> dict:
    return {k: [{'x': float(p[0]), 'y': float(p[1])} for p in v] for k, v in points.items()}


def px(points_px: dict) -> dict:
    """{class: [(x, y) in pixels]} -> annotation."""
    return {k: [{'x': x / W, 'y': y / H} for x, y in v] for k, v in points_px.items()}


def fixture_frames():
    cases = json.load(open(os.path.join(GOLD, 'annotations.json')))
    return [to_annot(c['points']) for c in cases], cases


def synthetic_frames(n=40):
    from sncal_amd import synth
    return [to_annot(synth.synthetic_annotation(seed)[0]) for seed in range(n)]


def _wide_camera(pos, target, f):
    from sncal_amd import synth
    cam = synth.Camera(960, 540)
    pos, target = np.asarray(pos, dtype=np.float64), np.asarray(target, dtype=np.float64)
    d = target - pos
    pan, tilt = np.arctan2(d[0], -d[1]), np.arctan2(np.hypot(d[0], d[1]), d[2])
    cam.position = pos
    cam.rotation = np.transpose(synth.pan_tilt_roll_to_orientation(pan, tilt, 0.0))
    cam.xfocal_length = cam.yfocal_length = np.float64(f)
    cam.calibration = np.array([[f, 0, 480.0], [0, f, 270.0], [0, 0, 1.0]])
    return cam


def camera_annotation(pos, target, f, seed=0):
    """synth.synthetic_annotation's polylines for a camera of the test's choosing."""
    from sncal_amd import synth
    with mock.patch.object(synth, 'random_camera', lambda rng: _wide_camera(pos, target, f)):
        return to_annot(synth.synthetic_annotation(seed)[0])


# behind-the-goal cameras: the lines perpendicular to the pitch's axis run horizontally in the image.  (position, target, focal):
# the first two see one half only (FixLRAmbiguous decides by the count of names), the last two both halves (by the medians)
BEHIND_GOAL = [((-90.0, 2.0, -14.0), (-46.0, 0.0, 0.0), 2000.0), ((78.0, -3.0, -10.0), (47.0, 1.0, 0.0), 1400.0),
               ((-95.0, 1.0, -30.0), (-10.0, 0.0, 0.0), 700.0), ((100.0, -2.0, -35.0), (5.0, 0.0, 0.0), 650.0)]


def behind_goal_frames():
    """Each camera's annotation as given and with its names mirrored (what FixLRAmbiguous exists to undo)."""
    from sncal_amd.augment import flip_annot_names
    out = []
    for i, (pos, target, f) in enumerate(BEHIND_GOAL):
        a = camera_annotation(pos, target, f, seed=100 + i)
        out += [a, flip_annot_names(a, swap_top_bottom=False, swap_posts=False)]
    return out


def _ellipse(cx, cy, rx, ry, n, a0=0.0, a1=2 * np.pi, rot=0.0):
    t = np.linspace(a0, a1, n, endpoint=False)
    c, s = np.cos(rot), np.sin(rot)
    return [(cx + rx * np.cos(u) * c - ry * np.sin(u) * s, cy + rx * np.cos(u) * s + ry * np.sin(u) * c) for u in t]


def hand_built():
    """name -> a batch of 1 to 3 annotations, each built for one path of the label code."""
    overhead = ((0.0, 75.0, -60.0), (0.0, 0.0, 0.0), 420.0)                # the whole pitch in view
    full = camera_annotation(*overhead, seed=7)

    # five clicks spread over the whole circle: five on a short arc make the exactly determined fit so ill-conditioned that the HOST's
    # own labels move by 2e-2 px when its inputs move by one ulp (measured), which no comparison can bound
    spread5 = full['Circle central'][::max(len(full['Circle central']) // 5, 1)][:5]

    def keep(*names):
        return {k: full[k] for k in names}
    cases = {
        'no annotation': [{}],
        'one class only': [px({'Middle line': [(480, 20), (470, 250), (455, 500)]}), {'Circle central': full['Circle central']}],
        'two vertical lines': [px({'Side line left': [(100, 50), (100.2, 300), (99.9, 500)], 'Big rect. left top': [(300, 60), (300.3, 200)],
                                   'Side line top': [(100.1, 40), (100.3, 45)]})],
        'one vertical and one sloped line': [px({'Middle line': [(480, 20), (480.2, 250), (479.9, 500)],
                                                 'Side line top': [(100, 80), (400, 70), (700, 61), (900, 55)],
                                                 'Side line bottom': [(50, 500), (900, 470)]})],
        '2-point polylines': [px({'Side line left': [(120, 60), (80, 480)], 'Side line top': [(110, 70), (800, 40)],
                                  'Side line bottom': [(90, 470), (850, 520)], 'Middle line': [(500, 50), (520, 500)]})],
        'circle of 4 and of 5 points': [dict(keep('Side line top', 'Side line bottom', 'Middle line', 'Side line left', 'Side line right'),
                                             **{'Circle central': full['Circle central'][:4]}),
                                        dict(keep('Side line top', 'Side line bottom', 'Middle line', 'Side line left', 'Side line right'),
                                             **{'Circle central': spread5})],
        '3, 4 and 5 known ground points': [keep('Side line left', 'Side line top', 'Side line bottom', 'Big rect. left top', 'Circle central'),
                                           keep('Side line left', 'Side line top', 'Side line bottom', 'Middle line', 'Circle central'),
                                           keep('Side line left', 'Side line top', 'Side line bottom', 'Middle line', 'Big rect. left top',
                                                'Circle left')],
        'tangent reference inside the ellipse': [px({'Middle line': [(480, 20), (480.1, 250), (480.2, 500)],
                                                     'Side line top': [(100, 205), (480, 200), (900, 195)],
                                                     'Side line bottom': [(100, 520), (900, 515)],
                                                     'Circle central': _ellipse(480, 260, 170, 110, 12)})],
        'near-horizontal cutting line': [px({'Middle line': [(200, 262), (480, 270), (760, 281)],
                                             'Circle central': _ellipse(480, 270, 120, 60, 16, rot=0.1),
                                             'Side line left': [(400, 30), (420, 500)], 'Small rect. left main': [(300, 400), (310, 520)]}),
                                         px({'Middle line': [(200, 262), (480, 270), (760, 281)],
                                             'Circle central': _ellipse(480, 270, 120, 60, 16, rot=0.1)}),
                                         px({'Big rect. right main': [(300, 300), (500, 304), (700, 311)],
                                             'Circle right': _ellipse(500, 330, 150, 70, 9, np.pi, 2 * np.pi)})],
        'long polylines': [px({'Circle central': _ellipse(480, 270, 200, 90, 300, rot=-0.05),
                               'Middle line': [(470 + 0.05 * i, 20 + 2.5 * i + 0.3 * np.sin(i)) for i in range(200)],
                               'Side line top': [(10 + 4.7 * i, 100 - 0.02 * i + 0.2 * np.cos(i)) for i in range(200)],
                               'Side line bottom': [(10 + 4.7 * i, 500 + 0.03 * i) for i in range(150)]})],
    }
    return cases


_CACHE = {}


def host_reference(annots, margin=0.0, key=None):
    """[(labels {id: (x, y) or None}, mask list, keypoints row, mask vector)] of get_intersections / annot_to_keypoints per
    frame; cached under `key`."""
    from sncal_amd import annotations as an
    from sncal_amd import frames
    k = (key, margin)
    if key is not None and k in _CACHE:
        return _CACHE[k]
    seen = []

    def spy(points, **kw):                                  # annot_to_keypoints' own call, so the frame's geometry runs once
        seen.append(an.get_intersections(points, **kw))
        return seen[-1]
    out = []
    with mock.patch.object(frames, 'get_intersections', spy):
        for a in annots:
            row, vec = frames.annot_to_keypoints(a, 57, margin)
            labels, mask = seen[-1]
            out.append((labels, sorted(mask), row, vec))
    if key is not None:
        _CACHE[k] = out
    return out
