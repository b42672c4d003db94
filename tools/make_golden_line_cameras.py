"""Capture tests/golden/line_cameras.npz from the imported reference (CPU): the dev-kit's cameras from line extremities
(baseline/baseline_cameras.py of the reference checkout) on two case sets.

    python tools/make_golden_line_cameras.py

The reference modules (baseline.baseline_cameras, baseline.camera, baseline.soccerpitch) are imported with empty stub modules for
cv2 and tqdm; everything stored comes from ITS normalization_transform, estimate_homography_from_line_correspondences,
Camera.from_homography, Camera.project_point and SoccerPitch, composed as its __main__ composes them (:174-236).  That block cannot
be imported, so the composition is restated here around the reference's functions (ref_flow).  Camera.refine_camera is never called
(it needs OpenCV): what is stored about the refinement is its start and its data, the matches.

Before anything is captured the tool asserts that the package's tables (baseline_cameras.LINE_ENDS, END_POINTS' coordinates,
on_lawn) equal the imported SoccerPitch's.

Frames are built as decoded peaks (float32 map cells at scale 4), so that both input forms of sncal_baseline_cameras describe the same
frame: the normalised dict holds float64(float32(cell * 4)) / (W - 1, H - 1), what export_extremities writes.  Dicts are in
ANNOT_CLASSES order.

Set A: seeded synthetic views through synth.random_camera; the extremities are the in-image ends of each visible line with noise of
0.5 / 1 / 2 / 4 px; even draws at 960 x 540, odd draws at 1283 x 721.  Set B: hand-built frames (see set_b).

Stored per set, one row per frame: pred.points / pred.offsets (pack_annotations), peaks, peaks_ok (the frame has a peaks form),
img_size, status (before refinement), n_lines, slots (per END_POINTS entry: class id * 2 + end, or -1), T1, T2, H, f, R, pos (NaN
where the reference has none), match_n / match_X / match_uv (the matches in the reference's order), E_ref, and for A the counts
drawn / dropped and the noise per frame.

E_ref is a frame's own conditioning: the largest relative change (max |difference| / max |value| per quantity) of the reference's
H, f, R and position over 8 seeded reruns with every normalised coordinate moved by up to 2^-48 relative.

The tool asserts, and writes nothing otherwise: every status and the four-line case occur in A; no decision of a kept frame of A
(inside-image tests, the depth cut, the 100 px rule, the gap between the nearest and the second candidate) lies within 1e-6 px of
its threshold, and none changes under the reruns; no kept frame's E_ref exceeds 1e-8; the frames dropped for these reasons are at
most 10 % of the frames drawn.
"""
import itertools
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = '/root/reference'
sys.path.insert(0, ROOT)

for _name in ('cv2', 'tqdm'):
    sys.modules[_name] = types.ModuleType(_name)
sys.modules['tqdm'].tqdm = None
sys.path.insert(0, REF)
from baseline import baseline_cameras as ref  # noqa: E402
from baseline.camera import Camera as RefCamera  # noqa: E402
from baseline.soccerpitch import SoccerPitch  # noqa: E402

from sncal_amd import baseline_cameras as bc  # noqa: E402
from sncal_amd.annotations import ANNOT_CLASSES, pack_annotations  # noqa: E402
from sncal_amd.lines import LINE_CLS  # noqa: E402
from sncal_amd.pitch import PITCH_POINTS  # noqa: E402
from sncal_amd.synth import random_camera  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
LINES = [LINE_CLS[i] for i in range(len(LINE_CLS))]
CID = {c: i for i, c in enumerate(ANNOT_CLASSES)}
FIELD = SoccerPitch()
SCALE, P_THRESHOLD, P_KEPT, P_DROPPED = 4, 0.2, 0.9, 0.1
MARGIN_PX, E_MAX, RERUNS, EPS_IN = 1e-6, 1e-8, 8, 2.0 ** -48


def assert_tables():
    assert FIELD.line_extremities_keys == bc.LINE_ENDS
    for name in bc.END_POINTS:
        assert np.array_equal(FIELD.point_dict[name], PITCH_POINTS[name]), name
    for c in ANNOT_CLASSES:
        assert (FIELD.get_2d_homogeneous_line(c) is not None) == bc.on_lawn(c), c
        if bc.on_lawn(c):
            assert np.array_equal(FIELD.get_2d_homogeneous_line(c), bc.pitch_line(c)), c


# ---- the reference's composition ------------------------------------------------------------------------------------

def ref_flow(predictions, W, H):
    """:174-236 around the reference's functions -> dict; the slot ids ride along with the candidates.  `predictions` holds no
    class with fewer than two points (the reference raises IndexError there; the package skips such a class)."""
    line_matches, potential_3d_2d_matches, slots_of, src_pts = [], {}, {}, []
    for k, v in predictions.items():
        if k == 'Circle central' or 'unknown' in k:
            continue
        P3D1, P3D2 = FIELD.line_extremities_keys[k]
        p1 = np.array([v[0]['x'] * W, v[0]['y'] * H, 1.])
        p2 = np.array([v[1]['x'] * W, v[1]['y'] * H, 1.])
        src_pts.extend([p1, p2])
        for P in (P3D1, P3D2):
            potential_3d_2d_matches.setdefault(P, []).extend([p1, p2])
            slots_of.setdefault(P, []).extend([CID[k] * 2, CID[k] * 2 + 1])
        line = np.cross(p1, p2)
        if np.isnan(np.sum(line)) or np.isinf(np.sum(line)):
            continue
        line_pitch = FIELD.get_2d_homogeneous_line(k)
        if line_pitch is not None:
            line_matches.append((line_pitch, line))
    out = {'status': 0, 'n_lines': len(line_matches), 'T1': None, 'T2': None, 'H': None, 'f': None, 'R': None, 'pos': None,
           'slots': {}, 'matches': [], 'margin': np.inf}
    if len(line_matches) < 4:
        return out
    target_pts = [FIELD.point_dict[k][:2] for k in potential_3d_2d_matches.keys()]
    out['T1'] = ref.normalization_transform(target_pts)
    out['T2'] = ref.normalization_transform(src_pts)
    success, homography = ref.estimate_homography_from_line_correspondences(line_matches, out['T1'], out['T2'])
    if not success:
        return out
    out['H'] = homography
    cam = RefCamera(W, H)
    if not cam.from_homography(homography):
        return out
    out.update(status=1, f=float(cam.xfocal_length), R=cam.rotation.copy(), pos=cam.position.copy())
    assert cam.xfocal_length == cam.yfocal_length or abs(cam.xfocal_length - cam.yfocal_length) <= 1e-9 * cam.xfocal_length
    margin = np.inf
    for k, potential_matches in potential_3d_2d_matches.items():
        p3D = FIELD.point_dict[k]
        depth = (cam.rotation @ (p3D - cam.position))[2]
        margin = min(margin, abs(depth - 1e-3) * 1e3)                 # the depth cut of project_point, in mm
        projected = cam.project_point(p3D)
        if depth > 1e-3:
            margin = min(margin, abs(projected[0]), abs(projected[0] - W), abs(projected[1]), abs(projected[1] - H))
        if 0 < projected[0] < W and 0 < projected[1] < H:
            dist = np.zeros(len(potential_matches))
            for i, potential_match in enumerate(potential_matches):
                dist[i] = np.sqrt((projected[0] - potential_match[0]) ** 2 + (projected[1] - potential_match[1]) ** 2)
            selected = np.argmin(dist)
            margin = min(margin, abs(dist[selected] - 100))
            if len(dist) > 1:
                margin = min(margin, np.partition(dist, 1)[1] - dist[selected])
            if dist[selected] < 100:
                out['slots'][k] = slots_of[k][selected]
                out['matches'].append((p3D, potential_matches[selected][:2]))
    out['margin'] = margin
    return out


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def conditioning(pred, W, H, base, seed):
    """(E_ref, decisions unchanged) over RERUNS perturbed reruns."""
    rng = np.random.Generator(np.random.PCG64(seed))
    e, same = 0.0, True
    for _ in range(RERUNS):
        moved = {c: [{'x': p['x'] * (1 + rng.uniform(-EPS_IN, EPS_IN)), 'y': p['y'] * (1 + rng.uniform(-EPS_IN, EPS_IN))} for p in pts]
                 for c, pts in pred.items()}
        with np.errstate(all='ignore'):
            r = ref_flow(moved, W, H)
        same = same and r['status'] == base['status'] and r['slots'] == base['slots'] and r['n_lines'] == base['n_lines']
        if r['H'] is not None and base['H'] is not None:               # a homography without a camera behind it is compared too
            e = max(e, rel(r['H'], base['H']))
        if r['status'] == base['status'] == 1:
            e = max(e, rel(r['f'], base['f']), rel(r['R'], base['R']), rel(r['pos'], base['pos']))
    return e, same


# ---- frames as cells ---------------------------------------------------------------------------------------------------

def to_forms(cells, W, H):
    """{class: [(cx, cy) float32 cells, one or two]} in any order -> (normalised dict in ANNOT_CLASSES order, peaks (23,2,3) or None)."""
    pred, peaks, ok = {}, np.zeros((23, 2, 3), np.float32), True
    for c in ANNOT_CLASSES:
        if c not in cells:
            continue
        pts = [(np.float32(x), np.float32(y)) for x, y in cells[c]]
        px = [(float(x * np.float32(SCALE)), float(y * np.float32(SCALE))) for x, y in pts]
        pred[c] = [{'x': x / (W - 1), 'y': y / (H - 1)} for x, y in px]
        if c in LINES and 1 <= len(pts) <= 2:
            k = LINES.index(c)
            for i in range(2):
                peaks[k, i] = (pts[i][0], pts[i][1], P_KEPT) if i < len(pts) else (3.0, 5.0, P_DROPPED)
        else:
            ok = False
    return pred, peaks, ok


def sized_camera(rng, W, H):
    cam = random_camera(rng)
    s = W / 960.0
    cam.image_width, cam.image_height = W, H
    cam._set_intrinsics(cam.xfocal_length * s, cam.yfocal_length * s, (W / 2, H / 2))
    return cam


def visible_ends(cam, name, W, H, samples=513):
    """The first and the last in-image sample of the line's 3-D segment, in pixels, or None when fewer than 20 px show."""
    a, b = (PITCH_POINTS[k] for k in bc.LINE_ENDS[name])
    t = np.linspace(0.0, 1.0, samples)[:, None]
    q = cam.project_points(a[None] * (1 - t) + b[None] * t)
    ins = np.nonzero((q[:, 2] != 0) & (q[:, 0] >= 0) & (q[:, 0] <= W - 1) & (q[:, 1] >= 0) & (q[:, 1] <= H - 1))[0]
    if len(ins) < 2 or np.hypot(*(q[ins[-1], :2] - q[ins[0], :2])) < 20:
        return None
    return q[ins[0], :2], q[ins[-1], :2]


def synthetic_cells(rng, W, H, sigma, classes=None):
    cam = sized_camera(rng, W, H)
    cells = {}
    for name in (classes or LINES):
        ends = visible_ends(cam, name, W, H)
        if ends is None:
            continue
        cells[name] = [tuple(np.float32((e + rng.normal(0, sigma, 2)) / SCALE)) for e in ends]
    return cells


def without_short(pred):
    return {c: v for c, v in pred.items() if len(v) >= 2 or c == 'Circle central' or 'unknown' in c}


def set_a(seed=20240607, draws=240, keep=48):
    rng = np.random.Generator(np.random.PCG64(seed))
    frames, dropped = [], 0
    for i in range(draws):
        W, H = (960, 540) if i % 2 == 0 else (1283, 721)
        sigma = (0.5, 1.0, 2.0, 4.0)[(i // 2) % 4]
        cells = synthetic_cells(rng, W, H, sigma)
        pred, peaks, ok = to_forms(cells, W, H)
        assert ok
        with np.errstate(all='ignore'):
            r = ref_flow(pred, W, H)
            e, same = conditioning(pred, W, H, r, seed + i)
        if not same or r['margin'] < MARGIN_PX or e > E_MAX:
            dropped += 1
            continue
        frames.append((pred, peaks, ok, (W, H), r, e, sigma))
    assert dropped <= 0.1 * draws, (dropped, draws)

    def kind(fr):
        r = fr[4]
        if r['n_lines'] < 4:
            return 'few'
        if r['status'] == 0:
            return 'failed'
        if r['n_lines'] == 4:
            return 'four'
        return 'refined' if len(r['matches']) > 3 else 'unrefined'
    quota = {'few': 6, 'failed': 6, 'unrefined': 6, 'four': 8}
    kept, seen = [], {}
    for fr in frames:
        k = kind(fr)
        if k in quota and seen.get(k, 0) >= quota[k]:
            continue
        if len(kept) < keep or (k in quota and seen.get(k, 0) < 2):
            kept.append(fr)
            seen[k] = seen.get(k, 0) + 1
    print('A: drawn', draws, 'dropped', dropped, 'kinds', {k: sum(kind(f) == k for f in frames) for k in ('few', 'failed', 'unrefined', 'four', 'refined')},
          'kept', seen)
    assert all(seen.get(k, 0) >= 2 for k in ('few', 'failed', 'unrefined', 'four', 'refined')), seen
    assert any(kind(f) == 'four' and f[4]['status'] == 1 for f in kept), 'no four-line frame with a camera'
    assert {f[3] for f in kept} == {(960, 540), (1283, 721)}
    return kept, draws, dropped


def set_b(seed=77):
    """Hand-built frames at 960 x 540, cut out of one noise-free synthetic view that shows 'Circle left' and at least six lawn lines."""
    W, H = 960, 540
    rng = np.random.Generator(np.random.PCG64(seed))
    for _ in range(4000):
        base = synthetic_cells(rng, W, H, 0.0, classes=LINES + ['Circle left'])
        lawn = [c for c in base if bc.on_lawn(c)]
        if 'Circle left' in base and len(lawn) >= 6 and any(not bc.on_lawn(c) for c in base if c != 'Circle left'):
            with np.errstate(all='ignore'):
                r = ref_flow(to_forms(base, W, H)[0], W, H)
            if r['status'] == 1 and len(r['matches']) > 3:
                break
    else:
        raise AssertionError('no base view')
    lines = {c: v for c, v in base.items() if c != 'Circle left'}
    one = dict(lines)
    one[lawn[0]] = lines[lawn[0]][:1]
    nan = dict(lines)
    nan[lawn[1]] = [(np.float32(np.nan), lines[lawn[1]][0][1]), lines[lawn[1]][1]]
    twice = dict(lines)
    twice[lawn[2]] = [lines[lawn[2]][0], lines[lawn[2]][0]]
    # four lawn lines whose homography (the vector of the smallest of eight singular values) is well conditioned: the first such
    # choice in the order of itertools.combinations
    four = None
    for pick in itertools.combinations(lawn, 4):
        pred4 = to_forms({c: lines[c] for c in pick}, W, H)[0]
        with np.errstate(all='ignore'):
            r4 = ref_flow(pred4, W, H)
            if r4['H'] is not None and conditioning(pred4, W, H, r4, seed)[0] <= 1e-3 * E_MAX:
                four = pick
                break
    assert four is not None
    frames = [
        ('every class absent', {}),
        ('three lawn lines', {c: lines[c] for c in lawn[:3]}),
        ('exactly four lawn lines', {c: lines[c] for c in four}),
        ('posts and crossbars only', {c: [(20.0 + 3 * i, 30.0), (22.0 + 3 * i, 50.0)] for i, c in enumerate(LINES) if not bc.on_lawn(c)}),
        ('a class with one point', one),
        ('a NaN coordinate', nan),
        ('two coincident extremities', twice),
        ('all points equal', {c: [(120.0, 67.5), (120.0, 67.5)] for c in lawn[:5]}),
        ('Circle left: candidates, no line', base),
        ('the base view', lines),
    ]
    out = []
    for i, (what, cells) in enumerate(frames):
        pred, peaks, ok = to_forms(cells, W, H)
        with np.errstate(all='ignore'):
            r = ref_flow(without_short(pred), W, H)
            e, _ = conditioning(without_short(pred), W, H, r, seed + i)
        print(f'B[{i}] {what}: status {r["status"]}, lines {r["n_lines"]}, matches {len(r["matches"])}, E_ref {e:.2e}, peaks form {ok}')
        out.append((pred, peaks, ok, (W, H), r, e, 0.0))
    st = [f[4] for f in out]
    assert [s['status'] for s in st] == [0, 0, st[2]['status'], 0, 1, 0, 1, 0, 1, 1], [s['status'] for s in st]
    assert st[2]['H'] is not None            # four lines: a homography (of the smallest of eight singular values), no camera behind it
    assert st[1]['n_lines'] == 3 and st[2]['n_lines'] == 4 and st[3]['n_lines'] == 0 and st[4]['n_lines'] == len(lawn) - 1
    assert st[5]['n_lines'] == len(lawn) - 1 and st[5]['T2'] is not None and st[5]['H'] is None        # NaN: the SVD raises
    assert st[6]['n_lines'] == len(lawn) and st[7]['n_lines'] == 5 and st[7]['H'] is None              # zero singular values
    assert st[8]['n_lines'] == st[9]['n_lines'] and len(st[8]['slots']) > len(st[9]['slots'])           # the arc's ends are matched
    assert [f[2] for f in out] == [True, True, True, True, True, True, True, True, False, True]
    assert all(f[5] <= E_MAX for f in out)
    return out


def store(out, key, frames):
    n, P = len(frames), len(bc.END_POINTS)
    pts, off, _ = pack_annotations([f[0] for f in frames])
    arr = {'pred.points': pts, 'pred.offsets': off, 'peaks': np.stack([f[1] for f in frames]), 'peaks_ok': np.array([f[2] for f in frames]),
           'img_size': np.array([f[3] for f in frames], np.int32), 'status': np.array([f[4]['status'] for f in frames], np.int32),
           'n_lines': np.array([f[4]['n_lines'] for f in frames], np.int32), 'slots': np.full((n, P), -1, np.int32),
           'T1': np.full((n, 3, 3), np.nan), 'T2': np.full((n, 3, 3), np.nan), 'H': np.full((n, 9), np.nan), 'f': np.full(n, np.nan),
           'R': np.full((n, 9), np.nan), 'pos': np.full((n, 3), np.nan), 'match_n': np.zeros(n, np.int32),
           'match_X': np.zeros((n, P, 3)), 'match_uv': np.zeros((n, P, 2)), 'E_ref': np.array([f[5] for f in frames]),
           'noise': np.array([f[6] for f in frames])}
    for b, f in enumerate(frames):
        r = f[4]
        for name, s in r['slots'].items():
            arr['slots'][b, bc.END_INDEX[name]] = s
        for k2 in ('T1', 'T2'):
            if r[k2] is not None:
                arr[k2][b] = r[k2]
        if r['H'] is not None:
            arr['H'][b] = r['H'].reshape(9)
        if r['status'] == 1:
            arr['f'][b], arr['R'][b], arr['pos'][b] = r['f'], r['R'].reshape(9), r['pos']
        arr['match_n'][b] = len(r['matches'])
        for j, (X, uv) in enumerate(r['matches']):
            arr['match_X'][b, j], arr['match_uv'][b, j] = X, uv
    out.update({f'{key}.{k}': v for k, v in arr.items()})


def main():
    assert_tables()
    out = {'scale': np.float32(SCALE), 'p_threshold': np.float32(P_THRESHOLD), 'end_points': np.array(bc.END_POINTS)}
    kept, draws, dropped = set_a()
    store(out, 'A', kept)
    out['A.drawn'], out['A.dropped'] = np.int32(draws), np.int32(dropped)
    store(out, 'B', set_b())
    path = os.path.join(GOLD, 'line_cameras.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
