"""Plain numpy references for the camera evaluation kernel (csrc/evaluate.hip).  No GPU, nothing from the product.

Three things live here, shared by tests/test_evaluate_host.py (CPU) and tests/test_evaluate_edges_gpu.py (GPU):

  hand_table()             a small pitch table and an identity camera whose polylines, distances and confusions are
                           WRITTEN OUT BY HAND below (every sample is a pixel, every distance a 3-4-5 triangle or an
                           axis-aligned offset); the host test holds these literals to the oracle, the GPU test holds
                           the kernel to them
  off_broadcast_cameras()  cameras the broadcast sampler never draws: a metre or two above the grass looking anywhere
                           (thousands of pitch samples behind the camera), and 3x zoomed ones (lines that enter and
                           leave the image many times)
  census() / frame_set() / oracle_results()
                           the oracle's (oracle/evaluate.py) answer on such cameras and a count of which branches of the
                           polyline walk they take
"""
import functools
import math

import numpy as np

from oracle import camera_math as cm
from oracle import evaluate as oe
from oracle import synth

NAN = float('nan')
T5_NEXT = float(np.nextafter(5.0, 6.0))
Z_SKIP = 1e-3                                   # project_point: rz <= 1e-3 is "behind" (camera.py:259)
Z_KEEP = float(np.nextafter(1e-3, 1.0))
UNKNOWN = 'Goal unknown'                        # an annotated class no table has: one FN per frame that carries it


# ------------------------------------------------------------------------------------------------ hand-built table

def hand_table(w=960, h=540, n_cls=16, threshold=5.0):
    """A table of n_cls in (1, 16, 32) classes seen by the identity camera (position 0, rotation I, fx = fy = 1,
    pp = (w/2, h/2)): a sample (X, Y, 1) lands on pixel (X + w/2, Y + h/2) exactly and rz is the sample's own Z.
    Every coordinate below is a PIXEL; the loop after the rows turns it into the table's 3-D point.  All in-image pixels fit in
    333 x 187 so the same rows serve both sizes; only the rows tied to the right / bottom border move with (w, h).

    threshold must be 5.0 or nextafter(5, 6): the two rows with an annotated point at d == 5.0 exactly ('single
    point', 'inside segment') are beyond at the first (strict <) and within at the second.

    Returns a dict: classes, points, class_start, mirror, symmetric, camera, frames (status, gt, gt_extra), and the
    expectations polylines, err (F, 2, C, max_gt), class_conf (F, 2, C, 4), out8 (F, 8), chosen (F,)."""
    assert n_cls in (1, 16, 32) and threshold in (5.0, T5_NEXT)
    at5 = threshold == 5.0

    # name, samples (px, py, Z), expected polyline, annotated points with their expected distance, expected
    # class_conf row [within, beyond, points of an undetected class, detected-but-not-annotated] for self-mirrored rows
    rows = [
        ('single point', [(50, 50, 1)],
         [(50, 50)],
         [((53, 54), 5.0), ((53, 53.9), 4.920365840057018)],                 # sqrt(9 + 3.9^2)
         [1, 1, 0, 0] if at5 else [2, 0, 0, 0]),
        ('inside segment', [(100, 100, 1), (200, 100, 1)],
         [(100, 100), (200, 100)],
         [((150, 103), 3.0), ((97, 96), 5.0), ((204, 103), 5.0), ((150, 100), 0.0)],   # 0<k<1, k<0, k>1, on the line
         [2, 2, 0, 0] if at5 else [4, 0, 0, 0]),
        ('enter', [(-10, 60, 1), (10, 60, 1), (20, 60, 1)],
         [(0, 60), (10, 60), (20, 60)],                                      # border point on x = 0 first
         [((0, 62), 2.0), ((15, 61), 1.0)],
         [2, 0, 0, 0]),
        ('leave', [(60, h - 20, 1), (60, h - 10, 1), (60, h + 10, 1)],
         [(60, h - 20), (60, h - 10), (60, h - 1)],                          # border point on y = h-1, not the sample
         [((63, h - 1), 3.0)],
         [1, 0, 0, 0]),
        ('re-enter', [(w - 20, 80, 1), (w + 20, 80, 1), (w - 20, 90, 1), (w + 20, 90, 1)],
         [(w - 20, 80), (w - 1, 80), (w - 1, 85.25), (w - 20, 90), (w - 1, 90)],    # in, leave, enter, in, leave
         [((w - 10, 93), 3.0), ((w + 2, 82), 3.0)],                          # to the last segment; to the one on the border
         [2, 0, 0, 0]),
        ('half-open x', [(w - 1, 40, 1), (w - 0.5, 40, 1), (w, 40, 1)],
         [(w - 1, 40), (w - 0.5, 40), (w - 1, 40)],                          # x = w is outside: border point, not (w, 40)
         [((w - 0.5, 44), 4.0), ((w + 2.5, 40), 3.0)],
         [2, 0, 0, 0]),
        ('half-open y', [(70, h - 1, 1), (70, h - 0.5, 1), (70, h, 1)],
         [(70, h - 1), (70, h - 0.5), (70, h - 1)],
         [((74, h - 0.5), 4.0), ((70, h + 2.5), 3.0)],
         [2, 0, 0, 0]),
        ('behind boundary', [(120, 20, Z_SKIP), (130, 20, Z_KEEP)],
         [(130, 20)],                                                        # rz == 1e-3 is skipped, the next float is kept
         [((127, 20), 3.0)],
         [1, 0, 0, 0]),
        ('all behind', [(5, 5, 0), (10, 10, -1), (-5, 3, -5)],
         [],
         [((10, 10), NAN), ((20, 20), NAN), ((30, 30), NAN)],                # annotated, not detected: 3 missed points
         [0, 0, 3, 0]),
        ('all behind, not annotated', [(7, 7, 0), (9, 9, -2)],
         [],
         [],
         [0, 0, 0, 0]),
        ('behind then inside', [(5, 5, 0), (-3, 2, -1), (40, 30, 1)],
         [(40, 30)],                                                         # prev is zeros(3): no border point
         [((40, 33), 3.0), ((20, 15), 25.0)],                                # (20, 15) sits on the line to (0, 0)
         [1, 1, 0, 0]),
        ('inside then behind', [(150, 30, 1), (1, 1, 0), (2, -1, -2)],
         [(150, 30)],
         [((150, 34), 4.0)],
         [1, 0, 0, 0]),
        ('duplicate sample', [(160, 50, 1), (160, 50, 1), (180, 50, 1)],
         [(160, 50), (160, 50), (180, 50)],                                  # zero-length segment: k = NaN, end points
         [((170, 53), 3.0)],
         [1, 0, 0, 0]),
        ('detected, not annotated', [(100, 120, 1), (200, 120, 1)],
         [(100, 120), (200, 120)],
         [],
         [0, 0, 0, 1]),
        ('pair A', [(100, 140, 1), (200, 140, 1)],
         [(100, 140), (200, 140)], None, None),
        ('pair B', [(100, 170, 1), (200, 170, 1)],
         [(100, 170), (200, 170)], None, None),
    ]
    if n_cls == 1:
        rows = rows[:1]
    for j in range(n_cls - len(rows)):          # fillers: y = 30 + 2j, annotated 1 px below; mirror swaps j with j ^ 1
        y = 30 + 2 * j
        rows.append((f'filler {j:02d}', [(220, y, 1), (300, y, 1)], [(220, y), (300, y)], [((260, y + 1), 1.0)], [1, 0, 0, 0]))
    classes = [r[0] for r in rows]
    C = len(classes)
    idx = {c: i for i, c in enumerate(classes)}

    mirror = list(range(C))
    if C >= 16:
        mirror[idx['pair A']], mirror[idx['pair B']] = idx['pair B'], idx['pair A']
        for j in range(0, C - 16, 2):
            mirror[16 + j], mirror[17 + j] = 17 + j, 16 + j
    symmetric = {classes[c]: classes[m] for c, m in enumerate(mirror)}
    symmetric[UNKNOWN] = UNKNOWN

    pts, start = [], [0]
    for r in rows:
        for px, py, z in r[1]:
            s = z if z > 0 else 1.0             # behind samples: X, Y are what they are
            pts.append(((px - w / 2.0) * s, (py - h / 2.0) * s, z))
        start.append(len(pts))
    camera = dict(position=np.zeros(3), rotation=np.eye(3), f=(1.0, 1.0), pp=(w / 2.0, h / 2.0))

    base_gt = {r[0]: [p for p, _ in r[3]] for r in rows if r[3]}
    A, B = (150, 141), (120, 142)
    if C == 1:
        frames = [dict(status=1, gt=dict(base_gt), gt_extra=0), dict(status=0, gt=dict(base_gt), gt_extra=0)]
        pair = [None, None]
        # plain = mirrored: the one class is FP at t = 5 (d == 5.0 is beyond), TP just above; acc1 == acc2 -> pass 2
        out8 = [[0, 1, 0, 0, 0, 1, 0, 0] if at5 else [1, 0, 0, 0, 1, 0, 0, 0], [0] * 8]
        chosen = [2, 0]
    else:
        # pair rows per frame: annotations of A and of B, then per pass (plain, mirrored) the distances and the
        # class_conf rows of A and of B.  Polyline A is y = 140, polyline B is y = 170, both x in [100, 200].
        pair = [
            dict(gtA=[(150, 171)], gtB=[A, B],          # labels swapped: only the mirrored pass matches
                 dA=([31.0], [1.0, 2.0]), dB=([29.0, 28.0], [1.0]),
                 ccA=([0, 1, 0, 0], [2, 0, 0, 0]), ccB=([0, 2, 0, 0], [1, 0, 0, 0])),
            dict(gtA=[A, B], gtB=[(150, 171)],          # plain labels
                 dA=([1.0, 2.0], [31.0]), dB=([1.0], [29.0, 28.0]),
                 ccA=([2, 0, 0, 0], [0, 1, 0, 0]), ccB=([1, 0, 0, 0], [0, 2, 0, 0])),
            dict(gtA=[A], gtB=[(150, 143)],             # both near A: A is TP and B is FP in either pass, a tie
                 dA=([1.0], [3.0]), dB=([27.0], [29.0]),
                 ccA=([1, 0, 0, 0], [1, 0, 0, 0]), ccB=([0, 1, 0, 0], [0, 1, 0, 0])),
            dict(gtA=[(150, 171)], gtB=[A, B], dA=None, dB=None, ccA=None, ccB=None),     # status 0
        ]
        frames = []
        for f, p in enumerate(pair):
            gt = dict(base_gt)
            gt['pair A'], gt['pair B'] = p['gtA'], p['gtB']
            frames.append(dict(status=0 if f == 3 else 1, gt=gt, gt_extra=1 if f == 2 else 0))
        # [TP, FP, FN, 0] plain then mirrored, counted over the 14 self-mirrored rows above:
        #   TP enter, leave, re-enter, half-open x, half-open y, behind boundary, inside then behind, duplicate    = 8
        #   FP behind then inside (25 px), detected not annotated (+ single point, inside segment at t = 5)        = 2 (+2)
        #   FN all behind                                                                                          = 1
        # then the pair (frame 0: FP FP | TP TP; frame 1: TP TP | FP FP; frame 2: TP FP | TP FP, one unknown class
        # annotated = one more FN) and, with 32 classes, 16 fillers that are TP in both passes.
        tp, fp, k = (8, 4, C - 16) if at5 else (10, 2, C - 16)
        out8 = [[tp + k, fp + 2, 1, 0, tp + 2 + k, fp, 1, 0],               # 8/15 < 10/15: mirrored, pass 2
                [tp + 2 + k, fp, 1, 0, tp + k, fp + 2, 1, 0],               # plain, pass 1
                [tp + 1 + k, fp + 1, 2, 0, tp + 1 + k, fp + 1, 2, 0],       # acc1 == acc2 must give pass 2
                [0] * 8]
        chosen = [2, 1, 2, 0]

    F = len(frames)
    max_gt = max(len(v) for fr in frames for v in fr['gt'].values())
    err = np.full((F, 2, C, max_gt), NAN)
    cc = np.zeros((F, 2, C, 4), dtype=np.int32)
    for f, fr in enumerate(frames):
        if not fr['status']:
            continue
        for c, r in enumerate(rows):
            for p in range(2):
                if r[3] is not None:
                    d = [v for _, v in r[3]]
                    if r[0].startswith('filler') and p == 1 and c % 2 == 0:
                        d = [3.0]               # judged against the neighbour's point, 3 px below this line
                    row = r[4]
                else:
                    d = pair[f]['dA' if r[0] == 'pair A' else 'dB'][p]
                    row = pair[f]['ccA' if r[0] == 'pair A' else 'ccB'][p]
                err[f, p, c, :len(d)] = d
                cc[f, p, c] = row
    polylines = {r[0]: [(float(x), float(y)) for x, y in r[2]] for r in rows if r[2]}
    return dict(classes=classes, points=np.array(pts, dtype=np.float64), class_start=np.array(start, dtype=np.int32),
                mirror=np.array(mirror, dtype=np.int32), symmetric=symmetric, camera=camera, frames=frames, width=w, height=h,
                threshold=threshold, polylines=polylines, err=err, class_conf=cc, out8=np.array(out8, dtype=np.float32),
                chosen=np.array(chosen, dtype=np.float32))


def oracle_gt(frame):
    """The annotation dict the oracle sees for a hand_table / frame_set frame (gt_extra = that many unknown classes)."""
    gt = {c: list(v) for c, v in frame['gt'].items()}
    for k in range(frame.get('gt_extra', 0)):
        gt[UNKNOWN if k == 0 else f'{UNKNOWN} {k}'] = [(1.0, 1.0)]
    return gt


def pack(gts, classes, extras=None):
    """Annotations -> the kernel's arrays: gt (B, C, max_gt, 2) float64, cnt (B, C) int32, extra (B,) int32, max_gt."""
    idx = {c: i for i, c in enumerate(classes)}
    B, C = len(gts), len(classes)
    max_gt = max([1] + [len(v) for g in gts for k, v in g.items() if k in idx])
    gt = np.zeros((B, C, max_gt, 2), dtype=np.float64)
    cnt = np.zeros((B, C), dtype=np.int32)
    extra = np.zeros((B,), dtype=np.int32) if extras is None else np.asarray(extras, dtype=np.int32).copy()
    for b, g in enumerate(gts):
        for name, pts in g.items():
            if name not in idx:
                extra[b] += 1
                continue
            cnt[b, idx[name]] = len(pts)
            gt[b, idx[name], :len(pts)] = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    return gt, cnt, extra, max_gt


def detail_arrays(per_class, errors, classes, max_gt):
    """evaluate_camera_prediction(detail=True)'s dictionaries -> the kernel's (C, 4) class_conf and (C, max_gt) err of
    one pass.  Keys of `errors` / `per_class` are PREDICTED class names (the labels were mirrored before the call)."""
    cc = np.zeros((len(classes), 4), dtype=np.int64)
    err = np.full((len(classes), max_gt), NAN)
    for c, name in enumerate(classes):
        if name not in per_class:
            continue
        m = per_class[name]
        if name in errors:
            cc[c, 0], cc[c, 1] = int(m[0, 0]), int(m[0, 1])
            err[c, :len(errors[name])] = errors[name]
        elif m[1, 0]:
            cc[c, 2] = int(m[1, 0])
        else:
            assert m[0, 1] in (2., 9.) and m[0, 0] == 0
            cc[c, 3] = 1
    return cc, err


# ------------------------------------------------------------------------------------------ off-broadcast cameras

def off_broadcast_cameras(kind, n, seed, w=960, h=540):
    """n deterministic cameras (PCG64(seed + i)); pp is always (w/2, h/2) and focal lengths scale with w / 960.
      'low'        1.5 .. 3 m above the grass, anywhere over the pitch, looking anywhere, tilt 80 .. 92 degrees
      'zoom'       synth.sample_camera with 3x its focal length
      'broadcast'  synth.sample_camera as is"""
    cams = []
    for i in range(n):
        rng = np.random.Generator(np.random.PCG64(seed + i))
        if kind == 'low':
            pos = np.array([rng.uniform(-50, 50), rng.uniform(-30, 30), rng.uniform(-3, -1.5)])
            pan = rng.uniform(-np.pi, np.pi)
            tilt = np.deg2rad(rng.uniform(80, 92))
            roll = np.deg2rad(rng.normal(0, 5.0))
            f = rng.uniform(600, 1500)
            cam = dict(position=pos, rotation=cm.rotation_from_ptr(pan, tilt, roll), f=f)
        else:
            assert kind in ('zoom', 'broadcast')
            cam = synth.sample_camera(rng)
            cam = dict(position=cam['position'], rotation=cam['rotation'], f=cam['f'] * (3.0 if kind == 'zoom' else 1.0))
        cam['f'] = float(cam['f']) * w / 960.0
        cam['pp'] = (w / 2.0, h / 2.0)
        cams.append(cam)
    return cams


KINDS_32 = (('low', 12), ('zoom', 12), ('broadcast', 8))
KINDS_24 = (('low', 12), ('zoom', 12))
SEED = 7000


def frame_set(w, h, table, kinds=KINDS_32, seed=SEED):
    """Predicted cameras and annotations the way test_evaluator_matches_oracle_on_random_cameras makes them: the
    annotation is every fifth point (at most 8) of the TRUE camera's polylines with 1 px noise, 80 % of the classes;
    the prediction is the true camera moved by N(0, 0.15 m) with its focal length off by N(0, 0.4 %).  Every third
    frame carries left/right-mirrored labels."""
    rng = np.random.default_rng(seed)
    cams = [c for kind, n in kinds for c in off_broadcast_cameras(kind, n, seed, w, h)]
    frames = []
    for i, cam in enumerate(cams):
        true_poly = oe.get_polylines(cam['position'], cam['rotation'], cam['f'], cam['f'], cam['pp'], w, h, table)
        f = cam['f'] * (1 + rng.normal(0, 0.004))
        pred = dict(position=cam['position'] + rng.normal(0, 0.15, 3), rotation=cam['rotation'], f=(f, f), pp=cam['pp'])
        gt = {c: [(x + rng.normal(0, 1.0), y + rng.normal(0, 1.0)) for (x, y) in v[::5][:8]]
              for c, v in true_poly.items() if rng.uniform() > 0.2}
        if i % 3 == 1:
            gt = oe.mirror_labels(gt)
        frames.append(dict(camera=pred, gt=gt))
    return frames


def census(cameras, table, w, h, annotations=None, thresholds=(5.0,), classes=None, symmetric=None):
    """Which branches the oracle takes on these cameras.  Returns (counts, results):
      counts   behind / enter / leave / no_border / first_prev_zero / len1 (get_polylines' stats), 'no_class' frames
               with no detected class, and per threshold t: conf[t] (2, 4) summed [TP, FP not annotated, FP beyond
               threshold, FN] per pass, chosen[t] = [frames choosing pass 1, pass 2], and 'min_gap', the smallest
               |distance - t| over every annotated point, pass and t in (5, 10, 20)
      results  per frame the polylines, and per threshold (c1, c2, acc1, acc2, chosen, (pc1, er1), (pc2, er2))"""
    classes = oe.CLASSES if classes is None else classes
    counts = dict(behind=0, enter=0, leave=0, no_border=0, first_prev_zero=0, len1=0, no_class=0, min_gap=math.inf,
                  conf={t: np.zeros((2, 4), dtype=np.int64) for t in thresholds}, chosen={t: [0, 0] for t in thresholds})
    results = []
    memo, plain_distance = {}, oe.distance_to_polyline

    def distance_once(point, polyline):         # the same (point, polyline) comes back once per threshold
        key = (point[0], point[1], id(polyline))
        if key not in memo:
            memo[key] = plain_distance(point, polyline)
        return memo[key]
    for b, cam in enumerate(cameras):
        memo.clear()
        poly = oe.get_polylines(cam['position'], cam['rotation'], cam['f'][0], cam['f'][1], cam['pp'], w, h, table, classes,
                                stats=counts)
        counts['no_class'] += not poly
        res = dict(poly=poly)
        if annotations is not None:
            gts = (annotations[b], oe.mirror_labels(annotations[b], symmetric))
            for t in thresholds:
                conf, det = [], []
                for p, gt in enumerate(gts):
                    oe.distance_to_polyline = distance_once
                    try:
                        c, pc, er = oe.evaluate_camera_prediction(poly, gt, t, detail=True)
                    finally:
                        oe.distance_to_polyline = plain_distance
                    conf.append(c); det.append((pc, er))
                    not_ann = len(set(poly) - set(gt))
                    counts['conf'][t][p] += [int(c[0, 0]), not_ann, int(c[0, 1]) - not_ann, int(c[1, 0])]
                    for v in er.values():
                        for d in v:
                            counts['min_gap'] = min([counts['min_gap']] + [abs(d - x) for x in (5.0, 10.0, 20.0)])
                a1, a2 = (c[0, 0] / c.sum() if c.sum() > 0 else 0. for c in conf)
                which = 1 if a1 > a2 else 2                     # evaluate_camera.py:303
                counts['chosen'][t][which - 1] += 1
                res[t] = (conf[0], conf[1], a1, a2, which, det[0], det[1])
        results.append(res)
    return counts, results


@functools.lru_cache(maxsize=None)
def field_table(sampling_factor):
    return oe.field_table(sampling_factor)


@functools.lru_cache(maxsize=None)
def oracle_results(w, h, thresholds=(5.0,), sampling_factor=0.9, kinds=KINDS_32):
    """(frames, counts, results) of frame_set(w, h) under census(); computed once per process and never modified."""
    table = field_table(sampling_factor)
    frames = frame_set(w, h, table, kinds)
    counts, results = census([fr['camera'] for fr in frames], table, w, h, [fr['gt'] for fr in frames], thresholds)
    return frames, counts, results


# the GPU cases and what the census of each must show (asserted in both test files)
CASES = [(960, 540, (5.0, 10.0, 20.0)), (1920, 1080, (5.0,)), (333, 187, (5.0,))]


def check_census(counts, thresholds):
    assert counts['behind'] >= 1000, counts
    assert counts['enter'] >= 20 and counts['leave'] >= 20, counts
    assert counts['no_class'] >= 1, counts
    for t in thresholds:
        assert min(counts['chosen'][t]) >= 1, counts
        tp, fp_na, fp_far, fn = counts['conf'][t].T
        assert (tp > 0).all() and (fp_na + fp_far > 0).all() and (fn > 0).all(), counts
    assert counts['min_gap'] > 1e-6, counts
