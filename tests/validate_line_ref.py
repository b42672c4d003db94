"""numpy fp64 restatement of what tests/golden/validate_line.npz captured from the reference (tools/make_golden_validate_line.py):
the two-peak target maps of EHMDataset (line/dataset.py:107-178), EHMLoss.forward (line/loss.py:34-108) and AccMetric
(line/metrics.py:53-137); plus the recipe that regenerates the loss cases' predictions (they are not stored).
tests/test_validate_line_host.py holds this file to the capture."""
import json

import numpy as np

# name -> (gmse_w, awing_w)
WEIGHTS = {'gmse': (1.0, 0.0), 'awing': (0.0, 1.0), 'default': (1.0, 1.0), 'mixed': (0.5, 2.0)}
TERMS = {'gmse': 1, 'awing': 2, 'default': 3, 'mixed': 3}
ALPHA, OMEGA, EPSILON, THETA = 2.1, 14.0, 1.0, 0.5           # line/loss.py:28-32
EPS32 = 2.0 ** -23
ACC_TS, ACC_WS = (5, 10, 20), (0.5, 0.35, 0.15)              # line/metrics.py:117-118


def centres(kp: np.ndarray, stride, hw):
    """mu of every point: (..., 2) int64 [mu_x, mu_y] = min(n - 1, rint(fp32(v) / fp32(stride))), ties to even, no lower clamp."""
    h, w = hw
    q = np.rint(np.asarray(kp, dtype=np.float32)[..., :2] / np.float32(stride)).astype(np.int64)
    return np.minimum(q, np.array([w - 1, h - 1]))


def keypoint_maps(kp: np.ndarray, sigma: float, stride, hw, as_dataset: bool = False) -> np.ndarray:
    """kp (B,C,2,3) [x, y, flag] in image pixels -> (B,C,h,w) maps.  fp64 by default (the exact recipe).  as_dataset=True repeats
    the dataset's own arithmetic: each Gaussian in fp64, divided by its maximum, added into a float32 map (one rounding per
    addition) -- the captured maps, bit for bit."""
    h, w = hw
    kp = np.asarray(kp, dtype=np.float32).reshape(kp.shape[0], -1, 2, 3)
    B, C = kp.shape[:2]
    mu = centres(kp, stride, hw)
    X, Y = np.meshgrid(np.arange(w).astype(float), np.arange(h).astype(float))
    out = np.zeros((B, C, h, w), dtype=np.float32 if as_dataset else np.float64)
    for b in range(B):
        for c in range(C):
            for p in range(2):
                if kp[b, c, p, 2] != 1:
                    continue
                g = np.exp(-((X - mu[b, c, p, 0]) ** 2 + (Y - mu[b, c, p, 1]) ** 2) / (2 * sigma ** 2))
                g /= np.max(g)
                out[b, c] += g
    return out


def make_pred(seed: int, shape, kp: np.ndarray, stride) -> np.ndarray:
    """(B,C,h,w) float32 'softmax outputs' k / 16384 with integer k in [0, 4096): exactly representable, no transcendental, the
    same bits wherever it runs.  Within 2 cells of every drawn point, on its own channel, the value is 1 - k / 16384 (in
    (0.75, 1]): close to the target at the peak and more than theta = 0.5 away from it two cells out, so both branches of the
    adaptive wing loss occur."""
    B, C, h, w = shape
    k = np.random.RandomState(seed).randint(0, 4096, size=shape).astype(np.int64)
    kp = np.asarray(kp, dtype=np.float32).reshape(B, C, 2, 3)
    mu = centres(kp, stride, (h, w))
    near = np.zeros(shape, dtype=bool)
    for b in range(B):
        for c in range(C):
            for p in range(2):
                if kp[b, c, p, 2] == 1:
                    cx, cy = int(mu[b, c, p, 0]), int(mu[b, c, p, 1])
                    near[b, c, max(cy - 2, 0):max(min(cy + 3, h), 0), max(cx - 2, 0):max(min(cx + 3, w), 0)] = True
    v = k.astype(np.float32) / np.float32(16384.0)
    return np.where(near, np.float32(1.0) - v, v).astype(np.float32)


def loss_terms64(pred: np.ndarray, target: np.ndarray, gmse_sigma: float, terms=(True, True)) -> np.ndarray:
    """(B,2) fp64: per-frame sums over C*h*w of the GMSE and adaptive-wing terms, evaluated in fp64 on the given arrays."""
    B = pred.shape[0]
    out = np.zeros((B, 2), dtype=np.float64)
    for b in range(B):
        p, t = pred[b].astype(np.float64), target[b].astype(np.float64)
        if terms[0]:
            sq = (p - t) ** 2
            out[b, 0] = np.sum(sq * np.exp(-sq / (2 * gmse_sigma ** 2)))
        if terms[1]:
            delta = np.abs(t - p)
            a = ALPHA - t
            P = np.power(THETA / EPSILON, a)
            A = OMEGA * (1 / (1 + P)) * a * np.power(THETA / EPSILON, a - 1) * (1 / EPSILON)
            C = THETA * A - OMEGA * np.log(1 + P)
            out[b, 1] = np.sum(np.where(delta < THETA, OMEGA * np.log(1 + np.power(delta / EPSILON, a)), A * delta - C))
    return out


def combine(sums: np.ndarray, weights, shape) -> float:
    """The scalar EHMLoss.forward returns: both terms are means over every element; terms with weight 0 left out."""
    n = float(np.prod(shape))
    s = np.asarray(sums, dtype=np.float64).sum(axis=0)
    loss = 0.0
    if weights[0] > 0:
        loss += weights[0] * s[0] / n
    if weights[1] > 0:
        loss += weights[1] * s[1] / n
    return float(loss)


def acc_counts(gt: np.ndarray, pred: np.ndarray, p_threshold: float, ts=ACC_TS) -> np.ndarray:
    """a_t_score's counting (line/metrics.py:70-98) -> (len(ts),3) int64 [tp, fp, fn]; distances in fp64 on the fp32 coordinates,
    the confidence compared in fp32 as torch compares a float32 tensor with a Python scalar."""
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 2, 3)
    pred = np.asarray(pred, dtype=np.float32).reshape(-1, 2, 3)
    ge = gt[:, :, 2] == 1
    pe = pred[:, :, 2] >= np.float32(p_threshold)
    d = gt[:, :, None, :2].astype(np.float64) - pred[:, None, :, :2].astype(np.float64)        # (n, gt slot, pred slot, 2)
    dmin = np.sqrt((d ** 2).sum(-1)).min(axis=2)
    out = np.zeros((len(ts), 3), dtype=np.int64)
    for k, t in enumerate(ts):
        within = dmin <= t
        out[k] = ((ge & pe & within).sum(), (pe & ~ge).sum() + (ge & pe & ~within).sum(), (ge & ~pe).sum())
    return out


def acc_value(counts) -> float:
    """AccMetric.update + compute over per-batch counts (n, 3, 3): the loop overwrites acc at each threshold and then adds
    acc * ws[i], so a batch is worth a@20 * 1.15; the epoch value is the plain mean (line/metrics.py:120-137)."""
    accs = []
    for batch in counts:
        acc = 0
        for i in range(len(ACC_TS)):
            tp, fp, fn = (int(v) for v in batch[i])
            acc = tp / (tp + fp + fn)
            acc += acc * ACC_WS[i]
        accs.append(acc)
    return float(np.mean(accs))


def cases(g):
    """The target / loss cases of validate_line.npz: name -> dict(shape, stride, sigma, gmse_sigma, seed, kp (B,C,2,3), maps or
    None (stored for the small shapes only))."""
    out = {}
    for name in [str(n) for n in g['case.names']]:
        out[name] = dict(shape=tuple(int(v) for v in g[f'case.{name}.shape']), stride=int(g[f'case.{name}.stride']),
                         sigma=float(g[f'case.{name}.sigma']), gmse_sigma=float(g[f'case.{name}.gmse_sigma']),
                         seed=int(g[f'case.{name}.seed']), kp=g[f'case.{name}.kp'],
                         maps=g[f'case.{name}.maps'] if f'case.{name}.maps' in g.files else None)
    return out


def acc_batches(g):
    return [(g[f'acc.{i}.gt'], g[f'acc.{i}.pred']) for i in range(int(g['acc.n']))]


def label_cases(g):
    """[{'points': {class: [[x, y], ...]}, 'usable': bool, 'labels': {str(id): None or [[x0, y0], [x1, y1], [slope, intercept]]}}]"""
    return json.loads(str(g['labels.json']))
