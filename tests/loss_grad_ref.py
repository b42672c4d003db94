"""numpy fp64 closed-form gradients of the two losses with respect to the prediction, written from the formulas (the target is not
differentiated), and the sampling recipe of tests/golden/loss_grad.npz (tools/make_golden_loss_grad.py captured it from the
reference under torch CPU autograd).  tests/test_loss_grad_host.py holds this file to the capture.

Keypoint loss (HRNetLoss.forward, hrnet/loss.py:89-144), x the logit, m the mask entry (1 if none), z = x m, e = exp(z), t = target m:
    MSE   2 (e - t) e m          KL   -t m          adaptive wing   w'(|t - e|) sign(e - t) e m
Line loss (EHMLoss.forward, line/loss.py:61-108), d = p - t, u = d^2 / (2 sigma^2):
    GMSE  2 d exp(-u) (1 - u)    adaptive wing   w'(|t - p|) sign(p - t)
w'(delta) = omega a delta^(a-1) / (1 + delta^a) for delta < theta, A(t) otherwise, a = alpha - t; sign(0) = 0.
grad = sum_k coef_k * term_k, coef_k the term's weight over its divisor."""
import numpy as np

ALPHA, OMEGA, EPSILON, THETA = 2.1, 14.0, 1.0, 0.5
EPS32 = 2.0 ** -23
N_SEEDED, N_TOP = 4096, 64
CORNER_DELTA, CORNER_T = 2.0 ** -14, 0.25          # the wing term's ill-conditioned corner: 0 < delta < 2^-14 and t > 0.25

KP_TERMS = {'mse': 1, 'kl': 2, 'awing': 4, 'default': 3, 'all': 7}
LINE_TERMS = {'gmse': 1, 'awing': 2, 'default': 3, 'mixed': 3}


def wing_term64(e: np.ndarray, t: np.ndarray) -> np.ndarray:
    """d adaptive_wing(e, t) / d e = w'(|t - e|) sign(e - t); exactly 0 where e == t."""
    delta = np.abs(t - e)
    a = ALPHA - t
    safe = np.where(delta > 0, delta, 1.0)                                     # delta^(a-1) is infinite at 0 when a < 1
    pw = np.power(safe, a - 1.0)
    small = OMEGA * a * pw / (1.0 + pw * safe)
    A = OMEGA * (1.0 / (1.0 + np.power(THETA / EPSILON, a))) * a * np.power(THETA / EPSILON, a - 1.0) * (1.0 / EPSILON)
    return np.where(delta < THETA, small, A) * np.sign(e - t)


def wing_curvature64(e: np.ndarray, t: np.ndarray) -> np.ndarray:
    """|w''(delta)|, the sensitivity of the wing term to the prediction it is evaluated at: for delta < theta
    omega a ((a-1) delta^(a-2) (1 + delta^a) - a delta^(2a-2)) / (1 + delta^a)^2, 0 on the linear branch and at delta == 0."""
    delta = np.abs(t - e)
    a = ALPHA - t
    safe = np.where(delta > 0, delta, 1.0)
    da = np.power(safe, a)
    w2 = OMEGA * a * ((a - 1.0) * da / safe ** 2 * (1.0 + da) - a * da * da / safe ** 2) / (1.0 + da) ** 2
    return np.where((delta > 0) & (delta < THETA), np.abs(w2), 0.0)


def kp_wing_exp_rounding(pred: np.ndarray, target: np.ndarray, mask, coef_wing: float) -> np.ndarray:
    """What one ulp of exp(p) in fp32 (relative 2^-23) moves the wing term's gradient by through delta = |t - e|, to first order:
    coef |w''(delta)| e^2 m 2^-23 per element.  No fp32 evaluation of the formula can be closer than this to the fp64 one; the part
    through the factor e itself is within the floor bound already."""
    m = np.ones(pred.shape[:2]) if mask is None else np.asarray(mask, dtype=np.float64)
    m = m[:, :, None, None]
    e = np.exp(pred.astype(np.float64) * m)
    return coef_wing * wing_curvature64(e, target.astype(np.float64) * m) * e * e * m * EPS32


def kp_coef(weights, shape):
    """(l2_w / n, kldiv_w / B, awing_w / n): MSELoss mean, KLDivLoss batchmean, torch.mean; 0 for a weight that is not > 0."""
    B, n = shape[0], float(np.prod(shape))
    return tuple(w / d if w > 0 else 0.0 for w, d in zip(weights, (n, float(B), n)))


def line_coef(weights, shape):
    n = float(np.prod(shape))
    return tuple(w / n if w > 0 else 0.0 for w in weights)


def kp_grad64(pred: np.ndarray, target: np.ndarray, mask, coef, terms: int = 7) -> np.ndarray:
    """(B,N+1,h,w) fp64 gradient of sum_k coef_k term_k with respect to the logits; a term whose bit is clear is left out."""
    out = np.zeros(pred.shape, dtype=np.float64)
    for b in range(pred.shape[0]):
        p, t = pred[b].astype(np.float64), target[b].astype(np.float64)
        m = np.ones((pred.shape[1], 1, 1)) if mask is None else np.asarray(mask[b], dtype=np.float64)[:, None, None]
        p, t = p * m, t * m
        e = np.exp(p)
        g = np.zeros_like(p)
        if terms & 1:
            g += coef[0] * (2.0 * (e - t) * e)
        if terms & 2:
            g += coef[1] * -t
        if terms & 4:
            g += coef[2] * (wing_term64(e, t) * e)
        out[b] = g * m
    return out


def kp_corner(pred: np.ndarray, target: np.ndarray, mask) -> np.ndarray:
    """Boolean map of the elements the wing term leaves to the rounding of exp: 0 < delta64 < 2^-14 and t > 0.25."""
    m = np.ones(pred.shape[:2]) if mask is None else np.asarray(mask, dtype=np.float64)
    m = m[:, :, None, None]
    t = target.astype(np.float64) * m
    delta = np.abs(t - np.exp(pred.astype(np.float64) * m))
    return (delta > 0) & (delta < CORNER_DELTA) & (t > CORNER_T)


def kp_wing_zero(pred: np.ndarray, target: np.ndarray, mask) -> np.ndarray:
    """Elements with delta64 exactly 0 (e == t in fp64): the wing term must contribute exactly 0 there."""
    m = np.ones(pred.shape[:2]) if mask is None else np.asarray(mask, dtype=np.float64)
    m = m[:, :, None, None]
    return np.exp(pred.astype(np.float64) * m) == target.astype(np.float64) * m


def line_grad64(pred: np.ndarray, target: np.ndarray, gmse_sigma: float, coef, terms: int = 3) -> np.ndarray:
    p, t = pred.astype(np.float64), target.astype(np.float64)
    g = np.zeros_like(p)
    if terms & 1:
        d = p - t
        u = d * d / (2.0 * gmse_sigma ** 2)
        g += coef[0] * (2.0 * d * np.exp(-u) * (1.0 - u))
    if terms & 2:
        g += coef[1] * wing_term64(p, t)
    return g


def line_corner(pred: np.ndarray, target: np.ndarray) -> np.ndarray:
    t = target.astype(np.float64)
    delta = np.abs(t - pred.astype(np.float64))
    return (delta > 0) & (delta < CORNER_DELTA) & (t > CORNER_T)


def seeded_positions(seed: int, n: int) -> np.ndarray:
    """The 4096 flat positions at which the fixture holds the reference gradient of a case (the same for all its combinations)."""
    return np.random.RandomState(1000 + seed).randint(0, n, size=N_SEEDED).astype(np.int64)


def top_positions(g: np.ndarray) -> np.ndarray:
    """The 64 flat positions of largest magnitude, largest first (ties by position)."""
    flat = np.abs(g.reshape(-1))
    if flat.size <= N_TOP:
        return np.argsort(-flat, kind='stable').astype(np.int64)
    part = np.argpartition(-flat, N_TOP)[:N_TOP]
    return part[np.lexsort((part, -flat[part]))].astype(np.int64)


def kp_combinations(cases):
    """(case name, mask name, weights name) of every captured keypoint combination: small and ragged with every mask x every
    weight set, train with mask zeros x all only."""
    import validate_ref as vr
    out = []
    for name in cases:
        for mname in ('none', 'zeros'):
            for wname in vr.WEIGHTS:
                if name != 'train' or (mname, wname) == ('zeros', 'all'):
                    out.append((name, mname, wname))
    return out
