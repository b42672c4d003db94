"""numpy fp64 restatement of what tests/golden/validate.npz captured from the reference (tools/make_golden_validate.py):
HRNetLoss.forward (loss.py:89-144), L2metric and the EvalAImetric aggregation (metrics.py:14-94, 181-229); plus the recipe that
regenerates the loss cases' predictions (they are not stored).  tests/test_validate_host.py holds this file to the capture."""
import numpy as np

from oracle import synth as osynth

# name -> (l2_w, kldiv_w, awing_w)
WEIGHTS = {'mse': (1.0, 0.0, 0.0), 'kl': (0.0, 1.0, 0.0), 'awing': (0.0, 0.0, 1.0), 'default': (1.0, 1.0, 0.0), 'all': (1.0, 1.0, 1.0)}
ALPHA, OMEGA, EPSILON, THETA = 2.1, 14.0, 1.0, 0.5           # loss.py:76-79
EPS32 = 2.0 ** -23


def make_pred(seed: int, shape, kp_img: np.ndarray, stride: float) -> np.ndarray:
    """(B,N+1,h,w) float32 'log-probabilities' -k/256 with integer k in [0, 4096): exactly representable, no transcendental, the
    same bits wherever it runs.  Within 2 cells of every keypoint with flag 1, on its own channel, k is divided by 64 (pred in
    (-0.25, 0], exp(pred) near the target's peak), so that both branches of the adaptive wing loss occur."""
    B, C, h, w = shape
    k = np.random.RandomState(seed).randint(0, 4096, size=shape).astype(np.int64)
    for b in range(B):
        for n in range(C - 1):
            x, y, f = kp_img[b, n]
            if f != 1:
                continue
            cx, cy = int(np.rint(np.float32(x) / np.float32(stride))), int(np.rint(np.float32(y) / np.float32(stride)))
            x0, x1, y0, y1 = max(cx - 2, 0), min(cx + 3, w), max(cy - 2, 0), min(cy + 3, h)
            if x0 < x1 and y0 < y1:
                k[b, n, y0:y1, x0:x1] //= 64
    return (-k.astype(np.float32)) / np.float32(256.0)


def target32(kp_img: np.ndarray, stride: float, sigma: float, hw) -> np.ndarray:
    """HRNetLoss.forward's target in fp32 (loss.py:90-93): keypoints / stride in fp32, then create_target."""
    kp = np.array(kp_img, dtype=np.float32).reshape(kp_img.shape[0], -1, 3).copy()
    kp[:, :, :2] = kp[:, :, :2] / np.float32(stride)
    return osynth.create_target(kp, float(sigma), tuple(hw))


def loss_terms64(pred: np.ndarray, target: np.ndarray, mask=None, terms=(True, True, True)) -> np.ndarray:
    """(B,3) fp64: per-frame sums over (N+1)*h*w of the MSE, KL and adaptive-wing terms, evaluated in fp64 on the fp32 prediction
    and the fp32 target (frame by frame, to bound the temporaries)."""
    B = pred.shape[0]
    out = np.zeros((B, 3), dtype=np.float64)
    for b in range(B):
        p, t = pred[b].astype(np.float64), target[b].astype(np.float64)
        if mask is not None:
            m = np.asarray(mask[b], dtype=np.float64)[:, None, None]
            p, t = p * m, t * m
        e = np.exp(p)
        if terms[0]:
            out[b, 0] = np.sum((e - t) ** 2)
        if terms[1]:
            pos = t > 0
            out[b, 1] = np.sum(t[pos] * (np.log(t[pos]) - p[pos]))              # xlogy(t, t) - t * p
        if terms[2]:
            delta = np.abs(t - e)
            a = ALPHA - t
            P = np.power(THETA / EPSILON, a)
            A = OMEGA * (1 / (1 + P)) * a * np.power(THETA / EPSILON, ALPHA - t - 1) * (1 / EPSILON)
            C = THETA * A - OMEGA * np.log(1 + P)
            out[b, 2] = np.sum(np.where(delta < THETA, OMEGA * np.log(1 + np.power(delta / EPSILON, a)), A * delta - C))
    return out


def combine(sums: np.ndarray, weights, shape) -> float:
    """The scalar HRNetLoss.forward returns: MSELoss mean, KLDivLoss batchmean, torch.mean; terms with weight 0 left out."""
    B, n = shape[0], float(np.prod(shape))
    s = np.asarray(sums, dtype=np.float64).sum(axis=0)
    loss = 0.0
    if weights[0] > 0:
        loss += weights[0] * s[0] / n
    if weights[1] > 0:
        loss += weights[1] * s[1] / B
    if weights[2] > 0:
        loss += weights[2] * s[2] / n
    return float(loss)


def l2_metrics(updates, num_keypoints: int, conf_threshold: float, pckhs_thres, phase='val') -> dict:
    """L2metric over a list of (prediction (B,N,3), target (B,3N)) updates, then epoch_complete."""
    total, num_el, gt_points, n_fp, n_fn = 0.0, 0, 0, 0, 0
    pck = [0] * len(pckhs_thres)
    for preds, target in updates:
        preds = np.asarray(preds, dtype=np.float32)
        kpts = np.asarray(target, dtype=np.float32).reshape(-1, num_keypoints, 3)
        d = (preds[:, :, :2] - kpts[:, :, :2]).astype(np.float32)
        l2 = np.sqrt((d.astype(np.float64) ** 2).sum(-1))
        gt_valid = kpts[:, :, 0] != -1
        pred_valid = preds[:, :, 2] > np.float32(conf_threshold)
        mask = gt_valid & pred_valid
        num_el += int(mask.sum())
        total += float(l2[mask].sum())
        gt_points += int(gt_valid.sum())
        n_fp = int((~gt_valid & pred_valid).sum())                 # assigned, not accumulated (metrics.py:67-68)
        n_fn = int((~pred_valid & gt_valid).sum())
        for i, t in enumerate(pckhs_thres):
            sel = l2[mask]
            pck[i] += int(np.count_nonzero(sel[sel < t]))          # an exactly-zero distance is not counted (metrics.py:70)
    p = f'{phase}_' if phase else ''
    out = {f'{p}precision': num_el / (num_el + n_fp) if num_el > 0 else 0.0,
           f'{p}recall': num_el / (num_el + n_fn) if num_el > 0 else 0.0}
    for i, t in enumerate(pckhs_thres):
        out[f'{p}pcks-{t}'] = pck[i] / gt_points if gt_points > 0 else 0.0
    out[f'{p}l2'] = total / num_el if num_el > 0 else float('inf')
    return out


def evalai_metrics(frames, phase='val') -> dict:
    """EvalAImetric.update + epoch_complete (metrics.py:185-229) over per-frame results: None (no camera) or
    (accuracy, confusion 2x2, {class: [reprojection errors]}) of the kept pass."""
    total = missed = n_acc = n_l2 = 0
    acc = tp = n_prec = n_rec = l2_sum = 0.0
    for res in frames:
        total += 1
        if res is None:
            missed += 1
            continue
        a, conf, errors = res
        conf = np.asarray(conf, dtype=np.float64)
        acc += float(a)
        n_acc += 1
        tp += conf[0, 0]
        n_prec += conf[0, :].sum()
        n_rec += conf[0, 0] + conf[1, 0]
        for v in errors.values():
            n_l2 += len(v)
            l2_sum += float(np.sum(np.asarray(v, dtype=np.float64)))
    completeness = (total - missed) / total if total > 0 else 0.0
    accuracy = acc / n_acc if n_acc > 0 else 0.0
    p = f'{phase}_' if phase else ''
    return {f'{p}l2_reprojection': l2_sum / n_l2 if n_l2 > 0 else float('inf'), f'{p}completeness': completeness,
            f'{p}eval_precision': tp / n_prec if n_prec > 0 else 0.0, f'{p}eval_recall': tp / n_rec if n_rec > 0 else 0.0,
            f'{p}eval_accuracy': accuracy, f'{p}evalai': completeness * accuracy}


def kept_pass(acc1, conf1, err1, acc2, conf2, err2):
    """metrics.py:127-136: the plain labels win only when strictly better."""
    return (acc1, conf1, err1) if acc1 > acc2 else (acc2, conf2, err2)


def loss_cases(g):
    """The loss cases of validate.npz: name -> dict(shape, stride, sigma, seed, kp, masks {'none': None, 'zeros': (B,N+1)})."""
    out = {}
    for name in [str(n) for n in g['loss.names']]:
        out[name] = dict(shape=tuple(int(v) for v in g[f'loss.{name}.shape']), stride=float(g[f'loss.{name}.stride']),
                         sigma=float(g[f'loss.{name}.sigma']), seed=int(g[f'loss.{name}.seed']), kp=g[f'loss.{name}.kp'],
                         masks={'none': None, 'zeros': g[f'loss.{name}.mask']})
    return out
