"""cv2.resize(src, (W, H)) with INTER_LINEAR on uint8, restated in numpy from the formulas of OpenCV 4.7's 8-bit path
(modules/imgproc/src/resize.cpp) as include/sncal.h states them -- and from nothing else in the product: no line here calls the
package.  The cases the resize tests share live here too.

Written without a cv2 at hand: tests/test_resize_cv2_optional.py holds this file to cv2.resize's bytes where one is installed.
"""
import numpy as np

# h, w -> H, W, B: the shapes tests/test_resize_gpu.py, test_resize_host.py and test_resize_cv2_optional.py run
CASES = [
    (7, 5, 3, 9, 1),            # mixed up and down, odd everything
    (33, 61, 32, 64, 1),
    (37, 53, 36, 52, 1),        # ratio just above 1, right and bottom clamps
    (1, 1, 4, 4, 1),
    (64, 96, 1, 1, 1),
    (360, 640, 540, 960, 1),    # the s = -1 first row
    (64, 96, 32, 48, 1),        # the area path
    (64, 96, 32, 96, 1),        # the general path at ratio 2
    (64, 96, 64, 96, 1),        # a copy
    (720, 1280, 540, 960, 2),   # one real shape
]

AXES = [(1280, 960), (720, 540), (1920, 960), (640, 960), (360, 540), (1, 4), (96, 1), (5, 9), (7, 3), (61, 64), (53, 52), (1024, 960)]


def tables(n_src, n_dst, zero_edges):
    """-> (ofs (n_dst,) int32, coef (n_dst, 2) int16) of one axis.  zero_edges: the x axis rule; else the y axis rule (ofs unclipped)."""
    scale = np.float64(1.0) / (np.float64(n_dst) / np.float64(n_src))
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    if zero_edges:
        lo, hi = s < 0, s >= n_src - 1
        s = np.where(lo, 0, np.where(hi, n_src - 1, s)).astype(np.int32)
        f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    assert f.dtype == np.float32
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int16)         # np.rint: half to even
    c1 = np.rint(f * np.float32(2048)).astype(np.int16)
    return s, np.stack([c0, c1], axis=1)


def takes_area_path(h, w, H, W):
    return w == 2 * W and h == 2 * H


def resize(src, size):
    """src (h,w,3) or (B,h,w,3) uint8, size = (W, H) -> the resized array, same rank."""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    if src.ndim == 4:
        return np.stack([resize(f, size) for f in src]) if len(src) else np.zeros((0, size[1], size[0], 3), np.uint8)
    W, H = size
    h, w = src.shape[:2]
    if (h, w) == (H, W):
        return src.copy()
    S = src.astype(np.int32)
    if takes_area_path(h, w, H, W):
        return ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    xo, xc = tables(w, W, True)
    yo, yc = tables(h, H, False)
    x0, x1 = xo, np.minimum(xo + 1, w - 1)
    y0, y1 = np.clip(yo, 0, h - 1), np.clip(yo + 1, 0, h - 1)
    a0, a1 = xc[:, 0].astype(np.int32)[None, :, None], xc[:, 1].astype(np.int32)[None, :, None]
    b0, b1 = yc[:, 0].astype(np.int32)[:, None, None], yc[:, 1].astype(np.int32)[:, None, None]
    h0 = S[y0][:, x0] * a0 + S[y0][:, x1] * a1
    h1 = S[y1][:, x0] * a0 + S[y1][:, x1] * a1
    out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def inputs(h, w, B=1, seed=0):
    """{'noise', 'ramp'} -> (B,h,w,3) uint8: uniform noise, and a diagonal ramp with a different slope per channel and frame."""
    rng = np.random.RandomState(seed + 7919 * h + 104729 * w)
    noise = rng.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    ramp = np.stack([np.stack([(x * (3 + c) + y * (5 - c) + 17 * b) % 256 for c in range(3)], axis=-1) for b in range(B)]).astype(np.uint8)
    return {'noise': noise, 'ramp': ramp}


def float_bilinear(src, size):
    """The independent geometry check: torch's F.interpolate(mode='bilinear', align_corners=False, antialias=False) in float64 on the
    CPU.  (B,h,w,3) uint8 -> (B,H,W,3) float64, not rounded."""
    import torch
    import torch.nn.functional as F
    t = torch.tensor(np.asarray(src)).permute(0, 3, 1, 2).to(torch.float64)
    out = F.interpolate(t, size=(size[1], size[0]), mode='bilinear', align_corners=False, antialias=False)
    return out.permute(0, 2, 3, 1).numpy()


def worst_level(got, src, size):
    """max |got - float bilinear| over a (B,H,W,3) result: the issue's condition is that this stays strictly below 1."""
    return float(np.abs(np.asarray(got).astype(np.float64) - float_bilinear(src, size)).max())
