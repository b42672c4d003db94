"""numpy restatement of libjpeg's scaled decode (scale 1 / d, d = 2, 4, 8), the reference of tests/test_jpeg_reduced_*.py.

jdmaster.c chooses per component the size of the inverse transform, jidctred.c holds the 4x4 / 2x2 / 1x1 transforms, jdsample.c
upsamples what is left.  Headers, the 8x8 transform, the fancy upsamplers and the colour conversion are oracle/jpeg.py's; the
coefficients come from the library's host stage (sncal_amd.jpeg.entropy_decode, no GPU), which tests/test_abi.py pins to the oracle.
Pinned to libjpeg-turbo itself by tests/golden/jpeg_reduced.npz (tests/test_jpeg_reduced_host.py)."""
import numpy as np

from oracle import jpeg as oj

FIX = {'0.211164243': 1730, '0.509795579': 4176, '0.601344887': 4926, '0.720959822': 5906, '0.765366865': 6270,
       '0.850430095': 6967, '0.899976223': 7373, '1.061594337': 8697, '1.272758580': 10426, '1.451774981': 11893,
       '1.847759065': 15137, '2.172734803': 17799, '2.562915447': 20995, '3.624509785': 29692}
for _k, _v in FIX.items():
    assert _v == int(float(_k) * 8192 + 0.5)


def range_limit(y):
    """The 4x4 and 2x2 transforms: saturated, as libjpeg-turbo's SIMD forms (jidctred-sse2) do."""
    return np.clip(y + 128, 0, 255)


def range_limit_table(y):
    """jpeg_idct_1x1 (plain C, no SIMD form): jdmaster.c's table, its index masked with RANGE_MASK."""
    y = y & 1023
    return np.where(y < 128, y + 128, np.where(y < 512, 255, np.where(y < 896, 0, y - 896)))


def _pass4(x, shift):
    """jpeg_idct_4x4, one pass over the last axis: (..., 8) -> (..., 4); index 4 is never read."""
    t0 = x[..., 0] << 14
    t2 = x[..., 2] * FIX['1.847759065'] - x[..., 6] * FIX['0.765366865']
    t10, t12 = t0 + t2, t0 - t2
    x7, x5, x3, x1 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    oa = -x7 * FIX['0.211164243'] + x5 * FIX['1.451774981'] - x3 * FIX['2.172734803'] + x1 * FIX['1.061594337']
    ob = -x7 * FIX['0.509795579'] - x5 * FIX['0.601344887'] + x3 * FIX['0.899976223'] + x1 * FIX['2.562915447']
    return np.stack([t10 + ob, t12 + oa, t12 - oa, t10 - ob], -1) + (1 << (shift - 1)) >> shift


def _pass2(x, shift):
    """jpeg_idct_2x2, one pass: (..., 8) -> (..., 2); only indices 0, 1, 3, 5, 7 are read."""
    t10 = x[..., 0] << 15
    t0 = -x[..., 7] * FIX['0.720959822'] + x[..., 5] * FIX['0.850430095'] - x[..., 3] * FIX['1.272758580'] + x[..., 1] * FIX['3.624509785']
    return np.stack([t10 + t0, t10 - t0], -1) + (1 << (shift - 1)) >> shift


def idct_reduced(coef: np.ndarray, qt: np.ndarray, s: int) -> np.ndarray:
    """(R, C, 64) int16 quantised blocks -> (R*s, C*s) uint8 sample plane with the s x s inverse transform."""
    R, C, _ = coef.shape
    qt = np.asarray(qt)
    if s == 8:
        return oj.idct_islow(coef, qt)
    if s == 1:
        return range_limit_table((coef[..., 0].astype(np.int64) * int(qt[0]) + 4) >> 3).astype(np.uint8)
    p, s1, s2 = {4: (_pass4, 12, 19), 2: (_pass2, 13, 20)}[s]
    x = (coef.astype(np.int64) * qt.astype(np.int64)).reshape(R, C, 8, 8)
    ws = p(x.swapaxes(-1, -2), s1).swapaxes(-1, -2)                  # pass 1 over columns: (R, C, s rows, 8 columns)
    return range_limit(p(ws, s2)).transpose(0, 2, 1, 3).reshape(R * s, C * s).astype(np.uint8)


def plan(height: int, width: int, samp, d: int) -> dict:
    """samp: [(h, v)] per component.  The dict sncal_amd.jpeg.scaled_layout returns."""
    m = 8 // d
    maxh, maxv = max(h for h, _ in samp), max(v for _, v in samp)
    block, hw, up = [], [], []
    for h, v in samp:
        s = m
        while s < 8 and (maxh * m) % (h * s * 2) == 0 and (maxv * m) % (v * s * 2) == 0:
            s *= 2
        block.append(s)
        hw.append((-(-height * v * s // (maxv * 8)), -(-width * h * s // (maxh * 8))))
        up.append(((maxv * m) // (v * s), (maxh * m) // (h * s)))
    return dict(out_hw=(-(-height * m // 8), -(-width * m // 8)), comp_block=block, comp_hw=hw, comp_up=up)


def decode_bgr(data: bytes, d: int, coefs=None) -> np.ndarray:
    """JPEG bytes -> (ceil(H / d), ceil(W / d), 3) uint8 BGR: cv2.imread(path, cv2.IMREAD_REDUCED_COLOR_<d>).
    coefs: the coefficient blocks to transform, where they shall not be the library's host stage's (oracle.jpeg.decode_coefficients)."""
    frame = oj.parse(data)
    if coefs is None:
        import sncal_amd
        coefs = sncal_amd.jpeg.entropy_decode(data)
    comps = frame['comps']
    samp = [(c['h'], c['v']) for c in comps] if len(comps) > 1 else [(1, 1)]
    pl = plan(frame['height'], frame['width'], samp, d)
    OH, OW = pl['out_hw']
    planes = []
    for cf, c, s, (ph, pw), (uv, uh) in zip(coefs, comps, pl['comp_block'], pl['comp_hw'], pl['comp_up']):
        p = idct_reduced(cf, frame['qt'][c['tq']], s)[:ph, :pw]
        fancy = d < 8 and pw > 2                                     # jinit_upsampler: do_fancy_upsampling && min_DCT_scaled_size > 1
        if (uv, uh) == (1, 2):
            p = oj._upsample_h2v1(p) if fancy else np.repeat(p, 2, 1)
        elif (uv, uh) == (2, 2):
            p = oj._upsample_h2v2(p) if fancy else np.repeat(np.repeat(p, 2, 0), 2, 1)
        else:
            assert (uv, uh) == (1, 1), (uv, uh)
        planes.append(np.asarray(p)[:OH, :OW].astype(np.uint8))
    if len(planes) == 1:
        return np.stack([planes[0]] * 3, -1)
    return oj.ycc_to_bgr(*planes)


def cases(gold_dir):
    """(npz, names, {name: [d, ...]}) of tests/golden/jpeg_reduced.npz."""
    import os
    g = np.load(os.path.join(gold_dir, 'jpeg_reduced.npz'))
    names = [str(n) for n in g['names']]
    return g, names, {n: [d for d in (2, 4, 8) if f'bgr.{n}.d{d}' in g.files] for n in names}
