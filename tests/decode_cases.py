"""Inputs of the decode edge tests (csrc/decode.hip), built in numpy; tests/test_decode_cases_host.py shows with the oracle alone
(oracle/decode.py) that each one discriminates, tests/test_decode_edges_gpu.py runs them through the kernels.

    plan(w, aligned)                 which kp_decode_kernel<VEC, NQ> sncal_heatmap_decode launches, restated
    collision_plane(...)             distinct log-probabilities that collapse to one float after exp
    variant_case(h, w) / big_case    the planes planted for every launch variant / for the largest admitted shapes
    line_shortcut_case(which)        equal maxima on either side of the line decode's `t > 17.5` shortcut (sigma 3)
    line_plateau(shape, seed)        a quantised plane: thousands of equal maxima
    tie_state_dict(sd, cfg)          a network whose logit planes are constant: every pixel ties

Everything is deterministic (PCG64 seeds) and nothing here touches a GPU."""
import numpy as np

# ---- D1: the launch variants -----------------------------------------------------------------------------------------------------
VEC4_WIDTHS = (256, 260, 512, 516, 1024, 1028, 2048)                          # w % 4 == 0, aligned base: 16-byte loads
SCALAR_WIDTHS = (65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2047)          # w % 4 != 0: scalar loads
OFFSET_WIDTHS = (64, 128, 1024, 2048)                                         # w % 4 == 0, base one float off 16 bytes: scalar loads
HEIGHTS = (1, 2, 3, 5, 7)                                                     # fewer rows than the 4 waves, and not a multiple of 4
VARIANT_CASES = [(w, True) for w in VEC4_WIDTHS + SCALAR_WIDTHS] + [(w, False) for w in OFFSET_WIDTHS]
ALL_VARIANTS = {(4, 1), (4, 2), (4, 4), (4, 8), (1, 1), (1, 2), (1, 4), (1, 8), (1, 16), (1, 32)}
DECODE_SIZES = ((540, 960), (537, 955))                                       # the second divides none of the widths / heights

LDS_MAX = 65536                                                               # bytes of LDS a decode workgroup may ask for
BIG_OK = ((6140, 2048), (8192, 1637))                                         # (h + 5 w + 4) * 4 = 65536 / 65524: the largest at either end
BIG_REFUSED = ((6141, 2048), (8192, 1638))                                    # 65540 / 65544


def plan(w, aligned):
    """(VEC, NQ) of the kp_decode_kernel instantiation sncal_heatmap_decode picks for width w: 16-byte loads iff w % 4 == 0 and the
    base pointer is 16-byte aligned; a lane owns column group lane + 64 q, q < NQ = ceil(nvec / 64) rounded up to its bucket."""
    vec = 4 if (w % 4 == 0 and aligned) else 1
    nvec = -(-w // vec)
    nq = -(-nvec // 64)
    for bucket in ((1, 2, 4, 8) if vec == 4 else (1, 2, 4, 8, 16, 32)):
        if nq <= bucket:
            return vec, bucket
    raise ValueError(f'width {w} has no launch variant')


def decode_lds_bytes(h, w):
    return (h + 5 * w + 4) * 4


def last_group_start(w, aligned):
    """First column of the last lane group (q = NQ_used - 1) of the variant that serves width w."""
    vec, _ = plan(w, aligned)
    nvec = -(-w // vec)
    return 64 * vec * ((nvec - 1) // 64)


def collision_plane(h, w, early, late, background=-5.0):
    """-3e-9 at `early` = (row, col) and -1e-9 at `late`: both are exp_ref -> 1.0f, so the reference's first occurrence after exp is
    the early row / column, while the argmax of the log-probabilities is the late one."""
    p = np.full((h, w), background, dtype=np.float32)
    p[early] = -3e-9
    p[late] = -1e-9
    return p


def raw_argmax_xy(plane):
    """What a decode that reduced the log-probabilities themselves would answer: argmax of the raw column / row maxima."""
    return int(plane.max(axis=0).argmax()), int(plane.max(axis=1).argmax())


def _noise(rng, shape):
    return (-4.0 - 8.0 * rng.random(shape)).astype(np.float32)                 # log-probabilities in (-12, -4]


def variant_case(h, w, aligned=True):
    """(3, 3, h, w) log-probabilities: six decoded planes (channel 2 is the dropped background) over noise in (-12, -4]

        [0,0]  the maximum in the last row and last column          [0,1]  the maximum in row 0 and column 0
        [1,0]  an exact tie: (last row, a column of lane group 0) and (the row before, a column of the last lane group)
        [1,1]  the collision plane over the same two column groups and two adjacent rows (adjacent rows belong to different waves)
        [2,0]  all -inf                                              [2,1]  noise alone

    The column of lane group 0 is 70 on the 16-byte path (lane 17; column 70 belongs to wave 1 in the final search over the columns,
    the tied later column to wave 0 whenever the last group starts at a multiple of 256) and 10 on the scalar path.  h = 1 has one row
    only: the row plants fall on row 0.  Also returns the planted positions {name: ((row, col) early, (row, col) late)}."""
    rng = np.random.Generator(np.random.PCG64(h * 10007 + w * 3 + int(aligned)))
    lp = _noise(rng, (3, 3, h, w))
    vec, _ = plan(w, aligned)
    c_early = 70 if vec == 4 else 10
    c_late = max(last_group_start(w, aligned), w // 2)
    r_late, r_early = h - 1, max(h - 2, 0)
    assert c_early < 64 * vec and c_early < c_late < w
    lp[0, 0, h - 1, w - 1] = -0.5
    lp[0, 1, 0, 0] = -0.25
    lp[1, 0, r_late, c_early] = -0.125                      # x: the early column, y: the row of the LATE column (two separate reductions)
    lp[1, 0, r_early, c_late] = -0.125
    lp[1, 1] = collision_plane(h, w, (r_early, c_early), (r_late, w - 1))
    lp[2, 0] = -np.inf
    where = {'last': (h - 1, w - 1), 'first': (0, 0), 'tie': ((r_late, c_early), (r_early, c_late)),
             'collision': ((r_early, c_early), (r_late, w - 1))}
    return lp, where


def big_case(h, w):
    """(1, 2, h, w) for the largest admitted shapes: one decoded plane of noise with the collision pair -3e-9 at (100, 100) and -1e-9 at
    (512, 512).  In the final search over the h row maxima / w column maxima thread t reads indices t, t + 256, ...: index 100 is
    wave 1's, 512 wave 0's, so a search that kept one wave's answer, or compared the log-probabilities, answers 512.  BIG_LAST is a
    second plant the test adds afterwards: the only maximum in the last row and column, the far ends of the LDS vectors."""
    rng = np.random.Generator(np.random.PCG64(h + w))
    lp = np.empty((1, 2, h, w), dtype=np.float32)
    lp[0, 0] = -4.0 - 8.0 * rng.random((h, w), dtype=np.float32)
    lp[0, 1] = -1.0
    lp[0, 0, 100, 100] = -3e-9
    lp[0, 0, 512, 512] = -1e-9
    return lp


BIG_FIRST = (100, 100)        # (row, col) the oracle answers on big_case
BIG_RAW = (512, 512)          # ... and the argmax of the log-probabilities
BIG_LAST = 0.5                # value the test then writes at (h - 1, w - 1)


# ---- L2: the line decode ---------------------------------------------------------------------------------------------------------
LINE_HW = (135, 240)
# (y1, x1) of the six planes of a (2, 3, 135, 240) batch; flat index % 256 = 188, 0, 76, 63, 218, 133: every wave finds a first peak
LINE_PEAKS = ((40, 60), (0, 0), (100, 140), (67, 111), (3, 10), (120, 5))


def line_shortcut_case(which):
    """(2, 3, 135, 240) heat maps for sigma 3 (2 sigma^2 = 18).  Every plane holds the same value three times over a background below it:
    the first peak at (y1, x1), a neighbour, and B far away at a later flat index.

        'below'  neighbour A  at (y1, x1 + 17):      d2 = 289, t = 16.06 -- the keep factor 1 - exp(-t) is 1 - 2^-23, A loses its last
                 bit and the second peak is B.  A decode that skipped the exp from t = 16 on would answer A.
        'above'  neighbour A' at (y1 + 12, x1 + 13): d2 = 313, t = 17.39 -- the keep factor is exactly 1.0f, A' ties with B and comes first.

    Returns (heat, expected second-peak (y, x) per plane)."""
    H, W = LINE_HW
    rng = np.random.Generator(np.random.PCG64(5 if which == 'below' else 6))
    heat = (rng.random((2, 3, H, W)) * 0.5 - 0.1).astype(np.float32)            # background in [-0.1, 0.4): relu matters, no tie with the peaks
    dy, dx = {'below': (0, 17), 'above': (12, 13)}[which]
    want = []
    for k, (y1, x1) in enumerate(LINE_PEAKS):
        plane = heat[k // 3, k % 3]
        yb, xb = H - 2, (x1 + 120) % W                      # B: the row before the last, at least 103 columns away
        assert (yb, xb) > (y1 + dy, x1 + dx) and y1 + dy < H and x1 + dx < W
        for (y, x) in ((y1, x1), (y1 + dy, x1 + dx), (yb, xb)):
            plane[y, x] = 0.75
        want.append((yb, xb) if which == 'below' else (y1 + dy, x1 + dx))
    return heat, want


def line_plateau(shape=(2, 3) + LINE_HW, seed=9):
    """round(u * 8) / 8 - 0.25 with u uniform in [0, 1): nine levels from -0.25 to 0.75, one pixel in sixteen at the maximum."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.round(rng.random(shape) * 8) / 8 - 0.25).astype(np.float32)


LINE_SMALL_SHAPES = ((1, 1), (1, 5), (3, 7), (7, 1), (16, 16), (17, 31))        # below one workgroup, w = 1, n = 256, n % 256 != 0


def line_all_negative(shape=(2, 3, 17, 31)):
    rng = np.random.Generator(np.random.PCG64(12))
    return (-0.01 - rng.random(shape)).astype(np.float32)


def line_single_pixel(at_last, shape=(2, 3, 17, 31)):
    """One positive pixel per plane, at flat index 0 or at the last one; everything else is negative (zero after the relu)."""
    heat = line_all_negative(shape)
    flat = heat.reshape(shape[0], shape[1], -1)
    flat[..., -1 if at_last else 0] = 0.6
    return heat


# ---- ties through the fused decodes ----------------------------------------------------------------------------------------------
def tie_bias(n):
    """The fixed BatchNorm bias of the head's hidden layer: channel 5 at +30, the rest spread evenly over [-2, 2], channels 7 and 11 equal."""
    b = np.linspace(-2.0, 2.0, n).astype(np.float32)
    b[5] = 30.0
    b[11] = b[7]
    return b


def tie_state_dict(sd, prefix='model.'):
    """A copy of state dict `sd` whose last_layer.1 (the BatchNorm behind the head's first convolution) has weight zero and the bias
    tie_bias: the hidden activation, and with it every logit plane, no longer depends on the pixel."""
    import torch
    out = {k: v.clone() for k, v in sd.items()}
    n = out[prefix + 'last_layer.1.weight'].numel()
    out[prefix + 'last_layer.1.weight'] = torch.zeros(n, dtype=torch.float32)
    out[prefix + 'last_layer.1.bias'] = torch.from_numpy(tie_bias(n))
    return out
