"""Shared by tests/test_jpeg_streams_*.py: tests/golden/jpeg_streams.npz (tools/make_golden_jpeg_streams.py) and hand-built streams.

The fixture holds what a folder of real frames adds to the well-formed goldens: other Huffman and quantisation tables, every restart
layout, long marker segments, fill bytes in front of markers, and streams cut inside the scan.  `bgr.<name>` is the frame libjpeg-turbo
(inside Pillow) decodes; for the family cut_masked it is binding outside `mask.<name>` only (the MCU in which the data ran out)."""
import os

import numpy as np

from oracle import jpeg as oj

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FAMILY_COUNTS = dict(tables=8, restarts=3, segments=4, fill=2, cut_exact=64, cut_masked=64)
SIZES = ((48, 64), (29, 37), (16, 16))
_G = None


def fixture():
    global _G
    if _G is None:
        _G = np.load(os.path.join(GOLD, 'jpeg_streams.npz'))
    return _G


def names():
    return [str(n) for n in fixture()['names']]


def family(name):
    return name.split('.')[0]


def stream(name):
    return fixture()['jpg.' + name].tobytes()


def frame(name):
    return fixture()['bgr.' + name]


def binding(name):
    """(h, w) bool: where bgr.<name> must be met."""
    g = fixture()
    shape = g['bgr.' + name].shape[:2]
    return ~g['mask.' + name] if family(name) == 'cut_masked' else np.ones(shape, bool)


def mcu_boxes(data):
    """[(y0, y1, x0, x1)] of every MCU in raster order, clipped to the frame."""
    f = oj.parse(data)
    H, W = f['height'], f['width']
    mh, mw = 8 * f['comps'][0]['v'], 8 * f['comps'][0]['h']
    return [(y, min(y + mh, H), x, min(x + mw, W)) for y in range(0, H, mh) for x in range(0, W, mw)]


def grey_mcus(data, bgr):
    """MCUs of `bgr` that hold nothing but zero coefficients: 128 in every channel.  The outermost pixel ring of an MCU inside the frame
    is not looked at, because the fancy upsampling mixes one chroma sample of the neighbour into it."""
    H, W = bgr.shape[:2]
    out = []
    for k, (y0, y1, x0, x1) in enumerate(mcu_boxes(data)):
        box = bgr[y0 + (y0 > 0):y1 - (y1 < H), x0 + (x0 > 0):x1 - (x1 < W)]
        if box.size and (box == 128).all():
            out.append(k)
    return out


def handmade_grey_8x8(scan: bytes, eoi: bool = True) -> bytes:
    """An 8x8 grey baseline stream around `scan`: quantisation table of ones, a DC table with the one code '0' (category 0), an AC table
    with '0' = 0xF1 (run 15, one value bit) and '10' = 0x00 (end of block).  Four 0xF1 symbols walk the index past 63."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + body
    dqt = seg(0xDB, bytes([0]) + bytes([1] * 64))
    sof = seg(0xC0, bytes([8, 0, 8, 0, 8, 1, 1, 0x11, 0]))
    dc = seg(0xC4, bytes([0x00, 1] + [0] * 15 + [0]))
    ac = seg(0xC4, bytes([0x10, 1, 1] + [0] * 14 + [0xF1, 0x00]))
    sos = seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0]))
    return b'\xff\xd8' + dqt + sof + dc + ac + sos + scan + (b'\xff\xd9' if eoi else b'')


def handmade_flat_8x8(positive: bool, q: int = 3) -> bytes:
    """A well-formed 8x8 grey stream of one flat block far outside 0..255: quantisation table of `q`, DC difference +2047 or -2047
    (category 11, the one DC code '0'), end of block at once.  With q = 3 every sample of the inverse transform is +768 or -768 around the
    level shift: libjpeg-turbo's SIMD 8x8, 4x4 and 2x2 transforms saturate it to 255 / 0, while jdmaster.c's clamp table, its index masked
    with RANGE_MASK, gives 0 / 255 -- which is what jpeg_idct_1x1, plain C, returns at scale 1/8 (held to libjpeg-turbo by the fixture's tool)."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + body
    scan = bytes([0x7F, 0xF7]) if positive else bytes([0x00, 0x07])          # '0', eleven value bits, '0' = end of block, padding ones
    return b'\xff\xd8' + seg(0xDB, bytes([0]) + bytes([q] * 64)) + seg(0xC0, bytes([8, 0, 8, 0, 8, 1, 1, 0x11, 0])) + \
        seg(0xC4, bytes([0x00, 1] + [0] * 15 + [11])) + seg(0xC4, bytes([0x10, 1] + [0] * 15 + [0x00])) + \
        seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + scan + b'\xff\xd9'


# reduce -> (value of every pixel for +2047, for -2047)
FLAT_WANT = {1: (255, 0), 2: (255, 0), 4: (255, 0), 8: (0, 255)}


def restart_markers(data):
    """Indices of the FF of every RSTn of the scan."""
    sos = data.find(b'\xff\xda')
    return [i for i in range(sos, len(data) - 2) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def interval_damage():
    """{name: (source case, stream)}: restart interval 1 (between RST0 and RST1) of two fixture streams short of data, every later
    marker intact -- its last 1 or 3 bytes or its second half gone (the bits that are left are genuine, then they run out), or 3
    bytes gone from its middle (genuine bits, then garbage).  libjpeg finishes the MCU in which the data runs out on zero bits, skips
    the rest of THAT interval and goes on at RST1; the fixture's tool holds the oracle to libjpeg-turbo's frame on each of these."""
    out = {}
    for src in ('restarts.every_mcu_420_48x64', 'restarts.every_row_422_29x37'):
        data = stream(src)
        at = restart_markers(data)
        lo, hi = at[0] + 2, at[1]                          # interval 1
        assert hi - lo >= 12
        for what, a, b in (('tail1', hi - 1, hi), ('tail3', hi - 3, hi), ('half', (lo + hi) // 2, hi), ('mid3', (lo + hi) // 2 - 1, (lo + hi) // 2 + 2)):
            cut = data[:a] + data[b:]
            if 0xFF in data[a - 1:b]:                      # neither take a stuffed byte apart nor make one
                continue
            out[f'{src}.{what}'] = (src, cut)
    return out


def wrong_marker_inside_an_interval():
    """restarts.every_mcu_420_48x64 with RST5 written over two bytes in the middle of interval 1: the data of that interval runs out at a
    marker that is not the one due at its end."""
    data = stream('restarts.every_mcu_420_48x64')
    at = restart_markers(data)
    m = (at[0] + 2 + at[1]) // 2
    assert 0xFF not in data[m - 1:m + 3]
    return data[:m] + b'\xff\xd5' + data[m + 2:]
