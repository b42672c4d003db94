"""tests/golden/jpeg_streams.npz: JPEG streams that are cut short, padded or otherwise unlike the well-formed goldens of
jpeg_cases.npz, and the frames libjpeg-turbo decodes from them (Pillow's decoder = the library cv2.imread wraps, same defaults).

    python tools/make_golden_jpeg_streams.py

    names                  case names, '<family>.<what>'; sizes are 48x64, 29x37 and 16x16
    family_counts          'family=count' strings, the plan below
    jpg.<name>             the stream
    bgr.<name>             (h, w, 3) uint8 BGR, what Pillow decodes from it
    mask.<name>            cut_masked only: (h, w) bool, the MCU in which the scan's data ran out, grown by 2 pixels

Families
    tables      optimised Huffman tables; quantisation tables of all 1 and all 255 on noise (the largest coefficient categories, blocks
                without EOB); tables of 300 (16-bit DQT, SOF1); quality 1 and 100 on noise
    restarts    an interval of one MCU (twelve intervals: RST7 wraps to RST0), of one MCU row, and one larger than the scan
    segments    a COM segment, a 100 KB ICC profile (several APP2 segments), both again with restart intervals
    fill        two restart streams with FF FF in front of every RSTn and of EOI (T.81 B.1.1.2); the frame is the unpadded stream's
    cut_exact   q95 streams cut inside the scan, FF D9 appended: every pixel equals libjpeg-turbo's
    cut_masked  the same cuts of q60 and q20 streams, each with the mask of the MCU in which the data ran out.  The zero bits that finish
                that MCU give coefficients whose samples leave the range jdmaster.c's clamp table covers; libjpeg-turbo's SIMD IDCT
                saturates there, jidctint.c wraps.  The oracle and the kernels saturate, so these frames are equal inside the mask too
                (asserted here and by the tests); the mask marks where a decoder that wraps would differ

Every frame is checked against oracle.jpeg.decode_bgr -- everywhere, for cut_masked outside the mask -- and nothing is written when
one differs.
A stream with no EOI at all is not here: Pillow's source manager suspends on it; jdatasrc.c's rule (the end of the data reads as
FF D9) is asserted by the tests as an identity.
"""
import io
import os
import sys
import zipfile

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import jpeg_test_image                 # noqa: E402
from oracle import jpeg as oj                           # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
MAX_BYTES = 350 * 1000
SUB = {'444': 0, '422': 1, '420': 2}
FAMILY_COUNTS = dict(tables=8, restarts=3, segments=4, fill=2, cut_exact=64, cut_masked=64)
CUTS = ('start', 'start1', 'half', 'last', 'seed0', 'seed1', 'seed2', 'ff')
# cut sources: (layout, (h, w), restart interval), each layout with and without restarts.  A cut_exact source has enough MCUs for the
# cut at half of the scan to leave a whole MCU without data; 4:2:2 at 16x16 has two MCUs and serves cut_masked only
SOURCES = dict(cut_exact=[('444', (16, 16), 0), ('422', (29, 37), 0), ('420', (48, 64), 0), ('gray', (16, 16), 0),
                          ('444', (16, 16), 3), ('422', (29, 37), 2), ('420', (29, 37), 2), ('gray', (16, 16), 2)],
               cut_masked=[('444', (16, 16), 0), ('422', (16, 16), 0), ('420', (29, 37), 0), ('gray', (16, 16), 0),
                           ('444', (16, 16), 3), ('422', (16, 16), 1), ('420', (29, 37), 2), ('gray', (16, 16), 2)])


def noise_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def encode(img, sub, **kw):
    im = Image.fromarray(img)
    if sub == 'gray':
        im = im.convert('L')
    else:
        kw['subsampling'] = SUB[sub]
    b = io.BytesIO()
    im.save(b, 'JPEG', **kw)
    return b.getvalue()


def pillow_bgr(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))[..., ::-1])


def scan_span(data):
    """(first byte of the entropy-coded segment, index of the EOI marker)."""
    i = 2
    while data[i + 1] != 0xDA:
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    start = i + 2 + ((data[i + 2] << 8) | data[i + 3])
    assert data[-2:] == b'\xff\xd9'
    return start, len(data) - 2


def pad_markers(data):
    """FF FF in front of every RSTn of the scan and of EOI."""
    start, end = scan_span(data)
    out, i = bytearray(data[:start]), start
    while i < end:
        if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7:
            out += b'\xff\xff'
        if data[i] == 0xFF:
            out += data[i:i + 2]
            i += 2
        else:
            out.append(data[i])
            i += 1
    return bytes(out) + b'\xff\xff' + data[end:]


def starved_mcu(data):
    """(raster index of the MCU in which the data ran out or None, MCU count, MCUs per row, (MCU height, MCU width))."""
    f = oj.parse(data)
    oj.decode_coefficients(f)
    hs, vs = f['comps'][0]['h'], f['comps'][0]['v']
    mx, my = -(-f['width'] // (8 * hs)), -(-f['height'] // (8 * vs))
    return f['starved_mcu'], mx * my, mx, (8 * vs, 8 * hs)


def fixed_cuts(data):
    """The whole scan missing, one byte of it, half of it, all but its last byte."""
    start, end = scan_span(data)
    return [start, start + 1, (start + end) // 2, end - 1]


def leaves_an_mcu_out(data, c):
    m, n, _, _ = starved_mcu(data[:c] + b'\xff\xd9')
    return m is not None and m < n - 1


def stuffed_cuts(data):
    """Cut lengths that end ON the FF of a stuffed FF 00, are none of the fixed cuts and leave at least one whole MCU without data."""
    start, end = scan_span(data)
    ff = [i + 1 for i in range(start, end - 1) if data[i] == 0xFF and data[i + 1] == 0x00]
    return [c for c in ff if c not in fixed_cuts(data) and leaves_an_mcu_out(data, c)]


def cut_offsets(data, rng):
    """The eight cut lengths of one source stream, in the order of CUTS.  The seeded cuts and the cut on a stuffed FF leave at least
    one whole MCU without data (the tests assert that such an MCU is grey)."""
    start, end = scan_span(data)
    ff = stuffed_cuts(data)
    ff = ff[len(ff) // 2]
    cuts = fixed_cuts(data)
    while len(cuts) < 7:
        c = int(rng.integers(start + 2, end - 1))
        if c not in cuts and c != ff and leaves_an_mcu_out(data, c):
            cuts.append(c)
    return cuts + [ff]


def main():
    assert features.check_feature('libjpeg_turbo')
    out, names = {}, []

    def add(name, data, want=None, masked=False):
        got_pil = pillow_bgr(data)
        if want is not None:
            assert np.array_equal(got_pil, want), name + ': Pillow does not give the expected frame'
        got = oj.decode_bgr(data)
        diff = (got != got_pil).any(-1)
        if masked:
            m, _, mx, (mh, mw) = starved_mcu(data)
            assert m is not None, name
            y0, x0 = (m // mx) * mh, (m % mx) * mw
            mask = np.zeros(got.shape[:2], bool)
            mask[max(0, y0 - 2):y0 + mh + 2, max(0, x0 - 2):x0 + mw + 2] = True
            assert mask.sum() <= 400
            out['mask.' + name] = mask
            assert not (diff & ~mask).any(), f'{name}: the oracle differs from libjpeg-turbo outside the mask'
        assert not diff.any(), f'{name}: the oracle differs from libjpeg-turbo in {int(diff.sum())} pixels'
        names.append(name)
        out['jpg.' + name] = np.frombuffer(data, np.uint8)
        out['bgr.' + name] = got_pil

    # ---- tables
    add('tables.opt_444_48x64', encode(jpeg_test_image(48, 64, 300), '444', quality=85, optimize=True))
    add('tables.opt_420_29x37', encode(jpeg_test_image(29, 37, 301), '420', quality=75, optimize=True))
    add('tables.opt_gray_16x16', encode(jpeg_test_image(16, 16, 302), 'gray', quality=75, optimize=True))
    add('tables.q1_noise_444_16x16', encode(noise_image(16, 16, 303), '444', qtables=[[1] * 64] * 2))
    add('tables.q255_noise_444_16x16', encode(noise_image(16, 16, 304), '444', qtables=[[255] * 64] * 2))
    d16 = encode(jpeg_test_image(29, 37, 305), '444', qtables=[[300] * 64] * 2)
    assert b'\xff\xc1' in d16[:700], 'tables of 300 should make a 16-bit DQT under SOF1'
    add('tables.q300_sof1_444_29x37', d16)
    add('tables.quality1_noise_420_29x37', encode(noise_image(29, 37, 306), '420', quality=1))
    add('tables.quality100_noise_420_16x16', encode(noise_image(16, 16, 307), '420', quality=100))

    # ---- restarts
    r_blocks = encode(jpeg_test_image(48, 64, 310), '420', quality=75, restart_marker_blocks=1)
    assert oj.parse(r_blocks)['restart'] == 1 and r_blocks.count(b'\xff\xd0') >= 2     # 12 MCUs: RST0..RST7, RST0..RST2
    add('restarts.every_mcu_420_48x64', r_blocks)
    r_rows = encode(jpeg_test_image(29, 37, 311), '422', quality=75, restart_marker_rows=1)
    assert oj.parse(r_rows)['restart'] == 3
    add('restarts.every_row_422_29x37', r_rows)
    r_big = encode(jpeg_test_image(16, 16, 312), '444', quality=75, restart_marker_blocks=1000)
    assert oj.parse(r_big)['restart'] == 1000
    add('restarts.beyond_the_scan_444_16x16', r_big)

    # ---- segments
    icc = (b'no real profile: libjpeg only carries these bytes along. ' * 1800)[:100 * 1024]      # (a built one would embed today's date)
    add('segments.com_420_16x16', encode(jpeg_test_image(16, 16, 320), '420', quality=75, comment=b'frame 00017 of the left camera'))
    d_icc = encode(jpeg_test_image(29, 37, 321), '444', quality=75, icc_profile=icc)
    assert d_icc.count(b'ICC_PROFILE\0') >= 2
    add('segments.icc_444_29x37', d_icc)
    add('segments.com_restart_422_16x16', encode(jpeg_test_image(16, 16, 322), '422', quality=75, comment=b'x' * 300, restart_marker_blocks=1))
    add('segments.icc_restart_420_16x16', encode(jpeg_test_image(16, 16, 323), '420', quality=75, icc_profile=icc, restart_marker_rows=1))

    # ---- fill
    for name, src in (('fill.every_mcu_420_48x64', r_blocks), ('fill.every_row_422_29x37', r_rows)):
        padded = pad_markers(src)
        assert padded.count(b'\xff\xff') >= 3 and len(padded) > len(src)
        add(name, padded, want=pillow_bgr(src))

    # ---- checked here against libjpeg-turbo, not stored: a cut right in front of a restart marker, behind its FF and behind the marker
    # (the interval that follows starves as a whole), and the hand-built stream whose index runs past 63 on the zeros behind the data
    n_edge = 0
    for src in (r_blocks, r_rows):
        start, end = scan_span(src)
        for i in range(start, end - 1):
            if src[i] == 0xFF and 0xD0 <= src[i + 1] <= 0xD7:
                for c in (i, i + 1, i + 2):
                    cut = src[:c] + b'\xff\xd9'
                    assert np.array_equal(oj.decode_bgr(cut), pillow_bgr(cut)), ('cut at a restart marker', i - start, c - i)
                    n_edge += 1
    assert n_edge == 3 * (11 + 3)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from jpeg_streams_cases import handmade_grey_8x8
    over = handmade_grey_8x8(bytes([0b00101010]))
    assert oj.decode_coefficients(oj.parse(over))[0][0, 0, 63] == -1 and np.array_equal(oj.decode_bgr(over), pillow_bgr(over))
    # ... and the flat blocks 768 beyond the level shift: the SIMD 8x8 / 4x4 / 2x2 transforms saturate, jpeg_idct_1x1 indexes the table
    from jpeg_streams_cases import handmade_flat_8x8, FLAT_WANT
    for k, positive in enumerate((True, False)):
        flat = handmade_flat_8x8(positive)
        assert abs(int(oj.decode_coefficients(oj.parse(flat))[0][0, 0, 0])) == 2047
        for d, want in FLAT_WANT.items():
            im = Image.open(io.BytesIO(flat))
            if d > 1:
                im.draft(im.mode, (8 // d, 8 // d))
                assert im.decoderconfig == (d, 0)
            got = np.asarray(im.convert('RGB'))
            assert got.shape == (8 // d, 8 // d, 3) and (got == want[k]).all(), (positive, d, got[0, 0], want[k])

    # ... an interval short of data with every later marker intact: libjpeg skips to the end of THAT interval and goes on
    from jpeg_streams_cases import interval_damage, wrong_marker_inside_an_interval
    n_damage = 0
    for name, (src, cut) in interval_damage().items():
        if name == 'restarts.every_row_422_29x37.mid3':       # garbage that uses up the interval's bits without running out: refused
            continue
        assert np.array_equal(oj.decode_bgr(cut), pillow_bgr(cut)), name
        n_damage += 1
    assert n_damage == 7
    for refused in (interval_damage()['restarts.every_row_422_29x37.mid3'][1], wrong_marker_inside_an_interval()):
        try:
            oj.decode_bgr(refused)
            raise AssertionError('damage inside genuine data was decoded')
        except oj.JpegError:
            pass

    # ---- cuts
    rng = np.random.default_rng(20240611)
    for family, qualities in (('cut_exact', (95,) * 8), ('cut_masked', (60, 20, 60, 20, 20, 60, 20, 60))):
        for k, ((sub, (h, w), rs), q) in enumerate(zip(SOURCES[family], qualities)):
            kw = dict(quality=q)
            if rs:
                kw['restart_marker_blocks'] = rs
            seed = (400 if family == 'cut_exact' else 500) + k
            while True:                                 # the first image of the series whose stream has a stuffed FF 00 to cut on
                src = encode(jpeg_test_image(h, w, seed), sub, **kw)
                if stuffed_cuts(src):
                    break
                seed += 10
            for what, c in zip(CUTS, cut_offsets(src, rng)):
                add(f'{family}.{h}x{w}_{sub}_q{q}_r{rs}.{what}', src[:c] + b'\xff\xd9', masked=family == 'cut_masked')

    # ... and the reduced decode of every 48x64 and 29x37 cut frame: the restatement the GPU tests compare with (tests/jpeg_reduced_ref.py),
    # fed the oracle's coefficients, equals libjpeg-turbo's scaled decode in every pixel
    import jpeg_reduced_ref as rr
    n_reduced = 0
    for name in names:
        data = out['jpg.' + name].tobytes()
        if name.startswith('cut') and out['bgr.' + name].shape[0] in (48, 29):
            for d in (2, 4):
                im = Image.open(io.BytesIO(data))
                w, h = im.size
                im.draft(im.mode, (w // d, h // d))
                assert im.decoderconfig == (d, 0)
                want = np.asarray(im.convert('RGB'))[..., ::-1]
                got = rr.decode_bgr(data, d, coefs=oj.decode_coefficients(oj.parse(data)))
                assert np.array_equal(got, want), (name, d)
                n_reduced += 1
    assert n_reduced == 2 * 8 * 6

    counts = {f: sum(n.startswith(f + '.') for n in names) for f in FAMILY_COUNTS}
    assert counts == FAMILY_COUNTS and sum(counts.values()) == len(names), counts
    out['names'] = np.array(names)
    out['family_counts'] = np.array([f'{f}={n}' for f, n in FAMILY_COUNTS.items()])
    path = os.path.join(GOLD, 'jpeg_streams.npz')
    blob = io.BytesIO()
    with zipfile.ZipFile(blob, 'w') as z:               # np.savez_compressed's layout with a fixed member date: the same bytes every run
        for key, arr in out.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, member.getvalue(), compresslevel=9)
    size = len(blob.getvalue())
    if size > MAX_BYTES:
        raise SystemExit(f'jpeg_streams.npz would be {size} bytes, over {MAX_BYTES}')
    with open(path, 'wb') as f:
        f.write(blob.getvalue())
    print('jpeg_streams ok:', len(names), 'cases', counts, 'file', size // 1024, 'KiB')


if __name__ == '__main__':
    main()
