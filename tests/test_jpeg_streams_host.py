"""CPU: the JPEG entropy stage on streams that are cut short, padded or otherwise unlike the well-formed goldens (tests/golden/jpeg_streams.npz,
tools/make_golden_jpeg_streams.py; tests/jpeg_streams_cases.py).  The oracle is held to libjpeg-turbo's frames, the library's host stage
(sncal_jpeg_entropy_decode, no GPU) to the oracle's coefficient blocks.  Every comparison is equality.

libjpeg's rules for a scan that ends early (jdhuff.c): the MCU in which the data runs out is finished on zero bits, every later MCU is
skipped and stays zero -- flat grey.  0xFF fill bytes in front of a marker are skipped (T.81 B.1.1.2).  A stream without EOI decodes as
the same bytes plus FF D9 (jdatasrc.c)."""
import numpy as np
import pytest

import jpeg_streams_cases as sc
from oracle import jpeg as oj


def _coefs_equal(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def test_fixture_keeps_its_own_promises():
    g, names = sc.fixture(), sc.names()
    assert len(set(names)) == len(names)
    counts = {f: sum(sc.family(n) == f for n in names) for f in sc.FAMILY_COUNTS}
    assert counts == sc.FAMILY_COUNTS and sum(counts.values()) == len(names)
    assert sorted(str(s) for s in g['family_counts']) == sorted(f'{f}={n}' for f, n in sc.FAMILY_COUNTS.items())
    assert sorted(g.files) == sorted(['names', 'family_counts'] + ['jpg.' + n for n in names] + ['bgr.' + n for n in names] +
                                     ['mask.' + n for n in names if sc.family(n) == 'cut_masked'])
    for n in names:
        bgr = sc.frame(n)
        assert bgr.dtype == np.uint8 and bgr.shape[:2] in sc.SIZES and bgr.shape[2] == 3, n
        data = sc.stream(n)
        if sc.family(n) == 'cut_masked':
            m = g['mask.' + n]
            assert m.dtype == np.bool_ and m.shape == bgr.shape[:2] and 0 < m.sum() <= 400, n
            ys, xs = np.nonzero(m)
            assert (ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1) == m.sum() <= 20 * 20, n        # one box
        if sc.family(n).startswith('cut'):
            assert data.endswith(b'\xff\xd9') and not data[:-2].endswith(b'\xff\xd9'), n
            if n.endswith('.ff'):
                assert data[-3] == 0xFF, n                       # cut on the FF of a stuffed FF 00
        if sc.family(n) == 'cut_exact' and not n.endswith('.last'):
            assert sc.grey_mcus(data, bgr), n                    # libjpeg-turbo left at least one MCU without any data flat grey
        if sc.family(n) == 'fill':
            assert data.endswith(b'\xff\xff\xff\xd9') and data.count(b'\xff\xff\xd0') >= 1, n
    assert sum(b'\xff\xc1' in sc.stream(n)[:800] for n in names if sc.family(n) == 'tables') == 1       # the 16-bit tables' SOF1
    every_mcu = sc.stream('restarts.every_mcu_420_48x64')
    assert [every_mcu.count(bytes([0xFF, 0xD0 + k])) >= 1 for k in range(8)] == [True] * 8              # RST7 wraps to RST0


@pytest.mark.parametrize('name', sc.names())
def test_oracle_equals_libjpeg_turbo(name):
    """Every pixel, and for cut_masked every pixel outside the starved MCU's mask."""
    got = oj.decode_bgr(sc.stream(name))
    want, where = sc.frame(name), sc.binding(name)
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = (got != want).any(-1) & where
    assert not diff.any(), (name, int(diff.sum()), int(np.abs(got.astype(int) - want)[diff].max()))


def test_the_starved_mcus_equal_libjpeg_turbo_too():
    """Inside the masks of cut_masked, and in the last MCU of the q95 stream that lost its last byte, the zero bits that finish the starved
    MCU give samples beyond the range jdmaster.c's clamp table covers (|x| >= 512, where its masked index wraps).  libjpeg-turbo's SIMD
    inverse DCT saturates there, and so does the oracle: equal everywhere.  The table's wrap is shown to differ on these very cases, so the
    fixture does tell the two apart."""
    def wrapped(coef, qt):
        R, C, _ = coef.shape
        x = (coef.astype(np.int64) * qt.astype(np.int64)).reshape(R, C, 8, 8)
        y = oj._idct_1d(oj._idct_1d(x.swapaxes(-1, -2), 11).swapaxes(-1, -2), 18) & 1023
        px = np.where(y < 128, y + 128, np.where(y < 512, 255, np.where(y < 896, 0, y - 896)))
        return px.transpose(0, 2, 1, 3).reshape(R * 8, C * 8).astype(np.uint8)
    told_apart = []
    for name in sc.names():
        data = sc.stream(name)
        assert np.array_equal(oj.decode_bgr(data), sc.frame(name)), name
        f = oj.parse(data)
        planes = [wrapped(cf, f['qt'][c['tq']]) for cf, c in zip(oj.decode_coefficients(f), f['comps'])]
        if any(not np.array_equal(p, q) for p, q in zip(planes, oj.decode_planes(oj.parse(data)))):
            told_apart.append(name)
    assert 'cut_exact.29x37_420_q95_r2.last' in told_apart and sum(sc.family(n) == 'cut_masked' for n in told_apart) >= 20
    assert all(sc.family(n).startswith('cut') for n in told_apart)


def test_flat_blocks_beyond_the_clamp_table_saturate_except_at_one_eighth(sncal):
    """tests/jpeg_streams_cases.py handmade_flat_8x8: what libjpeg-turbo returns for them is asserted by the fixture's tool."""
    import jpeg_reduced_ref as rr
    for k, positive in enumerate((True, False)):
        data = sc.handmade_flat_8x8(positive)
        coefs = oj.decode_coefficients(oj.parse(data))
        assert coefs[0][0, 0, 0] == (2047 if positive else -2047) and not coefs[0][0, 0, 1:].any()
        assert _coefs_equal(sncal.jpeg.entropy_decode(data), coefs)
        assert (oj.decode_bgr(data) == sc.FLAT_WANT[1][k]).all()
        for d in (2, 4, 8):
            got = rr.decode_bgr(data, d, coefs=coefs)
            assert got.shape == (8 // d, 8 // d, 3) and (got == sc.FLAT_WANT[d][k]).all(), (positive, d)


def test_host_stage_equals_the_oracles_coefficients_on_every_case(sncal):
    for name in sc.names():
        data = sc.stream(name)
        f = oj.parse(data)
        want = oj.decode_coefficients(f)
        info = sncal.jpeg.probe(data)
        assert (info['height'], info['width'], info['components'], info['restart_interval']) == \
               (f['height'], f['width'], len(f['comps']), f['restart']), name
        assert _coefs_equal(sncal.jpeg.entropy_decode(data), want), name
        if sc.family(name).startswith('cut'):
            boxes = sc.mcu_boxes(data)
            assert f['starved_mcu'] is not None and f['starved_mcu'] < len(boxes), name
            if name.endswith('.start'):
                assert f['starved_mcu'] == 0, name
            if name.endswith('.last'):
                assert f['starved_mcu'] == len(boxes) - 1, name
        else:
            assert f['starved_mcu'] is None, name


def test_missing_mcus_hold_zero_coefficients(sncal):
    """Behind the MCU in which the data ran out nothing is decoded: no DC prediction is carried on, no zero-bit symbols are read."""
    for name in sc.names():
        if not sc.family(name).startswith('cut'):
            continue
        data = sc.stream(name)
        f = oj.parse(data)
        oj.decode_coefficients(f)
        comps = f['comps']
        mcus_x = -(-f['width'] // (8 * comps[0]['h']))
        for cf, c in zip(sncal.jpeg.entropy_decode(data), comps):
            by, bx = np.mgrid[0:cf.shape[0], 0:cf.shape[1]]
            mcu = (by // c['v']) * mcus_x + bx // c['h']
            assert not cf[mcu > f['starved_mcu']].any(), name


def test_a_stream_without_eoi_decodes_as_the_same_bytes_plus_eoi(sncal):
    """jdatasrc.c fill_input_buffer inserts FF D9 when the data ends; Pillow cannot show it (its source suspends instead)."""
    n = 0
    for name in sc.names():
        if not sc.family(name).startswith('cut'):
            continue
        data = sc.stream(name)
        bare = data[:-2]
        want = oj.decode_coefficients(oj.parse(data))
        assert _coefs_equal(oj.decode_coefficients(oj.parse(bare)), want), name
        assert _coefs_equal(sncal.jpeg.entropy_decode(bare), want), name
        n += 1
    assert n == 128
    for name in ('tables.opt_444_48x64', 'restarts.every_mcu_420_48x64', 'fill.every_row_422_29x37'):       # a whole scan that lost its EOI
        data = sc.stream(name)
        want = oj.decode_coefficients(oj.parse(data))
        for bare in (data[:-2], data[:-1]):
            assert _coefs_equal(sncal.jpeg.entropy_decode(bare), want) and _coefs_equal(oj.decode_coefficients(oj.parse(bare)), want), name


def test_fill_bytes_decode_as_the_unpadded_stream(sncal):
    for name, src in (('fill.every_mcu_420_48x64', 'restarts.every_mcu_420_48x64'), ('fill.every_row_422_29x37', 'restarts.every_row_422_29x37')):
        assert np.array_equal(sc.frame(name), sc.frame(src))
        want = sncal.jpeg.entropy_decode(sc.stream(src))
        assert _coefs_equal(sncal.jpeg.entropy_decode(sc.stream(name)), want)
        longer = sc.stream(name).replace(b'\xff\xff\xd3', b'\xff' * 9 + b'\xd3')      # any number of fill bytes
        assert _coefs_equal(sncal.jpeg.entropy_decode(longer), want) and _coefs_equal(oj.decode_coefficients(oj.parse(longer)), want)


def test_index_overflow_lands_in_position_63_only_on_the_zeros_behind_the_data(sncal):
    """libjpeg does not check the index: jpeg_natural_order has 16 spare entries, all 63.  Here that holds only in the starved MCU; on bits
    the scan really held, an index beyond 63 stays an error."""
    L = sncal._lib
    # DC '0'; three times '0' '1' = run 15, value +1 at zigzag 16, 32, 48; then '0' and the data is over: the value bit is a zero -> -1 at 64
    starved = sc.handmade_grey_8x8(bytes([0b00101010]))
    want = np.zeros(64, np.int16)
    want[oj.ZIGZAG[[16, 32, 48]]] = 1
    want[63] = -1
    for data in (starved, starved[:-2]):
        f = oj.parse(data)
        assert np.array_equal(oj.decode_coefficients(f)[0][0, 0], want) and f['starved_mcu'] == 0
        assert np.array_equal(sncal.jpeg.entropy_decode(data)[0][0, 0], want)
    genuine = sc.handmade_grey_8x8(bytes([0b00101010, 0xFF, 0x00]))                # the fourth value bit is the scan's own
    with pytest.raises(oj.JpegError, match='index out of range'):
        oj.decode_coefficients(oj.parse(genuine))
    with pytest.raises(L.SncalError, match='coefficient index out of range'):
        sncal.jpeg.entropy_decode(genuine)


def test_damage_inside_genuine_data_is_still_refused(sncal):
    L = sncal._lib
    good = sc.stream('restarts.every_mcu_420_48x64')
    at = good.index(b'\xff\xd0')
    assert good[at - 1] != 0xFF
    damaged = {
        'wrong restart number': good[:at] + b'\xff\xd1' + good[at + 2:],
        'restart marker gone': good[:at] + good[at + 2:],
        'another marker in its place': good[:at] + b'\xff\xe0' + good[at + 2:],
        'fill bytes but no marker': good[:at] + b'\xff\xff' + good[at + 2:],
    }
    for what, data in damaged.items():
        with pytest.raises(oj.JpegError, match='restart marker'):
            oj.decode_coefficients(oj.parse(data))
        with pytest.raises(L.SncalError, match='restart marker RST0 missing'):
            sncal.jpeg.entropy_decode(data)
    plain = sc.stream('tables.opt_444_48x64')
    sos = plain.find(b'\xff\xda')
    start = sos + 2 + ((plain[sos + 2] << 8) | plain[sos + 3])
    ones = plain[:start + 40] + b'\xff\x00' * 8 + plain[start + 56:]                 # 64 one-bits: no code of the tables is that long
    with pytest.raises(oj.JpegError, match='bad Huffman code'):
        oj.decode_coefficients(oj.parse(ones))
    with pytest.raises(L.SncalError, match='corrupt Huffman data'):
        sncal.jpeg.entropy_decode(ones)


def test_a_scan_that_ends_where_a_restart_marker_is_due_starves_the_next_interval(sncal):
    """Cut right in front of RSTn, behind its FF, and behind the whole marker: jpeg_resync_to_restart leaves EOI in place, the first MCU of the
    interval is decoded on zero bits (from a reset DC prediction) and the rest is skipped.  The fixture's tool holds these very cuts to
    libjpeg-turbo's frames; here the host stage is held to the oracle."""
    n = 0
    for name in ('restarts.every_mcu_420_48x64', 'restarts.every_row_422_29x37'):
        data = sc.stream(name)
        ri = oj.parse(data)['restart']
        at = [i for i in range(data.find(b'\xff\xda'), len(data) - 2) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
        for k, i in enumerate(at):
            for c in (i, i + 1, i + 2):
                for cut in (data[:c], data[:c] + b'\xff\xd9', data[:c] + b'\xff\xff\xff\xd9'):
                    f = oj.parse(cut)
                    want = oj.decode_coefficients(f)
                    assert f['starved_mcu'] == (k + 1) * ri, (name, k, c - i)
                    assert _coefs_equal(sncal.jpeg.entropy_decode(cut), want), (name, k, c - i)
                    n += 1
    assert n == 9 * (11 + 3)


def test_an_interval_short_of_data_is_skipped_to_its_end_and_the_next_one_decodes(sncal):
    """jdhuff.c process_restart ends insufficient_data at the marker that was due.  Every block outside the damaged interval equals the
    undamaged stream's (the DC prediction starts afresh at a restart marker); inside it, behind the MCU in which the data ran out, all
    is zero.  The fixture's tool holds the oracle's frames of these streams to libjpeg-turbo's."""
    L = sncal._lib
    seen = 0
    for name, (src, cut) in sc.interval_damage().items():
        f = oj.parse(cut)
        if name == 'restarts.every_row_422_29x37.mid3':          # the garbage uses up the interval's bits without running out: refused
            with pytest.raises(oj.JpegError, match='restart marker'):
                oj.decode_coefficients(f)
            with pytest.raises(L.SncalError, match='restart marker RST1 missing'):
                sncal.jpeg.entropy_decode(cut)
            continue
        want = oj.decode_coefficients(f)
        got = sncal.jpeg.entropy_decode(cut)
        assert _coefs_equal(got, want), name
        whole = sncal.jpeg.entropy_decode(sc.stream(src))
        ri, comps = f['restart'], f['comps']
        mcus_x = -(-f['width'] // (8 * comps[0]['h']))
        for cf, wf, c in zip(got, whole, comps):
            by, bx = np.mgrid[0:cf.shape[0], 0:cf.shape[1]]
            mcu = (by // c['v']) * mcus_x + bx // c['h']
            outside = (mcu < ri) | (mcu >= 2 * ri)
            assert np.array_equal(cf[outside], wf[outside]) and wf[mcu >= 2 * ri].any(), name
            if f['starved_mcu'] is not None:
                assert ri <= f['starved_mcu'] < 2 * ri and not cf[(mcu > f['starved_mcu']) & ~outside].any(), name
        if not name.endswith('.mid3'):
            assert f['starved_mcu'] is not None, name
        seen += 1
    assert seen == 7


def test_a_wrong_restart_marker_inside_an_interval_is_refused(sncal):
    data = sc.wrong_marker_inside_an_interval()
    with pytest.raises(oj.JpegError, match='restart marker'):
        oj.decode_coefficients(oj.parse(data))
    with pytest.raises(sncal._lib.SncalError, match='restart marker RST1 missing'):
        sncal.jpeg.entropy_decode(data)
