"""GPU: JpegDecoder on streams that are cut short, padded or otherwise unlike the well-formed goldens (tests/golden/jpeg_streams.npz,
tools/make_golden_jpeg_streams.py; tests/jpeg_streams_cases.py), bit for bit.  The host stage hands jpeg_idct_kernel coefficient
magnitudes (quantisation tables of 1 and of 255 on noise), 16-bit tables and all-zero block runs (the MCUs a cut scan never reached)
that tests/golden/jpeg_cases.npz does not contain.  tests/test_jpeg_streams_host.py holds the oracle to libjpeg-turbo on the same cases."""
import numpy as np
import pytest

import jpeg_reduced_ref as rr
import jpeg_streams_cases as sc
from oracle import jpeg as oj

pytestmark = pytest.mark.gpu


def _group(h, w):
    return [n for n in sc.names() if sc.frame(n).shape[:2] == (h, w)]


@pytest.fixture(scope='module')
def decoded(sncal, cuda):
    """{(h, w): (names, (B, h, w, 3) uint8)}: every case of one frame size in ONE launch, which so mixes intact, cut, padded, grey and
    16-bit-table frames of every sampling layout."""
    out = {}
    for h, w in sc.SIZES:
        group = _group(h, w)
        dec = sncal.JpegDecoder(h, w, max_batch=len(group), threads=4, device=cuda)
        out[(h, w)] = (group, dec.decode([sc.stream(n) for n in group]).cpu().numpy())
        dec.close()
    return out


@pytest.fixture(scope='module')
def oracle_frames():
    return {n: oj.decode_bgr(sc.stream(n)) for n in sc.names()}


def test_every_case_is_in_a_batch(decoded):
    assert sorted(n for names, _ in decoded.values() for n in names) == sorted(sc.names())
    for (h, w), (names, _) in decoded.items():
        fams = {sc.family(n) for n in names}
        assert {'cut_exact', 'cut_masked'} & fams and fams - {'cut_exact', 'cut_masked'}, (h, w)          # cut and whole frames side by side
        assert len({oj.parse(sc.stream(n))['comps'][0]['h'] * 10 + len(oj.parse(sc.stream(n))['comps']) for n in names}) >= 2, (h, w)


@pytest.mark.parametrize('size', sc.SIZES, ids=lambda s: '%dx%d' % s)
def test_decoded_frames_equal_the_oracles(decoded, oracle_frames, size):
    """Every pixel of every case, the starved MCUs included: the kernels and the oracle restate one arithmetic."""
    names, got = decoded[size]
    bad = [n for i, n in enumerate(names) if not np.array_equal(got[i], oracle_frames[n])]
    assert not bad, bad


@pytest.mark.parametrize('size', sc.SIZES, ids=lambda s: '%dx%d' % s)
def test_decoded_frames_equal_libjpeg_turbo(decoded, size):
    """Every pixel, the starved MCUs and the masks of cut_masked included: there the samples leave the range of jdmaster.c's clamp table,
    libjpeg-turbo's SIMD inverse DCT saturates, and so does jpeg_idct_kernel."""
    names, got = decoded[size]
    bad = []
    for i, n in enumerate(names):
        diff = (got[i] != sc.frame(n)).any(-1)
        if diff.any():
            bad.append((n, int(diff.sum()), int(np.abs(got[i].astype(int) - sc.frame(n))[diff].max())))
    assert not bad, bad


def test_missing_mcus_are_grey_and_hold_nothing_of_the_batch_before(sncal, cuda, oracle_frames):
    """Both staging slots of a decoder are filled with whole frames; cut frames of the same size then go through the same decoder.  The MCUs
    their scans never reached must be flat grey: the coefficients of the frame that used the slot before are not left standing."""
    whole = ['tables.opt_444_48x64', 'restarts.every_mcu_420_48x64', 'fill.every_mcu_420_48x64', 'restarts.every_mcu_420_48x64']
    cuts = ['cut_exact.48x64_420_q95_r0.' + c for c in ('start', 'start1', 'half', 'seed0')]
    dec = sncal.JpegDecoder(48, 64, max_batch=4, threads=2, device=cuda)
    for _ in range(3):                                               # slots 0, 1, 0
        out = dec.decode([sc.stream(n) for n in whole]).cpu().numpy()
    for i, n in enumerate(whole):
        assert np.array_equal(out[i], oracle_frames[n]), n
        assert not sc.grey_mcus(sc.stream(n), out[i]), n             # nothing grey to begin with
    for rnd in range(2):                                             # slots 1, 0
        out = dec.decode([sc.stream(n) for n in cuts]).cpu().numpy()
        for i, n in enumerate(cuts):
            data = sc.stream(n)
            f = oj.parse(data)
            oj.decode_coefficients(f)
            n_mcu = len(sc.mcu_boxes(data))
            assert sc.grey_mcus(data, out[i]) == list(range(f['starved_mcu'] + 1, n_mcu)) and f['starved_mcu'] + 1 < n_mcu, (n, rnd)
            assert np.array_equal(out[i], oracle_frames[n]) and np.array_equal(out[i], sc.frame(n)), (n, rnd)
    dec.close()


@pytest.mark.parametrize('reduce', (2, 4))
@pytest.mark.parametrize('size', ((48, 64), (29, 37)), ids=lambda s: '%dx%d' % s)
def test_reduced_decode_of_cut_frames_equals_the_restatement(sncal, cuda, size, reduce):
    """reduce=2 / 4 (jidctred.c) on every cut frame of the size: the numpy restatement of libjpeg's scaled decode, fed the ORACLE's
    coefficient blocks."""
    h, w = size
    names = [n for n in _group(h, w) if sc.family(n).startswith('cut')]
    assert len(names) >= 8
    dec = sncal.JpegDecoder(h, w, max_batch=len(names), threads=4, device=cuda, reduce=reduce)
    got = dec.decode([sc.stream(n) for n in names]).cpu().numpy()
    dec.close()
    assert got.shape[1:3] == sncal.jpeg.reduced_size(h, w, reduce)
    for i, n in enumerate(names):
        data = sc.stream(n)
        want = rr.decode_bgr(data, reduce, coefs=oj.decode_coefficients(oj.parse(data)))
        assert np.array_equal(got[i], want), n


@pytest.mark.parametrize('reduce', (1, 2, 4, 8))
def test_flat_blocks_beyond_the_clamp_table_saturate_except_at_one_eighth(sncal, cuda, reduce):
    """Samples 768 beyond the level shift, in a well-formed stream: the 8x8, 4x4 and 2x2 kernels' paths saturate as libjpeg-turbo's SIMD
    transforms do, the 1x1 path indexes jdmaster.c's table as jpeg_idct_1x1 does (tests/jpeg_streams_cases.py handmade_flat_8x8)."""
    dec = sncal.JpegDecoder(8, 8, max_batch=2, threads=1, device=cuda, reduce=reduce)
    got = dec.decode([sc.handmade_flat_8x8(True), sc.handmade_flat_8x8(False)]).cpu().numpy()
    dec.close()
    assert got.shape == (2, 8 // reduce, 8 // reduce, 3)
    assert (got[0] == sc.FLAT_WANT[reduce][0]).all() and (got[1] == sc.FLAT_WANT[reduce][1]).all(), (got[0, 0, 0], got[1, 0, 0])


def test_an_interval_short_of_data_leaves_the_later_intervals_whole(sncal, cuda):
    """tests/jpeg_streams_cases.py interval_damage: only the rest of the damaged interval is grey.  The oracle's frames of these streams
    are held to libjpeg-turbo's by the fixture's tool."""
    cases = {n: v for n, v in sc.interval_damage().items() if n != 'restarts.every_row_422_29x37.mid3'}
    for size in ((48, 64), (29, 37)):
        group = [n for n in cases if n.split('.')[1].endswith('%dx%d' % size)]
        assert len(group) >= 3
        dec = sncal.JpegDecoder(*size, max_batch=len(group), threads=2, device=cuda)
        got = dec.decode([cases[n][1] for n in group]).cpu().numpy()
        dec.close()
        for i, n in enumerate(group):
            assert np.array_equal(got[i], oj.decode_bgr(cases[n][1])), n
            boxes = sc.mcu_boxes(cases[n][1])
            ri = oj.parse(cases[n][1])['restart']
            y0, y1, x0, x1 = boxes[2 * ri]                          # the first MCU behind the damaged interval is the undamaged stream's
            assert np.array_equal(got[i][y0 + 2:y1 - 2, x0 + 2:x1 - 2], sc.frame(cases[n][0])[y0 + 2:y1 - 2, x0 + 2:x1 - 2]), n
