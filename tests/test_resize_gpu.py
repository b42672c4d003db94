"""GPU: sncal_resize_u8 (cv2.resize's INTER_LINEAR on uint8 BGR frames) byte for byte against the numpy restatement of
tests/resize_ref.py, and strictly less than one level from float64 bilinear, on the shapes of resize_ref.CASES with noise and ramp
inputs; the wide and the byte path against each other; batch independence, determinism and the argument rules."""
import functools

import numpy as np
import pytest
import torch

import resize_ref as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(h, w, H, W, B):
    """{kind: (source, the restatement's result)} of one case, computed once and shared (never written to)."""
    out = {}
    for kind, src in ref.inputs(h, w, B).items():
        want = ref.resize(src, (W, H))
        src.setflags(write=False)
        want.setflags(write=False)
        out[kind] = (src, want)
    return out


@pytest.mark.parametrize('case', ref.CASES, ids=lambda c: '%dx%d-%dx%d' % c[:4])
def test_kernel_equals_the_restatement_and_stays_within_one_level(sncal, cuda, case):
    h, w, H, W, B = case
    for kind, (src, want) in _case(*case).items():
        got = sncal.resize.resize_u8(torch.from_numpy(src.copy()).to(cuda), (W, H))
        assert got.shape == (B, H, W, 3) and got.dtype == torch.uint8 and got.is_contiguous()
        got = got.cpu().numpy()
        assert np.array_equal(got, want), (kind, int((got != want).sum()))
        worst = ref.worst_level(got, src, (W, H))
        print(case, kind, worst)
        assert worst < 1.0, (kind, worst)


@pytest.mark.parametrize('shape', [(33, 61, 32, 64), (64, 96, 32, 48), (360, 640, 540, 960)], ids=lambda s: '%dx%d-%dx%d' % s)
def test_wide_and_byte_paths_write_the_same_bits(sncal, cuda, shape):
    """H * W % 16 == 0 into an aligned destination takes 16-byte stores; the same case from bases one byte off a 16-byte boundary
    (slices of larger buffers) takes the byte path.  Which one ran is not observable."""
    h, w, H, W = shape
    src, want = _case(h, w, H, W, 1)['noise']
    flat = torch.from_numpy(src.copy()).to(cuda).reshape(-1)
    big = torch.zeros(flat.numel() + 1, dtype=torch.uint8, device=cuda)
    big[1:] = flat
    off_src = big[1:].view(1, h, w, 3)
    assert off_src.data_ptr() % 16 == 1 and off_src.is_contiguous()
    dst_big = torch.full((H * W * 3 + 2,), 0xA5, dtype=torch.uint8, device=cuda)
    off_dst = dst_big[1:-1].view(1, H, W, 3)
    assert off_dst.data_ptr() % 16 == 1
    aligned = sncal.resize.resize_u8(flat.view(1, h, w, 3), (W, H))
    assert aligned.data_ptr() % 16 == 0 and np.array_equal(aligned.cpu().numpy(), want)
    assert torch.equal(sncal.resize.resize_u8(off_src, (W, H)), aligned)                     # source off, destination aligned
    sncal.resize.resize_u8(off_src, (W, H), out=off_dst)                                     # both off: byte stores
    assert torch.equal(off_dst, aligned)
    assert int(dst_big[0]) == 0xA5 and int(dst_big[-1]) == 0xA5                              # nothing written beside the destination


def test_sizes_that_rule_out_16_byte_stores_give_the_same_values(sncal, cuda):
    """W = 63: with H = 32 the frame is still whole 16-byte pieces (H * W % 16 == 0: the wide path, its last tile short); with H = 31 it
    is not, and the byte path runs.  Both against the restatement."""
    src = ref.inputs(33, 61, 2)['noise']
    for size in ((63, 32), (63, 31)):
        got = sncal.resize.resize_u8(torch.from_numpy(src).to(cuda), size).cpu().numpy()
        assert np.array_equal(got, ref.resize(src, size)) and ref.worst_level(got, src, size) < 1.0, size
    # the columns of W = 63 and W = 64 differ, the rows do not: same y taps, so a constant-per-row image gives the same rows
    rows = np.repeat(np.arange(33, dtype=np.uint8)[:, None, None] * 7, 61, axis=1).repeat(3, axis=2)[None]
    a = sncal.resize.resize_u8(torch.from_numpy(rows).to(cuda), (63, 32)).cpu().numpy()
    b = sncal.resize.resize_u8(torch.from_numpy(rows).to(cuda), (64, 32)).cpu().numpy()
    assert np.array_equal(a[:, :, :1], b[:, :, :1]) and (a == a[:, :, :1]).all() and (b == b[:, :, :1]).all()


def test_a_frame_of_a_batch_equals_the_frame_alone_and_two_runs_agree(sncal, cuda):
    src = torch.from_numpy(ref.inputs(37, 53, 3)['noise']).to(cuda)
    for size in ((52, 36), (51, 35), (26, 18)):                    # wide path, byte path, and (37, 53) -> (18, 26): no area path
        both = sncal.resize.resize_u8(src, size)
        again = sncal.resize.resize_u8(src, size)
        assert torch.equal(both, again)
        for b in range(3):
            assert torch.equal(sncal.resize.resize_u8(src[b:b + 1].contiguous(), size)[0], both[b]), (size, b)
    area = torch.from_numpy(ref.inputs(64, 96, 3)['ramp']).to(cuda)
    both = sncal.resize.resize_u8(area, (48, 32))
    for b in range(3):
        assert torch.equal(sncal.resize.resize_u8(area[b:b + 1].contiguous(), (48, 32))[0], both[b])


def test_the_last_pixels_of_the_buffer_are_read_inside_it(sncal, cuda):
    """The two taps of a row are read as one 8-byte load where 8 bytes lie inside the source and byte by byte at its end: a source that
    ends exactly at the end of its allocation's used range gives the restatement's values at the last pixels, area path included."""
    for h, w, H, W in ((2, 2, 1, 1), (2, 3, 3, 2), (4, 6, 2, 3), (1, 2, 1, 16), (3, 1, 2, 32)):
        src = ref.inputs(h, w, 2)['noise']
        got = sncal.resize.resize_u8(torch.from_numpy(src).to(cuda), (W, H)).cpu().numpy()
        assert np.array_equal(got, ref.resize(src, (W, H))), (h, w, H, W)


def test_argument_rules(sncal, cuda):
    E = sncal._lib.SncalError
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=cuda)
    # B == 0 is fine and touches nothing
    empty = sncal.resize.resize_u8(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=cuda), (4, 4))
    assert empty.shape == (0, 4, 4, 3)
    assert sncal._lib.lib().sncal_resize_u8(None, 0, 8, 8, None, 4, 4, None) == 0
    # out= is honoured: the result lands in it and it is what comes back
    out = torch.full((2, 4, 4, 3), 9, dtype=torch.uint8, device=cuda)
    x[:] = 200
    assert sncal.resize.resize_u8(x, (4, 4), out=out) is out and int(out.min()) == 200
    for bad_out in (torch.zeros((2, 4, 5, 3), dtype=torch.uint8, device=cuda), torch.zeros((2, 4, 4, 3), dtype=torch.float32, device=cuda),
                    torch.zeros((2, 4, 4, 3), dtype=torch.uint8)):
        with pytest.raises(E):
            sncal.resize.resize_u8(x, (4, 4), out=bad_out)
    # overlap: the destination inside the source's range
    flat = torch.zeros(2 * 8 * 8 * 3 + 2 * 4 * 4 * 3, dtype=torch.uint8, device=cuda)
    src = flat[:2 * 8 * 8 * 3].view(2, 8, 8, 3)
    with pytest.raises(E, match='overlap'):
        sncal.resize.resize_u8(src, (4, 4), out=flat[96:96 + 96].view(2, 4, 4, 3))
    with pytest.raises(E, match='overlap'):
        sncal.resize.resize_u8(src, (8, 8), out=src)                                         # the copy case too
    sncal.resize.resize_u8(src, (4, 4), out=flat[2 * 8 * 8 * 3:].view(2, 4, 4, 3))           # adjacent is not overlapping
    # non-contiguous input, wrong rank, wrong channel count, wrong dtype
    for bad in (x[:, :, ::2], x.permute(0, 2, 1, 3), x[0], torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device=cuda), x.float()):
        with pytest.raises(E):
            sncal.resize.resize_u8(bad, (4, 4))
    with pytest.raises(E):
        sncal.resize.resize_u8(x, (4, 0))
    # the C entry's own checks: a dimension < 1, B past 65535, a frame past 2^31 elements -- refused before any pointer is read
    lib = sncal._lib.lib()
    p, q = x.data_ptr(), out.data_ptr()
    for args in ((p, 2, 0, 8, q, 4, 4), (p, 2, 8, 8, q, 4, -1), (p, 65536, 8, 8, q, 4, 4), (p, -1, 8, 8, q, 4, 4),
                 (p, 1, 32768, 32768, q, 4, 4), (p, 1, 8, 8, q, 32768, 32768), (None, 1, 8, 8, q, 4, 4), (p, 1, 8, 8, None, 4, 4)):
        assert lib.sncal_resize_u8(*args, None) == -1, args


def test_the_copy_case_copies(sncal, cuda):
    src = torch.from_numpy(ref.inputs(64, 96, 2)['noise']).to(cuda)
    got = sncal.resize.resize_u8(src, (96, 64))
    assert torch.equal(got, src) and got.data_ptr() != src.data_ptr()
