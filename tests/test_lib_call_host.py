"""CPU: the one call path of the Python wrappers into libsncal (_lib.call / launch / workspace / pack_parts) -- size queries against
direct ctypes calls, the error text and classes, what each kind of argument is passed as, the 8-byte alignment of packed uploads,
and the header convention launch() rests on: a `void* stream` parameter is always the last one."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUERIES = [('sncal_heatmap_loss_workspace', (2, 57, 8, 12)), ('sncal_line_loss_workspace', (2, 23, 8, 12)),
           ('sncal_augment_workspace', (2, 9, 13)), ('sncal_keypoint_labels_workspace', (2, 31))]


@pytest.mark.parametrize('name,dims', QUERIES, ids=[q[0] for q in QUERIES])
def test_workspace_bytes_equals_the_direct_query(sncal, name, dims):
    L = sncal._lib
    n = ctypes.c_size_t(12345)
    assert getattr(L.lib(), name)(*dims, ctypes.byref(n)) == 0
    assert L.workspace_bytes(name, *dims) == n.value
    empty = ctypes.c_size_t(12345)                          # B = 0 is a valid query everywhere
    assert getattr(L.lib(), name)(0, *dims[1:], ctypes.byref(empty)) == 0
    assert L.workspace_bytes(name, 0, *dims[1:]) == empty.value


def test_workspace_is_a_uint8_tensor_of_at_least_16_bytes(sncal):
    L = sncal._lib
    for name, dims in QUERIES:
        ws = L.workspace(name, *dims, device='cpu')
        assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.numel() == max(L.workspace_bytes(name, *dims), 16)
    assert L.workspace_bytes('sncal_keypoint_labels_workspace', 0, 0) == 0
    ws = L.workspace('sncal_keypoint_labels_workspace', 0, 0, device='cpu')
    assert ws.numel() == 16 and ws.data_ptr() != 0


def test_call_raises_with_the_symbol_name_and_the_library_message(sncal):
    L = sncal._lib
    n = ctypes.c_size_t()
    with pytest.raises(L.SncalError) as e:
        L.call('sncal_heatmap_loss_workspace', -1, 57, 8, 12, ctypes.byref(n))
    assert not isinstance(e.value, L.SncalRangeError)
    last = L.lib().sncal_last_error().decode()
    assert 'B=-1' in last
    assert 'sncal_heatmap_loss_workspace failed with status -1' in str(e.value) and last in str(e.value)
    with pytest.raises(L.SncalError, match='sncal_augment_workspace failed with status -1'):
        L.workspace_bytes('sncal_augment_workspace', 2, -9, 13)
    with pytest.raises(L.SncalError, match='sncal_line_loss_workspace'):
        L.workspace('sncal_line_loss_workspace', 2, 0, 8, 12, device='cpu')
    assert L.call('sncal_heatmap_loss_workspace', 1, 57, 8, 12, ctypes.byref(n)) is None and n.value > 0


def test_status_minus_6_is_a_range_error(sncal, monkeypatch):
    L = sncal._lib
    assert L.ERR_RANGE == -6
    with pytest.raises(L.SncalRangeError, match='sncal_hrnet_finalize failed with status -6'):
        L.check(-6, 'sncal_hrnet_finalize')
    monkeypatch.setattr(L.lib(), 'sncal_stub_range', lambda *a: -6, raising=False)
    with pytest.raises(L.SncalRangeError, match='sncal_stub_range failed with status -6'):
        L.call('sncal_stub_range', 1, None)
    monkeypatch.setattr(L.lib(), 'sncal_stub_other', lambda *a: -2, raising=False)
    with pytest.raises(L.SncalError) as e:
        L.call('sncal_stub_other')
    assert not isinstance(e.value, L.SncalRangeError)


def test_arguments_are_passed_as_documented(sncal, monkeypatch):
    L = sncal._lib
    seen = []
    monkeypatch.setattr(L.lib(), 'sncal_stub_echo', lambda *a: seen.append(a) or 0, raising=False)
    t = torch.arange(6, dtype=torch.float32)
    view = t[2:]                                            # a view's address, not its storage's
    empty = torch.empty((0, 3), dtype=torch.uint8)
    arr = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
    n = ctypes.c_size_t()
    ref = ctypes.byref(n)
    host = np.zeros(4, np.int16)
    args = (t, view, empty, None, 7, 2.5, arr, ref, host.ctypes.data, b'bytes', ctypes.c_void_p(16))
    L.call('sncal_stub_echo', *args)
    got, = seen
    assert len(got) == len(args)
    assert got[0] == t.data_ptr() and type(got[0]) is int and got[0] != 0
    assert got[1] == t.data_ptr() + 8
    assert got[2] == 0                                      # an empty tensor is NULL, as the explicit None of an empty batch was
    assert got[3] is None
    assert got[4] == 7 and type(got[4]) is int and got[5] == 2.5 and type(got[5]) is float
    for i in range(6, len(args)):
        assert got[i] is args[i], i


def test_a_tensor_reaches_the_library_as_its_address(sncal, gold_dir):
    """The real thing once: the JPEG entropy stage writes its coefficients through a CPU tensor handed to call()."""
    L = sncal._lib
    data = np.load(os.path.join(gold_dir, 'jpeg_cases.npz'))['jpg.full'].tobytes()
    want = np.concatenate([c.reshape(-1) for c in sncal.jpeg.entropy_decode(data)])
    buf = torch.full((want.size + 8,), 0x5A5A, dtype=torch.int16)
    info = L.JpegInfo()
    L.call('sncal_jpeg_entropy_decode', data, len(data), buf, want.size, ctypes.byref(info))
    assert np.array_equal(buf.numpy()[:want.size], want) and (buf.numpy()[want.size:] == 0x5A5A).all()
    assert info.width > 0


PARTS = {'f64': np.array([1.5, -2.25, 3e300]), 'i32': np.arange(5, dtype=np.int32) - 2, 'u8': np.arange(7, dtype=np.uint8) + 250,
         'none': np.zeros((0, 2), np.float64)}


@pytest.mark.parametrize('order', [('f64', 'i32', 'u8', 'none'), ('u8', 'none', 'i32', 'f64')], ids=['wide_first', 'narrow_first'])
def test_pack_parts_aligns_every_part_whatever_the_order(sncal, order):
    parts = [PARTS[k] for k in order]
    flat, offsets = sncal._lib.pack_parts(parts)
    assert flat.dtype == np.uint8 and flat.ndim == 1 and len(offsets) == len(parts)
    end = 0
    for p, at in zip(parts, offsets):
        assert at % 8 == 0 and at >= end                   # aligned, and no part lies on the one before it
        assert flat[at:at + p.nbytes].tobytes() == p.tobytes()
        if p.nbytes:
            assert np.array_equal(flat[at:at + p.nbytes].view(p.dtype), p.reshape(-1))     # readable as its own type in place
        end = at + p.nbytes
    assert len(flat) >= end
    assert len(flat) <= sum(-(-p.nbytes // 8) * 8 for p in parts)                           # padding only, nothing else


def test_pack_parts_takes_views_that_are_not_contiguous(sncal):
    a = np.arange(24, dtype=np.int32).reshape(4, 6)[:, ::2]
    flat, (at,) = sncal._lib.pack_parts([a])
    assert at == 0 and np.array_equal(flat[:a.nbytes].view(np.int32).reshape(a.shape), a)


def test_upload_returns_one_address_per_part(sncal):
    """upload() on the host device: the addresses are the tensor's plus pack_parts' offsets, and the bytes are pack_parts'."""
    L = sncal._lib
    parts = [PARTS[k] for k in ('i32', 'f64', 'u8')]
    flat, offsets = L.pack_parts(parts)
    d, ptrs = L.upload(parts, 'cpu')
    assert d.dtype == torch.uint8 and np.array_equal(d.numpy(), flat)
    assert ptrs == [d.data_ptr() + at for at in offsets] and all(p % 8 == 0 for p in ptrs)


def _declarations():
    src = open(os.path.join(ROOT, 'include', 'sncal.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    return {name: [' '.join(p.split()) for p in params.split(',')]
            for name, params in re.findall(r'\b(sncal_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', src)}


def test_a_stream_parameter_is_always_the_last_one(sncal):
    decl = _declarations()
    assert sorted(decl) == sorted(sncal._lib.SIGNATURES)    # the parse sees every function tests/test_abi.py sees
    is_stream = re.compile(r'^void\s*\*\s*stream$')
    with_stream = {n: p for n, p in decl.items() if any(is_stream.match(q) for q in p)}
    assert len(with_stream) >= 30 and 'sncal_hrnet_forward' in with_stream and 'sncal_resize_u8' in with_stream
    for name, params in with_stream.items():
        if name == 'sncal_stream_destroy':                  # its only argument is the handle it destroys
            assert params == ['void* stream']
            continue
        assert [i for i, q in enumerate(params) if is_stream.match(q)] == [len(params) - 1], name
        assert sncal._lib.SIGNATURES[name][1][-1] is ctypes.c_void_p, name
