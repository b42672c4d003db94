"""JPEG input stage: the `cv2.imread` of /root/reference/src/utils/make_submit.py:62 and
/root/reference/src/utils/export_line_result.py:176, producing the BGR uint8 frames on the GPU.

Host threads do what is bit-serial (markers, Huffman); the device does the inverse DCT, chroma upsampling and
colour conversion exactly as libjpeg-turbo's defaults (what cv2 wraps) compute them.  See csrc/jpeg.hip.

reduce=2 / 4 / 8 is libjpeg's scaled decode, the array `cv2.imread(path, cv2.IMREAD_REDUCED_COLOR_2 / _4 / _8)` returns
(ceil(H / reduce) x ceil(W / reduce), shrunk in the DCT domain, bit-exact).  It is not `cv2.resize` of the full decode.
"""
import ctypes
import operator
from typing import Sequence

import numpy as np
import torch

from . import _lib


def probe(data: bytes) -> dict:
    """Header fields of one JPEG (host only)."""
    info = _lib.JpegInfo()
    _lib.call('sncal_jpeg_probe', data, len(data), ctypes.byref(info))
    return dict(width=info.width, height=info.height, components=info.components, h_samp=info.h_samp,
                v_samp=info.v_samp, restart_interval=info.restart_interval, blocks=list(info.blocks))


def entropy_decode(data: bytes):
    """Quantised coefficient blocks of one JPEG, per component (block_rows, block_cols, 64) int16 in natural
    order (host only; the layout the device kernels consume)."""
    info = probe(data)
    n = sum(info['blocks']) * 64
    buf = np.zeros(n, np.int16)
    ci = _lib.JpegInfo()
    _lib.call('sncal_jpeg_entropy_decode', data, len(data), buf.ctypes.data, n, ctypes.byref(ci))
    hs, vs = info['h_samp'], info['v_samp']
    mx = -(-info['width'] // (8 * hs))
    my = -(-info['height'] // (8 * vs))
    out, off = [], 0
    for c in range(info['components']):
        bh, bw = (my * vs, mx * hs) if c == 0 else (my, mx)
        out.append(buf[off:off + bh * bw * 64].reshape(bh, bw, 64))
        off += bh * bw * 64
    return out


REDUCE = (1, 2, 4, 8)


def check_reduce(reduce) -> int:
    """reduce as an int, or SncalError when it is not a scale libjpeg's reduced decode has."""
    try:
        d = operator.index(reduce)
    except TypeError:
        d = 0
    if d not in REDUCE:
        raise _lib.SncalError(f'reduce={reduce!r}: libjpeg scales by 1, 2, 4 or 8')
    return d


def reduced_size(height: int, width: int, reduce: int):
    """(height, width) of a height x width frame decoded at 1 / reduce (host only): libjpeg rounds up."""
    d = check_reduce(reduce)
    return -(-int(height) // d), -(-int(width) // d)


def scaled_layout(info: dict, reduce: int) -> dict:
    """The plan of a scaled decode for one header (a probe() dict), host only -- the function the decoder itself fills its frame
    descriptors with: {'out_hw': (H, W) of the decoded frame, 'comp_block': side of each component's inverse transform,
    'comp_hw': (height, width) of each component's sample plane, 'comp_up': (vertical, horizontal) upsampling left to do}."""
    ci = _lib.JpegInfo(width=info['width'], height=info['height'], components=info['components'], h_samp=info['h_samp'],
                       v_samp=info['v_samp'], restart_interval=info.get('restart_interval', 0))
    out_hw, block = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 3)()
    hw, up = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 6)()
    _lib.call('sncal_jpeg_scaled_layout', ctypes.byref(ci), check_reduce(reduce), out_hw, block, hw, up)
    n = info['components']
    return dict(out_hw=(out_hw[0], out_hw[1]), comp_block=list(block[:n]), comp_hw=[(hw[2 * c], hw[2 * c + 1]) for c in range(n)],
                comp_up=[(up[2 * c], up[2 * c + 1]) for c in range(n)])


class JpegDecoder:
    """Batched decoder for frames of one size.  decode(list of bytes) -> (B,H,W,3) uint8 BGR CUDA tensor, the
    stacked `cv2.imread` results; feed it to HRNet.forward / CalibrationPipeline.submit directly.  Calls on one
    decoder must use one stream (its device buffers are reused in stream order).

    height, width are the SOURCE size of the frames.  reduce=2 / 4 / 8 decodes them at that fraction, as
    `cv2.imread(path, cv2.IMREAD_REDUCED_COLOR_2 / _4 / _8)` does: decode() then returns (B, out_height, out_width, 3)."""

    def __init__(self, height: int, width: int, max_batch: int = 64, threads: int = 0, device='cuda:0', reduce: int = 1):
        self.device = torch.device(device)
        self.height, self.width, self.max_batch = int(height), int(width), int(max_batch)
        self.reduce = check_reduce(reduce)
        self._h = None
        h = ctypes.c_void_p()
        _lib.call('sncal_jpeg_create_scaled', self.max_batch, self.height, self.width, self.reduce, int(threads), ctypes.byref(h),
                  device=self.device)
        self._h = h
        oh, ow = ctypes.c_int(), ctypes.c_int()
        _lib.call('sncal_jpeg_output_size', self._h, ctypes.byref(oh), ctypes.byref(ow))
        self.out_height, self.out_width = oh.value, ow.value

    def decode(self, frames: Sequence[bytes], out: torch.Tensor = None) -> torch.Tensor:
        B = len(frames)
        if out is None:
            out = torch.empty((B, self.out_height, self.out_width, 3), dtype=torch.uint8, device=self.device)
        _lib.require_device(out, torch.uint8, 'out')
        if tuple(out.shape) != (B, self.out_height, self.out_width, 3):
            raise _lib.SncalError(f'out must be ({B},{self.out_height},{self.out_width},3)')
        ptrs = (ctypes.c_char_p * max(B, 1))(*[bytes(f) for f in frames])
        lens = (ctypes.c_size_t * max(B, 1))(*[len(f) for f in frames])
        _lib.launch('sncal_jpeg_decode', self.device, self._h, ptrs, lens, B, out)
        return out

    def decode_files(self, paths: Sequence[str], out: torch.Tensor = None) -> torch.Tensor:
        blobs = []
        for p in paths:
            with open(p, 'rb') as f:
                blobs.append(f.read())
        return self.decode(blobs, out)

    def close(self):
        if self._h:
            _lib.lib().sncal_jpeg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
