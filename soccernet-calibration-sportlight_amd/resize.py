"""Frames of any size: the `cv2.resize(img, (W, H))` of the reference's line dataset (src/models/line/dataset.py:73) and of the
dev-kit (baseline/dataloader.py:62, baseline/detect_extremities.py:237) on the device, between the JPEG stage's uint8 BGR frames
and everything that consumes them.  See csrc/resize.hip and the block in include/sncal.h for the arithmetic (OpenCV 4.7's 8-bit
INTER_LINEAR path, its 2x2 area exception included).

    frames = JpegDecoder(720, 1280).decode(blobs)           # (B,720,1280,3)
    small = resize_u8(frames, (960, 540))                   # (B,540,960,3), cv2.resize(frame, (960, 540)) per frame

What it is pinned to: a numpy restatement of the formulas (tests/resize_ref.py) byte for byte, and float64 bilinear within less
than one level.  OpenCV's own bytes are pinned only once tests/test_resize_cv2_optional.py has run on a machine with a cv2.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def check_size(size, name='resize'):
    """size = (W, H) as cv2 takes it -> (W, H) as ints, or SncalError."""
    try:
        W, H = (int(v) for v in size)
        if (W, H) != tuple(size):
            raise ValueError
    except (TypeError, ValueError):
        raise _lib.SncalError(f'{name}={size!r}: (W, H), two integers, as cv2.resize takes its dsize') from None
    if W < 1 or H < 1:
        raise _lib.SncalError(f'{name}={size!r}: both at least 1')
    return W, H


def add_resize_argument(ap):
    """--resize W H, shared by the validate, submit and baseline_cameras command lines; parsed_resize() reads it back."""
    ap.add_argument('--resize', type=int, nargs=2, default=None, metavar=('W', 'H'),
                    help="bring every frame to W x H after the decode (cv2.resize's bilinear shrink, on the device): frames of any "
                         'size, mixed sizes included, e.g. --resize 960 540 for a 1280x720 folder; composes with --reduce')


def parsed_resize(a):
    """The resize= keyword of a parsed command line: None, or (W, H)."""
    return None if a.resize is None else check_size(tuple(a.resize), '--resize')


def tables(n_src: int, n_dst: int, zero_edges: bool):
    """The taps of one axis (host only, no GPU) -> (ofs (n_dst,) int32, coef (n_dst, 2) int16): the first source index and the two
    weights (of 2048) of every destination index.  zero_edges=True is the x axis rule (an index past either edge is pinned to it
    with weights (2048, 0)), False the y axis rule (the fraction is kept, ofs may be -1, and the two rows are clipped apart)."""
    n_dst = int(n_dst)
    ofs = np.zeros(max(n_dst, 0), np.int32)
    coef = np.zeros((max(n_dst, 0), 2), np.int16)
    _lib.call('sncal_resize_tables', int(n_src), n_dst, int(bool(zero_edges)), ofs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
              coef.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)))
    return ofs, coef


def resize_u8(frames: torch.Tensor, size, out: torch.Tensor = None) -> torch.Tensor:
    """(B,h,w,3) uint8 on the GPU -> (B,H,W,3) uint8, size = (W, H): cv2.resize(frame, size) with its default INTER_LINEAR, per
    frame, one launch on the current stream.  out: the destination, (B,H,W,3) uint8 contiguous on the same device; it may not overlap
    the source.  SncalError off the GPU or on a non-contiguous tensor."""
    W, H = check_size(size, 'size')
    frames = _lib.require_device(frames, torch.uint8, 'frames')
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise _lib.SncalError(f'frames {tuple(frames.shape)} must be (B,h,w,3)')
    B, h, w = frames.shape[:3]
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=frames.device)
    _lib.require_device(out, torch.uint8, 'out')
    if tuple(out.shape) != (B, H, W, 3) or out.device != frames.device:
        raise _lib.SncalError(f'out must be ({B},{H},{W},3) on {frames.device}')
    _lib.launch('sncal_resize_u8', frames.device, frames, B, h, w, out, H, W)         # an empty batch's tensors go as NULL
    return out
