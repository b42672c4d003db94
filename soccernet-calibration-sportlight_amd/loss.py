"""Heatmap targets and the validation loss on the GPU: create_heatmaps / HRNetLoss of
/root/reference/src/models/hrnet/loss.py, same names and arguments.

  create_target / create_heatmaps   loss.py:21-52, 81-87   csrc/target.hip writes the (B,N+1,H,W) target
  HRNetLoss.forward                 loss.py:89-144         csrc/loss.hip: MSE + KLDiv + adaptive wing in one read of the heatmap,
                                                           the target rebuilt on the fly, never written

Forward values only: the backward pass (training) and refinement stages (num_refinement_stages > 0) are out of scope.
"""
import ctypes
from typing import Tuple

import torch

from . import _lib


def create_target(keypoints: torch.Tensor, sigma: float, pred_size: Tuple[int, int] = (68, 120)) -> torch.Tensor:
    """HRNetLoss.create_target (loss.py:81-87): keypoints (B,N,3) [x, y, visibility] in heatmap pixels ->
    (B,N+1,H,W) fp32 heatmaps, last channel = 1 - max over the keypoint channels."""
    kp = _lib.require_device(keypoints.contiguous(), torch.float32, 'keypoints')
    if kp.dim() != 3 or kp.shape[2] != 3:
        raise _lib.SncalError('keypoints must be (B,N,3)')
    B, N = kp.shape[0], kp.shape[1]
    h, w = int(pred_size[0]), int(pred_size[1])
    out = torch.empty((B, N + 1, h, w), dtype=torch.float32, device=kp.device)
    with torch.cuda.device(kp.device):
        _lib.check(_lib.lib().sncal_create_target(kp.data_ptr(), B, N, float(sigma), h, w, out.data_ptr(),
                                                  _lib.current_stream_ptr()), 'sncal_create_target')
    return out


def create_heatmaps(keypoints: torch.Tensor, sigma: float, pred_size: Tuple[int, int] = (68, 120)) -> torch.Tensor:
    """loss.py:21-52: (B,N,H,W) Gaussian heatmaps.  keypoints (B,N,2) or (B,N,3); visibility is the reference's test
    any(keypoints == 1, dim=-1) over the components given."""
    kp = keypoints
    if kp.shape[-1] == 2:          # no third component: it cannot make a point visible
        kp = torch.cat([kp, torch.zeros_like(kp[..., :1])], dim=-1)
    return create_target(kp, sigma, pred_size)[:, :-1]


TERM_MSE, TERM_KL, TERM_AWING = 1, 2, 4


def heatmap_loss_sums(logp: torch.Tensor, keypoints: torch.Tensor, mask, sigma: float, stride: float, terms: int = 3) -> torch.Tensor:
    """sncal_heatmap_loss: logp (B,N+1,h,w) fp32 log-probabilities, keypoints (B,N,3) fp32 in IMAGE pixels, mask (B,N+1) fp32
    or None -> (B,3) fp64 per-frame sums of the MSE, KL and adaptive-wing terms (0 where the term's bit is clear).
    Asynchronous on the current stream."""
    logp = _lib.require_device(logp, torch.float32, 'pred')
    kp = _lib.require_device(keypoints, torch.float32, 'keypoints')
    if logp.dim() != 4 or kp.dim() != 3 or kp.shape[2] != 3 or kp.shape[0] != logp.shape[0] or kp.shape[1] + 1 != logp.shape[1]:
        raise _lib.SncalError(f'pred {tuple(logp.shape)} must be (B,N+1,h,w) for keypoints {tuple(kp.shape)} = (B,N,3)')
    B, C, h, w = logp.shape
    if mask is not None:
        mask = _lib.require_device(mask, torch.float32, 'mask')
        if tuple(mask.shape) != (B, C):
            raise _lib.SncalError(f'mask {tuple(mask.shape)} must be (B,N+1) = {(B, C)}')
    out = torch.zeros((B, 3), dtype=torch.float64, device=logp.device)
    n = ctypes.c_size_t()
    _lib.check(_lib.lib().sncal_heatmap_loss_workspace(B, C - 1, h, w, ctypes.byref(n)), 'sncal_heatmap_loss_workspace')
    with torch.cuda.device(logp.device):
        ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=logp.device)
        _lib.check(_lib.lib().sncal_heatmap_loss(logp.data_ptr(), kp.data_ptr(), mask.data_ptr() if mask is not None else None,
                                                 B, C - 1, h, w, float(sigma), float(stride), int(terms), out.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()), 'sncal_heatmap_loss')
    return out


class HRNetLoss:
    """HRNetLoss (loss.py:55-144), forward value only, for num_refinement_stages = 0 (anything else raises SncalError).

    forward(pred, target, mask=None): `pred` is the list the network returns (its only entry (B,N+1,h,w) log-probabilities; a bare
    tensor is taken as that entry), `target` (B, 3*num_keypoints) or (B,N,3) [x, y, flag] in image pixels, `mask` (B,N+1) or None.
    Returns a 0-dim fp32 tensor on the device, with no host synchronisation:
        l2_w * MSELoss(exp(pred), t) + kldiv_w * KLDivLoss(batchmean)(pred, t) + awing_w * adaptive_wing(exp(pred), t)
    Terms whose weight is not > 0 are not computed, as in the reference.  An empty batch (B == 0) gives nan, as torch's means of
    nothing do."""

    def __init__(self, num_refinement_stages: int = 0, sigma: float = 1.0, stride: int = 1, pred_size: Tuple[int, int] = (540, 960),
                 num_keypoints: int = 57, l2_w: float = 1.0, kldiv_w: float = 1.0, awing_w: float = 0.0):
        if int(num_refinement_stages) != 0:
            raise _lib.SncalError(f'HRNetLoss: num_refinement_stages = {num_refinement_stages}; only 0 (one heatmap) is built')
        self.sigma = sigma
        self.stride = stride
        self.pred_size = tuple(int(v) for v in pred_size)
        self.num_keypoints = int(num_keypoints)
        self.n_losses = 1
        self.l2_w, self.kldiv_w, self.awing_w = l2_w, kldiv_w, awing_w

    @property
    def terms(self) -> int:
        return (TERM_MSE if self.l2_w > 0.0 else 0) | (TERM_KL if self.kldiv_w > 0.0 else 0) | (TERM_AWING if self.awing_w > 0.0 else 0)

    def create_target(self, keypoints: torch.Tensor) -> torch.Tensor:
        """loss.py:81-87; keypoints (B,N,3) already in heatmap pixels."""
        return create_target(keypoints, self.sigma, self.pred_size)

    def _inputs(self, pred, target, mask):
        logp = pred[0] if isinstance(pred, (list, tuple)) else pred
        if isinstance(pred, (list, tuple)) and len(pred) != self.n_losses:
            raise _lib.SncalError(f'HRNetLoss: pred holds {len(pred)} heatmaps, expected {self.n_losses}')
        if not isinstance(logp, torch.Tensor) or logp.dim() != 4 or tuple(logp.shape[2:]) != self.pred_size:
            raise _lib.SncalError(f'HRNetLoss: pred {tuple(getattr(logp, "shape", ()))} does not end in pred_size {self.pred_size}')
        kp = target.detach().to(logp.device, torch.float32).reshape(-1, self.num_keypoints, 3).contiguous()
        if mask is not None:
            mask = mask.detach().to(logp.device, torch.float32).contiguous()
        return logp.detach().contiguous(), kp, mask

    def components(self, pred, target, mask=None) -> torch.Tensor:
        """(B,3) fp64 on the device: per-frame sums over (N+1)*h*w of the MSE, KL and adaptive-wing terms (only those with a
        weight > 0; the others are 0)."""
        logp, kp, mask = self._inputs(pred, target, mask)
        return heatmap_loss_sums(logp, kp, mask, self.sigma, self.stride, self.terms)

    def forward(self, pred, target, mask=None) -> torch.Tensor:
        logp, kp, mask = self._inputs(pred, target, mask)
        s = heatmap_loss_sums(logp, kp, mask, self.sigma, self.stride, self.terms).sum(dim=0)
        B = logp.shape[0]
        n = float(logp.numel())
        loss = torch.zeros((), dtype=torch.float64, device=logp.device)
        if self.l2_w > 0.0:
            loss = loss + self.l2_w * (s[0] / n)                  # nn.MSELoss(): mean over every element
        if self.kldiv_w > 0.0:
            loss = loss + self.kldiv_w * (s[1] / float(B))        # nn.KLDivLoss(reduction='batchmean')
        if self.awing_w > 0.0:
            loss = loss + self.awing_w * (s[2] / n)               # torch.mean
        return loss.to(torch.float32)

    __call__ = forward
