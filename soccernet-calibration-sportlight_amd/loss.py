"""Heatmap targets and the validation loss on the GPU: create_heatmaps / HRNetLoss of
/root/reference/src/models/hrnet/loss.py, same names and arguments.

  create_target / create_heatmaps   loss.py:21-52, 81-87   csrc/target.hip writes the (B,N+1,H,W) target
  HRNetLoss.forward                 loss.py:89-144         csrc/loss.hip: MSE + KLDiv + adaptive wing in one read of the heatmap,
                                                           the target rebuilt on the fly, never written
  its gradient (torch autograd)     loss.py:89-144         csrc/loss.hip: heatmap_loss_grad, one more read and one write

  EHMDataset._generate_keypoint_maps line/dataset.py:107-178   create_keypoint_maps: csrc/line_loss.hip writes the (B,C,h,w) two-peak maps
  EHMLoss.forward                   line/loss.py:34-108        csrc/line_loss.hip: GMSE + adaptive wing in one read of the softmax heatmap;
                                                           the target read from maps, or rebuilt from the endpoints and never written
  its gradient (torch autograd)     line/loss.py:61-108        csrc/line_loss.hip: line_loss_grad, both forms

Both classes are differentiable with respect to the prediction (first derivative only; the target is not differentiated): when
the prediction requires grad, forward runs the sums kernel inside a torch.autograd.Function that saves the prediction, the
keypoints (or maps) and the mask, and backward launches the gradient kernel.  The network's backward pass, a train_step,
optimisers and refinement stages (num_refinement_stages > 0) are out of scope.
"""
import ctypes
from typing import Tuple

import torch
from torch.autograd.function import once_differentiable

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
    _lib.launch('sncal_create_target', kp.device, kp, B, N, float(sigma), h, w, out)
    return out


def create_heatmaps(keypoints: torch.Tensor, sigma: float, pred_size: Tuple[int, int] = (68, 120)) -> torch.Tensor:
    """loss.py:21-52: (B,N,H,W) Gaussian heatmaps.  keypoints (B,N,2) or (B,N,3); visibility is the reference's test
    any(keypoints == 1, dim=-1) over the components given."""
    kp = keypoints
    if kp.shape[-1] == 2:          # no third component: it cannot make a point visible
        kp = torch.cat([kp, torch.zeros_like(kp[..., :1])], dim=-1)
    return create_target(kp, sigma, pred_size)[:, :-1]


TERM_MSE, TERM_KL, TERM_AWING = 1, 2, 4


def _coef(coef, n):
    if len(coef) != n:
        raise _lib.SncalError(f'coef must hold {n} values, got {len(coef)}')
    return (ctypes.c_double * n)(*[float(c) for c in coef])


def _grad_output(grad_output, device):
    """The upstream gradient as the kernels take it: None, or a one-element fp32 tensor on the device."""
    if grad_output is None:
        return None
    if not isinstance(grad_output, torch.Tensor) or grad_output.numel() != 1:
        raise _lib.SncalError('grad_output must be None or a one-element tensor')
    return _lib.require_device(grad_output.detach().to(device, torch.float32).contiguous(), torch.float32, 'grad_output')


def _heatmap_inputs(logp, keypoints, mask):
    """The tensors of heatmap_loss_sums / heatmap_loss_grad, checked -> (logp, keypoints, mask, (B, N+1, h, w))."""
    logp = _lib.require_device(logp, torch.float32, 'pred')
    kp = _lib.require_device(keypoints, torch.float32, 'keypoints')
    if logp.dim() != 4 or kp.dim() != 3 or kp.shape[2] != 3 or kp.shape[0] != logp.shape[0] or kp.shape[1] + 1 != logp.shape[1]:
        raise _lib.SncalError(f'pred {tuple(logp.shape)} must be (B,N+1,h,w) for keypoints {tuple(kp.shape)} = (B,N,3)')
    B, C, h, w = logp.shape
    if mask is not None:
        mask = _lib.require_device(mask, torch.float32, 'mask')
        if tuple(mask.shape) != (B, C):
            raise _lib.SncalError(f'mask {tuple(mask.shape)} must be (B,N+1) = {(B, C)}')
    return logp, kp, mask, (B, C, h, w)


def heatmap_loss_sums(logp: torch.Tensor, keypoints: torch.Tensor, mask, sigma: float, stride: float, terms: int = 3) -> torch.Tensor:
    """sncal_heatmap_loss: logp (B,N+1,h,w) fp32 log-probabilities, keypoints (B,N,3) fp32 in IMAGE pixels, mask (B,N+1) fp32
    or None -> (B,3) fp64 per-frame sums of the MSE, KL and adaptive-wing terms (0 where the term's bit is clear).
    Asynchronous on the current stream."""
    logp, kp, mask, (B, C, h, w) = _heatmap_inputs(logp, keypoints, mask)
    out = torch.zeros((B, 3), dtype=torch.float64, device=logp.device)
    ws = _lib.workspace('sncal_heatmap_loss_workspace', B, C - 1, h, w, device=logp.device)
    _lib.launch('sncal_heatmap_loss', logp.device, logp, kp, mask, B, C - 1, h, w, float(sigma), float(stride), int(terms), out, ws,
                ws.numel())
    return out


def heatmap_loss_grad(logp: torch.Tensor, keypoints: torch.Tensor, mask, sigma: float, stride: float, coef, terms: int = 3,
                      grad_output=None) -> torch.Tensor:
    """sncal_heatmap_loss_grad: the arguments of heatmap_loss_sums, `coef` = (l2_w / n, kldiv_w / B, awing_w / n) with n the
    number of elements, and `grad_output` a one-element fp32 tensor on the device or None (= 1) -> the gradient of
    sum_k coef_k * term_k with respect to logp, fp32, shaped like logp.  Asynchronous on the current stream."""
    logp, kp, mask, (B, C, h, w) = _heatmap_inputs(logp, keypoints, mask)
    cf = _coef(coef, 3)
    gout = _grad_output(grad_output, logp.device)
    grad = torch.empty_like(logp)
    ws = _lib.workspace('sncal_heatmap_loss_workspace', B, C - 1, h, w, device=logp.device)
    _lib.launch('sncal_heatmap_loss_grad', logp.device, logp, kp, mask, B, C - 1, h, w, float(sigma), float(stride), int(terms), cf,
                gout, grad, ws, ws.numel())
    return grad


class _HeatmapLossFn(torch.autograd.Function):
    """HRNetLoss.forward on the autograd tape: the value is _value's (the sums kernel), the backward is heatmap_loss_grad.  What
    is saved: the prediction, the keypoints and the mask -- nothing of the gradient's size."""

    @staticmethod
    def forward(ctx, logp, kp, mask, loss):
        logp = logp.detach().contiguous()
        ctx.save_for_backward(logp, kp, mask)
        ctx.loss_args = (loss.sigma, loss.stride, loss.coef(logp), loss.terms)
        return loss._value(logp, kp, mask)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        logp, kp, mask = ctx.saved_tensors
        sigma, stride, coef, terms = ctx.loss_args
        return heatmap_loss_grad(logp, kp, mask, sigma, stride, coef, terms, grad_output), None, None, None


class HRNetLoss:
    """HRNetLoss (loss.py:55-144) for num_refinement_stages = 0 (anything else raises SncalError), differentiable once with
    respect to the prediction.

    forward(pred, target, mask=None): `pred` is the list the network returns (its only entry (B,N+1,h,w) log-probabilities; a bare
    tensor is taken as that entry), `target` (B, 3*num_keypoints) or (B,N,3) [x, y, flag] in image pixels, `mask` (B,N+1) or None.
    Returns a 0-dim fp32 tensor on the device, with no host synchronisation:
        l2_w * MSELoss(exp(pred), t) + kldiv_w * KLDivLoss(batchmean)(pred, t) + awing_w * adaptive_wing(exp(pred), t)
    Terms whose weight is not > 0 are not computed, as in the reference.  An empty batch (B == 0) gives nan, as torch's means of
    nothing do.  When the prediction requires grad (and grad mode is on) the same value comes back with a grad_fn whose backward
    is the fused gradient kernel; otherwise the value carries no grad_fn.  components() is never differentiable."""

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

    def coef(self, logp) -> Tuple[float, float, float]:
        """Each term's weight over its divisor, as heatmap_loss_grad takes them (0 for a term that is off)."""
        B, n = max(int(logp.shape[0]), 1), float(max(logp.numel(), 1))
        return (self.l2_w / n if self.l2_w > 0.0 else 0.0, self.kldiv_w / B if self.kldiv_w > 0.0 else 0.0,
                self.awing_w / n if self.awing_w > 0.0 else 0.0)

    def forward(self, pred, target, mask=None) -> torch.Tensor:
        logp, kp, mask = self._inputs(pred, target, mask)
        raw = pred[0] if isinstance(pred, (list, tuple)) else pred
        if raw.requires_grad and torch.is_grad_enabled():
            return _HeatmapLossFn.apply(raw, kp, mask, self)
        return self._value(logp, kp, mask)

    def _value(self, logp, kp, mask) -> torch.Tensor:
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


def _endpoints(keypoints, device) -> torch.Tensor:
    """(B, C*6) or (B,C,2,3) [x, y, flag] rows in image pixels -> (B,C,2,3) fp32 contiguous on `device`."""
    kp = keypoints.detach().to(device, torch.float32)
    if kp.dim() == 2 and kp.shape[1] % 6 == 0:
        kp = kp.reshape(kp.shape[0], kp.shape[1] // 6, 2, 3)
    if kp.dim() != 4 or tuple(kp.shape[2:]) != (2, 3):
        raise _lib.SncalError(f'keypoints {tuple(keypoints.shape)} must be (B, C*6) or (B,C,2,3)')
    return kp.contiguous()


def create_keypoint_maps(keypoints: torch.Tensor, sigma: float = 1.0, stride: float = 4.0, size: Tuple[int, int] = (135, 240)) -> torch.Tensor:
    """EHMDataset._generate_keypoint_maps (line/dataset.py:107-178) for a batch: keypoints (B, C*6) or (B,C,2,3) [x, y, flag] in
    image pixels (any device) -> (B,C,h,w) fp32 maps on the GPU, size = (h, w) of the map (the frame's size over the stride).
    Asynchronous on the current stream."""
    if not keypoints.is_cuda:
        raise _lib.SncalError('keypoints must be a tensor on the GPU (libsncal has no CPU path)')
    kp = _endpoints(keypoints, keypoints.device)
    B, C = kp.shape[0], kp.shape[1]
    h, w = int(size[0]), int(size[1])
    out = torch.empty((B, C, h, w), dtype=torch.float32, device=kp.device)
    _lib.launch('sncal_line_target', kp.device, kp, B, C, float(sigma), float(stride), h, w, out)
    return out


TERM_GMSE, TERM_LINE_AWING = 1, 2


def _line_inputs(pred, target, keypoints):
    """The tensors of line_loss_sums / line_loss_grad, checked -> (pred, target, keypoints, (B, C, h, w))."""
    pred = _lib.require_device(pred, torch.float32, 'pred')
    if (target is None) == (keypoints is None):
        raise _lib.SncalError('exactly one of target and keypoints must be given')
    if pred.dim() != 4:
        raise _lib.SncalError(f'pred {tuple(pred.shape)} must be (B,C,h,w)')
    B, C, h, w = pred.shape
    if target is not None:
        target = _lib.require_device(target, torch.float32, 'target')
        if target.shape != pred.shape:
            raise _lib.SncalError(f'target {tuple(target.shape)} must have the shape of pred {tuple(pred.shape)}')
    else:
        keypoints = _lib.require_device(keypoints, torch.float32, 'keypoints')
        if tuple(keypoints.shape) != (B, C, 2, 3):
            raise _lib.SncalError(f'keypoints {tuple(keypoints.shape)} must be (B,C,2,3) = {(B, C, 2, 3)}')
    return pred, target, keypoints, (B, C, h, w)


def line_loss_sums(pred: torch.Tensor, target=None, keypoints=None, target_sigma: float = 1.0, stride: float = 4.0,
                   gmse_sigma: float = 4.0, terms: int = 3) -> torch.Tensor:
    """sncal_line_loss: pred (B,C,h,w) fp32 softmax output; exactly one of target (B,C,h,w) fp32 maps and keypoints (B,C,2,3) fp32
    endpoints in image pixels (the target is then rebuilt, never written) -> (B,2) fp64 per-frame sums of the GMSE and
    adaptive-wing terms (0 where the term's bit is clear).  Asynchronous on the current stream."""
    pred, target, keypoints, (B, C, h, w) = _line_inputs(pred, target, keypoints)
    out = torch.zeros((B, 2), dtype=torch.float64, device=pred.device)
    ws = _lib.workspace('sncal_line_loss_workspace', B, C, h, w, device=pred.device)
    _lib.launch('sncal_line_loss', pred.device, pred, target, keypoints, B, C, h, w, float(target_sigma), float(stride),
                float(gmse_sigma), int(terms), out, ws, ws.numel())
    return out


def line_loss_grad(pred: torch.Tensor, target=None, keypoints=None, target_sigma: float = 1.0, stride: float = 4.0,
                   gmse_sigma: float = 4.0, coef=(0.0, 0.0), terms: int = 3, grad_output=None) -> torch.Tensor:
    """sncal_ehm_loss_grad: the arguments of line_loss_sums, `coef` = (gmse_w / n, awing_w / n) with n the number of elements, and
    `grad_output` a one-element fp32 tensor on the device or None (= 1) -> the gradient of sum_k coef_k * term_k with respect to
    pred, fp32, shaped like pred.  Asynchronous on the current stream."""
    pred, target, keypoints, (B, C, h, w) = _line_inputs(pred, target, keypoints)
    cf = _coef(coef, 2)
    gout = _grad_output(grad_output, pred.device)
    grad = torch.empty_like(pred)
    ws = _lib.workspace('sncal_line_loss_workspace', B, C, h, w, device=pred.device)
    _lib.launch('sncal_ehm_loss_grad', pred.device, pred, target, keypoints, B, C, h, w, float(target_sigma), float(stride),
                float(gmse_sigma), int(terms), cf, gout, grad, ws, ws.numel())
    return grad


class _LineLossFn(torch.autograd.Function):
    """EHMLoss.forward on the autograd tape: the value is _value's (the sums kernel), the backward is line_loss_grad.  What is
    saved: the prediction and the maps or the endpoints -- nothing of the gradient's size."""

    @staticmethod
    def forward(ctx, pred, target, is_maps, loss):
        pred = pred.detach().contiguous()
        ctx.save_for_backward(pred, target)
        n = float(max(pred.numel(), 1))
        ctx.is_maps = is_maps
        ctx.loss_args = dict(target_sigma=loss.target_sigma, stride=loss.stride, gmse_sigma=loss.sigma, terms=loss.terms,
                             coef=(loss.gmse_w / n if loss.gmse_w > 0 else 0.0, loss.awing_w / n if loss.awing_w > 0 else 0.0))
        return loss._value(pred, target, is_maps)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        pred, target = ctx.saved_tensors
        where = dict(target=target) if ctx.is_maps else dict(keypoints=target)
        return line_loss_grad(pred, grad_output=grad_output, **where, **ctx.loss_args), None, None, None


class EHMLoss:
    """EHMLoss (line/loss.py:5-108) for num_refinement_stages = 0 (anything else raises SncalError; the default here is 0 where the
    reference's is 1, because 0 is what is built and what train_config.yaml sets), differentiable once with respect to the
    prediction.

    forward(pred, target): `pred` is the list the network returns (its entry 0, (B,C,h,w) softmax output, is used; a bare tensor is
    taken as that entry).  A 4-D `target` holds maps (batch['keypoint_maps']); a (B, C*6) or (B,C,2,3) `target` holds the
    endpoints (batch['keypoints'], image pixels) and the maps are rebuilt on the fly with `target_sigma` and `stride` -- this
    build's additions, defaults = data_params of line/train_config.yaml.  Returns a 0-dim fp32 tensor on the device, with no host
    synchronisation:  gmse_w * mean(d^2 exp(-d^2 / (2 sigma^2))) + awing_w * mean(adaptive_wing(pred, target)).
    Terms whose weight is not > 0 are not computed, as in the reference.  B == 0 gives nan, as torch's means of nothing do.
    When the prediction requires grad (and grad mode is on) the same value comes back with a grad_fn whose backward is the fused
    gradient kernel; otherwise the value carries no grad_fn.  components() is never differentiable."""

    def __init__(self, num_refinement_stages: int = 0, gmse_w: float = 1.0, awing_w: float = 1.0, sigma: float = 4,
                 target_sigma: float = 1, stride: float = 4):
        if int(num_refinement_stages) != 0:
            raise _lib.SncalError(f'EHMLoss: num_refinement_stages = {num_refinement_stages}; only 0 (one heatmap) is built')
        self.n_losses = 1
        self.gmse_w, self.awing_w = gmse_w, awing_w
        self.sigma = sigma
        self.target_sigma, self.stride = target_sigma, stride

    @property
    def terms(self) -> int:
        return (TERM_GMSE if self.gmse_w > 0 else 0) | (TERM_LINE_AWING if self.awing_w > 0 else 0)

    def create_keypoint_maps(self, keypoints: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
        return create_keypoint_maps(keypoints, self.target_sigma, self.stride, size)

    def _inputs(self, pred_list, target):
        """-> (pred detached and contiguous, maps or endpoints on its device, whether those are maps)"""
        pred = pred_list[0] if isinstance(pred_list, (list, tuple)) else pred_list
        if not isinstance(pred, torch.Tensor) or pred.dim() != 4:
            raise _lib.SncalError(f'EHMLoss: pred {tuple(getattr(pred, "shape", ()))} must be (B,C,h,w)')
        pred = pred.detach().contiguous()
        # 4-D means maps; (B,C,2,3) means endpoints unless the heatmap itself is 2 x 3
        if target.dim() == 4 and (tuple(target.shape[2:]) != (2, 3) or tuple(pred.shape[2:]) == (2, 3)):
            return pred, target.detach().to(pred.device, torch.float32).contiguous(), True
        return pred, _endpoints(target, pred.device), False

    def _sums(self, pred, target, is_maps) -> torch.Tensor:
        if is_maps:
            return line_loss_sums(pred, target=target, gmse_sigma=self.sigma, terms=self.terms)
        return line_loss_sums(pred, keypoints=target, target_sigma=self.target_sigma, stride=self.stride, gmse_sigma=self.sigma,
                              terms=self.terms)

    def components(self, pred_list, target) -> torch.Tensor:
        """(B,2) fp64 on the device: per-frame sums over C*h*w of the GMSE and adaptive-wing terms (only those with a weight > 0;
        the others are 0)."""
        return self._sums(*self._inputs(pred_list, target))

    def forward(self, pred_list, target) -> torch.Tensor:
        pred, target, is_maps = self._inputs(pred_list, target)
        raw = pred_list[0] if isinstance(pred_list, (list, tuple)) else pred_list
        if raw.requires_grad and torch.is_grad_enabled():
            return _LineLossFn.apply(raw, target, is_maps, self)
        return self._value(pred, target, is_maps)

    def _value(self, pred, target, is_maps) -> torch.Tensor:
        s = self._sums(pred, target, is_maps).sum(dim=0)
        n = float(pred.numel())
        loss = torch.zeros((), dtype=torch.float64, device=pred.device)
        if self.gmse_w > 0:
            loss = loss + self.gmse_w * (s[0] / n)
        if self.awing_w > 0:
            loss = loss + self.awing_w * (s[1] / n)
        return loss.to(torch.float32)

    __call__ = forward
