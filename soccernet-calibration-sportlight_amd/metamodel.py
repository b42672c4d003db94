"""Model surface: ``load_model(path, device=...)`` -> object with ``.predict(x)``, ``.val_step(batch)``, ``.nn_module``, ``.device``.

Mirrors argus.load_model + HRNetMetaModel.predict / val_step  (/root/reference/src/models/hrnet/metamodel.py:127-134, :59-86,
checkpoint schema :108-124; callers: /root/reference/src/utils/make_submit.py:51,68 and
/root/reference/src/utils/export_line_result.py:168,181).  pytorch-argus itself is not a dependency: the
checkpoint is the plain ``torch.save`` dict {'model_name', 'params', 'nn_state_dict'}.
"""
import torch

from . import _lib
from .hrnet import HRNetHeatmap, _plain
from .loss import EHMLoss, HRNetLoss, create_keypoint_maps
from .transforms import HRNetPredictionTransform, EHMPredictionTransform


class HRNetMetaModel:
    """Inference-side mirror of the argus Model subclasses (keypoint: HRNetMetaModel, line: EHMMetaModel)."""
    prediction_transform_cls = HRNetPredictionTransform
    loss_cls = HRNetLoss
    # what the model CLASS fixes in code, whatever the yaml says (None = read the yaml): the keypoint network's head and
    # upscale come from its config (src/models/hrnet/hrnet.py:306-330)
    head = None
    upscale = None

    def __init__(self, params: dict, dtype: str = None):
        self.params = params
        dev = params.get('device', 'cuda:0')
        self.device = torch.device(dev[0] if isinstance(dev, (list, tuple)) else dev)
        nn_params = _plain(params['nn_module'])
        self.nn_module = HRNetHeatmap(nn_params['hrnet_config'],
                                      num_refinement_stages=nn_params.get('num_refinement_stages', 0),
                                      num_heatmaps=nn_params.get('num_heatmaps'), dtype=dtype, device=self.device,
                                      head=self.head, upscale=self.upscale)
        pt = _plain(params.get('prediction_transform', {}) or {})
        self.prediction_transform = self.prediction_transform_cls(**pt) if pt else None
        self.loss = None                 # built from params['loss'] by the first val_step(), or set by the caller / load_model(loss=...)

    def predict(self, x: torch.Tensor, check_range: bool = True) -> torch.Tensor:
        """x (B,3,H,W) float32 BGR in [0,1] (any device) -> prediction_transform(net(x)[-1]) on `device`.
        On the split-fp16 engine the range flag of THIS call is read before the result is handed out (SncalRangeError on the
        offending call, never one call late): that waits for the forward, which the reference's only callers do anyway on the next
        line (`.cpu().numpy()`, make_submit.py:68-69, export_line_result.py:181).  check_range=False returns without waiting; the
        caller then owes a check_range() before trusting the results."""
        if self.prediction_transform is None:
            raise _lib.SncalError('predict(): params hold no prediction_transform')
        x = x.to(self.device, non_blocking=True)
        pt = self.prediction_transform
        if isinstance(pt, HRNetPredictionTransform):     # fused: decode straight from the engine
            out = self.nn_module.forward(x, want_heat=False, decode_size=(pt.H, pt.W))[1]
        else:
            out = pt(self.nn_module(x)[-1])
        if check_range:
            self.check_range()
        return out

    def _loss(self):
        """The loss object of val_step: the one the caller set, else HRNetLoss(**params['loss']) (built on first use, so a checkpoint
        whose loss this build does not cover -- refinement stages -- still loads and predicts)."""
        if self.loss is None:
            lp = _plain(self.params.get('loss', None) or {})
            if not lp:
                name = self.loss_cls.__name__
                raise _lib.SncalError(f"val_step(): params hold no 'loss' section; set model.loss = {name}(...) "
                                      f'or pass load_model(..., loss={name}(...))')
            self.loss = self.loss_cls(**lp)
        return self.loss

    def val_step(self, batch: dict, state=None, sync: bool = False) -> dict:
        """metamodel.py:59-86: batch {'image', 'keypoints', 'mask', 'raw_annot', 'img_name'} as the reference's loader collates it
        ('image' (B,3,H,W) float32 BGR in [0,1], or (B,H,W,3) uint8 frames) -> {'prediction' (B,57,3), 'target', 'loss',
        'raw_annots', 'img_name'}.  ONE forward gives the heatmap (for the loss) and the decoded keypoints (want_heat=True with
        decode_size).  'loss' stays a 0-dim device tensor and nothing waits for the GPU unless sync=True, which returns it as a
        float (the reference's loss.item()) and checks the split-fp16 engine's range flag as predict() does; with sync=False the
        caller owes a check_range() before trusting the results.  The batch dict is not modified."""
        if not isinstance(self.prediction_transform, HRNetPredictionTransform):
            raise _lib.SncalError('val_step(): only the keypoint model (HRNetPredictionTransform) has a validation step')
        loss_fn = self._loss()
        image = batch['image'].to(self.device, non_blocking=True)
        keypoints = batch['keypoints'].to(self.device, non_blocking=True)
        mask = batch.get('mask')
        if mask is not None:
            mask = mask.to(self.device, non_blocking=True)
        pt = self.prediction_transform
        heat, prediction = self.nn_module.forward(image.contiguous(), want_heat=True, decode_size=(pt.H, pt.W))
        loss = loss_fn([heat], keypoints, mask)
        if sync:
            self.check_range()
            loss = loss.item()
        return {'prediction': prediction, 'target': keypoints.detach(), 'loss': loss,
                'raw_annots': batch['raw_annot'], 'img_name': batch['img_name']}

    def check_range(self):
        """Raise SncalRangeError if a forward since the last check left the split-fp16 engine's range (HRNetHeatmap.range_status):
        its output was NOT the reference's fp32 result.  Synchronises the current stream.  predict() calls it on its own forward."""
        if self.nn_module.dtype_name == 'fp16x3':
            self.nn_module.range_status(clear=True, check=True)

    def eval(self):
        return self


class EHMMetaModel(HRNetMetaModel):
    """Line model.  Its network ends in a hard-coded Softmax and never upscales (src/models/line/hrnet.py:86-102,
    236-245); the yaml inside a genuine checkpoint (line/model_config/hrnet_w48.yaml) has no 'head' / 'upscale' key."""
    prediction_transform_cls = EHMPredictionTransform
    loss_cls = EHMLoss
    head = 'softmax'
    upscale = 1

    def val_step(self, batch: dict, state=None, sync: bool = False, want_target: bool = False) -> dict:
        """line/metamodel.py:51-71: batch {'image', 'keypoints' (B,138), 'line_para', ['keypoint_maps']} as the reference's loader
        collates it ('image' (B,3,H,W) float32 BGR in [0,1], or (B,H,W,3) uint8 frames) -> {'prediction' (B,23,2,3), 'target',
        'keypoints', 'line_para', 'loss'}.  ONE forward; the loss reads the batch's maps if it carries them, else rebuilds the target
        from the endpoints inside the kernel (EHMLoss target_sigma / stride) and writes none.  'target' is the batch's maps, or
        create_keypoint_maps(...) when want_target, else None.  'loss' stays a 0-dim device tensor and nothing waits for the GPU
        unless sync=True (a float, after the range check of the split-fp16 engine, as in the keypoint val_step); with sync=False the
        caller owes a check_range().  The batch dict is not modified."""
        if self.prediction_transform is None:
            raise _lib.SncalError('val_step(): params hold no prediction_transform')
        loss_fn = self._loss()
        image = batch['image'].to(self.device, non_blocking=True)
        keypoints = batch['keypoints'].to(self.device, non_blocking=True)
        maps = batch.get('keypoint_maps')
        if maps is not None:
            maps = maps.to(self.device, non_blocking=True)
        heat = self.nn_module(image.contiguous())[-1]
        loss = loss_fn([heat], maps if maps is not None else keypoints)
        prediction = self.prediction_transform(heat)
        target = maps
        if target is None and want_target:
            target = create_keypoint_maps(keypoints, loss_fn.target_sigma, loss_fn.stride, tuple(heat.shape[2:]))
        if sync:
            self.check_range()
            loss = loss.item()
        return {'prediction': prediction, 'target': None if target is None else target.detach(), 'keypoints': keypoints.detach(),
                'line_para': batch.get('line_para'), 'loss': loss}


_MODELS = {'HRNetMetaModel': HRNetMetaModel, 'EHMMetaModel': EHMMetaModel}


def load_model(file_path, loss=None, optimizer=None, device='cuda:0', dtype: str = None, **_ignored):
    """argus.load_model(path, loss=None, optimizer=None, device=...) for the two inference models.
    loss: None (default) leaves val_step() to build HRNetLoss from the checkpoint's params['loss']; an HRNetLoss instance (EHMLoss for the line
    model) or a dict of its arguments replaces that.
    dtype: None (default) = 'fp16x3' WITH a fall-back to 'fp32' when the checkpoint's folded weights do not fit the split-fp16 range
    (SNCAL_ERR_RANGE at finalize; a warning names the layer).  'fp16x3' is the fp32-class engine bench.py measures (fp32 tensors, split-fp16 products, fp32 accumulation):
    on 2048 deep-path frames it reproduced the exact engine's keypoint indices on every usable row and its camera on every frame
    (tools/parity_large.py, profiles/r04_parity_large_*), and the reference capture's indices on the W48 golden.  'fp32' is the
    reference's own arithmetic (predict() is fp32, metamodel.py:127-134) on the exact-fp32 MFMA engine, 2.8x slower.  'bf16' / 'fp8'
    are OPT-IN throughput modes: they move 1-3 % of the usable keypoints by one heatmap cell (near-ties of the fp32 heatmap) and
    change the reprojection error by more than 1e-4 on about a third of the frames (tests/test_parity_gpu.py)."""
    try:
        state = torch.load(file_path, map_location='cpu', weights_only=False)
    except ModuleNotFoundError as e:       # checkpoints written under hydra pickle OmegaConf nodes inside params
        raise _lib.SncalError(f'{file_path}: unpickling the checkpoint needs the module {e.name!r} (argus checkpoints of the '
                              'reference hold OmegaConf nodes in params: `pip install omegaconf`)') from e
    params = dict(_plain(state['params']))
    params['device'] = device
    cls = _MODELS.get(state.get('model_name', 'HRNetMetaModel'), HRNetMetaModel)
    model = cls(params, dtype=dtype)
    try:
        model.nn_module.load_state_dict(state['nn_state_dict'])
    except _lib.SncalRangeError as e:
        # the default engine refuses weights that do not fit fp16 hi + lo halves (sncal_hrnet_finalize): the drop-in default must load
        # every checkpoint the reference's fp32 predict() loads, so it falls back to the exact-fp32 engine and says so; an engine the
        # caller asked for by name is not replaced behind their back
        if dtype is not None:
            raise
        import warnings
        warnings.warn(f'{file_path}: {e}; falling back to the exact-fp32 engine (dtype=\'fp32\', about 3x slower)')
        model = cls(params, dtype='fp32')
        model.nn_module.load_state_dict(state['nn_state_dict'])
    if loss is not None:
        model.loss = loss if isinstance(loss, (HRNetLoss, EHMLoss)) else cls.loss_cls(**_plain(loss))
    return model
