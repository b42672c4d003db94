"""GPU: the line model's validation surface on the W18 line golden (line_hrnet_w18, 64x96 input, heat 16x24, fp32 engine):
EHMMetaModel.val_step and validate_line() against the parts they are composed of, which have tests of their own
(EHMPredictionTransform: tests/test_decode_gpu.py; EHMLoss, AccMetric: tests/test_line_loss_gpu.py)."""
import os

import numpy as np
import pytest
import torch

import validate_line_ref as vr
from oracle import hrnet_ref as hr

pytestmark = pytest.mark.gpu

LOSS = {'num_refinement_stages': 0, 'gmse_w': 1.0, 'awing_w': 1.0, 'sigma': 4}


@pytest.fixture(scope='module')
def line_model(sncal, cuda, tmp_path_factory, gold_dir):
    g = np.load(os.path.join(gold_dir, 'line_w18_64x96.npz'))
    cfg = hr.load_config('line_hrnet_w18')
    bare = {k: v for k, v in cfg.items() if k not in ('head', 'upscale')}
    sd = hr.seeded_state_dict(cfg, int(g['seed']), float(g['head_gain']))
    ck = {'model_name': 'EHMMetaModel',
          'params': {'nn_module': {'hrnet_config': bare, 'num_refinement_stages': 0, 'num_heatmaps': 23}, 'loss': dict(LOSS),
                     'prediction_transform': {'scale': 4, 'sigma': 6}, 'device': 'cuda:0'},
          'nn_state_dict': sd}
    path = str(tmp_path_factory.mktemp('line') / 'line.pth')
    torch.save(ck, path)
    model = sncal.load_model(path, loss=None, optimizer=None, device='cuda:0', dtype='fp32')
    return model, path, ck, g


def _batches(g, n=3):
    """n batches (the golden's input first) of 64x96 frames with endpoints inside the 96x64 image; the middle one carries maps."""
    rng = np.random.Generator(np.random.PCG64(17))
    B, H, W = int(g['batch']), int(g['hw'][0]), int(g['hw'][1])
    out = []
    for i in range(n):
        b = B if i != 1 else B + 1                                  # step sizes differ: the weighted mean is not the plain one
        kp = np.zeros((b, 23, 2, 3), dtype=np.float32)
        kp[..., :2] = -1
        has = rng.uniform(size=(b, 23)) < 0.5
        pts = np.stack([rng.uniform(0, W, (b, 23, 2)), rng.uniform(0, H, (b, 23, 2))], -1).astype(np.float32)
        kp[..., :2] = np.where(has[..., None, None], pts, -1)
        kp[..., 2] = has[..., None]
        batch = {'image': hr.seeded_input(b, H, W, int(g['seed']) + 1 + i), 'keypoints': torch.from_numpy(kp.reshape(b, -1)),
                 'line_para': torch.full((b, 23, 2), float('nan'), dtype=torch.float64)}
        out.append(batch)
    return out


def test_val_step_returns_the_reference_keys_and_values(sncal, cuda, line_model):
    model, path, ck, g = line_model
    batch = _batches(g)[0]
    keys = sorted(batch)
    out = model.val_step(batch)                                     # raised SncalError before this feature existed
    assert sorted(out) == ['keypoints', 'line_para', 'loss', 'prediction', 'target'] and sorted(batch) == keys
    assert isinstance(model.loss, sncal.EHMLoss) and model.loss.target_sigma == 1 and model.loss.stride == 4
    heat = model.nn_module(batch['image'].to(cuda))[-1]
    assert heat.shape[1:] == (23, 16, 24) and np.abs(heat.cpu().numpy() - g['out']).max() <= 2e-5
    assert out['prediction'].shape == (heat.shape[0], 23, 2, 3)
    assert torch.equal(out['prediction'], sncal.EHMPredictionTransform(scale=4, sigma=6)(heat))
    assert torch.equal(out['prediction'], model.predict(batch['image']))
    want = sncal.EHMLoss(**LOSS)([heat], batch['keypoints'])
    assert out['loss'].is_cuda and out['loss'].dim() == 0 and out['loss'].dtype == torch.float32
    assert torch.equal(out['loss'], want) and torch.isfinite(want) and float(want) > 0
    assert out['target'] is None and torch.equal(out['keypoints'].cpu(), batch['keypoints']) and out['line_para'] is batch['line_para']
    # the fp64 restatement on the same heat: the bound of tests/test_line_loss_gpu.py at its floor (no capture for this heat)
    kp = batch['keypoints'].numpy().reshape(-1, 23, 2, 3)
    h = heat.cpu().numpy()
    v64 = vr.combine(vr.loss_terms64(h, vr.keypoint_maps(kp, 1, 4, (16, 24), as_dataset=True), 4.0), (1.0, 1.0), h.shape)
    assert abs(float(want) - v64) <= (4 * vr.EPS32 + 2.0 ** -24) * abs(v64)
    # maps in the batch and endpoints only: the same loss bits; want_target hands the maps out
    withmaps = model.val_step(batch, want_target=True)
    maps = sncal.loss.create_keypoint_maps(batch['keypoints'].to(cuda), 1, 4, (16, 24))
    assert torch.equal(withmaps['target'], maps) and torch.equal(withmaps['loss'], out['loss'])
    b2 = dict(batch, keypoint_maps=maps.cpu())
    out2 = model.val_step(b2)
    assert torch.equal(out2['loss'], out['loss']) and torch.equal(out2['target'].cpu(), b2['keypoint_maps'])
    # sync=True hands the loss out as a float
    assert model.val_step(batch, sync=True)['loss'] == float(want)
    # a loss handed in replaces the checkpoint's; a checkpoint without a loss section says what to do
    other = sncal.load_model(path, loss={'gmse_w': 0.0, 'sigma': 2, 'target_sigma': 2}, device='cuda:0', dtype='fp32')
    assert isinstance(other.loss, sncal.EHMLoss) and other.loss.terms == 2 and other.loss.target_sigma == 2
    mine = sncal.EHMLoss(awing_w=0.0)
    assert sncal.load_model(path, loss=mine, device='cuda:0', dtype='fp32').loss is mine
    bare = sncal.EHMMetaModel({k: v for k, v in ck['params'].items() if k != 'loss'}, dtype='fp32')
    with pytest.raises(sncal._lib.SncalError, match='EHMLoss'):
        bare.val_step(batch)


def test_validate_line_equals_the_parts_composed_step_by_step(sncal, cuda, line_model):
    model, path, ck, g = line_model
    batches = _batches(g)
    batches[1]['keypoint_maps'] = sncal.loss.create_keypoint_maps(batches[1]['keypoints'].to(cuda), 1, 4, (16, 24)).cpu()
    acc = sncal.AccMetric(num_keypoints=23, conf_threshold=0.01)
    total, frames = 0.0, 0
    for b in batches:
        out = model.val_step(b)
        acc.update(out)
        n = out['prediction'].shape[0]
        total += float(out['loss'].double()) * n
        frames += n
    own = model.loss
    res = sncal.validate.validate_line(model, batches, conf_threshold=0.01)
    assert isinstance(res, sncal.validate.ValidationResult) and sorted(res) == ['val_acc', 'val_loss']
    assert res.frames == frames and res.skipped == [] and model.loss is own
    assert res['val_acc'] == acc.compute() and 0.0 <= res['val_acc'] <= 1.15
    assert abs(res['val_loss'] - total / frames) <= 1e-12 * res['val_loss']
    plain = sum(float(model.val_step(b)['loss']) for b in batches) / len(batches)
    assert abs(res['val_loss'] - plain) > 1e-9                       # weighted by step size, not the plain mean of the steps
    # a loss passed in is used for this call only
    other = sncal.EHMLoss(gmse_w=0.0, awing_w=2.0)
    res2 = sncal.validate.validate_line(model, batches, loss=other, conf_threshold=0.01)
    assert model.loss is own and res2['val_acc'] == res['val_acc'] and res2['val_loss'] != res['val_loss']
    assert sncal.validate.validate_line(model, batches, conf_threshold=0.01) == res


def test_keypoint_model_still_has_its_own_val_step(sncal):
    """The line model's step overrides, it does not replace: the keypoint class keeps the inherited method, and an EHMMetaModel
    no longer reaches it."""
    assert sncal.EHMMetaModel.val_step is not sncal.HRNetMetaModel.val_step
    assert 'want_target' not in sncal.HRNetMetaModel.val_step.__code__.co_varnames


def test_validate_line_over_a_split_folder(sncal, cuda, line_model, gold_dir, tmp_path):
    """960x540 frames from files: unusable annotations are dropped as the reference's dataset drops them, a frame of another size and
    a frame the decoder refuses are skipped and named, 'info' files are ignored; the result equals the steps composed by hand."""
    import json
    model, path, ck, g = line_model
    jpg = np.load(os.path.join(gold_dir, 'jpeg_cases.npz'))
    labels = vr.label_cases(np.load(os.path.join(gold_dir, 'validate_line.npz')))
    usable = [c for c in labels if c['usable']][:4]
    horizontal = labels[-4]
    assert not horizontal['usable']
    files = [('00000', usable[0], 'jpg.full'), ('00001', horizontal, 'jpg.full'), ('00002', usable[1], 'jpg.full'),
             ('00003', usable[2], 'jpg.48x64_420_q95_r0'), ('00004', usable[3], 'jpg.progressive'), ('00005', usable[3], 'jpg.full'),
             ('match_info', usable[0], 'jpg.full')]
    for name, case, key in files:
        with open(tmp_path / f'{name}.json', 'w') as f:
            json.dump({cls: [{'x': x, 'y': y} for x, y in pts] for cls, pts in case['points'].items()}, f)
        with open(tmp_path / f'{name}.jpg', 'wb') as f:
            f.write(jpg[key].tobytes())
    names, labs = sncal.frames.list_line_split(str(tmp_path))
    assert names == ['00000.jpg', '00002.jpg', '00003.jpg', '00004.jpg', '00005.jpg'] and len(labs) == 5
    with pytest.warns(UserWarning, match='skipped'):
        res = sncal.validate.validate_line(model, str(tmp_path), batch_size=2)
    assert res.skipped == ['00003.jpg', '00004.jpg'] and res.frames == 5
    skipped = []
    acc = sncal.AccMetric(num_keypoints=23, conf_threshold=0.2)
    total, frames, seen = 0.0, 0, []
    with pytest.warns(UserWarning, match='skipped'):
        for b in sncal.frames.line_folder_batches(str(tmp_path), 2, cuda, 23, (960, 540), 0, skipped):
            assert b['image'].dtype == torch.uint8 and b['image'].shape[1:] == (540, 960, 3) and b['keypoints'].shape[1:] == (138,)
            out = model.val_step(b)
            acc.update(out)
            total += float(out['loss'].double()) * len(b['img_name'])
            frames += len(b['img_name'])
            seen += b['img_name']
    assert seen == ['00000.jpg', '00002.jpg', '00005.jpg'] and skipped == res.skipped
    assert res['val_acc'] == acc.compute() and abs(res['val_loss'] - total / frames) <= 1e-12 * res['val_loss']
    kp0, _ = sncal.annotations.line_keypoints(labs[0])
    first = next(iter(sncal.frames.line_folder_batches(str(tmp_path), 1, cuda, 23, (960, 540), 0, [])))
    assert np.array_equal(first['keypoints'][0].numpy(), kp0) and first['line_para'].shape == (1, 23, 2)
