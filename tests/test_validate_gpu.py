"""GPU: the validation metrics on the device and validate() end to end.

L2metric and EvalAImetric against the reference capture (tests/golden/validate.npz); validate() against the same metrics composed
step by step from parts that have tests of their own (predict -> solve_device -> CameraEvaluator.evaluate -> the fp64 aggregation
of tests/validate_ref.py).  Counts must be identical, so ratios of counts are equal; a float sum of n terms taken in another order
is within n * 2^-24 relative."""
import json
import os
import types

import numpy as np
import pytest
import torch

import validate_ref as vr
from oracle import hrnet_ref as hr
from test_evaluate_gpu import _records
from test_validate_host import _check_l2, _l2_updates, check_evalai, evalai_frames

pytestmark = pytest.mark.gpu

KW = dict(conf_thresh=0.5, conf_threshs=[0.5, 0.35, 0.2], algorithm='iterative_voter', max_rmse=55.0, max_rmse_rel=5.0,
          min_points=5, min_focal_length=10.0, min_points_per_plane=6, min_points_for_refinement=6, reliable_thresh=57)
LOSS = {'num_refinement_stages': 0, 'stride': 2, 'sigma': 2.0, 'pred_size': [270, 480], 'num_keypoints': 57}


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'validate.npz'))


def test_l2metric_on_the_device_matches_reference_capture(sncal, cuda, gold):
    m = sncal.L2metric(num_keypoints=57, conf_threshold=0.5, pckhs_thres=[float(t) for t in gold['l2.thres']])
    for p, t in _l2_updates(gold):
        m.update({'prediction': torch.from_numpy(p).to(cuda), 'target': torch.from_numpy(t).to(cuda)})
    assert m._acc.is_cuda and m._last.is_cuda                              # accumulators stay on the device
    state = types.SimpleNamespace(phase='val', metrics={})
    m.epoch_complete(state)
    _check_l2(state.metrics, gold)
    assert all(isinstance(v, float) for v in state.metrics.values())


def test_evalai_metric_matches_reference_capture(sncal, cuda, gold, gold_dir):
    """The capture's cameras as solved records, three updates of 4, 4 and 2 frames, two frames without a camera."""
    frames, per_frame = evalai_frames(gold, gold_dir)
    m = sncal.EvalAImetric(sncal.CameraCreator(sncal.PITCH_POINTS, **KW), threshold=5, img_size=(960, 540))
    assert m.compute() == 0.0
    for lo, hi in gold['evalai.batches']:
        sel = [None if per_frame[i] is None else frames[i] for i in range(lo, hi)]
        m.update_records(_records(sncal, sel, cuda), [frames[i]['gt'] for i in range(lo, hi)])
    assert m._acc.is_cuda and m.total_frames == 10
    state = types.SimpleNamespace(phase='val', metrics={})
    m.epoch_complete(state)
    check_evalai(state.metrics, gold, reproj_tol=1e-9)                     # the device's distances: 1e-9 relative (tests/test_evaluate_gpu.py)
    assert abs(m.compute() - 0.8) < 1e-15
    m.add_missed(2)                                                        # frames that never reached the network
    assert abs(m.compute() - 8 / 12) < 1e-15


def _stamped_frame(sncal, cam, rng, sigma_cells=2.0):
    """One 540x960 frame carrying the keypoint stamps of `cam` (the construction of synth.stamped_frames for a given camera), so
    that frame and annotation can come from ONE camera."""
    from sncal_amd.pitch import PITCH_ARRAY
    codes = sncal.synth.stamp_codes()
    H, W, hc, wc = 540, 960, 270, 480
    frame = 0.25 + 0.5 * rng.random((3, H, W), dtype=np.float32)
    R = int(np.ceil(2.4 * sigma_cells))
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    env0 = np.exp(-(dy * dy + dx * dx) / (2.0 * sigma_cells ** 2)).astype(np.float32)
    q = cam.project_points(PITCH_ARRAY)
    vis = (q[:, 2] != 0) & (q[:, 0] >= 0) & (q[:, 0] < 960) & (q[:, 1] >= 0) & (q[:, 1] < 540)
    owner = np.zeros((hc, wc), dtype=np.float32)
    cells = frame.reshape(3, hc, 2, wc, 2)
    for k in np.nonzero(vis)[0]:
        cj = int(min(max(round(q[k, 0] * wc / 960.0), 0), wc - 1))
        ci = int(min(max(round(q[k, 1] * hc / 540.0), 0), hc - 1))
        i0, i1, j0, j1 = max(ci - R, 0), min(ci + R, hc - 1), max(cj - R, 0), min(cj + R, wc - 1)
        env = env0[i0 - ci + R:i1 - ci + R + 1, j0 - cj + R:j1 - cj + R + 1]
        take = env > owner[i0:i1 + 1, j0:j1 + 1]
        owner[i0:i1 + 1, j0:j1 + 1] = np.where(take, env, owner[i0:i1 + 1, j0:j1 + 1])
        stamp = 0.5 + 0.5 * env[None, :, None, :, None] * codes[k][:, None, :, None, :]
        blk = cells[:, i0:i1 + 1, :, j0:j1 + 1, :]
        blk[...] = np.where(take[None, :, None, :, None], stamp, blk)
    return frame


def _as_dicts(annot):
    return {c: [{'x': float(x), 'y': float(y)} for x, y in pts] for c, pts in annot.items()}


def _dataset(sncal, n=11):
    """n frames + SoccerNet-style annotations: frames 0..5 show the camera their annotation was drawn from, 6 is noise only (no
    camera can be found), the rest are synth.stamped_frames images under an unrelated annotation."""
    rng = np.random.Generator(np.random.PCG64(2024))
    other, _ = sncal.synth.stamped_frames(n, seed=31)
    images, annots = [], []
    seeds = [103, 104, 107, 108, 109, 110, 100, 101, 105, 106, 102]          # the first six: cameras that see 12 keypoints or more
    for i in range(n):
        annot, cam = sncal.synth.synthetic_annotation(seed=seeds[i])
        annots.append(_as_dicts(annot))
        if i < 6:
            images.append(_stamped_frame(sncal, cam, rng))
        elif i == 6:
            images.append(0.25 + 0.5 * rng.random((3, 540, 960), dtype=np.float32))
        else:
            images.append(other[i])
    return np.stack(images), annots


def _batches(sncal, images, annots, names, size):
    out = []
    for i in range(0, len(images), size):
        pairs = [sncal.frames.annot_to_keypoints(a, 57, margin=LOSS['sigma']) for a in annots[i:i + size]]
        out.append({'image': torch.from_numpy(images[i:i + size]), 'keypoints': torch.from_numpy(np.stack([p[0] for p in pairs])),
                    'mask': torch.from_numpy(np.stack([p[1] for p in pairs])),
                    'raw_annot': [sncal.evaluate.scale_points(a, 960, 540) for a in annots[i:i + size]], 'img_name': names[i:i + size]})
    return out


def _model(sncal, tmp_path, dtype='fp32'):
    import bench
    cfg = hr.load_config('hrnet_w18')
    sd = sncal.synth.deep_state_dict(bench.seeded_weights('hrnet_w18', seed=1))
    ck = {'model_name': 'HRNetMetaModel',
          'params': {'nn_module': {'hrnet_config': cfg, 'num_refinement_stages': 0, 'num_heatmaps': 58}, 'loss': LOSS,
                     'prediction_transform': {'size': [540, 960]}, 'device': 'cuda:0'},
          'nn_state_dict': sd}
    path = str(tmp_path / 'model.pth')
    torch.save(ck, path)
    return sncal.load_model(path, device='cuda:0', dtype=dtype)


def _composed(sncal, model, cc, batches):
    """The metrics of validate() from the parts that have their own tests."""
    ev = sncal.CameraEvaluator(model.device, 960, 540, threshold=5)
    loss_fn = sncal.HRNetLoss(**LOSS)
    l2_updates, per_frame, losses = [], [], []
    for b in batches:
        x = b['image'].to(model.device)
        if x.dtype == torch.uint8:
            heat, pred = model.nn_module.forward(x, want_heat=True, decode_size=(540, 960))
        else:
            pred = model.predict(x)
            heat = model.nn_module(x)[-1]
        losses.append((float(loss_fn([heat], b['keypoints'], b['mask'])), len(pred)))
        l2_updates.append((pred.cpu().numpy(), b['keypoints'].numpy()))
        rec = cc.solve_device(pred)
        out, err, cls = ev.evaluate(rec, b['raw_annot'], detail=True)
        o = out.cpu().numpy()
        for i in range(len(pred)):
            if o[i, 11] <= 0:
                per_frame.append(None)
                continue
            p = int(o[i, 10])
            pc, er = ev.frame_detail(out, err, cls, b['raw_annot'], i, p)
            per_frame.append((o[i, 7 + p], o[i, 4 * (p - 1):4 * p].reshape(2, 2), er))
    n = sum(k for _, k in losses)
    want = {'val_loss': sum(v * k for v, k in losses) / n}
    want.update(vr.l2_metrics(l2_updates, 57, 0.5, [2.0, 5.0, 10.0, 50.0]))
    want.update(vr.evalai_metrics(per_frame))
    return want, per_frame, l2_updates


def _assert_same(got, want, n_terms):
    assert set(got) == set(want)
    for k in want:
        g, w = got[k], want[k]
        print(f'{k:22s} validate {g!r}  composed {w!r}')
        if k in ('val_completeness', 'val_precision', 'val_recall', 'val_eval_precision', 'val_eval_recall') or k.startswith('val_pcks'):
            assert g == w, k                                               # ratios of identical counts
        elif np.isinf(w):
            assert g == w, k
        else:
            assert abs(g - w) <= n_terms[k] * 2.0 ** -24 * abs(w), (k, g, w)


def test_validate_equals_the_metrics_composed_step_by_step(sncal, cuda, tmp_path):
    model = _model(sncal, tmp_path)
    images, annots = _dataset(sncal)
    names = [f'{i:05d}.jpg' for i in range(len(images))]
    batches = _batches(sncal, images, annots, names, 4)
    assert [len(b['img_name']) for b in batches] == [4, 4, 3]               # a ragged last batch
    cc = sncal.CameraCreator(sncal.PITCH_POINTS, **KW)
    got = sncal.validate.validate(model, batches, cc)
    assert got.frames == 11 and got.skipped == [] and all(isinstance(v, float) for v in got.values())
    want, per_frame, l2_updates = _composed(sncal, model, cc, batches)
    assert per_frame[6] is None and sum(r is not None for r in per_frame) >= 6   # the noise frame has no camera, the stamped ones do
    assert want['val_eval_accuracy'] > 0 and 0 < want['val_l2'] < float('inf')   # frame and annotation share a camera: not all zero
    n_pts = sum(len(v) for r in per_frame if r is not None for v in r[2].values())
    n_el = sum(int(((t.reshape(-1, 57, 3)[:, :, 0] != -1) & (p[:, :, 2] > 0.5)).sum()) for p, t in l2_updates)
    terms = {'val_loss': 3, 'val_l2': n_el, 'val_l2_reprojection': n_pts, 'val_eval_accuracy': 11, 'val_evalai': 11}
    _assert_same(got, want, terms)
    # two calibrators in one call (the network runs once per batch) == two separate calls
    cc2 = sncal.CameraCreator(sncal.PITCH_POINTS, **dict(KW, conf_thresh=0.8, conf_threshs=[0.8], min_points=12))
    both = sncal.validate.validate(model, batches, [cc, cc2])
    assert isinstance(both, list) and len(both) == 2
    assert dict(both[0]) == dict(got) and dict(both[1]) == dict(sncal.validate.validate(model, batches, cc2))
    # val_step leaves the loss on the device; validate() with a loss handed in uses it
    heavier = sncal.HRNetLoss(**dict(LOSS, awing_w=0.5))
    own = model.loss
    assert sncal.validate.validate(model, batches[:1], cc, loss=heavier)['val_loss'] > sncal.validate.validate(model, batches[:1], cc, loss=sncal.HRNetLoss(**LOSS))['val_loss']
    assert model.loss is own                                               # a loss handed in holds for that call only


def test_validate_over_a_split_folder(sncal, cuda, gold_dir, tmp_path):
    """The golden 960x540 JPEG five times beside synthetic .json annotations, an `info` file and one unreadable .jpg: the same
    result as the iterable form on the decoded frames; the unreadable frame is reported as skipped and counted as missed."""
    g = np.load(os.path.join(gold_dir, 'jpeg_cases.npz'))
    full = g['jpg.full'].tobytes()
    folder = tmp_path / 'valid'
    folder.mkdir()
    annots = []
    for i in range(6):
        annot, _ = sncal.synth.synthetic_annotation(seed=300 + i)
        annots.append(_as_dicts(annot))
        (folder / f'{i:05d}.json').write_text(json.dumps(annots[-1]))
        (folder / f'{i:05d}.jpg').write_bytes(full if i != 2 else b'\xff\xd8' + bytes(range(256)) * 4)
    (folder / 'match_info.json').write_text(json.dumps({'not': 'an annotation'}))
    (folder / 'match_info.jpg').write_bytes(full)
    (folder / '00009.json').write_text(json.dumps(annots[0]))               # an annotation without its image
    model = _model(sncal, tmp_path)
    cc = sncal.CameraCreator(sncal.PITCH_POINTS, **KW)
    with pytest.warns(UserWarning, match='00002.jpg: skipped'):
        got = sncal.validate.validate(model, str(folder), cc, batch_size=2, decoder_threads=2)
    assert got.frames == 6 and got.skipped == ['00002.jpg']                 # frames: the camera metric's own total, scored + skipped
    keep = [0, 1, 3, 4, 5]
    dec = sncal.JpegDecoder(540, 960, max_batch=5, device=cuda)
    frames = dec.decode([full] * 5).cpu()
    dec.close()
    batches = []
    for lo, hi in ((0, 2), (2, 3), (3, 5)):                                 # the folder's batches of two, frame 2 left out of its batch
        idx = keep[lo:hi]
        pairs = [sncal.frames.annot_to_keypoints(annots[i], 57, margin=LOSS['sigma']) for i in idx]
        batches.append({'image': frames[lo:hi], 'keypoints': torch.from_numpy(np.stack([p[0] for p in pairs])),
                        'mask': torch.from_numpy(np.stack([p[1] for p in pairs])),
                        'raw_annot': [sncal.evaluate.scale_points(annots[i], 960, 540) for i in idx],
                        'img_name': [f'{i:05d}.jpg' for i in idx]})
    same = sncal.validate.validate(model, batches, cc)
    assert same.frames == 5 and same.skipped == []
    for k in got:
        if k in ('val_completeness', 'val_evalai'):
            continue
        assert got[k] == same[k] or (np.isnan(got[k]) and np.isnan(same[k])), (k, got[k], same[k])
    # the skipped frame is one more missed frame out of one more frame
    done5 = same['val_completeness'] * 5
    assert abs(got['val_completeness'] - done5 / 6) < 1e-12 and abs(got['val_evalai'] - got['val_completeness'] * got['val_eval_accuracy']) < 1e-12
