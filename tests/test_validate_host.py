"""CPU: the fp64 restatement of the validation loss and of both metric aggregations (tests/validate_ref.py) against what
tools/make_golden_validate.py captured from the reference (tests/golden/validate.npz); L2metric itself on CPU tensors (it is plain
torch); argument checks of the new C entry points and of HRNetLoss that need no device."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import validate_ref as vr
from test_oracle_goldens import _eval_frames


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'validate.npz'))


def test_loss_helper_matches_reference_capture(gold):
    """The helper rebuilds the target with the correctly rounded exp (oracle.synth.create_target), the capture used torch's: the two
    targets differ by at most 4 ulp = 2^-21 relative per element (tests/test_oracle_goldens._target_close), which bounds the move of
    any sum of the loss; on top of that the reference's fp32 result is d_ref away from the fp64 value by definition."""
    cases = vr.loss_cases(gold)
    assert set(cases) == {'small', 'train', 'ragged'}
    assert cases['small']['shape'] == (3, 58, 68, 120) and cases['train']['shape'] == (2, 58, 270, 480) and cases['ragged']['shape'] == (1, 7, 33, 257)
    for name, c in cases.items():
        pred = vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        assert pred.dtype == np.float32 and pred.max() <= 0 and np.array_equal(pred * 256, np.rint(pred * 256))
        target = vr.target32(c['kp'], c['stride'], c['sigma'], c['shape'][2:])
        for mname, m in c['masks'].items():
            sums = vr.loss_terms64(pred, target, m)
            stored = gold[f'loss.{name}.{mname}.sums64']
            assert np.all(np.abs(sums - stored) <= 2.0 ** -21 * np.abs(stored)), (name, mname)
            for wname, wts in vr.WEIGHTS.items():
                key = f'loss.{name}.{mname}.{wname}'
                v = vr.combine(sums, wts, c['shape'])
                v64, ref, d_ref = float(gold[key + '.v64']), float(gold[key + '.ref']), float(gold[key + '.d_ref'])
                assert abs(v - v64) <= 2.0 ** -21 * abs(v64), key
                assert abs(v - ref) <= (d_ref + 2.0 ** -21 + 2.0 ** -24) * abs(ref), key
    # the quirks the cases were built for
    c = cases['small']
    t = vr.target32(c['kp'], c['stride'], c['sigma'], c['shape'][2:])
    assert not t[1, :-1].any() and (t[1, -1] == 1).all()                 # a frame with no visible point
    assert c['kp'][2, 0, 2] == 0 and t[2, 0].max() > 0.5                  # x / stride == 1.0, flag 0: visible
    assert c['kp'][2, 2, 0] == 1.0 and not t[2, 2].any()                  # x == 1.0 before the division: not visible
    assert t[2, 3].max() == 1.0 and t[2, -1].min() == 0.0                 # a peak on a cell centre: background exactly 0


def _l2_updates(gold):
    return [(gold[f'l2.{i}.pred'], gold[f'l2.{i}.target']) for i in range(int(gold['l2.n']))]


def _check_l2(got, gold):
    """Counts are exact, so their ratios agree to the capture's own fp32 rounding (the reference divides integer tensors into
    fp32: 2^-24 relative); the fp32 sum of n distances taken in any order is within n * 2^-24 relative."""
    n = int(gold['l2.num_el'])
    for k, v in zip([str(k) for k in gold['l2.keys']], gold['l2.values']):
        tol = n * 2.0 ** -24 if k == 'val_l2' else 2.0 ** -24
        assert abs(got[k] - v) <= tol * abs(v), (k, got[k], v)
    assert set(got) == {str(k) for k in gold['l2.keys']}


def test_l2_helper_matches_reference_capture(gold):
    ups = _l2_updates(gold)
    assert [len(p) for p, _ in ups] == [4, 4, 2]
    _check_l2(vr.l2_metrics(ups, 57, 0.5, [float(t) for t in gold['l2.thres']]), gold)


def test_l2metric_on_cpu_tensors_matches_reference_capture(gold):
    import sncal_amd
    m = sncal_amd.L2metric(num_keypoints=57, conf_threshold=0.5, pckhs_thres=[float(t) for t in gold['l2.thres']])
    assert m.compute() == float('inf')
    for p, t in _l2_updates(gold):
        m.update({'prediction': torch.from_numpy(p), 'target': torch.from_numpy(t)})
    state = types.SimpleNamespace(phase='val', metrics={})
    m.epoch_complete(state)
    _check_l2(state.metrics, gold)
    assert abs(m.compute() - state.metrics['val_l2']) == 0
    # n_fp / n_fn are those of the LAST update only: an epoch that ends on a batch without false positives has precision 1
    p, t = _l2_updates(gold)[0]
    t2 = t.reshape(-1, 57, 3).copy()
    p2 = p.copy()
    p2[..., 2] = np.where(t2[..., 0] == -1, 0.0, 0.9)
    m.update({'prediction': torch.from_numpy(p2), 'target': torch.from_numpy(t2.reshape(len(t2), -1))})
    m.epoch_complete(state)
    assert state.metrics['val_precision'] == 1.0 and state.metrics['val_recall'] == 1.0
    m.reset()
    state = types.SimpleNamespace(phase='', metrics={})
    m.epoch_complete(state)
    assert state.metrics == {'precision': 0.0, 'recall': 0.0, 'pcks-2.0': 0.0, 'pcks-5.0': 0.0, 'pcks-10.0': 0.0, 'pcks-50.0': 0.0,
                             'l2': float('inf')}


def evalai_frames(gold, gold_dir):
    """Per-frame results of the kept pass for the capture's frames, from tests/golden/evaluator_batch.npz."""
    _, frames = _eval_frames(gold_dir)
    none = set(int(i) for i in gold['evalai.none'])
    out = []
    for i, fr in enumerate(frames):
        if i in none:
            out.append(None)
            continue
        out.append(vr.kept_pass(np.float32(fr['acc'][0]), fr['conf1'], fr['err1'], np.float32(fr['acc'][1]), fr['conf2'], fr['err2']))
    return frames, out


def check_evalai(got, gold, n_frames=10, reproj_tol=1e-12):
    """The capture ran under numpy 2, where the reference's running sums of np.float32 per-frame values (accuracy, confusion
    entries) stay float32: a sum of n terms plus the final division, (n + 1) * 2^-24 relative.  The reprojection errors are
    float64 lists summed in float64."""
    for k, v in zip([str(k) for k in gold['evalai.keys']], gold['evalai.values']):
        tol = reproj_tol if k == 'val_l2_reprojection' else 1e-12 if k == 'val_completeness' else (n_frames + 2) * 2.0 ** -24
        assert abs(got[k] - v) <= tol * abs(v), (k, got[k], v)
    assert set(got) >= {str(k) for k in gold['evalai.keys']}


def test_evalai_helper_matches_reference_capture(gold, gold_dir):
    _, per_frame = evalai_frames(gold, gold_dir)
    assert sum(r is None for r in per_frame) == 2
    assert sum(len(v) for r in per_frame if r is not None for v in r[2].values()) == int(gold['evalai.n_l2_proj'])
    check_evalai(vr.evalai_metrics(per_frame), gold)


def test_evalai_aggregation_on_cpu_tensors(gold, gold_dir):
    """EvalAImetric.update_records over the (out, err, cls) arrays sncal_evaluate_cameras_detail returns, built here from the
    capture's per-frame confusions and errors (the kernel itself: tests/test_evaluate_gpu.py): the aggregation is plain torch."""
    import sncal_amd
    from sncal_amd.evaluate import CLASSES
    frames, per_frame = evalai_frames(gold, gold_dir)
    C, G = len(CLASSES), 12

    class FakeEvaluator:
        device = torch.device('cpu')

        def evaluate(self, records, annots, detail=False):
            B = len(annots)
            out = torch.zeros((B, 12), dtype=torch.float32)
            err = torch.full((B, 2, C, G), float('nan'), dtype=torch.float64)
            cls = torch.zeros((B, 2, C, 4), dtype=torch.int32)
            for b, i in enumerate(records.tolist()):
                fr = frames[i]
                if per_frame[i] is None:
                    continue
                out[b, 0:4] = torch.from_numpy(fr['conf1'].reshape(-1))
                out[b, 4:8] = torch.from_numpy(fr['conf2'].reshape(-1))
                out[b, 8], out[b, 9] = float(fr['acc'][0]), float(fr['acc'][1])
                out[b, 10], out[b, 11] = (1 if fr['acc'][0] > fr['acc'][1] else 2), 1
                for p, tag in enumerate(('1', '2')):
                    for name, m in fr['pc' + tag].items():
                        c = CLASSES.index(name)
                        if name in fr['err' + tag]:
                            e = fr['err' + tag][name]
                            cls[b, p, c, 0], cls[b, p, c, 1] = int(m[0, 0]), int(m[0, 1])
                            err[b, p, c, :len(e)] = torch.from_numpy(np.asarray(e))
                        elif m[1, 0] > 0:
                            cls[b, p, c, 2] = int(m[1, 0])
                        else:
                            cls[b, p, c, 3] = 1
            return out, err, cls
    m = sncal_amd.EvalAImetric(pred2cam=None, threshold=5, img_size=(960, 540))
    m._evaluator = FakeEvaluator()
    for lo, hi in gold['evalai.batches']:
        m.update_records(torch.arange(lo, hi), [frames[i]['gt'] for i in range(lo, hi)])
    state = types.SimpleNamespace(phase='val', metrics={})
    m.epoch_complete(state)
    check_evalai(state.metrics, gold)
    m.reset()
    m.epoch_complete(state)
    assert state.metrics['val_l2_reprojection'] == float('inf') and state.metrics['val_evalai'] == 0.0


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    import sncal_amd
    L = sncal_amd._lib
    lib = L.lib()
    one = ctypes.c_void_p(16)
    n = ctypes.c_size_t()
    assert lib.sncal_heatmap_loss_workspace(16, 57, 270, 480, ctypes.byref(n)) == 0
    tables = 16 * 57 * (270 + 480) * 8
    assert tables <= n.value <= tables + 16 * 17 * 8 * 24 + 3 * 256      # Gaussian tables + one partial per workgroup, padded
    assert lib.sncal_heatmap_loss_workspace(16, 65, 270, 480, ctypes.byref(n)) == -1
    assert lib.sncal_heatmap_loss_workspace(16, 57, 270, 480, None) == -1
    assert lib.sncal_heatmap_loss(None, None, None, 0, 57, 270, 480, 2.0, 2.0, 3, None, None, 0, None) == 0       # empty batch
    assert lib.sncal_heatmap_loss(one, one, None, 1, 65, 8, 8, 2.0, 2.0, 3, one, one, 1 << 20, None) == -1 and b'N=65' in lib.sncal_last_error()
    assert lib.sncal_heatmap_loss(one, one, None, 1, 5, 8, 8, 0.0, 2.0, 3, one, one, 1 << 20, None) == -1 and b'sigma' in lib.sncal_last_error()
    assert lib.sncal_heatmap_loss(one, one, None, 1, 5, 8, 8, 2.0, 0.0, 3, one, one, 1 << 20, None) == -1 and b'stride' in lib.sncal_last_error()
    assert lib.sncal_heatmap_loss(one, one, None, 1, 5, 8, 8, 2.0, 2.0, 8, one, one, 1 << 20, None) == -1 and b'terms' in lib.sncal_last_error()
    assert lib.sncal_heatmap_loss(None, one, None, 1, 5, 8, 8, 2.0, 2.0, 3, one, one, 1 << 20, None) == -1 and b'null' in lib.sncal_last_error()
    assert lib.sncal_heatmap_loss(one, one, None, 1, 5, 8, 8, 2.0, 2.0, 3, one, one, 64, None) == -4 and b'workspace' in lib.sncal_last_error()
    with pytest.raises(L.SncalError, match='num_refinement_stages'):
        sncal_amd.HRNetLoss(num_refinement_stages=1)
    loss = sncal_amd.HRNetLoss(sigma=2.0, stride=2, pred_size=(270, 480), kldiv_w=0.0, awing_w=0.5)
    assert loss.terms == 5 and loss.n_losses == 1
    with pytest.raises(L.SncalError, match='pred_size'):
        loss([torch.zeros(1, 58, 68, 120)], torch.zeros(1, 171))
    with pytest.raises(L.SncalError):                                    # no CPU path
        loss([torch.zeros(1, 58, 270, 480)], torch.zeros(1, 171))


def test_annotation_to_keypoints_is_the_dataset_rule():
    """dataset.py:73-87 over annotations.get_intersections: [x, y, 1] for a produced point, [-1, -1, 0] otherwise, mask 0 for the
    circle ids get_intersections lists as not produced."""
    import sncal_amd
    annot, _ = sncal_amd.synth.synthetic_annotation(seed=3)
    as_dicts = {c: [{'x': x, 'y': y} for x, y in pts] for c, pts in annot.items()}
    kp, mask = sncal_amd.frames.annot_to_keypoints(as_dicts, 57, margin=2.0)
    labels, missing = sncal_amd.annotations.get_intersections(annot, margin=2.0)
    assert kp.dtype == np.float32 and kp.shape == (171,) and mask.shape == (58,) and mask.dtype == np.int64
    kp = kp.reshape(57, 3)
    for i in range(57):
        if labels[i] is None:
            assert tuple(kp[i]) == (-1.0, -1.0, 0.0)
        else:
            assert kp[i, 2] == 1 and np.allclose(kp[i, :2], labels[i], rtol=1e-6)
    assert [i for i in range(58) if mask[i] == 0] == sorted(missing)
    assert (kp[:, 2] == 1).sum() >= 4
