"""GPU: sncal_evaluate_cameras_detail on hand-built pitch tables and on cameras off the broadcast sampler's range.

Every comparison is against values written out by hand (evaluate_ref.hand_table, held to the oracle by
tests/test_evaluate_host.py) or against the oracle (oracle/evaluate.py), never against another run of the kernel.

Census of the committed seeds (PCG64(7000 + i); 12 'low' + 12 'zoom' + 8 'broadcast' predicted cameras on the 1187
samples of the default table).  The three sizes see the same cameras, scaled, and take the same branches: 4692 samples
behind the camera, 62 enter and 86 leave crossings, none without an in-image border point, 1 frame with no class.
[TP, FP not annotated, FP beyond threshold, FN] summed over the 32 frames, plain | mirrored labels, and the number of
frames that keep pass 1 / pass 2:

  960x540    t = 5   [64, 78, 50, 41] | [39, 116, 37, 79]   10 / 22
             t = 10  [90, 78, 24, 41] | [59, 116, 17, 79]   16 / 16
             t = 20  [105, 78, 9, 41] | [70, 116, 6, 79]    19 / 13
  1920x1080  t = 5   [39, 78, 75, 41] | [26, 116, 50, 79]    8 / 24
  333x187    t = 5   [100, 78, 14, 41] | [64, 116, 12, 79]  19 / 13
  sampling_factor = 0.5 (1762 samples, 92 456 B of LDS), the 24 'low' + 'zoom' cameras at 960x540, t = 5:
             7275 behind, 47 enter, 53 leave, none without a border point, 1 frame with no class,
                     [53, 43, 24, 25] | [21, 77, 22, 59]     9 / 15

Smallest |distance - t|, t in (5, 10, 20), over every annotated point and both passes: 7.4e-4 px (960x540), 7.4e-3 px
(1920x1080), 1.2e-2 px (333x187), 6.9e-2 px (sampling_factor 0.5): no result hangs on rounding.  None of these
cameras reaches "first valid sample inside while prev is zeros(3)" or a one-point polyline; the hand table does (2 and
4 times), with 10 samples behind, 2 enter and 5 leave crossings.
"""
import ctypes

import numpy as np
import pytest
import torch

import evaluate_ref as er
from oracle import evaluate as oe

pytestmark = pytest.mark.gpu


def _records(sncal, cameras, cuda):
    """sncal_camera records; None = status 0 (no camera)."""
    Cam = sncal._lib.Camera
    buf = (Cam * len(cameras))()
    for i, cam in enumerate(cameras):
        if cam is None:
            continue
        for k in range(3):
            buf[i].position[k] = float(cam['position'][k])
        for k in range(9):
            buf[i].rotation[k] = float(np.asarray(cam['rotation']).reshape(-1)[k])
        buf[i].fx, buf[i].fy = float(cam['f'][0]), float(cam['f'][1])
        buf[i].cx, buf[i].cy = cam['pp']                # not read: the metric's centre is (w/2, h/2)
        buf[i].status = 1
    raw = np.frombuffer(bytes(buf), dtype=np.uint8).reshape(len(cameras), ctypes.sizeof(Cam)).copy()
    return torch.from_numpy(raw).to(cuda)


def _call(sncal, cuda, ht, n_cls=None):
    """The hand table through the C ABI, the way CameraEvaluator.evaluate calls it -> status, out, err, class_conf."""
    frames, classes = ht['frames'], ht['classes']
    C = len(classes) if n_cls is None else n_cls
    gt, cnt, extra, max_gt = er.pack([fr['gt'] for fr in frames], classes, [fr['gt_extra'] for fr in frames])
    assert max_gt == ht['err'].shape[3]
    rec = _records(sncal, [ht['camera'] if fr['status'] else None for fr in frames], cuda)
    dev = [torch.from_numpy(a).to(cuda) for a in (ht['points'], ht['class_start'], ht['mirror'], gt, cnt, extra)]
    B = len(frames)
    out = torch.full((B, 12), -7.0, dtype=torch.float32, device=cuda)
    err = torch.full((B, 2, len(classes), max_gt), -7.0, dtype=torch.float64, device=cuda)
    cls = torch.full((B, 2, len(classes), 4), -7, dtype=torch.int32, device=cuda)
    with torch.cuda.device(cuda):
        status = sncal._lib.lib().sncal_evaluate_cameras_detail(
            rec.data_ptr(), B, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), C, dev[3].data_ptr(), dev[4].data_ptr(),
            dev[5].data_ptr(), max_gt, ht['threshold'], ht['width'], ht['height'], out.data_ptr(), err.data_ptr(), cls.data_ptr(),
            sncal._lib.current_stream_ptr())
        torch.cuda.synchronize()
    return status, out.cpu().numpy(), err.cpu().numpy(), cls.cpu().numpy()


def _check_hand(sncal, cuda, ht):
    status, out, err, cls = _call(sncal, cuda, ht)
    sncal._lib.check(status, 'sncal_evaluate_cameras_detail')
    names = ht['classes']
    for f, fr in enumerate(ht['frames']):
        for p in range(2):
            bad = [(names[c], cls[f, p, c].tolist(), ht['class_conf'][f, p, c].tolist())
                   for c in range(len(names)) if not np.array_equal(cls[f, p, c], ht['class_conf'][f, p, c])]
            assert not bad, (f, p, bad)
            nan = [names[c] for c in range(len(names)) if not np.array_equal(np.isnan(err[f, p, c]), np.isnan(ht['err'][f, p, c]))]
            assert not nan, (f, p, nan)
            far = [(names[c], err[f, p, c].tolist(), ht['err'][f, p, c].tolist()) for c in range(len(names))
                   if not np.allclose(err[f, p, c], ht['err'][f, p, c], rtol=1e-9, atol=1e-9, equal_nan=True)]
            assert not far, (f, p, far)
        assert np.array_equal(out[f, 0:8], ht['out8'][f]), (f, out[f], ht['out8'][f])
        assert out[f, 10] == ht['chosen'][f] and out[f, 11] == fr['status'], (f, out[f])
        if fr['status']:
            a = [ht['out8'][f, 4 * p] / ht['out8'][f, 4 * p:4 * p + 4].sum() for p in range(2)]      # float32 / float32
            assert out[f, 8] == a[0] and out[f, 9] == a[1], (f, out[f], a)
        else:
            assert not out[f].any()
    return out, err, cls


@pytest.mark.parametrize('threshold', [5.0, er.T5_NEXT], ids=['t5', 't5next'])
@pytest.mark.parametrize('n_cls', [1, 16, 32])
@pytest.mark.parametrize('w,h', [(960, 540), (333, 187)])
def test_hand_table_through_the_c_abi(sncal, cuda, w, h, n_cls, threshold):
    """Identity camera, every sample a pixel: out[0:8], class_conf and the chosen pass equal the hand values exactly,
    err within 1e-9 and NaN exactly where no such point exists.  The rows pin: rz > 1e-3 strict, the skip leaving prev
    and in_img alone, the NaN border point with prev = 0, one-point polylines, half-open image bounds, border points
    on entering and leaving and their order, k <= 0 / k >= 1 / 0 < k < 1 / k = NaN, d < threshold strict, mirror[],
    gt_extra, status 0 and max_gt padding; 333x187 puts the principal point on a half-integer."""
    ht = er.hand_table(w, h, n_cls, threshold)
    out, err, cls = _check_hand(sncal, cuda, ht)
    assert err[0, 0, 0, 0] == 5.0                                       # the point that sits on the threshold
    assert cls[0, 0, 0].tolist() == ([1, 1, 0, 0] if threshold == 5.0 else [2, 0, 0, 0])
    if n_cls > 1:
        assert out[:, 10].tolist() == [2, 1, 2, 0] and out[2, 8] == out[2, 9]      # mirrored, plain, tie -> 2, no camera


def _check_against_oracle(sncal, cuda, ev, frames, results, t):
    ann = [fr['gt'] for fr in frames]
    out, err, cls = ev.evaluate(_records(sncal, [fr['camera'] for fr in frames], cuda), ann, detail=True)
    out, err, cls = out.cpu().numpy(), err.cpu().numpy(), cls.cpu().numpy()
    max_gt = err.shape[3]
    bad, n_err = [], 0
    for i, res in enumerate(results):
        c1, c2, a1, a2, which, d1, d2 = res[t]
        if not (np.array_equal(out[i, 0:4], c1.reshape(-1)) and np.array_equal(out[i, 4:8], c2.reshape(-1))):
            bad.append((i, out[i, 0:8].tolist(), c1.reshape(-1).tolist(), c2.reshape(-1).tolist()))
    assert not bad, f'{len(bad)} of {len(frames)} frames differ from the oracle: {bad}'
    for i, res in enumerate(results):
        c1, c2, a1, a2, which, d1, d2 = res[t]
        assert out[i, 8] == np.float32(a1) and out[i, 9] == np.float32(a2), (i, out[i], a1, a2)
        assert out[i, 10] == which and out[i, 11] == 1, (i, out[i], which)
        for p, (pc, errs) in enumerate((d1, d2)):
            cc, e = er.detail_arrays(pc, errs, oe.CLASSES, max_gt)
            assert np.array_equal(cls[i, p], cc), (i, p, cls[i, p].tolist(), cc.tolist())
            assert np.array_equal(np.isnan(err[i, p]), np.isnan(e)), (i, p)
            assert np.allclose(err[i, p], e, rtol=1e-9, atol=1e-9, equal_nan=True), (i, p, np.nanmax(np.abs(err[i, p] - e)))
            n_err += int(np.isfinite(e).sum())
            pcs, ers = ev.frame_detail(out, err, cls, ann, i, p + 1)    # the dictionaries the product hands out
            assert set(pcs) == set(pc) and set(ers) == set(errs), (i, p)
            assert all(np.array_equal(pcs[k], pc[k]) for k in pc), (i, p)
    assert n_err > 500
    return out


@pytest.mark.parametrize('w,h,t', [(w, h, t) for w, h, ts in er.CASES for t in ts])
def test_off_broadcast_cameras_match_the_oracle(sncal, cuda, w, h, t):
    """12 'low' + 12 'zoom' + 8 'broadcast' cameras on the real pitch table: both confusions on every frame, both
    accuracies, the chosen pass and the detail outputs in both passes, at three image sizes and three thresholds."""
    thresholds = next(ts for cw, ch, ts in er.CASES if (cw, ch) == (w, h))
    frames, counts, results = er.oracle_results(w, h, thresholds)
    assert len(frames) == 32
    er.check_census(counts, thresholds)
    out = _check_against_oracle(sncal, cuda, sncal.CameraEvaluator(cuda, w, h, threshold=t), frames, results, t)
    assert sorted(set(out[:, 10].tolist())) == [1.0, 2.0]


def test_large_table_launch_matches_the_oracle(sncal, cuda):
    """sampling_factor = 0.5: 1762 samples need 92 456 B of dynamic LDS, the first launch above 64 KiB."""
    frames, counts, results = er.oracle_results(960, 540, (5.0,), 0.5, er.KINDS_24)
    assert len(frames) == 24 and len(er.field_table(0.5)[0]) == 1762
    er.check_census(counts, (5.0,))
    ev = sncal.CameraEvaluator(cuda, 960, 540, threshold=5.0, sampling_factor=0.5)
    assert ev._field.shape == (1762, 3) and torch.equal(ev._field.cpu(), torch.from_numpy(er.field_table(0.5)[0]))
    _check_against_oracle(sncal, cuda, ev, frames, results, 5.0)


def test_loud_failures_leave_the_evaluator_usable(sncal, cuda):
    """A table beyond the kernel's 2048 samples, more than 32 classes: an error that names the figure; an empty
    batch: an empty result.  After each, the next call is right."""
    ht = er.hand_table(960, 540, 32, 5.0)
    frames = er.oracle_results(333, 187, (5.0,))[0][:1]
    rec = _records(sncal, [fr['camera'] for fr in frames], cuda)
    big = sncal.CameraEvaluator(cuda, sampling_factor=0.2)              # the reference's own default argument
    assert big._field.shape[0] == 3692
    with pytest.raises(sncal._lib.SncalError, match='3692'):
        big.evaluate(rec, [frames[0]['gt']])
    _check_hand(sncal, cuda, ht)

    status, *_ = _call(sncal, cuda, ht, n_cls=33)
    assert status != 0
    with pytest.raises(sncal._lib.SncalError, match='n_cls=33'):
        sncal._lib.check(status, 'sncal_evaluate_cameras_detail')
    _check_hand(sncal, cuda, ht)

    ev = sncal.CameraEvaluator(cuda)
    out = ev.evaluate(rec[:0], [])
    assert out.shape == (0, 12) and out.dtype == torch.float32
    out, err, cls = ev.evaluate(rec[:0], [], detail=True)
    assert out.shape == (0, 12) and err.shape[0] == 0 and cls.shape[0] == 0
    assert sncal.CameraEvaluator.summarize(out)['completeness'] == 0.0
    _check_hand(sncal, cuda, ht)
