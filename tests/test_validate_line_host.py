"""CPU: the fp64 restatement of the line model's target maps, loss and metric (tests/validate_line_ref.py) against what
tools/make_golden_validate_line.py captured from the reference (tests/golden/validate_line.npz); the host-side labels
(annotations.sort_anno / get_extreme_points) and AccMetric's aggregation against the same capture; argument checks of the new C
entry points and of EHMLoss that need no device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import validate_line_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'validate_line.npz'))


def test_maps_helper_reproduces_the_captured_maps_exactly(gold):
    cases = vr.cases(gold)
    assert {n: c['shape'] for n, c in cases.items()} == {'small': (2, 23, 16, 24), 'wide': (1, 5, 33, 61), 'mid': (3, 23, 34, 60)}
    assert [c['sigma'] for c in cases.values()] == [1.0, 7.0, 2.0]
    for name, c in cases.items():
        hw = c['shape'][2:]
        maps = vr.keypoint_maps(c['kp'], c['sigma'], c['stride'], hw, as_dataset=True)
        assert maps.dtype == np.float32 and float(maps.max()) == float(gold[f'case.{name}.max'])
        if c['maps'] is not None:
            assert np.array_equal(maps, c['maps']), name
        # the dataset adds fp64 Gaussians into a float32 map: one rounding per addition away from the exact recipe
        exact = vr.keypoint_maps(c['kp'], c['sigma'], c['stride'], hw)
        assert np.all(np.abs(maps - exact) <= 2.0 ** -23 * exact + 2.0 ** -149), name
    assert cases['small']['maps'] is not None and cases['wide']['maps'] is not None and cases['mid']['maps'] is None


def test_the_edge_cases_the_fixture_was_built_for(gold):
    for name, c in vr.cases(gold).items():
        B, C, h, w = c['shape']
        s = c['stride']
        kp, mu = c['kp'], vr.centres(c['kp'], c['stride'], (h, w))
        t = vr.keypoint_maps(kp, c['sigma'], s, (h, w))
        assert kp[0, 0, 0, 0] / s == 2.5 and kp[0, 0, 1, 0] / s == 3.5 and mu[0, 0, :, 0].tolist() == [2, 4]       # ties to even
        assert mu[0, 0, :, 1].tolist() == [2, 6]
        assert kp[0, 1, 0, 0] > w * s and kp[0, 1, 0, 1] > h * s and mu[0, 1, 0].tolist() == [w - 1, h - 1]        # clamped
        assert t[0, 1, h - 1, w - 1] >= 1.0
        assert mu[0, 2, 0].tolist() == [-3, -2] and mu[0, 2, 1].tolist() == [1, -3]                                # mu < 0
        one = np.zeros((1, 1, 2, 3), dtype=np.float32)
        one[0, 0, 0] = kp[0, 2, 0]
        assert vr.keypoint_maps(one, c['sigma'], s, (h, w))[0, 0, 0, 0] == 1.0                                     # normalised by its maximum
        assert np.abs(mu[0, 3, 0] - mu[0, 3, 1]).max() <= 1 and t[0, 3].max() > 1.5                                # 3 px apart: sum near 2
        assert kp[0, 4, :, 2].tolist() == [0, 1] and t[0, 4, mu[0, 4, 1, 1], mu[0, 4, 1, 0]] >= 1.0                # one flag 0
        assert t[0, 4, int(np.rint(2.2)), int(np.rint(7.3))] < 1.0
        if B > 1:
            assert not kp[1, :, :, 2].any() and not t[1].any()                                                     # an empty frame


def test_loss_helper_matches_reference_capture(gold):
    """On the reference's own fp32 maps the fp64 helper IS the stored v64 (up to the summation order of fp64: 1e-12), and the
    reference's fp32 result is d_ref away from it by definition; 2^-24 is the rounding of the captured value to fp32."""
    for name, c in vr.cases(gold).items():
        pred = vr.make_pred(c['seed'], c['shape'], c['kp'], c['stride'])
        assert pred.dtype == np.float32 and 0 <= pred.min() and pred.max() <= 1 and np.array_equal(pred * 16384, np.rint(pred * 16384))
        maps = vr.keypoint_maps(c['kp'], c['sigma'], c['stride'], c['shape'][2:], as_dataset=True)
        sums = vr.loss_terms64(pred, maps, c['gmse_sigma'])
        assert np.all(np.abs(sums - gold[f'case.{name}.sums64']) <= 1e-12 * np.abs(sums)), name
        for wname, wts in vr.WEIGHTS.items():
            key = f'case.{name}.{wname}'
            v = vr.combine(sums, wts, c['shape'])
            v64, ref, d_ref = float(gold[key + '.v64']), float(gold[key + '.ref']), float(gold[key + '.d_ref'])
            assert abs(v - v64) <= 1e-12 * abs(v64), key
            assert abs(v - ref) <= (d_ref + 2.0 ** -24) * abs(v64), key
        # both branches of the adaptive wing occur
        delta = np.abs(maps.astype(np.float64) - pred)
        assert (delta < vr.THETA).any() and (delta >= vr.THETA).any()


def _same_labels(got, want):
    """Extreme points are the annotation's own points times the image size: exact.  Slope and intercept come out of numpy's
    least-squares solver (LAPACK), whose last bits are not portable between builds: 1e-9 relative."""
    assert set(got) == set(range(23)) and set(want) == {str(i) for i in range(23)}
    for i in range(23):
        g, w = got[i], want[str(i)]
        assert (g is None) == (w is None), i
        if g is not None:
            assert np.asarray(g[0][0]).tolist() == w[0] and np.asarray(g[0][1]).tolist() == w[1], i
            assert np.allclose(np.array(g[1], dtype=np.float64), w[2], rtol=1e-9, atol=0), i


def test_labels_equal_the_capture(gold):
    from sncal_amd import annotations as an
    cases = vr.label_cases(gold)
    assert len(cases) == 28 and [c['usable'] for c in cases[-4:]] == [False, False, True, True]
    lines = 0
    for c in cases:
        pts = {k: [tuple(p) for p in v] for k, v in c['points'].items()}
        res, usable = an.sort_anno(pts, img_size=(960, 540))
        assert usable == c['usable']
        assert not any(k.startswith('Circle') or k == 'Line unknown' for k in res)
        labels = an.get_extreme_points(res, img_size=(960, 540))
        _same_labels(labels, c['labels'])
        lines += sum(v is not None for v in labels.values())
        kp, paras = an.line_keypoints(labels)
        assert kp.shape == (138,) and kp.dtype == np.float32 and len(paras) == 23
        for i in range(23):
            row = kp[i * 6:i * 6 + 6]
            if labels[i] is None:
                assert row.tolist() == [-1, -1, 0, -1, -1, 0] and all(math.isnan(v) for v in paras[i])
            else:
                assert row[2] == 1 and row[5] == 1 and tuple(paras[i]) == tuple(labels[i][1])
    assert lines > 100
    # the quirks: a horizontal line has no fit and spoils the frame, and so does a one-point line; a NaN point stays in the list
    horizontal, one_point, with_nan, tie = [c for c in cases[-4:]]
    assert an.sort_points_on_line([tuple(p) for p in horizontal['points']['Side line top']], (960, 540))[1:] == (None, None)
    assert with_nan['labels']['2'] is not None and len(with_nan['points']['Middle line']) == 4
    assert tie['labels']['4'] is not None
    with pytest.raises(ValueError):
        an.sort_points_on_line([(float('nan'), 0.5), (0.5, float('nan'))], (960, 540))


def test_acc_helper_and_aggregation_match_the_capture(gold):
    from sncal_amd import metrics
    batches = vr.acc_batches(gold)
    assert [len(g) for g, _ in batches] == [2, 3, 1]
    thr = float(gold['acc.conf_threshold'])
    counts = np.stack([vr.acc_counts(g, p, thr) for g, p in batches])
    assert np.array_equal(counts, gold['acc.counts'])
    assert np.array_equal(counts[:, :, 0] / counts.sum(axis=2), gold['acc.a_t'])          # the reference's own a_t_score values
    assert vr.acc_value(counts) == float(gold['acc.value'])
    assert metrics.acc_from_counts(gold['acc.counts']) == float(gold['acc.value'])        # the product's aggregation, fed stored counts
    for i, c in enumerate(gold['acc.counts']):
        assert metrics.acc_from_counts(c[None]) == float(gold['acc.per_batch'][i]) == c[2, 0] / c[2].sum() * 1 + c[2, 0] / c[2].sum() * 0.15
    with pytest.raises(ZeroDivisionError):
        metrics.acc_from_counts(np.zeros((1, 3, 3), dtype=np.int64))
    # the constructed channels of batch 0: the low-confidence prediction that is nearest still decides `within` of slot 0 ...
    g, p = batches[0]
    c0 = vr.acc_counts(g[0, 0:1], p[0, 0:1], thr)
    assert c0[:, 0].tolist() == [0, 0, 0] and c0[0, 2] == 1 and c0[0, 1] == 1            # slot 0: fn (not confident); slot 1: 100 px off, fp
    assert vr.acc_counts(g[0, 1:2], p[0, 1:2], thr)[0].tolist() == [0, 1, 0]              # no ground truth, one confident prediction
    assert vr.acc_counts(g[0, 2:3], p[0, 2:3], thr)[0].tolist() == [2, 0, 0]              # distance exactly 5 and confidence == threshold count


def test_ehmloss_refuses_refinement_stages():
    import sncal_amd
    with pytest.raises(sncal_amd._lib.SncalError, match='num_refinement_stages'):
        sncal_amd.EHMLoss(num_refinement_stages=1)
    loss = sncal_amd.loss.EHMLoss()
    assert (loss.n_losses, loss.gmse_w, loss.awing_w, loss.sigma, loss.target_sigma, loss.stride, loss.terms) == (1, 1.0, 1.0, 4, 1, 4, 3)
    assert sncal_amd.EHMLoss(gmse_w=0.0).terms == 2 and sncal_amd.EHMLoss(awing_w=0).terms == 1
    assert sncal_amd.AccMetric().num_keypoints == 23 and sncal_amd.AccMetric().conf_threshold == 0.2
    assert sncal_amd.EHMMetaModel.loss_cls is sncal_amd.EHMLoss and sncal_amd.HRNetMetaModel.loss_cls is sncal_amd.HRNetLoss


def test_header_declarations_are_exported_and_bound():
    import sncal_amd
    L = sncal_amd._lib.lib()
    with open(os.path.join(ROOT, 'include', 'sncal.h')) as f:
        declared = set(re.findall(r'\b(sncal_line_\w+)\s*\(', f.read()))
    assert declared == {'sncal_line_decode', 'sncal_line_target', 'sncal_line_loss_workspace', 'sncal_line_loss', 'sncal_line_acc_counts'}
    for name in declared:
        assert hasattr(L, name) and name in sncal_amd._lib.SIGNATURES and name not in sncal_amd._lib.MISSING


def test_argument_checks_need_no_device():
    import sncal_amd
    L = sncal_amd._lib.lib()
    n = ctypes.c_size_t()
    assert L.sncal_line_loss_workspace(8, 23, 135, 240, ctypes.byref(n)) == 0 and n.value > 0 and n.value % 256 == 0
    assert L.sncal_line_loss_workspace(1, 65, 8, 8, ctypes.byref(n)) == -1 and b'C=65' in L.sncal_last_error()
    assert L.sncal_line_loss_workspace(1, 23, 8, 8, None) == -1
    assert L.sncal_line_target(None, 0, 23, 1.0, 4.0, 8, 8, None, None) == 0                       # B == 0: nothing to do
    assert L.sncal_line_target(None, 1, 23, 0.0, 4.0, 8, 8, None, None) == -1 and b'sigma' in L.sncal_last_error()
    assert L.sncal_line_target(None, 1, 23, 1.0, 0.0, 8, 8, None, None) == -1 and b'stride' in L.sncal_last_error()
    assert L.sncal_line_target(None, 1, 23, 1.0, 4.0, 8, 8, None, None) == -1 and b'null' in L.sncal_last_error()
    one = ctypes.c_void_p(16)
    assert L.sncal_line_loss(None, one, None, 0, 23, 8, 8, 1.0, 4.0, 4.0, 3, None, None, 0, None) == 0       # B == 0
    assert L.sncal_line_loss(None, one, one, 1, 23, 8, 8, 1.0, 4.0, 4.0, 3, None, None, 0, None) == -1 and b'exactly one' in L.sncal_last_error()
    assert L.sncal_line_loss(None, None, None, 1, 23, 8, 8, 1.0, 4.0, 4.0, 3, None, None, 0, None) == -1 and b'exactly one' in L.sncal_last_error()
    assert L.sncal_line_loss(None, one, None, 1, 23, 8, 8, 1.0, 4.0, 4.0, 4, None, None, 0, None) == -1 and b'terms' in L.sncal_last_error()
    assert L.sncal_line_loss(None, one, None, 1, 23, 8, 8, 1.0, 4.0, 0.0, 1, None, None, 0, None) == -1 and b'gmse_sigma' in L.sncal_last_error()
    assert L.sncal_line_loss(None, None, one, 1, 23, 8, 8, 0.0, 4.0, 4.0, 3, None, None, 0, None) == -1 and b'target_sigma' in L.sncal_last_error()
    ts = (ctypes.c_float * 3)(5, 10, 20)
    assert L.sncal_line_acc_counts(None, None, 1, 23, 0.2, ts, 9, one, None) == -1 and b'n_t' in L.sncal_last_error()
    assert L.sncal_line_acc_counts(None, None, 1, 23, 0.2, ts, 3, one, None) == -1 and b'null' in L.sncal_last_error()


def test_list_line_split_lists_what_the_dataset_lists(gold, tmp_path):
    """EHMDataset.__init__: json + jpg pairs, names without 'info', annotations sort_anno finds usable (here sorted by name)."""
    import json
    from sncal_amd import frames
    cases = vr.label_cases(gold)
    files = {'00002': cases[0], '00000': cases[1], '00001': cases[-4], 'x_info': cases[2], '00003': cases[3], '00004': cases[-2]}
    for name, c in files.items():
        with open(tmp_path / f'{name}.json', 'w') as f:
            json.dump({cls: [{'x': x, 'y': y} for x, y in pts] for cls, pts in c['points'].items()}, f)
        if name != '00003':
            (tmp_path / f'{name}.jpg').write_bytes(b'')
    (tmp_path / 'notes.txt').write_text('x')
    names, labels = frames.list_line_split(str(tmp_path))
    assert names == ['00000.jpg', '00002.jpg', '00004.jpg']                 # 00001: horizontal line; 00003: no image; x_info: ignored
    _same_labels(labels[0], cases[1]['labels'])
    _same_labels(labels[1], cases[0]['labels'])
    _same_labels(labels[2], cases[-2]['labels'])                            # NaN survives the json round trip
