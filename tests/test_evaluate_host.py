"""CPU: the references tests/test_evaluate_edges_gpu.py holds the evaluation kernel to.

The hand-written expectations of evaluate_ref.hand_table() must equal what the generalised oracle computes from the
same table (this is the only place the two meet), and the off-broadcast camera sets must take the branches, and keep
the distance from the thresholds, that the GPU tests rely on."""
import numpy as np
import pytest

import evaluate_ref as er
from oracle import evaluate as oe


@pytest.mark.parametrize('threshold', [5.0, er.T5_NEXT], ids=['t5', 't5next'])
@pytest.mark.parametrize('n_cls', [1, 16, 32])
@pytest.mark.parametrize('w,h', [(960, 540), (333, 187)])
def test_hand_table_expectations_equal_the_oracle(w, h, n_cls, threshold):
    ht = er.hand_table(w, h, n_cls, threshold)
    cam, classes = ht['camera'], ht['classes']
    table = (ht['points'], ht['class_start'])
    assert len(classes) == n_cls and len(set(classes)) == n_cls
    assert sorted(ht['mirror']) == list(range(n_cls)) and all(ht['mirror'][ht['mirror'][c]] == c for c in range(n_cls))
    stats = {}
    poly = oe.get_polylines(cam['position'], cam['rotation'], cam['f'][0], cam['f'][1], cam['pp'], w, h, table, classes, stats)
    assert poly == ht['polylines']                                      # equal as floats
    if n_cls > 1:                                                       # every branch of the walk is taken
        assert stats['behind'] == 10 and stats['enter'] == 2 and stats['leave'] == 5 and stats['first_prev_zero'] == 2
        assert stats['len1'] == 4 and stats.get('no_border', 0) == 0
    max_gt = ht['err'].shape[3]
    assert len({len(v) for v in ht['frames'][0]['gt'].values()}) > 1 or n_cls == 1      # max_gt padding is exercised
    seen = set()
    for f, fr in enumerate(ht['frames']):
        if not fr['status']:
            assert not ht['out8'][f].any() and np.isnan(ht['err'][f]).all() and not ht['class_conf'][f].any()
            continue
        gt = er.oracle_gt(fr)
        conf, acc = [], []
        for p, labels in enumerate((gt, oe.mirror_labels(gt, ht['symmetric']))):
            c, pc, errs = oe.evaluate_camera_prediction(poly, labels, threshold, detail=True)
            cc, e = er.detail_arrays(pc, errs, classes, max_gt)
            assert np.array_equal(cc, ht['class_conf'][f, p]), (f, p, cc, ht['class_conf'][f, p])
            assert np.array_equal(np.isnan(e), np.isnan(ht['err'][f, p])), (f, p)
            assert np.allclose(e, ht['err'][f, p], rtol=0, atol=1e-12, equal_nan=True), (f, p)
            assert np.array_equal(c.reshape(-1), ht['out8'][f, 4 * p:4 * p + 4]), (f, p, c)
            conf.append(c)
        full = oe.evaluate_frame(cam['position'], cam['rotation'], cam['f'][0], cam['f'][1], cam['pp'], gt, threshold, w, h,
                                 table, classes, ht['symmetric'])
        assert np.array_equal(full[2], conf[0]) and np.array_equal(full[3], conf[1])
        a1, a2 = (c[0, 0] / c.sum() for c in conf)
        assert ht['chosen'][f] == (1 if a1 > a2 else 2)
        seen.add((int(ht['chosen'][f]), bool(a1 == a2)))
    if n_cls > 1:
        assert seen == {(2, False), (1, False), (2, True)}              # mirrored wins, plain wins, a tie goes to 2
    # the d == 5.0 points are beyond at 5 and within at the next float
    assert ht['err'][0, 0, 0, 0] == 5.0 and ht['class_conf'][0, 0, 0].tolist() == ([1, 1, 0, 0] if threshold == 5.0 else [2, 0, 0, 0])


def test_default_arguments_of_the_oracle_are_unchanged():
    """classes= / symmetric= / stats= default to the pitch model's: same polylines, same frame result."""
    fr = er.oracle_results(333, 187)[0][13]
    cam = fr['camera']
    a = oe.get_polylines(cam['position'], cam['rotation'], cam['f'][0], cam['f'][1], cam['pp'], 333, 187, er.field_table(0.9))
    b = oe.get_polylines(cam['position'], cam['rotation'], cam['f'][0], cam['f'][1], cam['pp'], 333, 187, er.field_table(0.9),
                         oe.CLASSES, {})
    assert a == b and len(a) > 0
    assert oe.mirror_labels(fr['gt']) == oe.mirror_labels(fr['gt'], oe.SYMMETRIC)


@pytest.mark.parametrize('w,h,thresholds', er.CASES, ids=lambda v: str(v))
def test_off_broadcast_sets_take_the_branches_the_gpu_tests_need(w, h, thresholds):
    frames, counts, results = er.oracle_results(w, h, thresholds)
    print(w, h, {k: (v if not isinstance(v, dict) else {t: np.asarray(x).tolist() for t, x in v.items()}) for k, v in counts.items()})
    assert len(frames) == 32
    er.check_census(counts, thresholds)


def test_large_table_set_takes_the_branches():
    """sampling_factor = 0.5: 1762 samples, the launch above 64 KiB of LDS; 0.2 (3692) is beyond the kernel's limit."""
    assert len(er.field_table(0.9)[0]) == 1187 and len(er.field_table(0.5)[0]) == 1762 and len(er.field_table(0.2)[0]) == 3692
    assert 52 * 1187 + 832 <= 65536 < 52 * 1762 + 832
    frames, counts, results = er.oracle_results(960, 540, (5.0,), 0.5, er.KINDS_24)
    print('0.5', {k: (v if not isinstance(v, dict) else {t: np.asarray(x).tolist() for t, x in v.items()}) for k, v in counts.items()})
    assert len(frames) == 24
    er.check_census(counts, (5.0,))


def test_broadcast_cameras_alone_put_nothing_behind():
    """Why the sets above exist: synth.sample_camera (seeds 5000.., the existing GPU test's) never skips a sample."""
    table = er.field_table(0.9)
    cams = er.off_broadcast_cameras('broadcast', 6, 5000)
    counts, _ = er.census([dict(c, f=(c['f'], c['f'])) for c in cams], table, 960, 540)
    assert counts['behind'] == 0
