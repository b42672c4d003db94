"""CPU: the host mirror of the dev-kit's baseline_cameras.py (sncal_amd.baseline_cameras) against tests/golden/line_cameras.npz,
captured from the reference's own functions (tools/make_golden_line_cameras.py).  Decisions (status, number of line matches, the
candidate chosen per 3-D end point) must be identical; values (T1, T2, H, f, R, position) must lie within 4 * max(E_ref, 2^-44)
of the capture in the capture's own measure (max |difference| / max |value|), E_ref being the frame's conditioning: the reference's
own change under input moves of 2^-48 relative.  4 is the project's habitual margin over a reference-derived distance."""
import importlib.util
import json
import os

import numpy as np
import pytest

import line_cameras_cases as lc

ROOT = lc.ROOT


@pytest.fixture(scope='module')
def gold():
    return lc.load()


def _slots(bc, r):
    out = np.full(len(bc.END_POINTS), -1, np.int32)
    for name, s in r['slots'].items():
        out[bc.END_INDEX[name]] = s
    return out


def _check_frame(bc, c, b, r, what=''):
    assert r['status'] == c['status'][b] and r['n_lines'] == c['n_lines'][b], (what, b)
    assert np.array_equal(_slots(bc, r), c['slots'][b]), (what, b)
    assert len(r['matches']) == c['match_n'][b]
    lim = lc.bound(c['E_ref'][b])
    for k in ('T1', 'T2'):
        if not np.isnan(c[k][b]).any():
            assert lc.rel(r[k], c[k][b]) <= lim, (what, b, k)
    if np.isfinite(c['H'][b]).all():
        assert lc.rel(r['H'], c['H'][b]) <= lim, (what, b, 'H', lc.rel(r['H'], c['H'][b]) / lim)
    if r['status']:
        cam = r['camera']
        got = {'f': cam.xfocal_length, 'R': cam.rotation, 'pos': cam.position}
        assert cam.xfocal_length == cam.yfocal_length and cam.principal_point == (c['sizes'][b][0] / 2, c['sizes'][b][1] / 2)
        for k, v in got.items():
            assert lc.rel(v, c[k][b]) <= lim, (what, b, k, lc.rel(v, c[k][b]) / lim)
        for j, (X, uv) in enumerate(r['matches']):
            if what == '':                                              # the reference's order of the matches: the dict's own
                assert np.array_equal(X, c['match_X'][b, j]) and np.array_equal(uv, c['match_uv'][b, j])


@pytest.mark.parametrize('key', ['A', 'B'])
def test_host_flow_equals_the_reference_capture(gold, key):
    from sncal_amd import baseline_cameras as bc
    c = lc.case(gold, key)
    for b in range(c['B']):
        _check_frame(bc, c, b, bc.frame_flow(c['pred'][b], c['sizes'][b]))


def test_the_three_functions_against_the_capture(gold):
    """normalization_transform and estimate_homography_from_line_correspondences on their own, fed as the flow feeds them;
    cameras_from_extremities(refine=False) gives the flow's cameras."""
    from sncal_amd import baseline_cameras as bc
    from sncal_amd.pitch import PITCH_POINTS
    c = lc.case(gold, 'A')
    seen = 0
    cams = bc.cameras_from_extremities(c['pred'], c['sizes'][0], refine=False)
    for b in range(c['B']):
        W, H = c['sizes'][b]
        if c['sizes'][b] == c['sizes'][0]:
            assert (cams[b] is not None) == bool(c['status'][b])
            if cams[b] is not None:
                assert lc.rel(cams[b].position, c['pos'][b]) <= lc.bound(c['E_ref'][b])
        if np.isnan(c['T1'][b]).any():
            continue
        pred = {k: v for k, v in c['pred'][b].items() if k in bc.LINE_ENDS}
        ends = list(dict.fromkeys(e for k in pred for e in bc.LINE_ENDS[k]))
        src = [(p['x'] * W, p['y'] * H) for v in pred.values() for p in v[:2]]
        T1 = bc.normalization_transform([PITCH_POINTS[e][:2] for e in ends])
        T2 = bc.normalization_transform(src)
        lim = lc.bound(c['E_ref'][b])
        assert lc.rel(T1, c['T1'][b]) <= lim and lc.rel(T2, c['T2'][b]) <= lim
        lines = [(bc.pitch_line(k), np.cross([v[0]['x'] * W, v[0]['y'] * H, 1.], [v[1]['x'] * W, v[1]['y'] * H, 1.]))
                 for k, v in pred.items() if bc.on_lawn(k)]
        ok, Hm = bc.estimate_homography_from_line_correspondences(lines, c['T1'][b], c['T2'][b])
        assert ok and lc.rel(Hm, c['H'][b]) <= lim
        seen += 1
    assert seen >= 30
    # the similarity's defining property, and the scale-1 branch of a cloud without extent
    pts = np.array([[3., 4.], [-1., 2.], [7., -5.], [0., 0.]])
    q = (bc.normalization_transform(pts) @ np.c_[pts, np.ones(4)].T).T
    assert np.allclose(q[:, :2].mean(axis=0), 0, atol=1e-15) and abs(np.linalg.norm(q[:, :2], axis=1).mean() - np.sqrt(2)) < 1e-14
    assert np.array_equal(bc.normalization_transform([[2., 3.]] * 3), [[1, 0, -2], [0, 1, -3], [0, 0, 1]])
    assert bc.estimate_homography_from_line_correspondences([(np.ones(3), np.zeros(3))] * 5)[0] is False


def test_a_shuffled_dict_stays_within_the_bound(gold):
    from sncal_amd import baseline_cameras as bc
    c = lc.case(gold, 'A')
    rng = np.random.Generator(np.random.PCG64(5))
    for b in range(c['B']):
        keys = list(c['pred'][b])
        rng.shuffle(keys)
        _check_frame(bc, c, b, bc.frame_flow({k: c['pred'][b][k] for k in keys}, c['sizes'][b]), what='shuffled')


def test_kernel_tables_regenerate_identically():
    spec = importlib.util.spec_from_file_location('make_linecam_tables', os.path.join(ROOT, 'tools', 'make_linecam_tables.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.path()) as f:
        assert f.read() == mod.text()
    from sncal_amd import baseline_cameras as bc
    assert len(bc.END_POINTS) == 34 and len(bc.LINE_ENDS) == 25 and sum(bc.on_lawn(k) for k in bc.LINE_ENDS) == 17


def test_fixture_branches_and_caps(gold):
    a, b = lc.case(gold, 'A'), lc.case(gold, 'B')
    few = a['n_lines'] < 4
    failed = (a['n_lines'] >= 4) & (a['status'] == 0)
    assert few.sum() >= 2 and failed.sum() >= 2
    assert ((a['status'] == 1) & (a['match_n'] <= 3)).sum() >= 2 and ((a['status'] == 1) & (a['match_n'] > 3)).sum() >= 20
    assert ((a['n_lines'] == 4) & (a['status'] == 1)).sum() >= 1                       # the four-line quirk with a camera behind it
    assert int(gold['A.dropped']) <= 0.1 * int(gold['A.drawn'])
    assert a['E_ref'].max() <= 1e-8 and b['E_ref'].max() <= 1e-8
    assert set(a['sizes']) == {(960, 540), (1283, 721)} and set(np.unique(a['noise'])) == {0.5, 1.0, 2.0, 4.0}
    assert 40 <= a['B'] <= 56
    assert b['status'].tolist() == [0, 0, 0, 0, 1, 0, 1, 0, 1, 1] and b['n_lines'][:4].tolist() == [0, 3, 4, 0]
    assert np.isfinite(b['H'][2]).all() and np.isnan(b['H'][5]).all() and np.isnan(b['H'][7]).all()
    assert np.isnan(b['packed'][0]).sum() == 1


@pytest.mark.parametrize('key', ['A', 'B'])
def test_pack_and_unpack_of_both_forms(gold, key, tmp_path):
    from sncal_amd.annotations import pack_annotations
    from sncal_amd.extremities import peaks_to_extremities, save_extremities
    c = lc.case(gold, key)
    pts, off, _ = pack_annotations(c['pred'])
    assert np.array_equal(pts, c['packed'][0], equal_nan=True) and np.array_equal(off, c['packed'][1])
    for b in range(c['B']):
        if not c['peaks_ok'][b]:
            continue
        d = peaks_to_extremities(c['peaks'][b], c['sizes'][b], c['p_threshold'], scale=c['scale'])
        one = pack_annotations([d])
        want = pack_annotations([c['pred'][b]])
        assert np.array_equal(one[0], want[0], equal_nan=True) and np.array_equal(one[1], want[1])
        path = str(tmp_path / f'extremities_{b}.json')
        save_extremities(d, path)
        with open(path) as f:
            back = pack_annotations([json.load(f)])
        assert np.array_equal(back[0], want[0], equal_nan=True) and np.array_equal(back[1], want[1])
    assert c['peaks_ok'].sum() >= c['B'] - 1
