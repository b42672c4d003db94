"""GPU: sncal_baseline_cameras (csrc/linecam.hip) and what stands on it -- line_cameras, the folder CLI, the one-pass form -- against
tests/golden/line_cameras.npz, captured from the reference's own functions (tools/make_golden_line_cameras.py).
refine=0: decisions (status, line matches, chosen candidates) identical, values within 4 * max(E_ref, 2^-44) of the capture
(tests/test_line_cameras_host.py explains the bound).  refine=1: the refined pose is scipy's minimum from the captured start on the
captured matches, at the bounds tests/test_solve_scipy_gpu.py holds sncal_pnp_refine_lm to."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import line_cameras_cases as lc
from oracle import hrnet_ref as hr

pytestmark = pytest.mark.gpu

NAMES = ('cams', 'status', 'H', 'n_lines', 'slots')


@pytest.fixture(scope='module')
def gold():
    return lc.load()


def run(sncal, cuda, c, idx=None, form='packed', refine=False):
    """The kernel on the frames `idx` of a case (one call per image size, frames in the order given) -> dict of numpy arrays, one
    row per frame of idx."""
    bc = sncal.baseline_cameras
    idx = list(range(c['B'])) if idx is None else list(idx)
    rec = ctypes.sizeof(sncal._lib.Camera)
    out = {'cams': np.zeros((len(idx), rec), np.uint8), 'status': np.zeros(len(idx), np.int32), 'H': np.zeros((len(idx), 9)),
           'n_lines': np.zeros(len(idx), np.int32), 'slots': np.zeros((len(idx), len(bc.END_POINTS)), np.int32)}
    for size in dict.fromkeys(c['sizes'][i] for i in idx):
        at = [k for k, i in enumerate(idx) if c['sizes'][i] == size]                        # (a frame may occur more than once)
        ids = [idx[k] for k in at]
        kw = dict(img_size=size, refine=refine, scale=c['scale'], p_threshold=c['p_threshold'])
        if form == 'peaks':
            got = bc.line_cameras(peaks=torch.from_numpy(c['peaks'][ids]).to(cuda), **kw)
        else:
            got = bc.line_cameras(pred_annots=[c['pred'][i] for i in ids], device=cuda, **kw)
        assert [o.dtype for o in got] == [torch.uint8, torch.int32, torch.float64, torch.int32, torch.int32] and all(o.is_cuda for o in got)
        for name, o in zip(NAMES, got):
            out[name][at] = o.cpu().numpy()
    return out


def records(sncal, out):
    return [sncal._lib.Camera.from_buffer_copy(r.tobytes()) for r in out['cams']]


def values(rec):
    return {'f': rec.fx, 'R': np.array(rec.rotation[:]), 'pos': np.array(rec.position[:])}


@pytest.fixture(scope='module')
def full(sncal, cuda, gold):
    """Sets A and B through the kernel once, packed form, refine=0: what the other tests compare against."""
    return {key: (lc.case(gold, key), run(sncal, cuda, lc.case(gold, key))) for key in ('A', 'B')}


@pytest.mark.parametrize('key', ['A', 'B'])
def test_kernel_equals_the_reference_capture(sncal, full, key):
    c, out = full[key]
    assert np.array_equal(out['status'], c['status']) and np.array_equal(out['n_lines'], c['n_lines'])
    assert np.array_equal(out['slots'], c['slots'])
    worst = {}
    for b, rec in enumerate(records(sncal, out)):
        raw = np.frombuffer(out['cams'][b].tobytes(), np.float64, 17)
        assert np.isfinite(raw).all() and np.isfinite(out['H'][b]).all()                  # nothing returns NaN in a record
        assert rec.status == c['status'][b] and rec.n_points == c['match_n'][b]
        if not c['status'][b]:
            assert not out['cams'][b].any() and (out['slots'][b] == -1).all()
        got = {'H': out['H'][b], **values(rec)} if c['status'][b] else {'H': out['H'][b]}
        ref = {k: c[k][b] for k in got if np.isfinite(c[k][b]).all()}
        if 'H' not in ref:
            assert not out['H'][b].any()
        for k in ref:
            share = lc.rel(got[k], ref[k]) / lc.bound(c['E_ref'][b])
            worst[k] = max(worst.get(k, 0.0), share)
            print(f'{key}[{b}] {k}: share of the bound {share:.3f}')
        if c['status'][b]:
            W, H = c['sizes'][b]
            assert (rec.cx, rec.cy) == (W / 2, H / 2) and rec.fx == rec.fy
            uv = c['match_uv'][b, :c['match_n'][b]]
            X = c['match_X'][b, :c['match_n'][b]]
            if len(X):
                Xc = (X - np.array(rec.position[:])) @ np.array(rec.rotation[:]).reshape(3, 3).T
                q = np.stack([rec.fx * Xc[:, 0] / Xc[:, 2] + rec.cx, rec.fy * Xc[:, 1] / Xc[:, 2] + rec.cy], axis=1)
                assert abs(rec.rmse - np.linalg.norm(q - uv, axis=1).mean()) <= 1e-9 * max(rec.rmse, 1.0)
            else:
                assert rec.rmse == 0.0
    print('largest share of the bound per quantity:', worst)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_refined_pose_is_scipys_minimum_on_the_captured_matches(sncal, cuda, gold):
    """refine=1 against scipy.optimize.least_squares (MINPACK lmder) from the captured start on the captured matches, at the bounds
    of tests/test_solve_scipy_gpu.py::test_pnp_refine_lm_returns_scipys_minimum."""
    scipy_opt = pytest.importorskip('scipy.optimize')
    Rot = pytest.importorskip('scipy.spatial.transform').Rotation
    c = lc.case(gold, 'A')
    out = run(sncal, cuda, c, refine=True)
    plain = run(sncal, cuda, c, refine=False)
    assert np.array_equal(out['slots'], c['slots']) and np.array_equal(out['n_lines'], c['n_lines']) and np.array_equal(out['H'], plain['H'])
    want = np.where(c['status'] == 0, 0, np.where(c['match_n'] > 3, 2, 1))
    assert np.array_equal(out['status'], want) and (want == 2).sum() >= 20 and (want == 1).sum() >= 2
    checked = 0
    for b, rec in enumerate(records(sncal, out)):
        if want[b] != 2:
            assert np.array_equal(out['cams'][b], plain['cams'][b])                        # not refined: the record of refine=0
            continue
        n = c['match_n'][b]
        X, uv, f = c['match_X'][b, :n], c['match_uv'][b, :n], c['f'][b]
        W, H = c['sizes'][b]
        R0, pos0 = c['R'][b].reshape(3, 3), c['pos'][b]

        def proj(R, t):
            Xc = X @ R.T + t
            return np.stack([f * Xc[:, 0] / Xc[:, 2] + W / 2, f * Xc[:, 1] / Xc[:, 2] + H / 2], axis=1)

        def res(p):
            return (proj(Rot.from_rotvec(p[:3]).as_matrix() @ R0, p[3:]) - uv).ravel()
        sp = scipy_opt.least_squares(res, np.r_[0, 0, 0, -R0 @ pos0], method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
        for _ in range(3):                    # MINPACK may stop in the flat valley of a few collinear matches: restarted from its own
            again = scipy_opt.least_squares(res, sp.x, method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)      # answer
            if not again.cost < sp.cost:
                break
            sp = again
        R, pos = np.array(rec.rotation[:]).reshape(3, 3), np.array(rec.position[:])
        r_hip = (proj(R, -R @ pos) - uv).ravel()
        l2 = lambda r: float(np.linalg.norm(r.reshape(-1, 2), axis=1).mean())             # noqa: E731
        c_hip, c_sp = float(r_hip @ r_hip), 2 * sp.cost
        print(f'A[{b}] n {n}: cost hip {c_hip:.9g} scipy {c_sp:.9g}; mean L2 hip {l2(r_hip):.9g} scipy {l2(sp.fun):.9g}; rmse {rec.rmse:.9g}')
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        assert c_hip <= c_sp * (1 + 1e-6) and c_hip >= c_sp * (1 - 1e-9), (b, c_hip, c_sp)
        assert abs(l2(r_hip) - l2(sp.fun)) <= 1e-4 * l2(sp.fun), (b, l2(r_hip), l2(sp.fun))
        assert abs(rec.rmse - l2(r_hip)) <= 1e-9 * rec.rmse
        assert rec.n_points == n and rec.status == 2 and rec.fx == plain_fx(sncal, plain, b)
        checked += 1
    assert checked >= 20


def plain_fx(sncal, plain, b):
    return sncal._lib.Camera.from_buffer_copy(plain['cams'][b].tobytes()).fx


@pytest.mark.parametrize('key', ['A', 'B'])
def test_peaks_form_and_json_route_are_byte_identical(sncal, cuda, full, key, tmp_path):
    from sncal_amd.extremities import peaks_to_extremities, save_extremities
    c, out = full[key]
    idx = [b for b in range(c['B']) if c['peaks_ok'][b]]
    assert len(idx) >= c['B'] - 1
    pk = run(sncal, cuda, c, idx, form='peaks')
    back = dict(c)
    back['pred'] = list(c['pred'])
    for b in idx:
        path = str(tmp_path / f'extremities_{b:05d}.json')
        save_extremities(peaks_to_extremities(c['peaks'][b], c['sizes'][b], c['p_threshold'], scale=c['scale']), path)
        with open(path) as f:
            back['pred'][b] = json.load(f)
    js = run(sncal, cuda, back, idx)
    for name in NAMES:
        assert np.array_equal(pk[name], out[name][idx]), name
        assert np.array_equal(js[name], out[name][idx]), name


@pytest.mark.parametrize('refine', [False, True])
def test_a_frame_does_not_depend_on_its_batch(sncal, cuda, gold, full, refine):
    c = lc.case(gold, 'A')
    whole = run(sncal, cuda, c, refine=True) if refine else full['A'][1]
    rng = np.random.Generator(np.random.PCG64(3))
    size = c['sizes'][0]
    same = [b for b in range(c['B']) if c['sizes'][b] == size]
    groups = [[b] for b in same[:4]] + [same[4:7], [int(v) for v in rng.permutation(np.resize(same, 67))]]
    assert [len(g) for g in groups[-2:]] == [3, 67]
    for g in groups:
        got = run(sncal, cuda, c, g, refine=refine)
        for name in NAMES:
            assert np.array_equal(got[name], whole[name][g]), (name, len(g))


def test_argument_errors_and_the_empty_batch(sncal, cuda):
    bc, L = sncal.baseline_cameras, sncal._lib
    lib = L.lib()
    out = bc.line_cameras(pred_annots=[], device=cuda)
    assert [tuple(o.shape) for o in out] == [(0, ctypes.sizeof(L.Camera)), (0,), (0, 9), (0,), (0, 34)]
    out = bc.line_cameras(peaks=torch.zeros((0, 23, 2, 3), device=cuda))
    assert out[1].numel() == 0
    with pytest.raises(L.SncalError, match='C=24'):
        bc.line_cameras(peaks=torch.zeros((1, 24, 2, 3), device=cuda))
    with pytest.raises(L.SncalError, match='two slots'):
        bc.line_cameras(peaks=torch.zeros((1, 23, 3, 3), device=cuda))
    with pytest.raises(L.SncalError, match='exactly one'):
        bc.line_cameras()
    one = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    p = one.data_ptr()
    args = (p, 23, 4.0, 0.2, None, 0, None, 1, 28, 960, 540, 0)
    assert lib.sncal_baseline_cameras(*args, p, p, p, p, None, 34, None) == -1 and b'null output' in lib.sncal_last_error()
    assert lib.sncal_baseline_cameras(*args, p, p, p, p, p, 33, None) == -1 and b'n_slots' in lib.sncal_last_error()
    assert lib.sncal_baseline_cameras(p, 23, 4.0, 0.2, p, 0, p, 1, 28, 960, 540, 0, p, p, p, p, p, 34, None) == -1
    assert lib.sncal_baseline_cameras(None, 0, 4.0, 0.2, None, 0, None, 0, 28, 960, 540, 0, None, None, None, None, None, 34, None) == 0
    assert lib.sncal_version() == 100


def test_folder_cli_writes_what_the_host_flow_writes(sncal, cuda, gold, tmp_path, capsys):
    """python -m sncal_amd.baseline_cameras -s ... -p ... on a split of 6 frames, one prediction file missing: the JSON of
    cameras_from_extremities + save_cameras, and CameraEvaluator scores the folder."""
    bc, interop = sncal.baseline_cameras, sncal.interop
    from sncal_amd.extremities import save_extremities
    c = lc.case(gold, 'A')
    size = (960, 540)
    ids = [b for b in range(c['B']) if c['sizes'][b] == size and c['status'][b] == 1 and c['match_n'][b] > 3][:4]
    ids += [b for b in range(c['B']) if c['sizes'][b] == size and c['status'][b] == 0][:2]
    assert len(ids) == 6
    split, preds = tmp_path / 'data' / 'valid', tmp_path / 'pred' / 'valid'
    os.makedirs(split), os.makedirs(preds)
    names = [f'{i:05d}' for i in range(6)]
    with open(split / 'per_match_info.json', 'w') as f:
        json.dump({'match_a': {n + '.jpg': {} for n in names[:3]}, 'match_b': {n + '.jpg': {} for n in names[3:]}}, f)
    missing = 2
    for k, b in enumerate(ids):
        if k != missing:
            save_extremities(c['pred'][b], str(preds / f'extremities_{names[k]}.json'))
    n = bc.main(['-s', str(tmp_path / 'data'), '-p', str(tmp_path / 'pred')])
    assert n == 3 and f'{n} cameras written' in capsys.readouterr().out
    have = [k for k in range(6) if k != missing]
    cams = bc.cameras_from_extremities([c['pred'][ids[k]] for k in have], size)
    assert interop.save_cameras(cams, [names[k] + '.jpg' for k in have], str(tmp_path / 'host')) == 3
    written = sorted(p for p in os.listdir(preds) if p.startswith('camera_'))
    assert written == sorted(os.listdir(tmp_path / 'host')) == [f'camera_{names[k]}.json' for k in (0, 1, 3)]
    for p in written:
        got, want = json.load(open(preds / p)), json.load(open(tmp_path / 'host' / p))
        assert list(got) == list(want)
        for key in want:
            # the same minimiser on the same matches from starts that differ by rounding: the north-star tolerance of the camera parameters
            assert np.allclose(got[key], want[key], rtol=1e-4, atol=1e-4), (p, key, got[key], want[key])
    # CameraEvaluator scores the folder: the records behind the files against the frames' own extremities as annotations
    cams_d, status = bc.line_cameras(pred_annots=[c['pred'][ids[k]] for k in have], img_size=size, device=cuda)[:2]
    for cam, p in zip([x for x in bc.records_to_cameras(cams_d, status, size) if x is not None], written):
        assert json.load(open(preds / p)) == json.loads(json.dumps(cam.to_json_parameters()))
    ev = sncal.evaluate.CameraEvaluator(cuda, *size, threshold=20.0)
    res = ev.summarize(ev.evaluate(cams_d, [sncal.evaluate.scale_points(c['pred'][ids[k]], *size) for k in have]))
    assert res['completeness'] == 3 / 5 and 0.5 < res['accuracy'] <= 1.0, res


LOSS = {'num_refinement_stages': 0, 'gmse_w': 1.0, 'awing_w': 1.0, 'sigma': 4}


@pytest.fixture(scope='module')
def line_model(sncal, cuda, tmp_path_factory, gold_dir):
    """The smallest designed line network of the line tests: W18 on the 64 x 96 golden's weights (tests/test_extremities_gpu.py)."""
    g = np.load(os.path.join(gold_dir, 'line_w18_64x96.npz'))
    cfg = hr.load_config('line_hrnet_w18')
    bare = {k: v for k, v in cfg.items() if k not in ('head', 'upscale')}
    ck = {'model_name': 'EHMMetaModel',
          'params': {'nn_module': {'hrnet_config': bare, 'num_refinement_stages': 0, 'num_heatmaps': 23}, 'loss': dict(LOSS),
                     'prediction_transform': {'scale': 4, 'sigma': 6}, 'device': 'cuda:0'},
          'nn_state_dict': hr.seeded_state_dict(cfg, int(g['seed']), float(g['head_gain']))}
    path = str(tmp_path_factory.mktemp('line_cam') / 'line.pth')
    torch.save(ck, path)
    return path


def test_one_pass_form_equals_line_cameras_on_the_decoded_peaks(sncal, cuda, line_model, gold_dir, tmp_path):
    bc = sncal.baseline_cameras
    jpg = np.load(os.path.join(gold_dir, 'jpeg_cases.npz'))
    os.makedirs(tmp_path / 'img')
    for i in range(5):
        with open(tmp_path / 'img' / f'{i:05d}.jpg', 'wb') as f:
            f.write(jpg['jpg.full'].tobytes())
    model = sncal.load_model(line_model, device='cuda:0', dtype='fp32')
    seen = []
    n = bc.line_model_cameras(str(tmp_path / 'img'), model, str(tmp_path / 'out'), batch_size=3, conf_threshold=0.01, collect=seen)
    assert [len(s[0]) for s in seen] == [3, 2]
    total = 0
    for names, peaks, cams, status in seen:
        assert peaks.is_cuda and tuple(peaks.shape[1:]) == (23, 2, 3)
        size = (960, 540)
        again = bc.line_cameras(peaks=peaks, img_size=size, scale=1, p_threshold=0.01)
        host = bc.line_cameras(pred_annots=[sncal.extremities.peaks_to_extremities(p, size, 0.01) for p in peaks.cpu().numpy()],
                               img_size=size, device=cuda)
        assert torch.equal(cams, again[0]) and torch.equal(status, again[1])
        assert torch.equal(cams, host[0]) and torch.equal(status, host[1])
        total += int((status != 0).sum())
    assert n == total == len(os.listdir(tmp_path / 'out'))
    # the command line's one-pass form
    assert bc.main(['--line-model', line_model, '--img-dir', str(tmp_path / 'img'), '--save-dir', str(tmp_path / 'cli')]) in range(6)
