"""CPU: the packaged hrnet_w48x4 / hrnet_w64 configs, the reference capture of the x4 network against the oracle, and the parts of
tools/bench_upscale4.py that need no device."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import decode as od
from oracle import hrnet_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packaged_configs_carry_the_references_fields():
    import sncal_amd
    cfg = sncal_amd.load_config('hrnet_w48x4')
    assert cfg['upscale'] == 4 and cfg['num_classes'] == 58 and cfg['head'] == 'logsoftmax'
    assert cfg['stage2']['num_channels'] == [48, 96] and cfg['stage3']['num_channels'] == [48, 96, 192]
    assert cfg['stage4']['num_channels'] == [48, 96, 192, 384]
    w48 = sncal_amd.load_config('hrnet_w48')
    assert {k: v for k, v in cfg.items() if k != 'upscale'} == {k: v for k, v in w48.items() if k != 'upscale'}      # the reference's two yamls differ in that field alone
    assert sncal_amd.hrnet._desc(cfg).upscale == 4
    w64 = sncal_amd.load_config('hrnet_w64')
    assert w64['upscale'] == 2 and w64['stage4']['num_channels'] == [64, 128, 256, 512] and w64['stage2']['num_channels'] == [64, 128]
    assert {k: v for k, v in w64.items() if not k.startswith('stage')} == {k: v for k, v in w48.items() if not k.startswith('stage')}
    assert hr.load_config('hrnet_w48x4') == cfg and hr.load_config('hrnet_w64') == w64


@pytest.mark.parametrize('hw', ['64x96', '70x102'])
def test_reference_capture_equals_the_oracle(gold_dir, hw):
    """tests/golden/hrnet_w48x4.npz (the reference's own HRNetHeatmap, tools/make_golden_upscale4.py) against hr.forward on the same
    seeds: samples within 1e-4, decode indices identical, and the decode gap the seed was chosen for (>= 1e-3)."""
    g = np.load(os.path.join(gold_dir, 'hrnet_w48x4.npz'))
    H, W = (int(v) for v in hw.split('x'))
    assert [H, W] in g['sizes'].tolist()
    cfg = hr.load_config('hrnet_w48x4')
    sd = hr.seeded_state_dict(cfg, int(g['seed']), float(g['head_gain']))
    out = hr.forward(sd, hr.seeded_input(1, H, W, int(g['seed']) + 1), cfg).numpy()
    b0 = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    assert out.shape == (1, 58, 4 * b0[0], 4 * b0[1])
    chans = g[hw + '.full_channels']
    assert chans.tolist() == [0, 8, 16, 24, 32, 40, 48, 56, 57]
    assert np.abs(out[:, :, ::4, ::4] - g[hw + '.out_strided']).max() < 1e-4
    assert np.abs(out[:, chans] - g[hw + '.full']).max() < 1e-4
    assert abs(float(np.sum(out.astype(np.float64))) - float(g[hw + '.checksum'])) < 1e-4 * out.size
    dec = od.keypoint_decode(out, (540, 960))
    assert np.array_equal(dec[..., :2], g[hw + '.decode'][..., :2])
    assert np.abs(dec[..., 2] - g[hw + '.decode'][..., 2]).max() < 1e-5
    assert np.abs(np.exp(out).max(axis=(2, 3)) - g[hw + '.maxp']).max() < 1e-5
    assert float(g[hw + '.gap']) >= 1e-3
    assert os.path.getsize(os.path.join(gold_dir, 'hrnet_w48x4.npz')) < 1 << 20


def _tool():
    spec = importlib.util.spec_from_file_location('bench_upscale4', os.path.join(ROOT, 'tools', 'bench_upscale4.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_tool_report_writer(tmp_path):
    bu = _tool()
    assert bu.head_macs_per_frame(270, 480) * 4 == bu.head_macs_per_frame(540, 960) == 540 * 960 * 800 * (208 + 32 + 64)
    st = {'median_ms': 100.0, 'p10_ms': 99.0, 'p90_ms': 101.0, 'reps': 5}
    rows = [{'variant': 'x4 fused', 'config': 'hrnet_w48x4', 'batch': 16, 'forward_ms': st, 'frames_per_s': 160.0, 'workspace_bytes': 3 << 30,
             'head_kernel': 'headx4_fused', 'head_ms_per_call': 10.5},
            {'variant': 'x4 SNCAL_FUSED_HEAD=0', 'config': 'hrnet_w48x4', 'batch': 16, 'forward_ms': dict(st, median_ms=400.0), 'frames_per_s': 40.0,
             'workspace_bytes': 5 << 30, 'head_kernel': None, 'head_ms_per_call': None},
            {'variant': 'x2', 'config': 'hrnet_w48', 'batch': 16, 'forward_ms': dict(st, median_ms=50.0), 'frames_per_s': 320.0, 'workspace_bytes': 1 << 30,
             'head_kernel': 'headx3_fused', 'head_ms_per_call': 2.6}]
    rep = {'device': 'test device', 'build': 'label-1', 'engine': 'fp16x3', 'size': [540, 960], 'rows': rows, 'bench': None}
    path = str(tmp_path / 'u.md')
    bu.write_md(rep, path)
    text = open(path).read()
    assert 'Build: label-1' in text
    assert '| x4 fused | hrnet_w48x4 | 16 | 100.0 (99.0-101.0) | 160.0 | 3.00 | headx4_fused | 10.5 |' in text
    assert '| x4 SNCAL_FUSED_HEAD=0 | hrnet_w48x4 | 16 | 400.0 (99.0-101.0) | 40.0 | 5.00 | - | - |' in text
    assert 'bench.py lines were not recorded' in text
    rep['bench'] = {'parent': {'value': 500.0}, 'this': {'value': 505.0}}
    bu.write_md(rep, path)
    text = open(path).read()
    assert '| parent commit | 500.0 |' in text and '| this commit | 505.0 |' in text and '+1.00 %' in text and 'inside' in text
    rep['bench']['this']['value'] = 480.0
    bu.write_md(rep, path)
    assert '-4.00 %' in open(path).read() and 'OUTSIDE' in open(path).read()
