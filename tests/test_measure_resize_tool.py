"""CPU: tools/measure_resize.py -- its report writer reproduces the committed report from the committed figures byte for byte, and its
trace reader tells the four kernels of a rocprofv3 kernel trace apart by name, template flag and grid."""
import csv
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('measure_resize', os.path.join(ROOT, 'tools', 'measure_resize.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_write_md_reproduces_the_committed_report(tmp_path):
    mod = _tool()
    stem = os.path.join(ROOT, 'profiles', 'resize')
    with open(stem + '.json') as f:
        rep = json.load(f)
    mod.write_md(rep, str(tmp_path / 'r.md'))
    with open(tmp_path / 'r.md', newline='') as got, open(stem + '.md', newline='') as want:
        assert got.read() == want.read()
    assert rep['notes'] == mod.NOTES and len(rep['kernel_trace']) == 8 and len(rep['cells']) == 4
    assert rep['bench']['parent']['min'] <= rep['bench']['this']['median'] <= rep['bench']['parent']['max']


def test_read_trace_groups_by_path_shape_and_batch(tmp_path):
    mod = _tool()
    rows, t = [], 1000
    for name, B, us in (('resize_wide_kernel<false>', 16, 40), ('resize_byte_kernel<false>', 16, 50), ('resize_wide_kernelILb1EE', 64, 120),
                        ('other_kernel', 16, 7)):
        for k in range(3):
            rows.append({'Kernel_Name': f'void (anonymous namespace)::{name}(unsigned char const*)', 'Start_Timestamp': t,
                         'End_Timestamp': t + (us + (100 if k == 0 else 0)) * 1000, 'Grid_Size_X': 2048 * 256 // B, 'Grid_Size_Y': B,
                         'Workgroup_Size_X': 256, 'Workgroup_Size_Y': 1})
            t += 10 ** 6
    d = tmp_path / 'trace' / 'host'
    d.mkdir(parents=True)
    with open(d / '1_kernel_trace.csv', 'w', newline='') as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    res = mod.read_trace(str(tmp_path / 'trace'))
    assert list(res) == ['720x1280 -> 540x960 B=16 wide path', '720x1280 -> 540x960 B=16 byte path', '1080x1920 -> 540x960 B=64 wide path']
    wide = res['720x1280 -> 540x960 B=16 wide path']
    assert wide['median_ms'] == 0.04 and wide['calls'] == 2                              # the first, cold call is left out
    assert wide['algorithmic_bytes'] == 16 * 3 * (720 * 1280 + 540 * 960)
    assert res['1080x1920 -> 540x960 B=64 wide path']['algorithmic_bytes'] == 64 * 3 * (1080 * 1920 + 540 * 960)
