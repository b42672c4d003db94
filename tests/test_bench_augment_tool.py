"""CPU: the parts of tools/bench_augment.py that need no device -- reading a kernel trace and writing the report."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        spec = importlib.util.spec_from_file_location('bench_augment', os.path.join(ROOT, 'tools', 'bench_augment.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    return mod


def test_kernel_trace_reader(tmp_path):
    ba = _tool()
    d = tmp_path / 'trace' / 'host' / '1'
    d.mkdir(parents=True)
    n = 16 * 540 * 960 * 3
    rows, t = ['Kernel_Name,Grid_Size_Y,Workgroup_Size_Y,Start_Timestamp,End_Timestamp'], 1000
    for call in range(12):                                               # six uint8 calls, then six fp32 CHW calls
        for name, us in (('augment_sums_kernel', 10), ('augment_apply_wide_kernel', 100 if call < 6 else 200)):
            if call in (0, 6):
                us *= 5                                                   # the cold call, which the reader drops
            rows.append(f'"_ZN12_GLOBAL__N_1{name}E",16,1,{t},{t + us * 1000}')
            t += us * 1000 + 500
    rows.append(f'"some_other_kernel",16,1,{t},{t + 5}')
    (d / '1_kernel_trace.csv').write_text('\n'.join(rows))
    got = ba.read_trace(str(tmp_path / 'trace'))
    assert sorted(got) == ['apply fp32 CHW B=16', 'apply uint8 B=16', 'sums B=16']
    assert got['apply uint8 B=16']['median_ms'] == 0.1 and got['apply uint8 B=16']['calls'] == 5
    assert got['apply uint8 B=16']['algorithmic_bytes'] == 6 * n and got['apply fp32 CHW B=16']['algorithmic_bytes'] == 15 * n
    assert got['sums B=16']['algorithmic_bytes'] == 3 * n and got['sums B=16']['calls'] == 11
    assert got['apply fp32 CHW B=16']['share_of_hbm_roof'] == round(15 * n / 0.2e-3 / 6.3e12, 3)


def test_report_writer(tmp_path):
    ba = _tool()
    st = {'median_ms': 2.0, 'p10_ms': 1.9, 'p90_ms': 2.1, 'reps': 16}
    cell = {'shape': [16, 540, 960, 3], 'output': 'uint8', 'speedup_median': 0.8, 'fused_frames_per_s': 8000, 'fused_peak_temp_bytes': 2 ** 25,
            'composed_peak_temp_bytes': 2 ** 31, 'fused': st, 'composed': dict(st, median_ms=1.6)}
    rep = {'device': 'test device', 'build': 'label-1', 'cells': [cell], 'cpu_frames_per_s': 12.34}
    ba.write_md(rep, str(tmp_path / 'r.md'))
    text = open(tmp_path / 'r.md').read()
    # a fused call that is NOT faster is reported as it is
    assert 'Build: label-1' in text
    assert '| (16, 540, 960, 3) | uint8 | 2.0 (1.9-2.1) | 1.6 (1.9-2.1) | 0.8x | 8000 | 32.0 MiB | 2048 MiB |' in text
    assert '12.3 frames/s per process' in text
    assert text.rstrip().endswith('not measured')                         # no kernel trace in this report
    rep['kernel_trace'] = {'apply uint8 B=16': {'median_ms': 0.3, 'min_ms': 0.29, 'max_ms': 0.31, 'calls': 4, 'share_of_hbm_roof': 0.5}}
    ba.write_md(rep, str(tmp_path / 'r.md'))
    assert '| apply uint8 B=16 | 0.3 (0.29-0.31) | 4 | 0.5 |' in open(tmp_path / 'r.md').read()
