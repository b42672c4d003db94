"""CPU: the parts of tools/bench_validate.py that need no device -- reading a rocprofv3 kernel trace and writing the report."""
import csv
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('bench_validate', os.path.join(ROOT, 'tools', 'bench_validate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trace_reader_and_report(tmp_path):
    bv = _tool()
    d = tmp_path / 'trace' / 'host' / '1234'
    d.mkdir(parents=True)
    name = {3: 'void (anonymous namespace)::loss_kernel<4, true, true, false>(float const*)', 7: '_ZN12_GLOBAL__N_111loss_kernelILi4ELb1ELb1ELb1EEEvPKf'}
    with open(d / '1234_kernel_trace.csv', 'w', newline='') as f:
        w = csv.DictWriter(f, fieldnames=['Kind', 'Kernel_Name', 'Start_Timestamp', 'End_Timestamp', 'Workgroup_Size_Z', 'Grid_Size_Z'])
        w.writeheader()
        t = 1000
        for B in (16, 64):
            for terms in (3, 7):
                for call in range(5):
                    ns = (9_000_000 if call == 0 else 1_000_000 + 1000 * call) * (B // 16)        # a cold first call
                    w.writerow({'Kind': 'KERNEL_DISPATCH', 'Kernel_Name': name[terms], 'Start_Timestamp': t, 'End_Timestamp': t + ns,
                                'Workgroup_Size_Z': 1, 'Grid_Size_Z': B})
                    t += ns + 500
        w.writerow({'Kind': 'KERNEL_DISPATCH', 'Kernel_Name': 'loss_fold_kernel', 'Start_Timestamp': t, 'End_Timestamp': t + 5, 'Workgroup_Size_Z': 1,
                    'Grid_Size_Z': 1})
    got = bv.read_trace(str(tmp_path / 'trace'))
    assert sorted(got) == ['mse+kl B=16', 'mse+kl B=64', 'mse+kl+awing B=16', 'mse+kl+awing B=64']
    r = got['mse+kl B=16']
    assert r['calls'] == 4 and abs(r['median_ms'] - 1.0025) < 1e-9 and r['max_ms'] < 2           # the cold call is left out
    bytes16 = 16 * 58 * 270 * 480 * 4
    assert abs(r['share_of_hbm_roof'] - round(bytes16 / (r['median_ms'] * 1e-3) / 6.3e12, 3)) < 1e-9
    assert abs(got['mse+kl B=64']['median_ms'] - 4.01) < 1e-9
    cell = {'shape': [16, 58, 270, 480], 'weights': 'default (l2 1, kldiv 1)', 'speedup_median': 3.0, 'fused_peak_temp_bytes': 2 ** 21,
            'composed_peak_temp_bytes': 2 ** 30, 'fused_call_share_of_hbm_roof': 0.4,
            'fused': {'median_ms': 1.0, 'p10_ms': 0.9, 'p90_ms': 1.1, 'reps': 24}, 'composed': {'median_ms': 3.0, 'p10_ms': 2.9, 'p90_ms': 3.1, 'reps': 24}}
    rep = {'device': 'test device', 'build': 'label-1', 'ab': [cell], 'kernel_trace': got, 'validate': None}
    bv.write_md(rep, str(tmp_path / 'r.md'))
    text = open(tmp_path / 'r.md').read()
    assert 'Build: label-1' in text and '| 16 | default (l2 1, kldiv 1) | 1.0 (0.9-1.1) | 3.0 (2.9-3.1) | 3.0x | 2.0 MiB | 1024 MiB | 0.4 |' in text
    assert '| mse+kl B=16 | 1.0025 ' in text and text.rstrip().endswith('not measured')           # no validate() rates in this report
