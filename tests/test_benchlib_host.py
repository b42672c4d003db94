"""CPU: tools/benchlib.py, the measurement method of the tools/bench_*.py report tools -- the kernel-trace reader, the template-flag
parser, stats() and the trace plumbing, on synthetic traces; and that the tools keep one owner for each of them."""
import csv
import glob
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ['Kind', 'Kernel_Name', 'Start_Timestamp', 'End_Timestamp', 'Workgroup_Size_Y', 'Grid_Size_Y']


@pytest.fixture(scope='module')
def bl():
    spec = importlib.util.spec_from_file_location('benchlib', os.path.join(ROOT, 'tools', 'benchlib.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trace(path, rows, fields=FIELDS):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w', newline='') as f:
        w = csv.DictWriter(f, fieldnames=fields)
        w.writeheader()
        for name, start, end in rows:
            w.writerow({k: v for k, v in {'Kind': 'KERNEL_DISPATCH', 'Kernel_Name': name, 'Start_Timestamp': start, 'End_Timestamp': end,
                                          'Workgroup_Size_Y': 1, 'Grid_Size_Y': 16}.items() if k in fields})


def test_rows_of_two_files_in_start_order_filtered_by_name(bl, tmp_path):
    # the later dispatches sit in the file glob finds first, and inside a file the rows are not in time order either
    _trace(str(tmp_path / 'a' / '1' / '1_kernel_trace.csv'), [('alpha_kernel<4>', 5000, 5100), ('beta_kernel', 7000, 7300), ('gamma_kernel', 6000, 6100)])
    _trace(str(tmp_path / 'b' / '2_kernel_trace.csv'), [('beta_kernel', 3000, 3200), ('alpha_kernel<4>', 1000, 1400), ('delta_kernel', 2000, 2100)])
    _trace(str(tmp_path / 'b' / '2_kernel_stats.csv'), [('alpha_kernel<4>', 1, 2)])                    # not a trace: never read
    rows = bl.trace_rows(str(tmp_path), 'alpha_', 'beta_')
    assert [(r['Kernel_Name'], int(r['Start_Timestamp'])) for r in rows] == [('alpha_kernel<4>', 1000), ('beta_kernel', 3000), ('alpha_kernel<4>', 5000),
                                                                            ('beta_kernel', 7000)]
    assert [bl.duration_ms(r) for r in rows] == [400 * 1e-6, 200 * 1e-6, 100 * 1e-6, 300 * 1e-6]
    assert [r['Kernel_Name'] for r in bl.trace_rows(str(tmp_path), 'gamma')] == ['gamma_kernel']
    assert bl.trace_rows(str(tmp_path), 'no_such_kernel') == [] and bl.trace_rows(str(tmp_path / 'nowhere'), 'alpha_') == []


def test_cold_call_dropped_only_when_there_is_another(bl):
    assert bl.call_stats([9.0, 1.00004, 3.0, 2.0]) == {'median_ms': 2.0, 'min_ms': 1.0, 'max_ms': 3.0, 'calls': 3}
    assert bl.call_stats([9.0, 1.25]) == {'median_ms': 1.25, 'min_ms': 1.25, 'max_ms': 1.25, 'calls': 1}
    assert bl.call_stats([9.12345]) == {'median_ms': 9.1235, 'min_ms': 9.1235, 'max_ms': 9.1235, 'calls': 1}
    assert bl.warm([9.0]) == [9.0] and bl.warm([9.0, 1.0]) == [1.0] and bl.warm([]) == []


def test_workgroup_size_absent_empty_or_zero_counts_as_one(bl):
    assert bl.workgroups({'Grid_Size_Z': '64', 'Workgroup_Size_Z': '4'}, 'Z') == 16
    assert bl.workgroups({'Grid_Size_Z': '64'}, 'Z') == 64
    assert bl.workgroups({'Grid_Size_Z': '64', 'Workgroup_Size_Z': ''}, 'Z') == 64
    assert bl.workgroups({'Grid_Size_Z': '64', 'Workgroup_Size_Z': '0'}, 'Z') == 64
    assert bl.workgroups({'Grid_Size_Y': '1024', 'Workgroup_Size_Y': '256', 'Grid_Size_Z': '3'}, 'Y') == 4
    with pytest.raises(KeyError):
        bl.workgroups({'Workgroup_Size_X': '64'}, 'X')


def test_trace_in_another_layout_is_recorded_not_raised(bl, tmp_path):
    _trace(str(tmp_path / 'x_kernel_trace.csv'), [('alpha_kernel', 1, 2)], fields=[f for f in FIELDS if f != 'Start_Timestamp'])
    with pytest.raises(bl.TRACE_ERRORS):
        bl.trace_rows(str(tmp_path), 'alpha_')
    rep = {}
    bl.add_trace(rep, str(tmp_path), lambda d: {'n': len(bl.trace_rows(d, 'alpha_'))})
    assert rep['kernel_trace'] is None and rep['kernel_trace_note'].startswith('not measured: the kernel trace could not be read (KeyError(')
    rep = {}
    bl.add_trace(rep, None, lambda d: 1 / 0)                                  # no trace directory: nothing read, nothing recorded
    assert rep == {}
    bl.add_trace(rep, str(tmp_path), lambda d: {})                            # a trace without the kernels: None, and no note
    assert rep == {'kernel_trace': None}
    bl.add_trace(rep, str(tmp_path), lambda d: {'k': 1}, key='stages')
    assert rep == {'kernel_trace': None, 'stages': {'k': 1}}


def test_template_flags_of_both_spellings(bl):
    # the names of tests/test_bench_validate_tool.py and tests/test_bench_loss_grad_tool.py
    assert bl.template_flags('loss_kernel', 'void (anonymous namespace)::loss_kernel<4, true, true, false>(float const*)') == [True, True, False]
    assert bl.template_flags('loss_kernel', '_ZN12_GLOBAL__N_111loss_kernelILi4ELb1ELb1ELb1EEEvPKf') == [True, True, True]
    assert bl.template_flags('loss_grad_kernel', 'void (anonymous namespace)::loss_grad_kernel<4, true, true, false>(float const*, ...)') == [True, True, False]
    assert bl.template_flags('loss_grad_kernel', '_ZN12_GLOBAL__N_116loss_grad_kernelILi4ELb1ELb1ELb1EEEvPKfS2_') == [True, True, True]
    assert bl.template_flags('line_grad_kernel', 'void (anonymous namespace)::line_grad_kernel<true, 4, true, false>(float const*)') == [True, True, False]
    assert bl.template_flags('line_grad_kernel', '_ZN12_GLOBAL__N_116line_grad_kernelILb1ELi4ELb1ELb1EEEvPKf') == [True, True, True]
    assert bl.template_flags('line_grad_kernel', '_ZN12_GLOBAL__N_116line_grad_kernelILb0ELi4ELb0ELb1EEEvPKf') == [False, False, True]
    for base in ('loss_kernel', 'loss_grad_kernel', 'line_grad_kernel'):
        assert bl.template_flags(base, 'loss_tables_kernel') is None and bl.template_flags(base, 'loss_fold_kernel(float*)') is None
    assert bl.template_flags('loss_kernel', 'void loss_grad_kernel<4, true, true, false>(float const*)') is None         # another kernel's flags


MS = [1.0, 3.59875, 6.19777, 8.79706, 2.48711, 5.08695, 7.68707, 1.37794, 3.97861, 6.57955, 9.18076, 2.87273, 5.47449, 8.07652, 1.76931, 4.3719,
      6.97475, 9.57788, 3.27177, 5.87545, 8.4794, 2.17411, 4.77861, 7.38338]


def test_stats_serves_the_three_definitions(bl):
    """Expected dicts: what the three stats() copies the tools had before benchlib returned for MS."""
    # tools/bench_validate.py's, shared by validate_line, loss_grad, augment, labels, extremities: 4 digits, index-rule p10 / p90
    got = bl.stats(MS)
    assert got == {'median_ms': 5.2807, 'min_ms': 1.0, 'max_ms': 9.5779, 'p10_ms': 1.7693, 'p90_ms': 8.7971, 'reps': 24}
    assert list(got) == ['median_ms', 'min_ms', 'max_ms', 'p10_ms', 'p90_ms', 'reps']                         # the order the reports' JSON has
    # tools/bench_jpeg_reduced.py's: 4 digits, min / max only
    got = bl.stats(MS, percentiles=None)
    assert got == {'median_ms': 5.2807, 'min_ms': 1.0, 'max_ms': 9.5779, 'reps': 24} and list(got) == ['median_ms', 'min_ms', 'max_ms', 'reps']
    # tools/bench_upscale4.py's: 3 digits, np.percentile
    got = bl.stats(MS, digits=3, minmax=False, percentiles='linear')
    assert got == {'median_ms': 5.281, 'p10_ms': 1.891, 'p90_ms': 8.702, 'reps': 24} and list(got) == ['median_ms', 'p10_ms', 'p90_ms', 'reps']
    assert all(type(v) is (int if k == 'reps' else float) for k, v in bl.stats(MS).items())                  # json.dump takes them


def test_one_owner_per_method():
    files = sorted(glob.glob(os.path.join(ROOT, 'tools', 'bench_*.py'))) + [os.path.join(ROOT, 'tools', 'benchlib.py')]
    assert len(files) == 10
    text = {os.path.basename(p): open(p).read() for p in files}
    for what in (r'\*kernel_trace\.csv', r'Event\(enable_timing=True\)', r'^HBM_ACHIEVABLE\s*=', r"'model_name':\s*'HRNetMetaModel'",
                 r"'model_name':\s*'EHMMetaModel'", r'^def stats\(', r'^def timed\(', r'^def wall\(', r'^def peak_temp\(', r'^def jpeg_folder\('):
        where = [name for name, t in text.items() for line in t.splitlines() if re.search(what, line)]          # the lines that hold it
        assert where == ['benchlib.py'], (what, where)
    for name, t in text.items():                       # no tool takes a method helper from another tool
        assert not re.search(r'\b(?:bv|bvl|bl|bench_\w+)\.(?:stats|timed|wall|jpeg_folder|peak_temp|HBM_ACHIEVABLE)\b', t), name
        if name not in ('bench_loss_grad.py', 'benchlib.py'):
            assert not re.search(r'^\s*(?:import|from) bench_\w+', t, re.M), name
