"""CPU: the parts of tools/bench_loss_grad.py that need no device -- naming the traced kernels and writing the report."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        spec = importlib.util.spec_from_file_location('bench_loss_grad', os.path.join(ROOT, 'tools', 'bench_loss_grad.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    return mod


def test_kernel_names_of_a_trace():
    bg = _tool()
    assert bg.variant('void (anonymous namespace)::loss_grad_kernel<4, true, true, false>(float const*, ...)') == 'keypoint mse+kl'
    assert bg.variant('_ZN12_GLOBAL__N_116loss_grad_kernelILi4ELb1ELb1ELb1EEEvPKfS2_') == 'keypoint mse+kl+awing'
    assert bg.variant('void (anonymous namespace)::line_grad_kernel<true, 4, true, false>(float const*)') == 'line gmse'
    assert bg.variant('_ZN12_GLOBAL__N_116line_grad_kernelILb1ELi4ELb1ELb1EEEvPKf') == 'line gmse+awing'
    assert bg.variant('loss_tables_kernel') == 'loss_tables_kernel'


def test_report_writer(tmp_path):
    bg = _tool()
    st = {'median_ms': 2.0, 'p10_ms': 1.9, 'p90_ms': 2.1, 'reps': 16}
    cell = {'shape': [16, 58, 270, 480], 'weights': 'default (l2 1, kldiv 1)', 'speedup_median': 0.8, 'fused_peak_temp_bytes': 2 ** 29,
            'composed_peak_temp_bytes': 2 ** 33, 'fused': st, 'composed': dict(st, median_ms=1.6), 'fused_grad_call': dict(st, median_ms=0.5),
            'grad_call_share_of_hbm_roof': 0.4}
    rep = {'device': 'test device', 'build': 'label-1', 'cells': [cell]}
    bg.write_md(rep, str(tmp_path / 'r.md'))
    text = open(tmp_path / 'r.md').read()
    # a fused step that is NOT faster is reported as it is
    assert 'Build: label-1' in text
    assert '| (16, 58, 270, 480) | default (l2 1, kldiv 1) | 2.0 (1.9-2.1) | 1.6 (1.9-2.1) | 0.8x | 512.0 MiB | 8192 MiB | 0.5 | 0.4 |' in text
    assert text.rstrip().endswith('not measured')                         # no kernel trace in this report
    rep['kernel_trace'] = {'keypoint mse+kl B=16': {'median_ms': 0.3, 'min_ms': 0.29, 'max_ms': 0.31, 'calls': 4, 'share_of_hbm_roof': 0.5}}
    bg.write_md(rep, str(tmp_path / 'r.md'))
    assert '| keypoint mse+kl B=16 | 0.3 (0.29-0.31) | 4 | 0.5 |' in open(tmp_path / 'r.md').read()
