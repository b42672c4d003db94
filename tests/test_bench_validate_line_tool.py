"""CPU: the part of tools/bench_validate_line.py that needs no device -- writing the report."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        spec = importlib.util.spec_from_file_location('bench_validate_line', os.path.join(ROOT, 'tools', 'bench_validate_line.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    return mod


def test_report_writer(tmp_path):
    bl = _tool()
    st = {'median_ms': 1.0, 'p10_ms': 0.9, 'p90_ms': 1.1, 'reps': 24}
    cell = {'shape': [8, 23, 135, 240], 'weights': 'default (gmse 1, awing 1)', 'speedup_median': 0.9, 'fused_peak_temp_bytes': 2 ** 19,
            'composed_peak_temp_bytes': 2 ** 27, 'fused': st, 'composed': dict(st, median_ms=0.9), 'fused_from_maps': dict(st, median_ms=0.8)}
    rep = {'device': 'test device', 'build': 'label-1', 'ab': [cell], 'validate': None}
    bl.write_md(rep, str(tmp_path / 'r.md'))
    text = open(tmp_path / 'r.md').read()
    # a fused form that is NOT faster is reported as it is
    assert 'Build: label-1' in text and '| 8 | default (gmse 1, awing 1) | 1.0 (0.9-1.1) | 0.9 (0.9-1.1) | 0.9x | 0.8 (0.9-1.1) | 0.50 MiB | 128.0 MiB |' in text
    assert text.rstrip().endswith('not measured')                         # no validate_line() rates in this report
    rep['validate'] = {'engine': 'fp16x3', 'network': 'net', 'frames_source': 'src', 'files': 4, 'usable_annotations': 3,
                       'rows': [{'batch_size': 8, 'frames': 3, 'frames_per_s': 10.0, 'seconds': [0.3, 0.3, 0.3], 'val_loss': 0.5, 'val_acc': 0.25}]}
    bl.write_md(rep, str(tmp_path / 'r.md'))
    text = open(tmp_path / 'r.md').read()
    assert '4 files, 3 with a usable annotation' in text and '| 8 | 3 | 10.0 | [0.3, 0.3, 0.3] | 0.5 | 0.25 |' in text
    assert (bl.C, bl.H, bl.W, bl.STRIDE) == (23, 135, 240, 4)
