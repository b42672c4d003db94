"""CPU: the report writer of tools/bench_labels.py."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        spec = importlib.util.spec_from_file_location('bench_labels', os.path.join(ROOT, 'tools', 'bench_labels.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    return mod


def test_report_writer(tmp_path):
    bl = _tool()
    st = {'median_ms': 2.0, 'p10_ms': 1.9, 'p90_ms': 2.1, 'reps': 16}
    cell = {'frames': 16, 'points': 1234, 'host_ms': 480.5, 'device_call_wall': st, 'device_events': dict(st, median_ms=0.4), 'pack_ms': 1.25,
            'speedup_wall_median': 240.2}
    rep = {'device': 'test device', 'build': 'label-1', 'host': {'frames': 64, 'mean_ms_per_frame': 30.1, 'median_ms_per_frame': 29.5,
                                                                 'min_ms_per_frame': 2.0, 'max_ms_per_frame': 40.0},
           'cells': [cell], 'agreement': {'frames': 64, 'presence_identical': True, 'max_label_distance_px': 3.2e-9},
           'pipeline': None, 'pipeline_note': 'not measured (--skip-pipeline)'}
    bl.write_md(rep, str(tmp_path / 'r.md'))
    text = open(tmp_path / 'r.md').read()
    assert 'Build: label-1' in text and '30.1 ms per frame (median 29.5, 2.0-40.0)' in text
    assert '| 16 | 1234 | 480.5 | 2.0 (1.9-2.1) | 1.25 | 0.4 | 240.2x |' in text
    assert 'presence identical, largest label distance 3.20e-09 px' in text
    assert text.rstrip().endswith('not measured (--skip-pipeline)')
    # a device path that is NOT faster, and a presence difference, are reported as they are
    row = {'batch_size': 16, 'frames': 256, 'validate_host_frames_per_s': 90.0, 'validate_device_frames_per_s': 85.5,
           'train_batches_host_frames_per_s': 30.0, 'train_batches_device_frames_per_s': 2000.0, 'make_submit_frames_per_s': 450.0}
    rep['pipeline'] = {'engine': 'fp16x3', 'frames_source': 'somewhere', 'rows': [row]}
    rep['agreement']['presence_identical'] = False
    bl.write_md(rep, str(tmp_path / 'r.md'))
    text = open(tmp_path / 'r.md').read()
    assert '| 16 | 256 | 90.0 | 85.5 | 30.0 | 2000.0 | 450.0 |' in text and 'presence DIFFERENT' in text
