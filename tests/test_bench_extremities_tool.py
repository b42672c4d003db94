"""CPU: the part of tools/bench_extremities.py that needs no device -- writing the report."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('bench_extremities', os.path.join(ROOT, 'tools', 'bench_extremities.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_report_writer(tmp_path):
    be = _tool()
    st = {'median_ms': 1.0, 'p10_ms': 0.9, 'p90_ms': 1.1, 'reps': 24}
    cell = {'B': 16, 'host': dict(st, median_ms=8.0), 'device_wall': st, 'device_events_packed': dict(st, median_ms=0.5), 'host_ms_per_frame': 0.5,
            'host_over_device_wall': 8.0}
    ulp = [{'set': 'A', 'form': 'packed', 'frames': 24, 'distances': 730, 'max_ulp': 1, 'nan_pattern_equal': True, 'counts_equal': True},
           {'set': 'B', 'form': 'peaks', 'frames': 12, 'distances': 56, 'max_ulp': 0, 'nan_pattern_equal': True, 'counts_equal': False}]
    rep = {'device': 'test device', 'build': 'label-1', 'ulp': ulp, 'host_vs_device': [cell], 'validate': None, 'parent': None}
    path = str(tmp_path / 'r.md')
    be.write_md(rep, path)
    text = open(path).read()
    assert 'Build: label-1' in text and '| A | packed | 24 | 730 | 1 | identical | identical |' in text
    assert '| B | peaks | 12 | 56 | 0 | identical | DIFFER |' in text                   # a mismatch is reported as it is
    assert 'asks for equality' not in text                                             # said only when every maximum is 0
    assert '| 16 | 8.0 (0.9-1.1) | 0.5 | 1.0 (0.9-1.1) | 0.5 (0.9-1.1) | 8.0x |' in text
    assert text.rstrip().endswith('not measured')                                      # no validate_line() rates in this report
    for r in ulp:
        r['max_ulp'] = 0
    row = {'batch_size': 8, 'extremities': 'on', 'frames': 512, 'frames_per_s': [430.0, 441.5, 436.0], 'frames_per_s_median': 436.0}
    rep['validate'] = {'engine': 'fp16x3', 'network': 'net', 'frames_source': 'src', 'files': 512, 'runs': 3, 'rows': [dict(row, extremities='off'), row]}
    be.write_md(rep, path)
    text = open(path).read()
    assert 'The maximum is 0 ulp' in text and 'asks for equality' in text
    assert '| 8 | this commit | on | 512 | 436.0 | [430.0, 441.5, 436.0] | 430.0-441.5 |' in text and '| 8 | this commit | off |' in text
    assert "parent commit's library was not measured" in text and '| parent commit |' not in text
    rep['parent'] = {'rows': [dict(row, extremities='off', frames_per_s=[440.0, 442.0, 438.0], frames_per_s_median=440.0)]}
    be.write_md(rep, path)
    text = open(path).read()
    assert '| 8 | parent commit | off | 512 | 440.0 | [440.0, 442.0, 438.0] | 438.0-442.0 |' in text and 'nothing is promised here' in text
    assert "* batch 8: with the metric on, 436.0 frames/s (median) is 0.5 % below the parent's range 438.0-442.0." in text
    rep['parent']['rows'][0]['frames_per_s'] = [430.0, 442.0, 438.0]
    be.write_md(rep, path)
    assert "is inside the parent's range 430.0-442.0." in open(path).read()
    assert be.TS == (5.0, 10.0, 20.0)
