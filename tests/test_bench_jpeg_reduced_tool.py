"""CPU: the parts of tools/bench_jpeg_reduced.py that need no device -- arguments, byte counts, reading a kernel trace and the
compiler's resource remarks, writing the report."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        spec = importlib.util.spec_from_file_location('bench_jpeg_reduced', os.path.join(ROOT, 'tools', 'bench_jpeg_reduced.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    return mod


def test_arguments():
    bj = _tool()
    a = bj.parse_args([])
    assert (a.batch, a.threads, a.reps, a.net_batch, a.kernel_only, a.resources, a.trace_dir) == (64, 16, 8, 16, False, False, None)
    a = bj.parse_args(['--kernel-only', '--batch', '8', '--threads', '0', '--build', 'x'])
    assert a.kernel_only and a.batch == 8 and a.threads == 0 and a.build == 'x'
    for bad in (['--batch', '0'], ['--reps', '0'], ['--threads', '-1'], ['--reduce', '2']):
        with pytest.raises(SystemExit):
            bj.parse_args(bad)


def test_byte_counts_of_the_hd_stream(sncal):
    """1920x1080 4:2:0: 120 x 68 MCUs of six blocks; at 1/2 the luma blocks are 4x4 and the chroma blocks stay 8x8."""
    bj = _tool()
    blob = bj.hd_stream()
    info = sncal.jpeg.probe(blob)
    assert (info['height'], info['width'], info['h_samp'], info['v_samp']) == (1080, 1920, 2, 2)
    mcus = 120 * 68
    assert info['blocks'] == [4 * mcus, mcus, mcus]
    full = bj.frame_bytes(info, sncal.jpeg.scaled_layout(info, 1))
    half = bj.frame_bytes(info, sncal.jpeg.scaled_layout(info, 2))
    assert full['coefficients_uploaded'] == half['coefficients_uploaded'] == 6 * mcus * 128
    assert full['planes_written'] == 6 * mcus * 64 and half['planes_written'] == 4 * mcus * 16 + 2 * mcus * 64
    assert full['frame_written'] == 1080 * 1920 * 3 and half['frame_written'] == 540 * 960 * 3
    assert half['device_total'] == 2 * 6 * mcus * 128 + 2 * half['planes_written'] + 540 * 960 * 3


def test_kernel_trace_reader(tmp_path):
    bj = _tool()
    d = tmp_path / 'trace' / 'host' / '1'
    d.mkdir(parents=True)
    rows, t = ['Kernel_Name,Start_Timestamp,End_Timestamp'], 1000
    for call in range(12):                                               # six calls at reduce 1, then six at reduce 2
        idct = 'jpeg_idct_kernel' if call < 6 else 'jpeg_idct_scaled_kernel'
        for name, us in ((idct, 100 if call < 6 else 60), ('jpeg_colour_kernel', 80 if call < 6 else 20)):
            if call in (0, 6):
                us *= 5                                                   # the cold call, which the reader drops
            rows.append(f'"_ZN12_GLOBAL__N_1{name}EPKs",{t},{t + us * 1000}')
            t += us * 1000 + 500
    rows.append(f'"some_other_kernel",{t},{t + 5}')
    (d / '1_kernel_trace.csv').write_text('\n'.join(rows))
    got = bj.read_trace(str(tmp_path / 'trace'))
    assert sorted(got) == ['jpeg_colour_kernel reduce=1', 'jpeg_colour_kernel reduce=2', 'jpeg_idct_kernel reduce=1', 'jpeg_idct_scaled_kernel reduce=2']
    assert got['jpeg_idct_kernel reduce=1'] == {'median_ms': 0.1, 'min_ms': 0.1, 'max_ms': 0.1, 'calls': 5}
    assert got['jpeg_idct_scaled_kernel reduce=2']['median_ms'] == 0.06
    assert got['jpeg_colour_kernel reduce=1']['median_ms'] == 0.08 and got['jpeg_colour_kernel reduce=2']['median_ms'] == 0.02


def test_resource_remarks_reader():
    bj = _tool()
    text = '\n'.join(f'csrc/jpeg.hip:1:1: remark: {ln} [-Rpass-analysis=kernel-resource-usage]' for ln in (
        'Function Name: _ZN12_GLOBAL__N_116jpeg_idct_kernelEPKs', '    TotalSGPRs: 31', '    VGPRs: 25', '    ScratchSize [bytes/lane]: 0',
        '    Occupancy [waves/SIMD]: 8', '    LDS Size [bytes/block]: 9216',
        'Function Name: _ZN12_GLOBAL__N_123jpeg_idct_scaled_kernelEPKs', '    TotalSGPRs: 38', '    VGPRs: 37', '    ScratchSize [bytes/lane]: 0',
        'Function Name: something_else', '    VGPRs: 99'))
    got = bj.parse_resources(text)
    assert got == {'jpeg_idct_kernel': {'TotalSGPRs': 31, 'VGPRs': 25, 'ScratchSize': 0, 'Occupancy': 8, 'LDS Size': 9216},
                   'jpeg_idct_scaled_kernel': {'TotalSGPRs': 38, 'VGPRs': 37, 'ScratchSize': 0}}


def test_report_writer(tmp_path):
    bj = _tool()
    bj.write_md({}, str(tmp_path / 'r.md'))
    assert open(tmp_path / 'r.md').read().count('not measured') == 5     # every section says so when it has no figures
    st = {'median_ms': 2.0, 'min_ms': 1.9, 'max_ms': 2.1, 'reps': 8}
    by = {'coefficients_uploaded': 100, 'planes_written': 50, 'frame_written': 30, 'device_total': 330}
    rep = {'device': 'test device', 'build': 'label-1', 'jpeg_bytes_per_frame': 84084,
           'decode': [{'reduce': 2, 'batch': 64, 'host_threads': 16, 'out_hw': [540, 960], 'host_share': st, 'drained_call': dict(st, median_ms=2.5),
                       'frames_per_s_drained': 25600, 'bytes_per_frame': by}],
           'net': [{'reduce': 2, 'network_input': [540, 960], 'batch': 16, 'step': st, 'frames_per_s': 8000.0}],
           'resources': {'jpeg_idct_scaled_kernel': {'VGPRs': 37, 'TotalSGPRs': 38, 'LDS Size': 9216, 'ScratchSize': 0, 'Occupancy': 8}}}
    bj.write_md(rep, str(tmp_path / 'r.md'))
    text = open(tmp_path / 'r.md').read()
    assert 'Build: label-1' in text and '84084 bytes, synthetic and smooth' in text
    assert '| 2 | 960x540 | 64, 16 | 2.0 (1.9-2.1) | 2.5 (1.9-2.1) | 25600 | 100 | 50 | 30 |' in text
    assert '| 2 | 960x540 | 16 | 2.0 (1.9-2.1) | 8000.0 |' in text
    assert '| jpeg_idct_scaled_kernel | 37 | 38 | 9216 | 0 | 8 |' in text
    assert text.count('not measured') == 2                                # the copy and the kernel trace
