"""Measure the scaled JPEG decode (JpegDecoder(reduce=2)) against the full-size one -> profiles/jpeg_reduced.json + .md.

    python tools/bench_jpeg_reduced.py [--reps 8] [--batch 64] [--threads 16] [--net-batch 16] [--build LABEL] [--out DIR]
    python tools/bench_jpeg_reduced.py --kernel-only     # just the decodes, a few each: the program to put behind
                                                         #   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_jpeg_reduced.py --kernel-only
    python tools/bench_jpeg_reduced.py --trace-dir DIR   # the run above, then read DIR's kernel trace into the report
    python tools/bench_jpeg_reduced.py --resources       # no GPU: compile csrc/jpeg.hip with -Rpass-analysis=kernel-resource-usage and
                                                         #   note registers / LDS / scratch of the kernels in the report

The frame is the 1920x1080 4:2:0 stream of tests/golden/jpeg_reduced.npz: synthetic and SMOOTH, so its Huffman stage is cheaper than
real footage's (fewer non-zero coefficients per block).  Same commit, same process, the variants alternated call by call.
  1. JpegDecoder.decode alone, reduce 1 against 2: the host share (wall time of the call up to its return: headers, Huffman, enqueue),
     the drained call, a pinned host-to-device copy of the coefficient bytes on its own, and -- from a kernel trace, a run of its
     own -- the two kernels.
  2. JPEG bytes -> cameras, HRNet-W48 fp16x3: reduce=2 into the 540p network against reduce=1 into the 1080p network, frames/s.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib  # noqa: E402
from benchlib import ROOT  # noqa: E402

H, W = 1080, 1920
KERNELS = ('jpeg_idct_kernel', 'jpeg_idct_scaled_kernel', 'jpeg_colour_kernel')


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=8, trace_dir=True, kernel_only=True)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--net-batch', type=int, default=16, help='batch of the bytes-to-cameras legs (the 1080p network is the C5 shape)')
    ap.add_argument('--net-steps', type=int, default=4)
    ap.add_argument('--no-net', action='store_true', help='leave out the bytes-to-cameras legs')
    a = ap.parse_args(argv)
    if a.reps < 1 or a.batch < 1 or a.threads < 0 or a.net_batch < 1 or a.net_steps < 1:
        ap.error('--reps, --batch, --net-batch and --net-steps are positive, --threads is not negative')
    return a


def hd_stream():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_reduced.npz'))
    return g['jpg.hd'].tobytes()


def frame_bytes(info: dict, layout: dict) -> dict:
    """Bytes per frame of a decode: the stream is not counted here.  info: jpeg.probe's dict; layout: jpeg.scaled_layout's.
    The coefficient upload does not depend on the scale (64 int16 per block); the sample planes and the frame do."""
    coef = sum(info['blocks']) * 64 * 2
    planes = 0
    for c in range(info['components']):
        n = info['blocks'][c]
        planes += n * layout['comp_block'][c] ** 2                   # whole blocks are written, padding included
    oh, ow = layout['out_hw']
    return {'coefficients_uploaded': coef, 'planes_written': planes, 'frame_written': oh * ow * 3,
            'device_total': 2 * coef + 2 * planes + oh * ow * 3}         # coefficients written by the copy and read once, planes written and read


def decode_cells(dev, a, blob):
    import torch
    import sncal_amd
    info = sncal_amd.jpeg.probe(blob)
    blobs = [blob] * a.batch
    decs, outs, host, total = {}, {}, {1: [], 2: []}, {1: [], 2: []}
    for r in (1, 2):
        decs[r] = sncal_amd.JpegDecoder(H, W, max_batch=a.batch, threads=a.threads, device=dev, reduce=r)
        outs[r] = torch.empty((a.batch, decs[r].out_height, decs[r].out_width, 3), dtype=torch.uint8, device=dev)
        for _ in range(2):
            decs[r].decode(blobs, outs[r])
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for r in (1, 2):                                              # alternated
            t0 = time.perf_counter()
            decs[r].decode(blobs, outs[r])
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[r].append((t1 - t0) * 1e3)
            total[r].append((t2 - t0) * 1e3)
    for r in (1, 2):
        decs[r].close()
    # the copy on its own: the same number of bytes from pinned memory (the decoder's own copy sits inside its call)
    nbytes = sum(info['blocks']) * 128 * a.batch
    src = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    copy = benchlib.timed(lambda: dst.copy_(src, non_blocking=True), a.reps + 2)[0][2:]          # the first two are warm-up
    cells = []
    for r in (1, 2):
        lay = sncal_amd.jpeg.scaled_layout(info, r)
        h, t = benchlib.stats(host[r], percentiles=None), benchlib.stats(total[r], percentiles=None)
        cells.append({'reduce': r, 'batch': a.batch, 'host_threads': a.threads, 'out_hw': list(lay['out_hw']), 'status': 'measured',
                      'host_share': h, 'drained_call': t, 'frames_per_s_drained': round(a.batch / (t['median_ms'] * 1e-3)),
                      'bytes_per_frame': frame_bytes(info, lay)})
    return cells, {'bytes': nbytes, 'status': 'measured', **benchlib.stats(copy, percentiles=None), 'GB_per_s': round(nbytes / (float(np.median(copy)) * 1e-3) / 1e9, 1)}


def net_cells(dev, a, blob):
    """JPEG bytes -> cameras: decode + forward + keypoint decode + batched solve, the host stage of batch k + 1 beside the GPU work of
    batch k.  Seeded weights: the pixels mean nothing to the network and the solve finds few cameras, so this is a figure of the
    decode and the network, not of the solve."""
    import torch
    import sncal_amd
    from oracle import hrnet_ref as hr
    sd = hr.seeded_state_dict(hr.load_config('hrnet_w48'), 3, 4.0)
    cc = sncal_amd.submit.default_calibrator()
    pipes = {}
    for r in (1, 2):                                                  # a network and a pipeline per input size: neither leg re-plans
        net = sncal_amd.HRNetHeatmap('hrnet_w48', dtype='fp16x3', device=dev)
        net.load_state_dict(sd)
        pipes[r] = sncal_amd.CalibrationPipeline(net, cc, decode_size=(540, 960))
    B = a.net_batch
    blobs = [blob] * B
    res, t = {}, {1: [], 2: []}
    decs = {r: sncal_amd.JpegDecoder(H, W, max_batch=B, threads=a.threads, device=dev, reduce=r) for r in (1, 2)}
    bufs = {r: [torch.empty((B, decs[r].out_height, decs[r].out_width, 3), dtype=torch.uint8, device=dev) for _ in range(2)] for r in (1, 2)}

    def run(r, steps):
        for k in range(steps):
            pipes[r].submit(decs[r].decode(blobs, bufs[r][k & 1]))
        pipes[r].join()
        torch.cuda.synchronize()
    for r in (1, 2):
        run(r, 2)
    for _ in range(max(1, a.reps // 4)):
        for r in (1, 2):                                              # alternated
            t0 = time.perf_counter()
            run(r, a.net_steps)
            t[r].append((time.perf_counter() - t0) / a.net_steps * 1e3)
    for r in (1, 2):
        decs[r].close()
        s = benchlib.stats(t[r], percentiles=None)
        res[r] = {'reduce': r, 'network_input': [decs[r].out_height, decs[r].out_width], 'batch': B, 'steps': a.net_steps, 'status': 'measured',
                  'step': s, 'frames_per_s': round(B / (s['median_ms'] * 1e-3), 1)}
    return [res[1], res[2]]


def kernel_only(dev, a, blob):
    """Six calls at reduce 1, then six at reduce 2: read_trace tells the colour kernel's two halves apart by this order."""
    import torch
    import sncal_amd
    blobs = [blob] * a.batch
    for r in (1, 2):
        dec = sncal_amd.JpegDecoder(H, W, max_batch=a.batch, threads=a.threads, device=dev, reduce=r)
        out = torch.empty((a.batch, dec.out_height, dec.out_width, 3), dtype=torch.uint8, device=dev)
        for _ in range(6):
            dec.decode(blobs, out)
        torch.cuda.synchronize()
        dec.close()


def read_trace(trace_dir):
    """Per kernel and scale the median time of rocprofv3's kernel trace, the first (cold) call of each dropped."""
    groups, reduce = {}, 1
    for r in benchlib.trace_rows(trace_dir, *KERNELS):
        name = next(k for k in KERNELS if k in r['Kernel_Name'])
        if name != 'jpeg_colour_kernel':
            reduce = 2 if name == 'jpeg_idct_scaled_kernel' else 1       # a colour dispatch follows the IDCT of its call
        groups.setdefault(f'{name} reduce={reduce}', []).append(benchlib.duration_ms(r))
    return {k: benchlib.call_stats(v) for k, v in groups.items()}


def resources():
    """Registers, LDS and scratch of the JPEG kernels as the compiler reports them for gfx950 (no GPU needed)."""
    src = os.path.join(ROOT, 'soccernet-calibration-sportlight_amd', 'csrc', 'jpeg.hip')
    hipcc = next((c for c in ('hipcc', '/opt/rocm/bin/hipcc') if subprocess.call(['which', c], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0), None)
    if hipcc is None:
        raise SystemExit('hipcc not found')
    out = subprocess.run([hipcc, '-x', 'hip', '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=off', '--cuda-device-only',
                          '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', os.devnull], stderr=subprocess.PIPE, stdout=subprocess.PIPE, check=True)
    return parse_resources(out.stderr.decode(errors='replace'))


def parse_resources(text: str) -> dict:
    res, cur = {}, None
    for line in text.splitlines():
        m = re.search(r'remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s*(\S+)', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            cur = next((k for k in KERNELS if k in m.group(2)), None)
            if cur:
                res[cur] = {}
        elif cur:
            res[cur][m.group(1).split(' [')[0]] = int(m.group(2))
    return res


def write_md(rep, path):
    L = ['# Scaled JPEG decode (reduce=2) against the full-size decode, 1920x1080 4:2:0', '',
         f"Device: {rep.get('device', 'none')}.  Build: {rep.get('build', 'unlabelled')}.  Every figure is **measured** by `tools/bench_jpeg_reduced.py` "
         'unless it says otherwise.', '',
         f"Frame: {rep.get('jpeg_bytes_per_frame', '?')} bytes, synthetic and smooth (tests/golden/jpeg_reduced.npz `jpg.hd`): its Huffman stage is "
         'cheaper than real footage\'s, so the host share below is a lower bound of a broadcast frame\'s.', '',
         '## 1. JpegDecoder.decode alone', '']
    if rep.get('decode'):
        L += ['| reduce | output | batch, host threads | host share median ms (min-max) | drained call median ms (min-max) | frames/s drained | '
              'coefficients uploaded / frame | planes written / frame | frame written |', '|---|---|---|---|---|---|---|---|---|']
        for c in rep['decode']:
            h, t, b = c['host_share'], c['drained_call'], c['bytes_per_frame']
            L.append(f"| {c['reduce']} | {c['out_hw'][1]}x{c['out_hw'][0]} | {c['batch']}, {c['host_threads']} | {h['median_ms']} ({h['min_ms']}-{h['max_ms']}) | "
                     f"{t['median_ms']} ({t['min_ms']}-{t['max_ms']}) | {c['frames_per_s_drained']} | {b['coefficients_uploaded']} | {b['planes_written']} | {b['frame_written']} |")
        L += ['', 'The host share is the wall time of the call up to its return: headers, Huffman decode on the host threads, the enqueue.  It does '
              'not depend on the scale -- libjpeg entropy-decodes everything at any scale too -- and neither does the coefficient upload.']
    else:
        L.append('not measured')
    L += ['', '### The copy', '']
    c = rep.get('copy')
    L.append(f"{c['bytes']} bytes (one batch of coefficients) from pinned memory, on its own: {c['median_ms']} ms median ({c['min_ms']}-{c['max_ms']}), "
             f"{c['GB_per_s']} GB/s.  The same at either scale." if c else 'not measured')
    L += ['', '### The two kernels (rocprofv3 --kernel-trace --stats, a run of its own)', '']
    if rep.get('kernel_trace'):
        L += ['| kernel, scale | median ms (min-max) | calls |', '|---|---|---|']
        for k, v in sorted(rep['kernel_trace'].items()):
            L.append(f"| {k} | {v['median_ms']} ({v['min_ms']}-{v['max_ms']}) | {v['calls']} |")
        L += ['', 'Both IDCT kernels read every coefficient block (128 bytes a block, the upload above per batch) whatever the scale: a packed '
              'upload of only the coefficients a reduced transform reads is not built, so the scaled IDCT is bounded by that read and only '
              'its stores shrink.  The colour kernel runs over the reduced frame and shrinks with it.']
    else:
        L.append(rep.get('kernel_trace_note') or 'not measured')
    L += ['', '## 2. JPEG bytes to cameras, HRNet-W48 fp16x3', '']
    if rep.get('net'):
        L += ['| reduce | network input | batch | step median ms (min-max) | frames/s |', '|---|---|---|---|---|']
        for c in rep['net']:
            s = c['step']
            L.append(f"| {c['reduce']} | {c['network_input'][1]}x{c['network_input'][0]} | {c['batch']} | {s['median_ms']} ({s['min_ms']}-{s['max_ms']}) | {c['frames_per_s']} |")
        L += ['', 'Decode, forward, keypoint decode and the batched solve, the host stage of batch k + 1 beside the GPU work of batch k; both rows in one '
              'process, alternated.  reduce=1 is the only path there was for such frames: the network at 1920x1080, a size the checkpoints '
              'were not trained at.  Seeded weights: the solve finds few cameras, so the rows compare decode + network, not the solve.']
    else:
        L.append('not measured')
    L += ['', '## Compiler resource usage (gfx950, -Rpass-analysis=kernel-resource-usage)', '']
    if rep.get('resources'):
        L += ['| kernel | VGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | occupancy waves / SIMD |', '|---|---|---|---|---|---|']
        for k, v in rep['resources'].items():
            L.append(f"| {k} | {v.get('VGPRs')} | {v.get('TotalSGPRs')} | {v.get('LDS Size')} | {v.get('ScratchSize')} | {v.get('Occupancy')} |")
        L += ['', 'jpeg_idct_scaled_kernel holds the 8 / 4 / 2 / 1 instantiations (the block size is the component\'s, chosen inside the one launch).']
    else:
        L.append('not measured')
    benchlib.write_lines(L, path)


def main(argv=None):
    a = parse_args(argv)
    jpath = os.path.join(a.out, 'jpeg_reduced.json')
    old = {}
    if os.path.exists(jpath):
        with open(jpath) as f:
            old = json.load(f)
    if a.resources:
        rep = dict(old, resources=resources())
    else:
        import torch
        dev = torch.device('cuda:0')
        blob = hd_stream()
        if a.kernel_only:
            kernel_only(dev, a, blob)
            return
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):        # never the legacy null stream: see pipeline.py
            cells, copy = decode_cells(dev, a, blob)
            net = None if a.no_net else net_cells(dev, a, blob)
        rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'jpeg_bytes_per_frame': len(blob), 'decode': cells, 'copy': copy,
               'net': net, 'resources': old.get('resources')}
        benchlib.add_trace(rep, a.trace_dir, read_trace)
    benchlib.write_report(rep, a.out, 'jpeg_reduced', write_md)


if __name__ == '__main__':
    main()
