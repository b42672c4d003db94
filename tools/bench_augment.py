"""Measure the fused train-time augmentation on the GPU -> profiles/augment.json + profiles/augment.md.

    python tools/bench_augment.py [--reps 16] [--build LABEL] [--out DIR]
    python tools/bench_augment.py --kernel-only          # just the fused calls, a few each: the program to put behind
                                                         #   rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_augment.py --kernel-only
    python tools/bench_augment.py --trace-dir DIR        # the run above, then read DIR's kernel trace into the report

Shapes (16 and 64, 540, 960, 3), all three stages on for every frame.  A/B at the same commit, same device, same process,
alternating, warmed, device events around the call: ONE fused call (uint8 out, and fp32 CHW out) against
  * the composed path on the device: the same arithmetic in torch ops -- fp64 colour with the fp64 mean, torch.randn noise, flip,
    permute and div -- with the peak temporary bytes of each (tools/benchlib.py's helpers);
  * the numpy per-frame restatement (tests/augment_ref.py) on the host, frames/s of ONE process: what a loader worker of the
    reference pays per frame.
From a kernel trace (a run of its own) the apply kernel's algorithmic bytes over its time against 6.3 TB/s: 3n read + 3n written
for uint8 out, 3n + 12n for fp32 CHW out; the sums pass (3n read) is listed separately.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib  # noqa: E402
sys.path.insert(0, os.path.join(benchlib.ROOT, 'tests'))

H, W = 540, 960
ALL = 7


def params_for(B, rng):
    import sncal_amd
    p = (sncal_amd._lib.AugmentParams * B)()
    for i in range(B):
        g = rng.uniform(0.8, 1.2) * rng.uniform(0.8, 1.2, 3)
        p[i].gain[0], p[i].gain[1], p[i].gain[2] = (float(x) for x in g)
        p[i].contrast, p[i].noise_sigma = float(rng.uniform(0.8, 1.2)), float(rng.uniform(0.0, 30.0))
        p[i].seed, p[i].flags = int(rng.integers(0, 2 ** 63)), ALL
    return p


def composed(img, gain, contrast, sigma, chw):
    """The same stages in torch ops: img (B,H,W,3) uint8, gain (B,1,1,3) fp64, contrast / sigma (B,1,1,1) fp64."""
    import torch
    p = img.to(torch.float64) * gain
    mean = p.mean(dim=(1, 2), keepdim=True)
    v = ((p - mean) * contrast + mean).clamp_(0.0, 255.0).to(torch.uint8)
    v = (v.to(torch.float32) + torch.randn(v.shape, device=v.device, dtype=torch.float32) * sigma.to(torch.float32)).clamp_(0.0, 255.0).to(torch.uint8)
    v = v.flip(2)
    return v.permute(0, 3, 1, 2).to(torch.float32).div(255) if chw else v.contiguous()


def cpu_frames_per_s(rng, frames=3):
    """The numpy restatement on one host process, all three stages, one frame at a time."""
    import augment_ref as ar
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ar.augment(img, ALL, (1.1, 0.9, 1.0), 1.1, rng.normal(0, 10.0, img.shape))
    t0 = time.perf_counter()
    for _ in range(frames):
        out, _ = ar.augment(img, ALL, (1.1, 0.9, 1.0), 1.1, rng.normal(0, 10.0, img.shape))
        ar.to_tensor(out)
    return frames / (time.perf_counter() - t0)


def cells(dev, reps):
    import torch
    import sncal_amd
    rng = np.random.Generator(np.random.PCG64(3))
    out = []
    for B in (16, 64):
        img = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
        p = params_for(B, rng)
        gain = torch.tensor([[p[i].gain[c] for c in range(3)] for i in range(B)], dtype=torch.float64, device=dev)[:, None, None, :]
        contrast = torch.tensor([p[i].contrast for i in range(B)], dtype=torch.float64, device=dev)[:, None, None, None]
        sigma = torch.tensor([p[i].noise_sigma for i in range(B)], dtype=torch.float64, device=dev)[:, None, None, None]
        for chw in (False, True):
            def fused():
                return sncal_amd.augment.augment_u8(img, p, want_u8=not chw, want_chw=chw)

            def comp():
                return composed(img, gain, contrast, sigma, chw)
            for _ in range(3):
                fused(), comp()
            torch.cuda.synchronize()
            t_f, t_c = benchlib.timed(fused, reps, comp)
            sf, sc = benchlib.stats(t_f), benchlib.stats(t_c)
            c = {'shape': [B, H, W, 3], 'output': 'fp32 CHW' if chw else 'uint8', 'status': 'measured', 'fused': sf, 'composed': sc,
                 'speedup_median': round(sc['median_ms'] / sf['median_ms'], 2),
                 'fused_frames_per_s': round(B / (sf['median_ms'] * 1e-3)), 'composed_frames_per_s': round(B / (sc['median_ms'] * 1e-3)),
                 'fused_peak_temp_bytes': benchlib.peak_temp(fused), 'composed_peak_temp_bytes': benchlib.peak_temp(comp)}
            print(json.dumps(c), flush=True)
            out.append(c)
        del img
        torch.cuda.empty_cache()
    return out


def kernel_only(dev):
    import torch
    import sncal_amd
    rng = np.random.Generator(np.random.PCG64(3))
    for B in (16, 64):
        img = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
        p = params_for(B, rng)
        for chw in (False, True):
            for _ in range(6):
                sncal_amd.augment.augment_u8(img, p, want_u8=not chw, want_chw=chw)
            torch.cuda.synchronize()
        del img


def read_trace(trace_dir):
    """Medians of the two kernels per batch size and output from rocprofv3's kernel trace.  The grid's y is the batch; a sums
    dispatch is followed by its apply dispatch; calls alternate uint8 (first six of a batch size) and fp32 CHW (last six)."""
    groups = {}
    for r in benchlib.trace_rows(trace_dir, 'augment_'):
        kind = 'sums' if 'augment_sums' in r['Kernel_Name'] else 'apply'
        groups.setdefault((kind, benchlib.workgroups(r, 'Y')), []).append(benchlib.duration_ms(r))
    res = {}
    for (kind, B), v in groups.items():
        n = B * H * W * 3
        halves = {'': v} if kind == 'sums' else {' uint8': v[:len(v) // 2], ' fp32 CHW': v[len(v) // 2:]}
        for tag, t in halves.items():
            if not t:
                continue
            nbytes = 3 * n if kind == 'sums' else (6 * n if tag == ' uint8' else 15 * n)
            res[f'{kind}{tag} B={B}'] = {**benchlib.call_stats(t), 'algorithmic_bytes': nbytes,
                                         'share_of_hbm_roof': benchlib.roof_share(nbytes, float(np.median(benchlib.warm(t))))}
    return res


def write_md(rep, path):
    L = ['# Fused train-time augmentation: one call against the composed path on the device and against numpy on the host', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Every figure below is **measured** by `tools/bench_augment.py` unless it says otherwise.", '',
         '## One batch, colour + noise + flip on every frame', '',
         '| shape | output | fused median ms (p10-p90) | composed median ms (p10-p90) | speed-up | fused frames/s | fused peak temp | composed peak temp |',
         '|---|---|---|---|---|---|---|---|']
    for c in rep['cells']:
        f, k = c['fused'], c['composed']
        L.append(f"| {tuple(c['shape'])} | {c['output']} | {f['median_ms']} ({f['p10_ms']}-{f['p90_ms']}) | {k['median_ms']} ({k['p10_ms']}-{k['p90_ms']}) | "
                 f"{c['speedup_median']}x | {c['fused_frames_per_s']} | {c['fused_peak_temp_bytes'] / 2 ** 20:.1f} MiB | "
                 f"{c['composed_peak_temp_bytes'] / 2 ** 20:.0f} MiB |")
    reps = rep['cells'][0]['fused']['reps'] if rep['cells'] else 0
    L += ['', f'Times are device events around the call, alternating fused / composed, {reps} repetitions after warm-up; the median is quoted and '
          'the spread shown.  The fused call is the upload of the parameter array, the sums kernel and the apply kernel, plus the '
          'allocation of its output; its peak temporaries include that output.  The composed path is fp64 colour with the fp64 mean, '
          'torch.randn noise in fp32, flip, permute and div, each a pass over the batch.  Both paths read the same resident batch in every repetition.', '',
          '## The same stages in numpy on the host', '']
    if rep.get('cpu_frames_per_s') is not None:
        L.append(f"{rep['cpu_frames_per_s']:.1f} frames/s per process (540x960, tests/augment_ref.py, normals drawn per frame as the reference "
                 'draws them): what one loader worker of the reference delivers.')
    else:
        L.append('not measured')
    L += ['', '## Kernel time (rocprofv3 --kernel-trace, a run of its own)', '']
    if rep.get('kernel_trace'):
        L += ['| kernel, output, batch | median ms (min-max) | calls | algorithmic bytes / time against 6.3 TB/s |', '|---|---|---|---|']
        for k, v in rep['kernel_trace'].items():
            L.append(f"| {k} | {v['median_ms']} ({v['min_ms']}-{v['max_ms']}) | {v['calls']} | {v['share_of_hbm_roof']} |")
        L += ['', 'Algorithmic bytes with n = B*H*W*3: apply uint8 3n read + 3n written, apply fp32 CHW 3n + 12n, sums 3n read.  The '
              'calls of the trace read the same batch again and again, and a batch of 16 frames (24 MiB) or 64 frames (95 MiB) stays in '
              'the 256 MiB last-level cache between them: a ratio above 1 says that the source came from that cache and not from HBM, so '
              'these ratios are upper bounds of the HBM share of a call on freshly decoded frames, not that share.  A ratio well below '
              '1 says the kernel is not bound by HBM -- the noise stage costs ten Philox rounds and a logarithm, a sine and a '
              'cosine per four elements, the colour stage fp64 arithmetic per element; the trace alone does not say which (no counters '
              'were collected).']
    else:
        L.append(rep.get('kernel_trace_note') or 'not measured')
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=16, trace_dir=True, kernel_only=True)
    a = ap.parse_args()
    import torch
    dev = torch.device('cuda:0')
    if a.kernel_only:
        kernel_only(dev)
        return
    rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'cells': cells(dev, a.reps),
           'cpu_frames_per_s': round(cpu_frames_per_s(np.random.Generator(np.random.PCG64(4))), 2)}
    benchlib.add_trace(rep, a.trace_dir, read_trace)
    benchlib.write_report(rep, a.out, 'augment', write_md)


if __name__ == '__main__':
    main()
