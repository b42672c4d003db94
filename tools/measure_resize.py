"""Measure the resize stage (cv2.resize's bilinear shrink on the device, csrc/resize.hip) -> profiles/resize.json + profiles/resize.md.

    python tools/measure_resize.py [--reps 16] [--build LABEL] [--out DIR]
    python tools/measure_resize.py --kernel-only         # just the calls, a few each: the program to put behind
                                                         #   rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_resize.py --kernel-only
    python tools/measure_resize.py --trace-dir DIR       # the run above, then read DIR's kernel trace into the report
    ... --bench-parent FILE --bench-this FILE            # the JSON lines of `python bench.py --gpus 1` on the parent commit and on
                                                         # this one (three runs each), quoted with their spreads

Shapes: 720x1280 -> 540x960 (the general path) and 1080x1920 -> 540x960 (exactly half both ways: the area path), B = 16 / 64.
  * kernel time from a trace (a run of its own): B*3*(h*w + H*W) bytes over the time against 6.3 TB/s, the wide path (16-byte stores)
    and the byte path (the same call into a destination one byte off a 16-byte boundary);
  * against torch: the same result composed in torch ops (permute, float, F.interpolate, round, uint8), alternating, device events;
  * make_submit on a synthetic 1280x720 folder with resize=(960, 540) against the same frames stored at 960x540 without it
    (and, for scale, against the stamped 960x540 split the 720p frames were enlarged from, whose keypoints the network still finds).
"""
import argparse
import io
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib  # noqa: E402

SHAPES = [(720, 1280), (1080, 1920)]
H, W = 540, 960
BATCHES = (16, 64)
CALLS = 6
# what the trace of THIS build cannot show: written into the report as it stands
NOTES = [
    'LDS.  What is staged through LDS is the OUTPUT tile of the wide path.  The first version of this kernel used augment.hip\'s tiling '
    'instead (a lane owns 16 pixels of a destination row and issues three 16-byte stores, no LDS); traced the same way on the same '
    'device it took 0.0504 / 0.1906 ms (720p, B = 16 / 64) and 0.0658 / 0.2436 ms (1080p) where the byte path of the same build took '
    '0.0402 / 0.159 and 0.0296 / 0.1265 ms: with 16 pixels per lane neighbouring lanes gather 48 source pixels apart and the kernel '
    'holds 255 registers, so the wide path was 1.2 - 2.2 x SLOWER than its fallback.  It was replaced by the tile above (24 - 28 '
    'registers).  Those figures are from that earlier build and cannot be reproduced from this tree.',
    'Staging the two SOURCE rows through LDS was not built and is therefore not measured.  On the general path the two store forms '
    'take the same time and the call sits at 0.3 of the byte bound, which says that stores and HBM are not what limits it; the per-pixel '
    'arithmetic (two taps in fp64, eighteen 24-bit multiplies) and the two 8-byte gathers per pixel are the candidates, and no counters '
    'were collected to tell them apart.  Moving the 32-bit multiplies of the pixel arithmetic to the 24-bit multiplier took the 720p '
    'call from 0.0408 to 0.0366 ms (B = 16, wide path, same device, consecutive builds).',
]


def nbytes(B, h, w):
    return B * 3 * (h * w + H * W)


def _dst(torch, B, dev, off):
    """A (B,H,W,3) destination `off` bytes behind a 16-byte boundary (off = 1: the byte path)."""
    buf = torch.empty(B * H * W * 3 + 16, dtype=torch.uint8, device=dev)
    return buf[off:off + B * H * W * 3].view(B, H, W, 3)


def composed(img):
    """What a user without the kernel composes on the device: five passes and fp32 temporaries."""
    import torch
    import torch.nn.functional as F
    x = img.permute(0, 3, 1, 2).to(torch.float32)
    y = F.interpolate(x, size=(H, W), mode='bilinear', align_corners=False, antialias=False)
    return y.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def kernel_only(dev):
    """Per shape and batch: CALLS wide calls, then CALLS byte-path calls.  read_trace tells them apart by the kernel's name."""
    import torch
    import sncal_amd
    rng = np.random.Generator(np.random.PCG64(3))
    for h, w in SHAPES:
        for B in BATCHES:
            img = torch.from_numpy(rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)).to(dev)
            for off in (0, 1):
                out = _dst(torch, B, dev, off)
                for _ in range(CALLS):
                    sncal_amd.resize.resize_u8(img, (W, H), out=out)
                torch.cuda.synchronize()
            del img
            torch.cuda.empty_cache()


def read_trace(trace_dir):
    """Medians per (path, shape, batch) from rocprofv3's kernel trace.  The kernel's name says wide / byte, its template flag says area
    (1080p) / general (720p), the grid's y is the batch."""
    groups = {}
    for r in benchlib.trace_rows(trace_dir, 'resize_wide_kernel', 'resize_byte_kernel'):
        base = 'resize_wide_kernel' if 'resize_wide_kernel' in r['Kernel_Name'] else 'resize_byte_kernel'
        flags = benchlib.template_flags(base, r['Kernel_Name'])
        if not flags:
            continue
        groups.setdefault((base, flags[0], benchlib.workgroups(r, 'Y')), []).append(benchlib.duration_ms(r))
    res = {}
    for (base, area, B), ms in sorted(groups.items(), key=lambda kv: (kv[0][1], kv[0][2], kv[0][0] != 'resize_wide_kernel')):
        h, w = SHAPES[1] if area else SHAPES[0]
        n = nbytes(B, h, w)
        res[f"{h}x{w} -> {H}x{W} B={B} {'wide' if base == 'resize_wide_kernel' else 'byte'} path"] = {
            **benchlib.call_stats(ms), 'algorithmic_bytes': n, 'share_of_hbm_roof': benchlib.roof_share(n, float(np.median(benchlib.warm(ms))))}
    return res


def cells(dev, reps):
    import torch
    import sncal_amd
    rng = np.random.Generator(np.random.PCG64(3))
    out = []
    for h, w in SHAPES:
        for B in BATCHES:
            img = torch.from_numpy(rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)).to(dev)
            dst = _dst(torch, B, dev, 0)

            def fused():
                return sncal_amd.resize.resize_u8(img, (W, H), out=dst)

            def comp():
                return composed(img)
            for _ in range(3):
                fused(), comp()
            torch.cuda.synchronize()
            diff = (fused().to(torch.int16) - comp().to(torch.int16)).abs()
            t_f, t_c = benchlib.timed(fused, reps, comp)
            sf, sc = benchlib.stats(t_f), benchlib.stats(t_c)
            c = {'shape': [B, h, w, 3], 'to': [H, W], 'status': 'measured', 'fused': sf, 'composed': sc,
                 'ratio_median': round(sc['median_ms'] / sf['median_ms'], 2), 'fused_call_share_of_hbm_roof': benchlib.roof_share(nbytes(B, h, w), sf['median_ms']),
                 'composed_peak_temp_bytes': benchlib.peak_temp(comp), 'max_level_difference': int(diff.max()),
                 'bytes_that_differ': round(float((diff != 0).float().mean()), 4)}
            print(json.dumps(c), flush=True)
            out.append(c)
            del img, dst
            torch.cuda.empty_cache()
    return out


def folders(tmp, n):
    """Three folders with the same names: the synthetic split of benchlib.jpeg_folder at 960x540 ('stamped'); the same frames at 1280x720
    (Pillow's bicubic enlargement of the decoded frames, encoded the same way); and those 1280x720 frames brought back to 960x540 by
    Pillow's bilinear filter and encoded the same way -- the 720p folder's frames 'stored at 960x540'."""
    from PIL import Image
    stamped, big, small = os.path.join(tmp, 'stamped'), os.path.join(tmp, 'p720'), os.path.join(tmp, 'p540')
    source = benchlib.jpeg_folder(stamped, n)
    os.makedirs(big, exist_ok=True)
    os.makedirs(small, exist_ok=True)
    cache = {}

    def enc(im):
        buf = io.BytesIO()
        im.save(buf, format='JPEG', quality=98, subsampling=0)
        return buf.getvalue()
    for name in sorted(f for f in os.listdir(stamped) if f.endswith('.jpg')):
        with open(os.path.join(stamped, name), 'rb') as f:
            blob = f.read()
        if blob not in cache:
            up = Image.open(io.BytesIO(blob)).convert('RGB').resize((1280, 720), Image.BICUBIC)
            cache[blob] = (enc(up), enc(up.resize((W, H), Image.BILINEAR)))
        for folder, data in zip((big, small), cache[blob]):
            with open(os.path.join(folder, name), 'wb') as f:
                f.write(data)
    return stamped, small, big, (source + '; the 1280x720 folder holds these frames enlarged by Pillow (bicubic), the 960x540 folder those '
                                 'enlarged frames reduced again by Pillow (bilinear), all encoded the same way')


def submit_rates(n_frames=256, bs=64):
    import torch
    import sncal_amd
    with tempfile.TemporaryDirectory(prefix='sncal_resize_', ignore_cleanup_errors=True) as tmp:
        stamped, small, big, source = folders(tmp, n_frames)
        model = benchlib.keypoint_model(tmp)
        cal = sncal_amd.submit.default_calibrator()
        runs = {'p540_stamped': lambda: sncal_amd.submit.make_submit(stamped, model, cal, os.path.join(tmp, 'out_s'), batch_size=bs),
                'p540_plain': lambda: sncal_amd.submit.make_submit(small, model, cal, os.path.join(tmp, 'out_a'), batch_size=bs),
                'p720_resize': lambda: sncal_amd.submit.make_submit(big, model, cal, os.path.join(tmp, 'out_b'), batch_size=bs, resize=(W, H))}
        row = {'batch_size': bs, 'frames': n_frames, 'status': 'measured'}
        for name, run in runs.items():
            run()                                                          # warm: workspaces, decoder, allocator
            ts, res = [], None
            for _ in range(3):
                dt, res = benchlib.wall(run)
                ts.append(dt)
            row[name + '_s'] = [round(t, 4) for t in ts]
            row[name + '_frames_per_s'] = round(n_frames / float(np.median(ts)), 1)
            row[name + '_completeness'] = round(float(res['completeness']), 3)
        # the stage itself: the resize call of one batch of the run, device events
        img = torch.zeros((bs, 720, 1280, 3), dtype=torch.uint8, device=model.nn_module.device)
        dst = torch.empty((bs, H, W, 3), dtype=torch.uint8, device=img.device)
        sncal_amd.resize.resize_u8(img, (W, H), out=dst)
        ms, _ = benchlib.timed(lambda: sncal_amd.resize.resize_u8(img, (W, H), out=dst), 16)
        per_batch = float(np.median(ms)) * 1e-3
        t_run = float(np.median(row['p720_resize_s']))
        row['resize_call_ms_per_batch'] = round(per_batch * 1e3, 4)
        row['resize_share_of_run'] = round(per_batch * (n_frames / bs) / t_run, 4)
        row['run_time_ratio_720_resize_over_540_plain'] = round(t_run / float(np.median(row['p540_plain_s'])), 3)
        print(json.dumps(row), flush=True)
        return {'engine': model.nn_module.dtype_name, 'network': 'hrnet_w48, random-init weights with the designed signal path', 'frames_source': source,
                'row': row}


def bench_lines(path):
    """The JSON result lines of bench.py runs kept in a file, one per run -> {'values': [...], 'min', 'max', 'metric'}."""
    vals, metric = [], None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line.startswith('{'):
                continue
            try:
                d = json.loads(line)
            except ValueError:
                continue
            if isinstance(d.get('value'), (int, float)):
                vals.append(float(d['value']))
                metric = d.get('metric', metric)
    if not vals:
        return None
    return {'values': vals, 'min': min(vals), 'max': max(vals), 'median': float(np.median(vals)), 'metric': metric}


def write_md(rep, path):
    L = ['# Resize stage (cv2.resize INTER_LINEAR on uint8 frames): measurements', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Every figure below is **measured** by `tools/measure_resize.py` unless it says otherwise.", '',
         '## Kernel time (rocprofv3 --kernel-trace, a run of its own)', '']
    if rep.get('kernel_trace'):
        L += ['| shape, batch, path | median ms (min-max) | calls | B*3*(h*w + H*W) bytes / time against 6.3 TB/s |', '|---|---|---|---|']
        for k, v in rep['kernel_trace'].items():
            L.append(f"| {k} | {v['median_ms']} ({v['min_ms']}-{v['max_ms']}) | {v['calls']} | {v['share_of_hbm_roof']} |")
        L += ['', 'Both paths give a lane one destination pixel.  The wide path gathers a workgroup\'s 256 pixels (768 B) in LDS and stores them as '
              '48 16-byte pieces; the byte path is the same call into a destination one byte off a 16-byte boundary and stores three single '
              'bytes per lane.  Both read the source the same way: one unaligned 8-byte load per source row and pixel.  1080x1920 -> 540x960 is the area path (2x2 means), 720x1280 -> 540x960 '
              'the general one (taps formed per pixel in fp64, four multiplies per channel).  The calls of the trace read the same '
              'batch again and again; a batch of 16 frames stays in the 256 MiB last-level cache between them, so a share is an upper '
              'bound of the HBM share of a call on freshly decoded frames.  A share well below 1 says the kernel is not bound by HBM.',
              ''] + [x for n in rep.get('notes', []) for x in (n, '')]
    else:
        L.append(rep.get('kernel_trace_note') or 'not measured')
    L += ['', '## Against the same result composed in torch ops', '',
          '| shape | to | one call median ms (p10-p90) | torch ops median ms (p10-p90) | torch / call | call: share of 6.3 TB/s | torch peak temp | bytes that differ (max levels) |',
          '|---|---|---|---|---|---|---|---|']
    for c in rep['cells']:
        f, k = c['fused'], c['composed']
        L.append(f"| {tuple(c['shape'])} | {tuple(c['to'])} | {f['median_ms']} ({f['p10_ms']}-{f['p90_ms']}) | {k['median_ms']} ({k['p10_ms']}-{k['p90_ms']}) | "
                 f"{c['ratio_median']}x | {c['fused_call_share_of_hbm_roof']} | {c['composed_peak_temp_bytes'] / 2 ** 20:.0f} MiB | "
                 f"{c['bytes_that_differ']} ({c['max_level_difference']}) |")
    reps = rep['cells'][0]['fused']['reps'] if rep['cells'] else 0
    L += ['', f'Device events around the call, alternating, {reps} repetitions after warm-up.  The torch path is permute, float, F.interpolate(bilinear, '
          'align_corners=False), round, clamp, uint8, permute: float bilinear, not OpenCV\'s fixed-point arithmetic, so its bytes differ from '
          'the kernel\'s by at most one level where the last column says so.', '', '## make_submit: a 1280x720 folder with resize=(960, 540) against the same frames stored at 960x540', '']
    s = rep.get('make_submit')
    if s:
        r = s['row']
        L += ['| frames | batch | 960x540 folder, no resize: frames/s (runs, s) | 1280x720 folder, resize: frames/s (runs, s) | run time ratio | resize call per batch | resize calls as a share of the run |',
              '|---|---|---|---|---|---|---|',
              f"| {r['frames']} | {r['batch_size']} | {r['p540_plain_frames_per_s']} ({r['p540_plain_s']}) | {r['p720_resize_frames_per_s']} ({r['p720_resize_s']}) | "
              f"{r['run_time_ratio_720_resize_over_540_plain']} | {r['resize_call_ms_per_batch']} ms | {r['resize_share_of_run']} |",
              '', f"Engine {s['engine']}; {s['network']}.  Frames: {s['frames_source']}.  The run time ratio also carries the larger files' "
              'Huffman decode on the host and their larger IDCT; the last column is the stage alone: its call per batch (device events) times '
              'the batches of the run over the run\'s wall time.  Completeness of the three runs (stamped 960x540 / 960x540 / 1280x720 with '
              f"resize): {r['p540_stamped_completeness']} / {r['p540_plain_completeness']} / {r['p720_resize_completeness']}.  The synthetic network "
              'reads 2x2-pixel codes stamped at the keypoints; resampling a frame, by Pillow or by the kernel, blurs them away, so the two '
              'compared runs find no keypoint and their camera solves are trivial, while decode, network and file work are those of any run.  '
              f"The stamped split, whose solves do run, takes {r['p540_stamped_s']} s ({r['p540_stamped_frames_per_s']} frames/s): against that "
              'run too the stage is the share of the last column at most.']
    else:
        L.append(rep.get('make_submit_note') or 'not measured')
    L += ['', '## python bench.py --gpus 1 on the parent commit and on this one', '']
    b = rep.get('bench')
    if b and b.get('parent') and b.get('this'):
        L += ['| build | runs | min | median | max |', '|---|---|---|---|---|']
        for k in ('parent', 'this'):
            v = b[k]
            L.append(f"| {k} | {v['values']} | {v['min']} | {v['median']} | {v['max']} |")
        L += ['', f"Metric: {b['this']['metric']}.  The resize is not on the benchmark's path; the line is expected inside the parent's own spread."]
    else:
        L.append((b or {}).get('note') or 'not measured')
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=16, trace_dir=True, kernel_only=True)
    ap.add_argument('--no-submit', action='store_true', help='leave out the make_submit comparison')
    ap.add_argument('--bench-parent', default=None, help="file with the parent commit's bench.py result lines")
    ap.add_argument('--bench-this', default=None, help="file with this commit's bench.py result lines")
    a = ap.parse_args()
    import torch
    dev = torch.device('cuda:0')
    if a.kernel_only:
        kernel_only(dev)
        return
    rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'cells': cells(dev, a.reps), 'notes': NOTES}
    if not a.no_submit:
        try:
            rep['make_submit'] = submit_rates()
        except ImportError as e:
            rep['make_submit'], rep['make_submit_note'] = None, f'not measured: {e!r}'
    if a.bench_parent and a.bench_this:
        rep['bench'] = {'parent': bench_lines(a.bench_parent), 'this': bench_lines(a.bench_this)}
    benchlib.add_trace(rep, a.trace_dir, read_trace)
    benchlib.write_report(rep, a.out, 'resize', write_md)


if __name__ == '__main__':
    main()
