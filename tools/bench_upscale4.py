"""Measure the keypoint network at upscale 4 on the GPU -> profiles/upscale4.json + profiles/upscale4.md.

    python tools/bench_upscale4.py [--batch 16] [--reps 5] [--bench-parent FILE --bench-this FILE] [--build LABEL] [--out DIR]

Full-depth hrnet_w48x4 on the default (fp16x3) engine, 960x540 frames, keypoints-only forwards (predict()'s path):

1. three variants alternated in one process, each forward timed by device events after warm-up: the fused x4 head (headx4.hip), the same
   network created with SNCAL_FUSED_HEAD=0 (the reference formulation, frames per sub-batch capped), and hrnet_w48 (x2) beside them;
2. per variant, in a separate profiled forward, the head kernel's time per call and the workspace bytes;
3. --bench-parent / --bench-this: files holding the JSON line bench.py printed on the parent commit and on this one; both go into the
   report with their difference against the +-2 % box-to-box spread the README states (nothing on the x2 path may have changed).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib  # noqa: E402

H, W = 540, 960
SPREAD = 0.02          # README: box-to-box spread of bench.py's value


def head_macs_per_frame(h, w, hidden=800, k1=208, classes=64):
    """MACs the fused split heads execute per frame for a head of h x w pixels: stage 1 (K1 blended channels), the two gathered boxes of
    16 pixels, stage 2 -- the same per pixel at x2 (headx3.hip) and x4 (headx4.hip); an x4 frame has four times the pixels."""
    return h * w * hidden * (k1 + 2 * 16 + classes)


def measure(batch, reps):
    import torch
    import sncal_amd
    from bench import seeded_weights
    dev = torch.device('cuda:0')
    x = torch.rand((batch, 3, H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    variants = []
    for name, cfg, fused in (('x4 fused', 'hrnet_w48x4', '1'), ('x4 SNCAL_FUSED_HEAD=0', 'hrnet_w48x4', '0'), ('x2', 'hrnet_w48', '1')):
        os.environ['SNCAL_FUSED_HEAD'] = fused                  # read when the network is created
        net = sncal_amd.HRNetHeatmap(cfg, device=dev)
        net.load_state_dict(seeded_weights(cfg, 1))
        variants.append((name, cfg, net))
    os.environ.pop('SNCAL_FUSED_HEAD', None)
    times = {name: [] for name, _, _ in variants}
    for _, _, net in variants:                                  # warm-up: workspaces, schedules, work lists
        net.forward(x, want_heat=False, decode_size=(H, W))
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, _, net in variants:
            times[name] += benchlib.timed(lambda: net.forward(x, want_heat=False, decode_size=(H, W)), 1)[0]
    rows = []
    for name, cfg, net in variants:
        net.set_profiling(1)
        net.forward(x, want_heat=False, decode_size=(H, W))
        prof = net.get_profile()
        net.set_profiling(0)
        head = [p for p in prof if p['kernel'] in ('headx4_fused', 'headx3_fused')]
        st = benchlib.stats(times[name], digits=3, minmax=False, percentiles='linear')
        rows.append({'variant': name, 'config': cfg, 'batch': batch, 'status': 'measured', 'forward_ms': st,
                     'frames_per_s': round(batch / st['median_ms'] * 1e3, 1), 'workspace_bytes': int(net.workspace_bytes(batch, H, W)),
                     'sub_batch': net.plan_tensor(0)['sub_batch'],
                     'head_kernel': head[0]['kernel'] if head else None,
                     'head_ms_per_call': round(head[0]['ms'] / head[0]['launches'], 3) if head else None,
                     'head_rows': sorted(((p['kernel'], round(p['ms'], 3), p['launches']) for p in prof
                                          if p['kernel'] in ('upsample_add', 'softmax_nchw', 'kp_finish', 'logsoftmax_decode_fused') or 'head' in p['kernel'] or
                                          'k1,s1' in p['kernel']), key=lambda r: -r[1])[:8]})
        print(json.dumps(rows[-1]), flush=True)
    return {'device': torch.cuda.get_device_name(0), 'engine': variants[0][2].dtype_name, 'size': [H, W], 'rows': rows}


def _bench_line(path):
    """The last JSON line of a file that holds bench.py's output."""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip().startswith('{')]
    return json.loads(lines[-1])


def write_md(rep, path):
    L = ['# Upscale 4 (hrnet_w48x4): measurements', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Engine {rep['engine']}, {rep['size'][1]}x{rep['size'][0]} frames, keypoints-only forwards; "
         'every figure is **measured** by `tools/bench_upscale4.py` unless it says otherwise.', '',
         '| variant | config | batch | forward, median ms (p10-p90) | frames/s | workspace GiB | head kernel | head ms per call |', '|---|---|---|---|---|---|---|---|']
    for r in rep['rows']:
        f = r['forward_ms']
        L.append(f"| {r['variant']} | {r['config']} | {r['batch']} | {f['median_ms']} ({f['p10_ms']}-{f['p90_ms']}) | {r['frames_per_s']} | "
                 f"{r['workspace_bytes'] / 2 ** 30:.2f} | {r['head_kernel'] or '-'} | {r['head_ms_per_call'] if r['head_ms_per_call'] is not None else '-'} |")
    L += ['', f'By MAC count a frame of the x4 head costs four times the x2 head\'s ({head_macs_per_frame(540, 960) / 1e9:.1f} against '
          f'{head_macs_per_frame(270, 480) / 1e9:.1f} GMAC executed): the same work per head pixel, four times the pixels.  The variants are alternated '
          'in one process; the head kernel\'s time comes from a separate profiled forward (events around every launch).', '',
          '## bench.py (the x2 flagship workload) on the parent commit and on this one', '']
    b = rep.get('bench')
    if not b:
        L.append('The bench.py lines were not recorded in this run.')
    else:
        p, t = b['parent']['value'], b['this']['value']
        d = (t - p) / p
        L += ['| build | frames/s |', '|---|---|', f'| parent commit | {p} |', f'| this commit | {t} |', '',
              f"Difference {d * 100:+.2f} %: {'inside' if abs(d) <= SPREAD else 'OUTSIDE'} the +-{SPREAD * 100:.0f} % box-to-box spread the README states."]
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--bench-parent', default=None, help="file with the parent commit's bench.py output")
    ap.add_argument('--bench-this', default=None, help="file with this commit's bench.py output")
    a = ap.parse_args()
    rep = measure(a.batch, a.reps)
    rep['build'] = a.build
    rep['bench'] = {'parent': _bench_line(a.bench_parent), 'this': _bench_line(a.bench_this)} if a.bench_parent and a.bench_this else None
    benchlib.write_report(rep, a.out, 'upscale4', write_md)


if __name__ == '__main__':
    main()
