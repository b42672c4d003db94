"""Measure the validation path on the GPU -> profiles/validate_loss.json + profiles/validate_loss.md.

    python tools/bench_validate.py                      # A/B of the loss, roof share, validate() vs make_submit rates
    python tools/bench_validate.py --kernel-only        # just the fused loss, a few calls: the program to put behind
                                                        #   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_validate.py --kernel-only
    python tools/bench_validate.py --trace-dir DIR      # the run above, then read DIR's kernel stats into the report

A/B: fused kernel (sncal_heatmap_loss) vs the composed path (sncal_create_target + the torch ops of HRNetLoss.forward, fp32, same
device, same process), alternating, warmed, device events.  The baseline is always the composed path.
"""
import argparse
import glob
import csv
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import sncal_amd  # noqa: E402

HBM_ACHIEVABLE = 6.3e12          # bytes/s, the achievable HBM rate of the MI355X
N, H, W, SIGMA, STRIDE = 57, 270, 480, 2.0, 2


def composed_loss(pred, kp_img, mask, l2_w, kldiv_w, awing_w):
    """HRNetLoss.forward as the reference composes it, target from sncal_create_target."""
    kp = kp_img.clone()
    kp[:, :, :2] /= STRIDE
    heat = sncal_amd.loss.create_target(kp, SIGMA, (H, W))
    if mask is not None:
        m = mask[:, :, None, None]
        heat, pred = heat * m, pred * m
    p01 = torch.exp(pred)
    loss = 0
    if l2_w > 0:
        loss = loss + l2_w * torch.nn.functional.mse_loss(p01, heat)
    if kldiv_w > 0:
        loss = loss + kldiv_w * torch.nn.functional.kl_div(pred, heat, reduction='batchmean')
    if awing_w > 0:
        alpha, omega, theta = 2.1, 14, 0.5
        delta = (heat - p01).abs()
        a = alpha - heat
        A = omega * (1 / (1 + torch.pow(theta, a))) * a * torch.pow(theta, alpha - heat - 1)
        C = theta * A - omega * torch.log(1 + torch.pow(theta, a))
        loss = loss + awing_w * torch.mean(torch.where(delta < theta, omega * torch.log(1 + torch.pow(delta, a)), A * delta - C))
    return loss


def inputs(B, dev, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    kp = torch.from_numpy(sncal_amd.synth.synthetic_keypoints(B, seed=seed)).clone()
    kp[..., 2] = (kp[..., 2] > 0.5).float()
    pred = torch.log_softmax(torch.randn((B, N + 1, H, W), generator=g), dim=1).to(dev)
    mask = torch.ones((B, N + 1))
    mask[:, 40] = 0
    return pred, kp.to(dev), mask.to(dev)


def timed(fn, reps, other=None):
    """reps timings of fn in ms (device events), alternating with `other` when given -> (ms list, ms list of other)."""
    out, out2 = [], []
    for _ in range(reps):
        for f, acc in ((fn, out), (other, out2)):
            if f is None:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return out, out2


def peak_temp(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    del r
    return torch.cuda.max_memory_allocated() - base


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {'median_ms': round(float(np.median(a)), 4), 'min_ms': round(float(a[0]), 4), 'max_ms': round(float(a[-1]), 4),
            'p10_ms': round(float(a[len(a) // 10]), 4), 'p90_ms': round(float(a[(9 * len(a)) // 10]), 4), 'reps': len(a)}


def ab_cells(dev, reps):
    cells = []
    for B in (16, 64):
        pred, kp, mask = inputs(B, dev)
        for label, wts in (('default (l2 1, kldiv 1)', (1.0, 1.0, 0.0)), ('with awing_w 0.5', (1.0, 1.0, 0.5))):
            loss = sncal_amd.HRNetLoss(sigma=SIGMA, stride=STRIDE, pred_size=(H, W), num_keypoints=N, l2_w=wts[0], kldiv_w=wts[1], awing_w=wts[2])

            def fused():
                return loss([pred], kp, mask)

            def composed():
                return composed_loss(pred, kp, mask, *wts)
            a, b = float(fused()), float(composed())
            for _ in range(3):
                fused(), composed()
            torch.cuda.synchronize()
            t_f, t_c = timed(fused, reps, composed)
            sf, sc = stats(t_f), stats(t_c)
            bytes_alg = B * (N + 1) * H * W * 4
            cells.append({'shape': [B, N + 1, H, W], 'weights': label, 'status': 'measured', 'fused': sf, 'composed': sc,
                          'speedup_median': round(sc['median_ms'] / sf['median_ms'], 2),
                          'fused_value': a, 'composed_value': b,
                          'fused_peak_temp_bytes': peak_temp(fused), 'composed_peak_temp_bytes': peak_temp(composed),
                          'algorithmic_bytes': bytes_alg,
                          'fused_call_share_of_hbm_roof': round(bytes_alg / (sf['median_ms'] * 1e-3) / HBM_ACHIEVABLE, 3),
                          'transcendentals_per_element': '1 exp' if wts[2] == 0 else '1 exp + 2 exp2 + 1 pow + 2 log1p (one of them behind the branch)'})
            print(json.dumps(cells[-1]), flush=True)
        del pred, kp, mask
        torch.cuda.empty_cache()
    return cells


def kernel_only(dev):
    for B in (16, 64):
        pred, kp, mask = inputs(B, dev)
        for terms in (3, 7):
            for _ in range(5):
                sncal_amd.loss.heatmap_loss_sums(pred, kp, mask, SIGMA, STRIDE, terms)
        torch.cuda.synchronize()
        del pred, kp, mask


def _variant(kernel_name):
    """loss_kernel<V, MSE, KL, AW> -> 'mse+kl' ...; the trace holds the name demangled or mangled, depending on the profiler's settings."""
    import re
    m = re.search(r'loss_kernel<\s*\d+,\s*(true|false),\s*(true|false),\s*(true|false)\s*>', kernel_name)
    flags = [f == 'true' for f in m.groups()] if m else None
    if flags is None:
        m = re.search(r'loss_kernelILi\d+ELb([01])ELb([01])ELb([01])E', kernel_name)
        flags = [f == '1' for f in m.groups()] if m else None
    if flags is None:
        return kernel_name
    return '+'.join(n for n, f in zip(('mse', 'kl', 'awing'), flags) if f)


def read_trace(trace_dir):
    """Per-kernel average of the loss kernels from rocprofv3's kernel trace (start / end timestamps per dispatch, grid size to tell
    the batch sizes apart)."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if 'loss_kernel' in r.get('Kernel_Name', '')]
    out = {}
    for r in rows:
        name = r['Kernel_Name']
        variant = _variant(name)
        frames = int(r['Grid_Size_Z']) // max(int(r.get('Workgroup_Size_Z', 1) or 1), 1)      # the trace gives work-items; one frame per grid z
        key = f"{variant} B={frames}"
        out.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-6)
    res = {}
    for k, v in out.items():
        v = v[1:] if len(v) > 1 else v                      # dispatches are in time order: drop the first (cold) call
        B = int(k.rsplit('B=', 1)[1])
        med = float(np.median(v))
        res[k] = {'median_ms': round(med, 4), 'min_ms': round(float(min(v)), 4), 'max_ms': round(float(max(v)), 4), 'calls': len(v),
                  'share_of_hbm_roof': round(B * (N + 1) * H * W * 4 / (med * 1e-3) / HBM_ACHIEVABLE, 3)}
    return res


def jpeg_folder(path, n):
    """n frames + annotations.  Stamped synthetic frames encoded with Pillow when it is installed (baseline, 4:4:4, quality 98);
    otherwise the golden 960x540 JPEG, whose pixels mean nothing to the network (no keypoints, trivial solves)."""
    os.makedirs(path, exist_ok=True)
    try:
        from PIL import Image
        import io
        frames, _ = sncal_amd.synth.stamped_frames(32, seed=7)
        blobs = []
        for f in frames:
            rgb = np.ascontiguousarray((f[::-1].transpose(1, 2, 0) * 255.0 + 0.5).astype(np.uint8))      # BGR planes -> RGB image
            buf = io.BytesIO()
            Image.fromarray(rgb).save(buf, format='JPEG', quality=98, subsampling=0)
            blobs.append(buf.getvalue())
        source = 'synth.stamped_frames, 32 distinct frames, Pillow baseline JPEG 4:4:4 q98'
    except ImportError:
        g = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz'))
        blobs = [g['jpg.full'].tobytes()]
        source = 'tests/golden/jpeg_cases.npz jpg.full (no JPEG encoder installed)'
    for i in range(n):
        annot, _ = sncal_amd.synth.synthetic_annotation(seed=i % 32)
        with open(os.path.join(path, f'{i:05d}.json'), 'w') as f:
            json.dump({c: [{'x': x, 'y': y} for x, y in pts] for c, pts in annot.items()}, f)
        with open(os.path.join(path, f'{i:05d}.jpg'), 'wb') as f:
            f.write(blobs[i % len(blobs)])
    return source


def validate_rates(dev, n_frames=256):
    tmp = tempfile.mkdtemp(prefix='sncal_validate_')
    try:
        source = jpeg_folder(os.path.join(tmp, 'valid'), n_frames)
        cfg = sncal_amd.load_config('hrnet_w48')
        ck = {'model_name': 'HRNetMetaModel',
              'params': {'nn_module': {'hrnet_config': cfg, 'num_refinement_stages': 0, 'num_heatmaps': 58},
                         'loss': {'num_refinement_stages': 0, 'stride': STRIDE, 'sigma': SIGMA, 'pred_size': [H, W], 'num_keypoints': N},
                         'prediction_transform': {'size': [540, 960]}, 'device': 'cuda:0'},
              'nn_state_dict': sncal_amd.synth.peaked_state_dict(bench.seeded_weights('hrnet_w48', seed=1), deep=True)}
        path = os.path.join(tmp, 'model.pth')
        torch.save(ck, path)
        model = sncal_amd.load_model(path, device='cuda:0')
        cal = sncal_amd.submit.default_calibrator()
        rows = []
        for bs in (16, 64):
            row = {'batch_size': bs, 'frames': n_frames, 'status': 'measured'}
            for name, run in (('validate', lambda: sncal_amd.validate.validate(model, os.path.join(tmp, 'valid'), cal, batch_size=bs)),
                              ('make_submit', lambda: sncal_amd.submit.make_submit(os.path.join(tmp, 'valid'), model, cal, os.path.join(tmp, 'out'),
                                                                                    batch_size=bs))):
                run()                                                      # warm: workspaces, decoder, allocator
                best = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = run()
                    torch.cuda.synchronize()
                    best.append(time.perf_counter() - t0)
                row[name + '_frames_per_s'] = round(n_frames / float(np.median(best)), 1)
                row[name + '_s'] = [round(t, 4) for t in best]
                row[name + '_completeness'] = round(float(res['val_completeness'] if name == 'validate' else res['completeness']), 3)
            row['scoring_cost_factor'] = round(row['make_submit_frames_per_s'] / row['validate_frames_per_s'], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        return {'engine': model.nn_module.dtype_name, 'network': 'hrnet_w48, random-init weights with the designed signal path (synth.peaked_state_dict(..., deep=True))', 'frames_source': source,
                'rows': rows}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def write_md(rep, path):
    L = ['# Fused validation loss and validate(): measurements', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Every figure below is **measured** by `tools/bench_validate.py` unless it says otherwise.", '',
         '## Fused kernel vs the composed path (create_target + torch ops), shape (B,58,270,480)', '',
         '| B | weights | fused median ms (p10-p90) | composed median ms (p10-p90) | speed-up | fused peak temp | composed peak temp | fused call: share of 6.3 TB/s |',
         '|---|---|---|---|---|---|---|---|']
    for c in rep['ab']:
        f, k = c['fused'], c['composed']
        L.append(f"| {c['shape'][0]} | {c['weights']} | {f['median_ms']} ({f['p10_ms']}-{f['p90_ms']}) | {k['median_ms']} ({k['p10_ms']}-{k['p90_ms']}) | "
                 f"{c['speedup_median']}x | {c['fused_peak_temp_bytes'] / 2 ** 20:.1f} MiB | {c['composed_peak_temp_bytes'] / 2 ** 20:.0f} MiB | "
                 f"{c['fused_call_share_of_hbm_roof']} |")
    L += ['', 'Times are device events around the whole call (tables kernel + loss kernel + fold + the host-side combine), alternating '
          f"fused / composed, {rep['ab'][0]['fused']['reps']} repetitions after warm-up.  Algorithmic bytes = B*58*270*480*4.", '']
    L += ['## Kernel time (rocprofv3 --kernel-trace, a run of its own)', '']
    if rep.get('kernel_trace'):
        L += ['| loss_kernel variant | median ms (min-max) | calls | algorithmic bytes / time against 6.3 TB/s |', '|---|---|---|---|']
        for k, v in rep['kernel_trace'].items():
            L.append(f"| {k} | {v['median_ms']} ({v['min_ms']}-{v['max_ms']}) | {v['calls']} | {v['share_of_hbm_roof']} |")
    else:
        L.append(rep.get('kernel_trace_note') or 'not measured')
    L += ['', '## validate() beside make_submit on the same folder', '']
    if rep.get('validate'):
        v = rep['validate']
        L += [f"{v['network']}, engine {v['engine']}; frames: {v['frames_source']}.", '',
              '| batch | validate frames/s | make_submit frames/s | make_submit / validate | completeness (validate / make_submit) |', '|---|---|---|---|---|']
        for r in v['rows']:
            L.append(f"| {r['batch_size']} | {r['validate_frames_per_s']} | {r['make_submit_frames_per_s']} | {r['scoring_cost_factor']} | "
                     f"{r['validate_completeness']} / {r['make_submit_completeness']} |")
    else:
        L.append('not measured')
    L.append('')
    with open(path, 'w') as f:
        f.write('\n'.join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--trace-dir', default=None)
    ap.add_argument('--reps', type=int, default=24)
    ap.add_argument('--skip-validate', action='store_true')
    ap.add_argument('--build', default='unlabelled', help='label of the build the figures come from (written into the report)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    if a.kernel_only:
        kernel_only(dev)
        return
    rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'ab': ab_cells(dev, a.reps)}
    if a.trace_dir:
        try:
            rep['kernel_trace'] = read_trace(a.trace_dir) or None
        except (KeyError, ValueError, OSError) as e:          # a trace in another layout: say so, keep the rest of the report
            rep['kernel_trace'], rep['kernel_trace_note'] = None, f'not measured: the kernel trace could not be read ({e!r})'
    rep['validate'] = None if a.skip_validate else validate_rates(dev)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'validate_loss.json'), 'w') as f:
        json.dump(rep, f, indent=1)
    write_md(rep, os.path.join(a.out, 'validate_loss.md'))
    print('wrote', os.path.join(a.out, 'validate_loss.json'))


if __name__ == '__main__':
    main()
