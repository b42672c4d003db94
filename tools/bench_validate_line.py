"""Measure the line model's validation tail on the GPU -> profiles/validate_line.json + profiles/validate_line.md.

    python tools/bench_validate_line.py [--reps 24] [--skip-validate] [--build LABEL] [--out DIR]

A/B: the fused loss in its rebuild form (sncal_line_loss from the endpoints: no target written) vs the composed path
(sncal_line_target + the torch ops of EHMLoss.forward, fp32, same device, same process) at (8,23,135,240) and (64,23,135,240),
alternating, warmed, device events around the whole call, spread reported.  The maps form (target read from memory) is timed beside
them.  Then validate_line() frames/s over a synthetic split folder.  The timing helpers are tools/benchlib.py's.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib  # noqa: E402
import sncal_amd  # noqa: E402

C, H, W, TARGET_SIGMA, STRIDE, GMSE_SIGMA = 23, 135, 240, 1.0, 4, 4.0


def composed_loss(pred, kp, gmse_w, awing_w):
    """EHMLoss.forward as the reference composes it (line/loss.py:34-108), target from sncal_line_target."""
    target = sncal_amd.loss.create_keypoint_maps(kp, TARGET_SIGMA, STRIDE, (H, W))
    loss = 0
    if gmse_w > 0:
        sq = (pred - target) ** 2
        loss = loss + gmse_w * (sq * torch.exp(-sq / (2 * GMSE_SIGMA ** 2))).mean()
    if awing_w > 0:
        alpha, omega, theta = 2.1, 14, 0.5
        delta = (target - pred).abs()
        a = alpha - target
        A = omega * (1 / (1 + torch.pow(theta, a))) * a * torch.pow(theta, alpha - target - 1)
        Cc = theta * A - omega * torch.log(1 + torch.pow(theta, a))
        loss = loss + awing_w * torch.mean(torch.where(delta < theta, omega * torch.log(1 + torch.pow(delta, a)), A * delta - Cc))
    return loss


def inputs(B, dev, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    kp = np.zeros((B, C, 2, 3), dtype=np.float32)
    kp[..., :2] = -1
    has = rng.uniform(size=(B, C)) < 0.4
    pts = np.stack([rng.uniform(0, W * STRIDE, (B, C, 2)), rng.uniform(0, H * STRIDE, (B, C, 2))], -1)
    kp[..., :2] = np.where(has[..., None, None], pts, -1)
    kp[..., 2] = has[..., None]
    pred = torch.softmax(torch.randn((B, C, H, W), generator=g), dim=1).to(dev)
    return pred, torch.from_numpy(kp).to(dev)


def ab_cells(dev, reps):
    cells = []
    for B in (8, 64):
        pred, kp = inputs(B, dev)
        maps = sncal_amd.loss.create_keypoint_maps(kp, TARGET_SIGMA, STRIDE, (H, W))
        for label, wts in (('default (gmse 1, awing 1)', (1.0, 1.0)), ('gmse only', (1.0, 0.0))):
            loss = sncal_amd.EHMLoss(gmse_w=wts[0], awing_w=wts[1], sigma=GMSE_SIGMA, target_sigma=TARGET_SIGMA, stride=STRIDE)

            def fused():
                return loss([pred], kp)

            def from_maps():
                return loss([pred], maps)

            def composed():
                return composed_loss(pred, kp, *wts)
            a, b = float(fused()), float(composed())
            for _ in range(3):
                fused(), composed(), from_maps()
            torch.cuda.synchronize()
            t_f, t_c = benchlib.timed(fused, reps, composed)
            t_m, _ = benchlib.timed(from_maps, reps)
            sf, sc, sm = benchlib.stats(t_f), benchlib.stats(t_c), benchlib.stats(t_m)
            cells.append({'shape': [B, C, H, W], 'weights': label, 'status': 'measured', 'fused': sf, 'composed': sc, 'fused_from_maps': sm,
                          'speedup_median': round(sc['median_ms'] / sf['median_ms'], 2), 'fused_value': a, 'composed_value': b,
                          'fused_peak_temp_bytes': benchlib.peak_temp(fused), 'composed_peak_temp_bytes': benchlib.peak_temp(composed),
                          'algorithmic_bytes': B * C * H * W * 4})
            print(json.dumps(cells[-1]), flush=True)
    return cells


def validate_rates(dev, n_frames=512):
    with tempfile.TemporaryDirectory(prefix='sncal_validate_line_', ignore_cleanup_errors=True) as tmp:
        folder = os.path.join(tmp, 'valid')
        source = benchlib.jpeg_folder(folder, n_frames)
        model = benchlib.line_model(tmp)
        usable = len(sncal_amd.frames.list_line_split(folder)[0])
        rows = []
        for bs in (8, 64):
            def run():
                return sncal_amd.validate.validate_line(model, folder, batch_size=bs)
            run()                                                          # warm: workspaces, decoder, allocator
            secs = []
            for _ in range(3):
                dt, res = benchlib.wall(run)
                secs.append(dt)
            rows.append({'batch_size': bs, 'frames': res.frames, 'skipped': len(res.skipped), 'status': 'measured',
                         'frames_per_s': round(res.frames / float(np.median(secs)), 1), 'seconds': [round(t, 4) for t in secs],
                         'val_loss': res['val_loss'], 'val_acc': res['val_acc']})
            print(json.dumps(rows[-1]), flush=True)
        return {'engine': model.nn_module.dtype_name, 'network': 'line_hrnet_w48, random-init weights with the designed signal path (synth.line_deep_state_dict)',
                'frames_source': source, 'files': n_frames, 'usable_annotations': usable, 'rows': rows}


def write_md(rep, path):
    L = ['# Line model: fused EHMLoss and validate_line(): measurements', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Every figure below is **measured** by `tools/bench_validate_line.py` unless it says otherwise.", '',
         '## Fused kernel (rebuild form) vs the composed path (sncal_line_target + torch ops), shape (B,23,135,240)', '',
         '| B | weights | fused median ms (p10-p90) | composed median ms (p10-p90) | composed / fused | fused, maps form, median ms (p10-p90) | fused peak temp | composed peak temp |',
         '|---|---|---|---|---|---|---|---|']
    for c in rep['ab']:
        f, k, m = c['fused'], c['composed'], c['fused_from_maps']
        L.append(f"| {c['shape'][0]} | {c['weights']} | {f['median_ms']} ({f['p10_ms']}-{f['p90_ms']}) | {k['median_ms']} ({k['p10_ms']}-{k['p90_ms']}) | "
                 f"{c['speedup_median']}x | {m['median_ms']} ({m['p10_ms']}-{m['p90_ms']}) | {c['fused_peak_temp_bytes'] / 2 ** 20:.2f} MiB | "
                 f"{c['composed_peak_temp_bytes'] / 2 ** 20:.1f} MiB |")
    L += ['', 'Times are device events around the whole call (tables kernel + loss kernel + fold + the host-side combine for the fused '
          'forms; target kernel + torch ops for the composed path), alternating fused / composed, '
          f"{rep['ab'][0]['fused']['reps']} repetitions after warm-up.  At these sizes a call is a handful of short launches, so the "
          'figures include launch overhead on both sides.', '']
    L += ['## validate_line() over a split folder', '']
    if rep.get('validate'):
        v = rep['validate']
        L += [f"{v['network']}, engine {v['engine']}; frames: {v['frames_source']}; {v['files']} files, {v['usable_annotations']} with a usable annotation.", '',
              '| batch | frames | frames/s (median of 3 runs) | seconds | val_loss | val_acc |', '|---|---|---|---|---|---|']
        for r in v['rows']:
            L.append(f"| {r['batch_size']} | {r['frames']} | {r['frames_per_s']} | {r['seconds']} | {r['val_loss']:.6g} | {r['val_acc']:.4g} |")
    else:
        L.append('not measured')
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=24)
    ap.add_argument('--skip-validate', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'ab': ab_cells(dev, a.reps)}
    rep['validate'] = None if a.skip_validate else validate_rates(dev)
    benchlib.write_report(rep, a.out, 'validate_line', write_md)


if __name__ == '__main__':
    main()
