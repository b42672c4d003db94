"""Measure the validation path on the GPU -> profiles/validate_loss.json + profiles/validate_loss.md.

    python tools/bench_validate.py                      # A/B of the loss, roof share, validate() vs make_submit rates
    python tools/bench_validate.py --kernel-only        # just the fused loss, a few calls: the program to put behind
                                                        #   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_validate.py --kernel-only
    python tools/bench_validate.py --trace-dir DIR      # the run above, then read DIR's kernel stats into the report

A/B: fused kernel (sncal_heatmap_loss) vs the composed path (sncal_create_target + the torch ops of HRNetLoss.forward, fp32, same
device, same process), alternating, warmed, device events.  The baseline is always the composed path.
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
            t_f, t_c = benchlib.timed(fused, reps, composed)
            sf, sc = benchlib.stats(t_f), benchlib.stats(t_c)
            bytes_alg = B * (N + 1) * H * W * 4
            cells.append({'shape': [B, N + 1, H, W], 'weights': label, 'status': 'measured', 'fused': sf, 'composed': sc,
                          'speedup_median': round(sc['median_ms'] / sf['median_ms'], 2),
                          'fused_value': a, 'composed_value': b,
                          'fused_peak_temp_bytes': benchlib.peak_temp(fused), 'composed_peak_temp_bytes': benchlib.peak_temp(composed),
                          'algorithmic_bytes': bytes_alg,
                          'fused_call_share_of_hbm_roof': benchlib.roof_share(bytes_alg, sf['median_ms']),
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
    """loss_kernel<V, MSE, KL, AW> -> 'mse+kl' ..."""
    flags = benchlib.template_flags('loss_kernel', kernel_name)
    return '+'.join(n for n, f in zip(('mse', 'kl', 'awing'), flags) if f) if flags else kernel_name


def read_trace(trace_dir):
    """Per-variant medians of the loss kernels from rocprofv3's kernel trace; the grid's z, one frame each, tells the batch sizes apart."""
    out = {}
    for r in benchlib.trace_rows(trace_dir, 'loss_kernel'):
        out.setdefault((_variant(r['Kernel_Name']), benchlib.workgroups(r, 'Z')), []).append(benchlib.duration_ms(r))
    return {f'{v} B={B}': {**benchlib.call_stats(ms), 'share_of_hbm_roof': benchlib.roof_share(B * (N + 1) * H * W * 4, float(np.median(benchlib.warm(ms))))}
            for (v, B), ms in out.items()}


def validate_rates(dev, n_frames=256):
    with tempfile.TemporaryDirectory(prefix='sncal_validate_', ignore_cleanup_errors=True) as tmp:
        source = benchlib.jpeg_folder(os.path.join(tmp, 'valid'), n_frames)
        model = benchlib.keypoint_model(tmp)
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
                    dt, res = benchlib.wall(run)
                    best.append(dt)
                row[name + '_frames_per_s'] = round(n_frames / float(np.median(best)), 1)
                row[name + '_s'] = [round(t, 4) for t in best]
                row[name + '_completeness'] = round(float(res['val_completeness'] if name == 'validate' else res['completeness']), 3)
            row['scoring_cost_factor'] = round(row['make_submit_frames_per_s'] / row['validate_frames_per_s'], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        return {'engine': model.nn_module.dtype_name, 'network': 'hrnet_w48, random-init weights with the designed signal path (synth.peaked_state_dict(..., deep=True))', 'frames_source': source,
                'rows': rows}


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
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=24, trace_dir=True, kernel_only=True)
    ap.add_argument('--skip-validate', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    if a.kernel_only:
        kernel_only(dev)
        return
    rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'ab': ab_cells(dev, a.reps)}
    benchlib.add_trace(rep, a.trace_dir, read_trace)
    rep['validate'] = None if a.skip_validate else validate_rates(dev)
    benchlib.write_report(rep, a.out, 'validate_loss', write_md)


if __name__ == '__main__':
    main()
