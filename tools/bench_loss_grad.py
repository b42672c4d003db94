"""Measure forward + backward of the two fused losses on the GPU -> profiles/loss_grad.json + profiles/loss_grad.md.

    python tools/bench_loss_grad.py [--reps 16] [--build LABEL] [--out DIR]
    python tools/bench_loss_grad.py --kernel-only        # just the gradient kernels, a few calls: the program to put behind
                                                         #   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_loss_grad.py --kernel-only
    python tools/bench_loss_grad.py --trace-dir DIR      # the run above, then read DIR's kernel trace into the report

A/B at the same commit, same device, same process, alternating, warmed, device events around the whole step (forward, backward,
the gradient left in .grad): the fused classes (HRNetLoss / EHMLoss on a prediction that requires grad) vs the composed path under
torch autograd (create_target or sncal_line_target + the torch ops of the reference's forward, fp32).  Shapes (16 / 64, 58, 270,
480) and (8 / 64, 23, 135, 240), with and without the wing term.  Peak temporaries are torch.cuda.max_memory_allocated over the
step minus what was allocated before it (the inputs and the previous step's gradient, released at the start of the step).  The
timing helpers are tools/benchlib.py's; the inputs and the composed forwards are those of tools/bench_validate.py and
tools/bench_validate_line.py.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib  # noqa: E402
import bench_validate as bv  # noqa: E402
import bench_validate_line as bl  # noqa: E402
import sncal_amd  # noqa: E402

KP_ROWS = (('default (l2 1, kldiv 1)', (1.0, 1.0, 0.0)), ('with awing_w 0.5', (1.0, 1.0, 0.5)))
LINE_ROWS = (('default (gmse 1, awing 1)', (1.0, 1.0)), ('gmse only (no wing term)', (1.0, 0.0)))


def step_of(loss_fn, pred):
    """One training-style step of a loss: forward, backward, the gradient left in pred.grad (dropped first, so nothing accumulates)."""
    def step():
        pred.grad = None
        v = loss_fn(pred)
        v.backward()
        return v
    return step


def cell(shape, label, fused, composed, grad_only, reps):
    a, b = float(fused().detach()), float(composed().detach())
    for _ in range(3):
        fused(), composed(), grad_only()
    torch.cuda.synchronize()
    t_f, t_c = benchlib.timed(fused, reps, composed)
    t_g, _ = benchlib.timed(grad_only, reps)
    sf, sc, sg = benchlib.stats(t_f), benchlib.stats(t_c), benchlib.stats(t_g)
    n = int(np.prod(shape))
    out = {'shape': list(shape), 'weights': label, 'status': 'measured', 'fused': sf, 'composed': sc, 'fused_grad_call': sg,
           'speedup_median': round(sc['median_ms'] / sf['median_ms'], 2), 'fused_value': a, 'composed_value': b,
           'fused_peak_temp_bytes': benchlib.peak_temp(fused), 'composed_peak_temp_bytes': benchlib.peak_temp(composed),
           'grad_algorithmic_bytes': 8 * n,
           'grad_call_share_of_hbm_roof': benchlib.roof_share(8 * n, sg['median_ms'])}
    print(json.dumps(out), flush=True)
    return out


def keypoint_cells(dev, reps):
    cells = []
    for B in (16, 64):
        pred, kp, mask = bv.inputs(B, dev)
        pred.requires_grad_()
        for label, wts in KP_ROWS:
            loss = sncal_amd.HRNetLoss(sigma=bv.SIGMA, stride=bv.STRIDE, pred_size=(bv.H, bv.W), num_keypoints=bv.N, l2_w=wts[0], kldiv_w=wts[1],
                                       awing_w=wts[2])
            fused = step_of(lambda p: loss([p], kp, mask), pred)
            composed = step_of(lambda p: bv.composed_loss(p, kp, mask, *wts), pred)
            plain = pred.detach()

            def grad_only():
                return sncal_amd.loss.heatmap_loss_grad(plain, kp, mask, bv.SIGMA, bv.STRIDE, loss.coef(plain), loss.terms)
            cells.append(cell(pred.shape, label, fused, composed, grad_only, reps))
        pred.grad = None
        del pred, kp, mask, plain
        torch.cuda.empty_cache()
    return cells


def line_cells(dev, reps):
    cells = []
    for B in (8, 64):
        pred, kp = bl.inputs(B, dev)
        pred.requires_grad_()
        for label, wts in LINE_ROWS:
            loss = sncal_amd.EHMLoss(gmse_w=wts[0], awing_w=wts[1], sigma=bl.GMSE_SIGMA, target_sigma=bl.TARGET_SIGMA, stride=bl.STRIDE)
            fused = step_of(lambda p: loss([p], kp), pred)
            composed = step_of(lambda p: bl.composed_loss(p, kp, *wts), pred)
            plain = pred.detach()
            n = float(plain.numel())

            def grad_only():
                return sncal_amd.loss.line_loss_grad(plain, keypoints=kp, target_sigma=bl.TARGET_SIGMA, stride=bl.STRIDE, gmse_sigma=bl.GMSE_SIGMA,
                                                     coef=(wts[0] / n, wts[1] / n), terms=loss.terms)
            cells.append(cell(pred.shape, label, fused, composed, grad_only, reps))
        pred.grad = None
        del pred, kp, plain
        torch.cuda.empty_cache()
    return cells


def kernel_only(dev):
    for B in (16, 64):
        pred, kp, mask = bv.inputs(B, dev)
        n = float(pred.numel())
        for terms, coef in ((3, (1.0 / n, 1.0 / B, 0.0)), (7, (1.0 / n, 1.0 / B, 0.5 / n))):
            for _ in range(5):
                sncal_amd.loss.heatmap_loss_grad(pred, kp, mask, bv.SIGMA, bv.STRIDE, coef, terms)
        torch.cuda.synchronize()
        del pred, kp, mask
    for B in (8, 64):
        pred, kp = bl.inputs(B, dev)
        n = float(pred.numel())
        for terms, coef in ((3, (1.0 / n, 1.0 / n)), (1, (1.0 / n, 0.0))):
            for _ in range(5):
                sncal_amd.loss.line_loss_grad(pred, keypoints=kp, target_sigma=bl.TARGET_SIGMA, stride=bl.STRIDE, gmse_sigma=bl.GMSE_SIGMA,
                                              coef=coef, terms=terms)
        torch.cuda.synchronize()
        del pred, kp


def variant(kernel_name):
    """loss_grad_kernel<V, MSE, KL, AW> / line_grad_kernel<REBUILD, V, GMSE, AW> -> 'keypoint mse+kl' ..."""
    for model, base, terms in (('keypoint', 'loss_grad_kernel', ('mse', 'kl', 'awing')), ('line', 'line_grad_kernel', (None, 'gmse', 'awing'))):
        flags = benchlib.template_flags(base, kernel_name)
        if flags:
            return model + ' ' + '+'.join(n for n, f in zip(terms, flags) if f and n)
    return kernel_name


def read_trace(trace_dir):
    """Per-variant medians of the gradient kernels from rocprofv3's kernel trace (start / end timestamps per dispatch; the grid's z
    tells the batch sizes apart)."""
    out = {}
    for r in benchlib.trace_rows(trace_dir, '_grad_kernel'):
        out.setdefault((variant(r['Kernel_Name']), benchlib.workgroups(r, 'Z')), []).append(benchlib.duration_ms(r))
    res = {}
    for (v, B), ms in out.items():
        nbytes = 8 * B * ((bv.N + 1) * bv.H * bv.W if v.startswith('keypoint') else bl.C * bl.H * bl.W)
        res[f'{v} B={B}'] = {**benchlib.call_stats(ms), 'algorithmic_bytes': nbytes,
                             'share_of_hbm_roof': benchlib.roof_share(nbytes, float(np.median(benchlib.warm(ms))))}
    return res


def write_md(rep, path):
    L = ['# Fused loss gradients: forward + backward against the composed path under torch autograd', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Every figure below is **measured** by `tools/bench_loss_grad.py` unless it says otherwise.", '',
         '## One step (forward, backward, gradient in .grad)', '',
         '| shape | weights | fused median ms (p10-p90) | composed median ms (p10-p90) | speed-up | fused peak temp | composed peak temp | fused gradient call ms | that call: 8n bytes against 6.3 TB/s |',
         '|---|---|---|---|---|---|---|---|---|']
    for c in rep['cells']:
        f, k, g = c['fused'], c['composed'], c['fused_grad_call']
        L.append(f"| {tuple(c['shape'])} | {c['weights']} | {f['median_ms']} ({f['p10_ms']}-{f['p90_ms']}) | {k['median_ms']} ({k['p10_ms']}-{k['p90_ms']}) | "
                 f"{c['speedup_median']}x | {c['fused_peak_temp_bytes'] / 2 ** 20:.1f} MiB | {c['composed_peak_temp_bytes'] / 2 ** 20:.0f} MiB | "
                 f"{g['median_ms']} | {c['grad_call_share_of_hbm_roof']} |")
    reps = rep['cells'][0]['fused']['reps'] if rep['cells'] else 0
    L += ['', f'Times are device events around the whole step, alternating fused / composed, {reps} repetitions after warm-up; the median is '
          'quoted and the spread shown.  The fused step is three passes over the tensor (sums kernel, gradient kernel, the hand-over of '
          'the gradient to .grad by torch) plus the table kernels.  Peak temporaries: torch.cuda.max_memory_allocated over a step minus what '
          'was allocated before it -- the inputs and the previous step\'s gradient, which the step releases first, so neither column counts '
          'the gradient it leaves behind (4n bytes).  The gradient call is tables kernel + gradient kernel + '
          'the allocation of its output; algorithmic bytes = 4n read + 4n written.', '',
          '## Gradient kernel time (rocprofv3 --kernel-trace, a run of its own)', '']
    if rep.get('kernel_trace'):
        L += ['| kernel variant | median ms (min-max) | calls | 8n bytes / time against 6.3 TB/s |', '|---|---|---|---|']
        for k, v in rep['kernel_trace'].items():
            L.append(f"| {k} | {v['median_ms']} ({v['min_ms']}-{v['max_ms']}) | {v['calls']} | {v['share_of_hbm_roof']} |")
        L += ['', 'A share well below 1 on a variant with the wing term says that variant is not bound by HBM; the trace alone does not '
              'say by what (no counters were collected).']
    else:
        L.append(rep.get('kernel_trace_note') or 'not measured')
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=16, trace_dir=True, kernel_only=True)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    if a.kernel_only:
        kernel_only(dev)
        return
    rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'cells': keypoint_cells(dev, a.reps) + line_cells(dev, a.reps)}
    benchlib.add_trace(rep, a.trace_dir, read_trace)
    benchlib.write_report(rep, a.out, 'loss_grad', write_md)


if __name__ == '__main__':
    main()
