"""Measure validate(..., sweep=grid) against validate(..., [one calibrator per grid point]) -> profiles/sweep.json + profiles/sweep.md.

    python tools/bench_sweep.py                      # the A/B on the reference's grid (optimize_valid.yaml: 15 x 6 = 90 points)
    python tools/bench_sweep.py --stages-only        # sweep passes alone: the program to put behind
                                                     #   rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_sweep.py --stages-only
    python tools/bench_sweep.py --trace-dir DIR [--bench-json FILE]      # the A/B, then DIR's kernel trace as the three stage times

Both forms score the same synthetic split (tools/benchlib.py's jpeg_folder) with the same network in the same process,
alternated, after one warm pass each.  The list form is the baseline; this change does not alter it.  No speed is asserted anywhere.
--bench-json: a file of `python bench.py` result lines labelled by build ({"build": ..., "result": {...}}), written into the report.
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
from sncal_amd.prediction import parse_range  # noqa: E402

GRID = {'max_rmse': parse_range('10:70:4'), 'max_rmse_rel': parse_range('4:16:2')}          # optimize_valid.yaml
STAGES = {'solve': ('first_pass_task_kernel', 'first_pass_combine_kernel', 'voter_task_kernel', 'sweep_mark_pending_kernel'),
          'outcome evaluation': ('evaluate_outcomes_kernel',),
          'select + fold': ('sweep_outcomes_kernel', 'sweep_select_kernel', 'sweep_fold_kernel')}


def calibrators():
    base = sncal_amd.submit.default_calibrator()
    cams = []
    for a in GRID['max_rmse']:
        for r in GRID['max_rmse_rel']:
            c = sncal_amd.submit.default_calibrator()
            c.max_rmse, c.max_rmse_rel = float(a), float(r)
            cams.append(c)
    return base, cams


def ab(model, folder, n_frames, reps):
    base, cams = calibrators()
    rows = []
    for bs in (16, 64):
        def run_list():
            return sncal_amd.validate.validate(model, folder, cams, batch_size=bs)

        def run_sweep():
            return sncal_amd.validate.validate(model, folder, base, batch_size=bs, sweep=GRID)

        def run_single():
            return sncal_amd.validate.validate(model, folder, base, batch_size=bs)
        for f in (run_list, run_sweep, run_single):
            f()                                                                  # warm: workspaces, decoder, allocator
        t = {'list': [], 'sweep': [], 'single': []}
        for _ in range(reps):
            for name, f in (('list', run_list), ('sweep', run_sweep), ('single', run_single)):
                dt, res = benchlib.wall(f)
                t[name].append(dt)
                if name == 'list':
                    want = res
                elif name == 'sweep':
                    got = res
        same = all(a[k] == b[k] or abs(a[k] - b[k]) <= 1e-12 * abs(b[k]) for a, b in zip(got, want) for k in b)
        row = {'batch_size': bs, 'frames': n_frames, 'grid_points': len(cams), 'status': 'measured',
               'list_s': [round(x, 3) for x in t['list']], 'sweep_s': [round(x, 3) for x in t['sweep']], 'single_s': [round(x, 3) for x in t['single']],
               'list_median_s': round(float(np.median(t['list'])), 3), 'sweep_median_s': round(float(np.median(t['sweep'])), 3),
               'single_median_s': round(float(np.median(t['single'])), 3), 'results_agree': bool(same),
               'best': got[got.best].params, 'best_val_evalai': got[got.best]['val_evalai'],
               'distinct_val_evalai': len({r['val_evalai'] for r in got})}
        row['speedup_list_over_sweep'] = round(row['list_median_s'] / row['sweep_median_s'], 2)
        row['sweep_over_single'] = round(row['sweep_median_s'] / row['single_median_s'], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def read_trace(trace_dir, passes_frames):
    """Kernel time of the three stages, summed over the traced passes -> ms per pass and per frame."""
    rows = benchlib.trace_rows(trace_dir, *(n for names in STAGES.values() for n in names))
    out = {}
    for stage, names in STAGES.items():
        sel = [r for r in rows if any(n in r['Kernel_Name'] for n in names)]
        ms = sum(benchlib.duration_ms(r) for r in sel)
        out[stage] = {'kernels': list(names), 'dispatches': len(sel), 'total_ms': round(ms, 3),
                      'ms_per_frame': round(ms / passes_frames, 5) if passes_frames else None}
    return out


def write_md(rep, path):
    L = ['# validate(sweep=) against validate([calibrators]): measurements', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Every figure is **measured** by `tools/bench_sweep.py` unless it says otherwise.", '',
         f"Grid: the reference's search space (optimize_valid.yaml), max_rmse {GRID['max_rmse'][0]}..{GRID['max_rmse'][-1]} x max_rmse_rel "
         f"{GRID['max_rmse_rel'][0]}..{GRID['max_rmse_rel'][-1]} = {len(GRID['max_rmse']) * len(GRID['max_rmse_rel'])} points.  "
         f"Split: {rep['frames_source']}; {rep['network']}, engine {rep['engine']}.", '',
         '| batch | frames | list of 90 calibrators, s (median; runs) | sweep, s (median; runs) | list / sweep | one calibrator, s | sweep / one | results agree |',
         '|---|---|---|---|---|---|---|---|']
    for r in rep['ab']:
        L.append(f"| {r['batch_size']} | {r['frames']} | {r['list_median_s']} ({', '.join(map(str, r['list_s']))}) | {r['sweep_median_s']} "
                 f"({', '.join(map(str, r['sweep_s']))}) | {r['speedup_list_over_sweep']}x | {r['single_median_s']} | {r['sweep_over_single']}x | {r['results_agree']} |")
    L += ['', 'Wall time of the whole call (decode, network, loss, solve, evaluation, host), same process, alternated list / sweep / single after one '
          'warm pass each.  "results agree": every key of every grid point equal between the two forms (the error sum to 1e-12 relative).  '
          f"On this split {rep['ab'][0]['distinct_val_evalai']} distinct val_evalai value(s) occur over the grid (best {rep['ab'][0]['best_val_evalai']}): "
          "the frames are clean, so the first pass settles nearly all of them and the list's 90 solves are cheap ones, and the split's "
          "annotations are drawn from other cameras than its frames (tools/bench_validate.py's folder) -- the figures are the COST of the two "
          'forms, not a tuning result.', '',
          'Extra work of the sweep against one calibrator: the outcome evaluation runs up to S = 1 + 5 T = 16 cameras per frame that reaches '
          'the voter (1 for a frame the first pass settles; empty slots leave at once) where the single form evaluates 1.', '',
          '## Stage times (rocprofv3 --kernel-trace, a run of its own)', '']
    if rep.get('stages'):
        L += [f"Kernel time summed over {rep['stage_passes']} sweep passes of {rep['stage_frames']} frames (batch {rep['stage_batch']}).", '',
              '| stage | kernels | dispatches | total ms | ms per frame |', '|---|---|---|---|---|']
        for k, v in rep['stages'].items():
            L.append(f"| {k} | {', '.join(v['kernels'])} | {v['dispatches']} | {v['total_ms']} | {v['ms_per_frame']} |")
    else:
        L.append(rep.get('stages_note') or 'not measured')
    L += ['', '## `python bench.py` against the parent commit', '']
    if rep.get('bench'):
        L += ['The single-configuration path is untouched by this change (the sweep adds kernels and entry points; `sncal_calibrate*` and '
              '`sncal_evaluate_cameras*` run the code they ran).  Same box, alternated; the README gives +-2 % as box-to-box noise:', '',
              '| build | frames/s | ms per step | steps / warmup | cameras found |', '|---|---|---|---|---|']
        for b in rep['bench']:
            r = b['result']
            L.append(f"| {b['build']} | {r['value']} | {r['ms_per_step']} | {r['steps']} / {r['warmup']} | {r['cameras_found']} |")
    else:
        L.append('not measured')
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=3, trace_dir=True)
    ap.add_argument('--stages-only', action='store_true')
    ap.add_argument('--bench-json', default=None)
    ap.add_argument('--frames', type=int, default=128)
    a = ap.parse_args()
    stage_passes, stage_batch = 2, 16
    with tempfile.TemporaryDirectory(prefix='sncal_sweep_', ignore_cleanup_errors=True) as tmp:
        folder = os.path.join(tmp, 'valid')
        source = benchlib.jpeg_folder(folder, a.frames)
        model = benchlib.keypoint_model(tmp)
        if a.stages_only:
            base, _ = calibrators()
            for _ in range(stage_passes):
                sncal_amd.validate.validate(model, folder, base, batch_size=stage_batch, sweep=GRID)
            torch.cuda.synchronize()
            return
        rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'frames_source': source, 'engine': model.nn_module.dtype_name,
               'network': 'hrnet_w48, random-init weights with the designed signal path (synth.peaked_state_dict(..., deep=True))',
               'ab': ab(model, folder, a.frames, a.reps)}
    benchlib.add_trace(rep, a.trace_dir, lambda d: read_trace(d, stage_passes * a.frames), key='stages')
    if rep.get('stages'):
        rep['stage_passes'], rep['stage_frames'], rep['stage_batch'] = stage_passes, a.frames, stage_batch
        if not any(v['dispatches'] for v in rep['stages'].values()):
            rep['stages'], rep['stages_note'] = None, 'not measured: the kernel trace holds none of the stage kernels'
    if a.bench_json and os.path.exists(a.bench_json):
        with open(a.bench_json) as f:
            lines = [json.loads(ln) for ln in f if ln.strip().startswith('{')]
        rep['bench'] = [{'build': b['build'], 'result': {**{k: b['result'][k] for k in ('metric', 'value', 'ms_per_step', 'steps', 'warmup', 'dtype')},
                                                           'cameras_found': b['result']['config']['cameras_found']}} for b in lines]
    benchlib.write_report(rep, a.out, 'sweep', write_md)


if __name__ == '__main__':
    main()
