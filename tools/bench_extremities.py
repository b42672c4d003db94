"""Measure the extremity metric on the GPU -> profiles/extremities.json + profiles/extremities.md.

    python tools/bench_extremities.py [--reps 24] [--runs 3] [--skip-validate] [--parent-lib PATH] [--build LABEL] [--out DIR]

1. The largest distance, in ulp, between d_err of sncal_extremity_counts and the reference capture (tests/golden/extremities.npz),
   both sets, both prediction forms.
2. The host restatement (extremities.host_counts: two evaluate_detection_prediction calls per frame and threshold) against ONE device
   call for the batch (extremity_counts: packing, one upload, the launch) at B = 16 and 64, thresholds 5 / 10 / 20, frames of set A
   repeated.  The device call is timed as the host sees it (wall clock, synchronised) and by device events around the launch.
3. validate_line(folder) frames/s with and without extremities=, on the synthetic split tools/bench_validate_line.py scores, runs
   alternating; --parent-lib PATH adds the same runs of validate_line() in a fresh process that loads the PARENT commit's library
   (SNCAL_LIB_PATH): the parent's own number on the same split.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib  # noqa: E402
sys.path.insert(0, os.path.join(benchlib.ROOT, 'tests'))

TS = (5.0, 10.0, 20.0)


def max_ulp(dev):
    import torch
    import extremities_cases as xc
    import sncal_amd
    g = xc.load()
    rows = []
    for key in ('A', 'B'):
        c = xc.case(g, key)
        for form in xc.FORMS:
            kw = dict(img_size=c['size'], ts=c['ts'], scale=c['scale'], p_threshold=c['p_threshold'])
            if form == 'peaks':
                out = sncal_amd.extremities.extremity_counts(c['gt'], peaks=torch.from_numpy(c['peak_rows']).to(dev), **kw)
            else:
                out = sncal_amd.extremities.extremity_counts(c['gt'], pred_annots=c['pred'], device=dev, **kw)
            frame, cls, err = (o.cpu().numpy() for o in out)
            want = c[form]
            fin = ~np.isnan(want['err'])
            same_nan = bool(np.array_equal(fin, ~np.isnan(err)))
            ulp = int(np.abs(err[fin].view(np.int64) - want['err'][fin].view(np.int64)).max()) if same_nan and fin.any() else None
            rows.append({'set': key, 'form': form, 'frames': c['B'], 'distances': int(fin.sum()), 'max_ulp': ulp, 'nan_pattern_equal': same_nan,
                         'counts_equal': bool(np.array_equal(frame, want['frame']) and np.array_equal(cls, want['cls']))})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def host_vs_device(dev, reps):
    import torch
    import extremities_cases as xc
    import sncal_amd
    ex = sncal_amd.extremities
    c = xc.case(xc.load(), 'A')
    W, H = c['size']
    cells = []
    for B in (16, 64):
        idx = [i % c['B'] for i in range(B)]
        gts = [c['gt'][i] for i in idx]
        peaks = torch.from_numpy(c['peak_rows'][idx]).to(dev)
        gts_px = [sncal_amd.evaluate.scale_points(a, W, H) for a in gts]
        preds_px = [ex.peaks_to_points(p, c['scale'], c['p_threshold']) for p in c['peak_rows'][idx]]
        packed = sncal_amd.annotations.pack_annotations(gts)

        def device():
            return ex.extremity_counts(gts, peaks=peaks, img_size=c['size'], ts=TS, scale=c['scale'], p_threshold=c['p_threshold'])

        def device_packed():
            return ex.extremity_counts(packed, peaks=peaks, img_size=c['size'], ts=TS, scale=c['scale'], p_threshold=c['p_threshold'])
        for _ in range(3):
            device()
        torch.cuda.synchronize()
        wall, host = [benchlib.wall(device)[0] * 1e3 for _ in range(reps)], []
        for _ in range(max(3, reps // 8)):
            t0 = time.perf_counter()
            ex.host_counts(preds_px, gts_px, TS)
            host.append((time.perf_counter() - t0) * 1e3)
        ev, _ = benchlib.timed(device_packed, reps)
        cells.append({'B': B, 'thresholds': list(TS), 'status': 'measured', 'host': benchlib.stats(host), 'device_wall': benchlib.stats(wall),
                      'device_events_packed': benchlib.stats(ev), 'host_ms_per_frame': round(float(np.median(host)) / B, 4),
                      'host_over_device_wall': round(float(np.median(host)) / float(np.median(wall)), 1)})
        print(json.dumps(cells[-1]), flush=True)
    return cells


def validate_rates(dev, runs, with_metric=True, n_frames=512):
    """validate_line(folder) over the synthetic split of tools/bench_validate_line.py: `runs` timed runs per setting, alternating."""
    import sncal_amd
    with tempfile.TemporaryDirectory(prefix='sncal_extremities_', ignore_cleanup_errors=True) as tmp:
        folder = os.path.join(tmp, 'valid')
        source = benchlib.jpeg_folder(folder, n_frames)
        model = benchlib.line_model(tmp)
        settings = [('off', {})] + ([('on', {'extremities': (5, 10, 20)})] if with_metric else [])
        rows = []
        for bs in (8, 64):
            secs = {name: [] for name, _ in settings}
            last = {}
            for name, kw in settings:
                sncal_amd.validate.validate_line(model, folder, batch_size=bs, **kw)          # warm: workspaces, decoder, allocator
            for _ in range(runs):
                for name, kw in settings:
                    dt, last[name] = benchlib.wall(lambda: sncal_amd.validate.validate_line(model, folder, batch_size=bs, **kw))
                    secs[name].append(dt)
            for name, _ in settings:
                res = last[name]
                rows.append({'batch_size': bs, 'extremities': name, 'frames': res.frames, 'status': 'measured', 'seconds': [round(t, 4) for t in secs[name]],
                             'frames_per_s': [round(res.frames / t, 1) for t in secs[name]],
                             'frames_per_s_median': round(res.frames / float(np.median(secs[name])), 1), 'metrics': dict(res)})
                print(json.dumps(rows[-1]), flush=True)
        return {'engine': model.nn_module.dtype_name, 'network': 'line_hrnet_w48, random-init weights with the designed signal path',
                'frames_source': source, 'files': n_frames, 'runs': runs, 'rows': rows}


def parent_rates(lib, runs):
    """The same validate_line() runs, metric off, in a fresh process that loads another build of the library."""
    env = dict(os.environ, SNCAL_LIB_PATH=os.path.abspath(lib))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--rates-child', '--runs', str(runs)], env=env, stdout=subprocess.PIPE,
                         check=True, timeout=900).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def _spread(v):
    return f'{min(v)}-{max(v)}'


def write_md(rep, path):
    L = ['# Extremity metric on the device: measurements', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Every figure below is **measured** by `tools/bench_extremities.py` unless it says otherwise.", '',
         '## d_err against the reference capture (tests/golden/extremities.npz)', '',
         '| set | form | frames | distances | max ulp | NaN pattern | counts, labelling, per-class rows |', '|---|---|---|---|---|---|---|']
    for r in rep['ulp']:
        L.append(f"| {r['set']} | {r['form']} | {r['frames']} | {r['distances']} | {r['max_ulp']} | {'identical' if r['nan_pattern_equal'] else 'DIFFERS'} | "
                 f"{'identical' if r['counts_equal'] else 'DIFFER'} |")
    worst = [r['max_ulp'] for r in rep['ulp'] if r['max_ulp'] is not None]
    if worst and max(worst) == 0:
        L += ['', 'The maximum is 0 ulp: the kernel writes numpy\'s bits on these cases, and tests/test_extremities_gpu.py asks for equality '
              '(the reasoned bound was 2 ulp: one for the sum, one for the square root).']
    L += ['', '## Host restatement per frame vs one device call per batch (thresholds 5 / 10 / 20)', '',
          '| B | host, whole batch, median ms (p10-p90) | host ms / frame | device call, wall, median ms (p10-p90) | device call, events, pre-packed, median ms (p10-p90) | host / device wall |',
          '|---|---|---|---|---|---|']
    for c in rep['host_vs_device']:
        h, w, e = c['host'], c['device_wall'], c['device_events_packed']
        L.append(f"| {c['B']} | {h['median_ms']} ({h['p10_ms']}-{h['p90_ms']}) | {c['host_ms_per_frame']} | {w['median_ms']} ({w['p10_ms']}-{w['p90_ms']}) | "
                 f"{e['median_ms']} ({e['p10_ms']}-{e['p90_ms']}) | {c['host_over_device_wall']}x |")
    L += ['', 'The host column is extremities.host_counts on pixel dicts that are already built.  The device wall column is extremity_counts as a '
          'caller sees it: pack_annotations on the host, one upload, the launch, then a synchronise that validate_line() does not do '
          '(it waits once, at the end).  The events column leaves the packing out.  This is a latency kernel: one wavefront per frame.', '',
          '## validate_line(folder) with and without extremities=', '']
    v = rep.get('validate')
    if v:
        L += [f"{v['network']}, engine {v['engine']}; frames: {v['frames_source']}; {v['files']} files; {v['runs']} runs per setting, alternating.", '',
              '| batch | build | extremities= | frames | frames/s, median | frames/s, each run | spread |', '|---|---|---|---|---|---|---|']
        for label, rows in (('this commit', v['rows']), ('parent commit', (rep.get('parent') or {}).get('rows', []))):
            for r in rows:
                L.append(f"| {r['batch_size']} | {label} | {r['extremities']} | {r['frames']} | {r['frames_per_s_median']} | {r['frames_per_s']} | "
                         f"{_spread(r['frames_per_s'])} |")
        if not rep.get('parent'):
            L += ['', 'The parent commit\'s library was not measured in this run.']
        else:
            L += ['', 'The parent rows are validate_line() in a fresh process that loads the parent commit\'s libsncal.so (SNCAL_LIB_PATH), on '
                  'the same synthetic split.  Its spread over the runs is the yardstick; nothing is promised here, the rows say:', '']
            for p in rep['parent']['rows']:
                on = [r for r in v['rows'] if r['batch_size'] == p['batch_size'] and r['extremities'] == 'on']
                if on:
                    lo, hi, m = min(p['frames_per_s']), max(p['frames_per_s']), on[0]['frames_per_s_median']
                    where = 'inside' if lo <= m <= hi else f'{abs(m - (lo if m < lo else hi)) / p["frames_per_s_median"] * 100:.1f} % {"below" if m < lo else "above"}'
                    L.append(f"* batch {p['batch_size']}: with the metric on, {m} frames/s (median) is {where} the parent's range {lo}-{hi}.")
            L += ['', 'What the metric adds per batch is pack_annotations on the host (two Python loops over the frames\' points), one upload from '
                  'pinned memory that does not wait for the stream, and one launch.']
    else:
        L.append('not measured')
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=24)
    ap.add_argument('--runs', type=int, default=3, help='timed validate_line() runs per setting')
    ap.add_argument('--skip-validate', action='store_true')
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libsncal.so: its validate_line() rates are measured beside this build's")
    ap.add_argument('--rates-child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    dev = torch.device('cuda:0')
    if a.rates_child:
        print(json.dumps(validate_rates(dev, a.runs, with_metric=False)))
        return
    rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'ulp': max_ulp(dev), 'host_vs_device': host_vs_device(dev, a.reps)}
    rep['validate'] = None if a.skip_validate else validate_rates(dev, a.runs)
    rep['parent'] = parent_rates(a.parent_lib, a.runs) if a.parent_lib and not a.skip_validate else None
    benchlib.write_report(rep, a.out, 'extremities', write_md)


if __name__ == '__main__':
    main()
