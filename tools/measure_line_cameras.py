"""Measure the cameras from line extremities on the GPU -> profiles/line_cameras.json + profiles/line_cameras.md.
(On tools/benchlib.py like the bench_* report tools; tests/test_benchlib_host.py pins that family to nine, hence the name.)

    python tools/measure_line_cameras.py [--reps 24] [--runs 3] [--skip-folder] [--trace-dir DIR] [--kernel-only] [--build LABEL] [--out DIR]

1. The largest measured share of the value bound 4 * max(E_ref, 2^-44) per quantity (H, f, R, position) against the reference capture
   (tests/golden/line_cameras.npz), both sets, and the largest distance of the refined rmse from scipy's minimum on the captured matches.
2. The host mirror (baseline_cameras.frame_flow per frame, no refinement) against ONE device call for the batch (line_cameras, refine
   off and on) at B = 16 and 64, frames of set A at 960 x 540 repeated: as the caller sees it (wall clock, synchronised, packing
   included) and by device events on pre-packed input.
3. Kernel time from a kernel trace (--trace-dir: a rocprofv3 --kernel-trace run of this tool with --kernel-only), with the share of
   frames that run the LM.
4. The one-pass folder run (line_model_cameras) in frames/s beside export_extremities alone, same synthetic split, runs alternating.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib  # noqa: E402
sys.path.insert(0, os.path.join(benchlib.ROOT, 'tests'))

SIZE = (960, 540)


def _records(sncal_amd, cams):
    return [sncal_amd._lib.Camera.from_buffer_copy(r.tobytes()) for r in cams.cpu().numpy()]


def shares(dev):
    import line_cameras_cases as lc
    import sncal_amd
    bc = sncal_amd.baseline_cameras
    g = lc.load()
    rows = []
    for key in ('A', 'B'):
        c = lc.case(g, key)
        worst, decisions = {k: (0.0, None) for k in lc.VALUES}, True
        for size, ids in lc.by_size(c).items():
            cams, status, H, n_lines, slots = bc.line_cameras(pred_annots=[c['pred'][i] for i in ids], img_size=size, refine=False, device=dev)
            decisions = decisions and np.array_equal(status.cpu().numpy(), c['status'][ids]) and np.array_equal(slots.cpu().numpy(), c['slots'][ids]) \
                and np.array_equal(n_lines.cpu().numpy(), c['n_lines'][ids])
            for k, (b, rec) in enumerate(zip(ids, _records(sncal_amd, cams))):
                got = {'H': H[k].cpu().numpy(), 'f': rec.fx, 'R': np.array(rec.rotation[:]), 'pos': np.array(rec.position[:])}
                for q in lc.VALUES:
                    if np.isfinite(c[q][b]).all() and (q == 'H' or c['status'][b]):
                        s = lc.rel(got[q], c[q][b]) / lc.bound(c['E_ref'][b])
                        if s > worst[q][0]:
                            worst[q] = (s, int(b))
        rows.append({'set': key, 'frames': c['B'], 'decisions_identical': bool(decisions),
                     'largest_share': {q: {'share': round(v[0], 4), 'frame': v[1]} for q, v in worst.items()}})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def scipy_distance(dev):
    try:
        from scipy import optimize
        from scipy.spatial.transform import Rotation as Rot
    except ImportError:
        return {'status': 'not measured: scipy is not installed'}
    import line_cameras_cases as lc
    import sncal_amd
    bc = sncal_amd.baseline_cameras
    c = lc.case(lc.load(), 'A')
    worst, n = (0.0, None), 0
    for size, ids in lc.by_size(c).items():
        cams, status = bc.line_cameras(pred_annots=[c['pred'][i] for i in ids], img_size=size, refine=True, device=dev)[:2]
        for b, rec in zip(ids, _records(sncal_amd, cams)):
            if rec.status != bc.STATUS_REFINED:
                continue
            m = c['match_n'][b]
            X, uv, f, R0, pos0 = c['match_X'][b, :m], c['match_uv'][b, :m], c['f'][b], c['R'][b].reshape(3, 3), c['pos'][b]

            def res(p):
                Xc = X @ (Rot.from_rotvec(p[:3]).as_matrix() @ R0).T + p[3:]
                return (np.stack([f * Xc[:, 0] / Xc[:, 2] + size[0] / 2, f * Xc[:, 1] / Xc[:, 2] + size[1] / 2], axis=1) - uv).ravel()
            sp = optimize.least_squares(res, np.r_[0, 0, 0, -R0 @ pos0], method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
            l2 = float(np.linalg.norm(sp.fun.reshape(-1, 2), axis=1).mean())
            d = abs(rec.rmse - l2) / l2
            n += 1
            if d > worst[0]:
                worst = (d, int(b))
    return {'status': 'measured', 'refined_frames': n, 'largest_relative_rmse_distance': worst[0], 'frame': worst[1], 'bound': 1e-4}


def _batch(c, B):
    same = [b for b in range(c['B']) if c['sizes'][b] == SIZE]
    return [same[i % len(same)] for i in range(B)]


def host_vs_device(dev, reps):
    import line_cameras_cases as lc
    import sncal_amd
    bc = sncal_amd.baseline_cameras
    c = lc.case(lc.load(), 'A')
    cells = []
    for B in (16, 64):
        idx = _batch(c, B)
        preds = [c['pred'][i] for i in idx]
        packed = sncal_amd.annotations.pack_annotations(preds)
        lm = int(sum(c['status'][i] == 1 and c['match_n'][i] > 3 for i in idx))
        for _ in range(3):
            bc.line_cameras(pred_annots=preds, img_size=SIZE, device=dev)
        host = []
        for _ in range(max(3, reps // 8)):
            t0 = time.perf_counter()
            for p in preds:
                bc.frame_flow(p, SIZE)
            host.append((time.perf_counter() - t0) * 1e3)
        cell = {'B': B, 'frames_with_lm': lm, 'status': 'measured', 'host': benchlib.stats(host), 'host_ms_per_frame': round(float(np.median(host)) / B, 4)}
        for name, refine in (('refine_off', False), ('refine_on', True)):
            wall = [benchlib.wall(lambda: bc.line_cameras(pred_annots=preds, img_size=SIZE, refine=refine, device=dev))[0] * 1e3 for _ in range(reps)]
            ev, _ = benchlib.timed(lambda: bc.line_cameras(pred_annots=packed, img_size=SIZE, refine=refine, device=dev), reps)
            cell[name] = {'device_wall': benchlib.stats(wall), 'device_events_packed': benchlib.stats(ev)}
        cell['host_over_device_wall_refine_off'] = round(float(np.median(host)) / cell['refine_off']['device_wall']['median_ms'], 1)
        cells.append(cell)
        print(json.dumps(cell), flush=True)
    return cells


def kernel_only(dev):
    """What a kernel trace should see: a few calls per batch size, refine on."""
    import torch
    import line_cameras_cases as lc
    import sncal_amd
    c = lc.case(lc.load(), 'A')
    for B in (16, 64):
        packed = sncal_amd.annotations.pack_annotations([c['pred'][i] for i in _batch(c, B)])
        for _ in range(6):
            sncal_amd.baseline_cameras.line_cameras(pred_annots=packed, img_size=SIZE, refine=True, device=dev)
    torch.cuda.synchronize()


def read_trace(trace_dir):
    out = {}
    for name in ('line_cameras_kernel', 'line_refine_kernel'):
        by_b = {}
        for r in benchlib.trace_rows(trace_dir, name):
            by_b.setdefault(benchlib.workgroups(r, 'X'), []).append(benchlib.duration_ms(r))
        out[name] = {str(B): benchlib.call_stats(ms) for B, ms in sorted(by_b.items())}
    return out if any(out.values()) else None


def folder_rates(dev, runs, n_frames=256):
    import sncal_amd
    with tempfile.TemporaryDirectory(prefix='sncal_baseline_cameras_', ignore_cleanup_errors=True) as tmp:
        folder = os.path.join(tmp, 'valid')
        source = benchlib.jpeg_folder(folder, n_frames)
        model = benchlib.line_model(tmp)
        runs_of = {'export_extremities': lambda d: sncal_amd.extremities.export_extremities(folder, model, d),
                   'line_model_cameras': lambda d: sncal_amd.baseline_cameras.line_model_cameras(folder, model, d)}
        secs, written = {k: [] for k in runs_of}, {}
        for k, fn in runs_of.items():
            fn(os.path.join(tmp, 'warm_' + k))
        for r in range(runs):
            for k, fn in runs_of.items():
                dt, written[k] = benchlib.wall(lambda: fn(os.path.join(tmp, f'{k}_{r}')))
                secs[k].append(dt)
        return {'status': 'measured', 'engine': model.nn_module.dtype_name, 'frames_source': source, 'files': n_frames, 'runs': runs,
                'rows': [{'run': k, 'files_written': written[k], 'seconds': [round(t, 4) for t in secs[k]],
                          'frames_per_s': [round(n_frames / t, 1) for t in secs[k]],
                          'frames_per_s_median': round(n_frames / float(np.median(secs[k])), 1)} for k in runs_of]}


def write_md(rep, path):
    L = ['# Cameras from line extremities on the device: measurements', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Every figure below is **measured** by `tools/measure_line_cameras.py` unless it says otherwise.  "
         "`bench.py`'s line does not pass through this code: it was not re-measured for this report.", '',
         '## Share of the value bound 4 * max(E_ref, 2^-44) against the reference capture (refine = 0)', '',
         '| set | frames | decisions | H | f | R | position |', '|---|---|---|---|---|---|---|']
    for r in rep['shares']:
        s = r['largest_share']
        L.append(f"| {r['set']} | {r['frames']} | {'identical' if r['decisions_identical'] else 'DIFFER'} | " +
                 ' | '.join(f"{s[q]['share']} (frame {s[q]['frame']})" for q in ('H', 'f', 'R', 'pos')) + ' |')
    over = [(r['set'], q, v) for r in rep['shares'] for q, v in r['largest_share'].items() if v['share'] > 1]
    L += ['', 'No share exceeds 1.' if not over else 'Shares above 1: ' + ', '.join(f"set {s} frame {v['frame']} {q} ({v['share']})" for s, q, v in over)]
    sc = rep['scipy']
    L += ['', '## Refined rmse against scipy.optimize.least_squares on the captured matches (set A)', '']
    L.append(f"{sc['refined_frames']} refined frames; largest |rmse - scipy| / scipy = {sc['largest_relative_rmse_distance']:.3g} (frame {sc['frame']}); "
             f"the tests' bound is {sc['bound']}." if sc['status'] == 'measured' else sc['status'])
    L += ['', '## Host mirror per frame vs one device call per batch (960 x 540, frames of set A repeated)', '',
          '| B | frames with LM | host flow, whole batch, median ms | host ms / frame | device wall, refine off / on, median ms (p10-p90) | device events, pre-packed, refine off / on, median ms | host / device wall (refine off) |',
          '|---|---|---|---|---|---|---|']
    for c in rep.get('host_vs_device') or []:
        w0, w1 = c['refine_off']['device_wall'], c['refine_on']['device_wall']
        e0, e1 = c['refine_off']['device_events_packed'], c['refine_on']['device_events_packed']
        L.append(f"| {c['B']} | {c['frames_with_lm']} | {c['host']['median_ms']} | {c['host_ms_per_frame']} | {w0['median_ms']} ({w0['p10_ms']}-{w0['p90_ms']}) / "
                 f"{w1['median_ms']} ({w1['p10_ms']}-{w1['p90_ms']}) | {e0['median_ms']} / {e1['median_ms']} | {c['host_over_device_wall_refine_off']}x |")
    L += ['', 'The host column is baseline_cameras.frame_flow without the refinement (the host refinement is one device call per frame).  The wall '
          'column is line_cameras as a caller sees it: pack_annotations, one pinned upload, the launches, a synchronise.  The events column '
          'leaves the packing out.  These are latency kernels: one wavefront per frame.', '', '## Kernel time (trace)', '']
    kt = rep.get('kernel_trace')
    if kt:
        L += ['| kernel | workgroups (frames) | median ms | min - max | calls |', '|---|---|---|---|---|']
        for name, by_b in kt.items():
            for B, s in by_b.items():
                L.append(f"| {name} | {B} | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} | {s['calls']} |")
        L += ['', 'Frames that run the LM per batch: the "frames with LM" column above; the other workgroups of line_refine_kernel leave at once.']
    else:
        L.append(rep.get('kernel_trace_note') or 'not measured: no kernel trace was given')
    L += ['', '## One pass over a folder: line network -> two-peak decode -> cameras, beside export_extremities alone', '']
    f = rep.get('folder')
    if f:
        L += [f"line_hrnet_w48, engine {f['engine']}; frames: {f['frames_source']}; {f['files']} files; {f['runs']} runs each, alternating.", '',
              '| run | files written | frames/s, median | frames/s, each run |', '|---|---|---|---|']
        for r in f['rows']:
            L.append(f"| {r['run']} | {r['files_written']} | {r['frames_per_s_median']} | {r['frames_per_s']} |")
    else:
        L.append('not measured')
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=24, trace_dir=True, kernel_only=True)
    ap.add_argument('--runs', type=int, default=3, help='timed folder runs per form')
    ap.add_argument('--skip-folder', action='store_true')
    a = ap.parse_args()
    import torch
    dev = torch.device('cuda:0')
    if a.kernel_only:
        kernel_only(dev)
        return
    rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'shares': shares(dev), 'scipy': scipy_distance(dev),
           'host_vs_device': host_vs_device(dev, a.reps)}
    benchlib.add_trace(rep, a.trace_dir, read_trace)
    rep['folder'] = None if a.skip_folder else folder_rates(dev, a.runs)
    benchlib.write_report(rep, a.out, 'line_cameras', write_md)


if __name__ == '__main__':
    main()
