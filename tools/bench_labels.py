"""Measure keypoint-label generation, host against device -> profiles/labels.json + profiles/labels.md.

    python tools/bench_labels.py [--reps 16] [--frames 256] [--build LABEL] [--out DIR] [--skip-pipeline]

(a) annotations.get_intersections on the host, ms per frame of ONE process (the 24 frames of tests/golden/annotations.json and 40
    of synth.synthetic_annotation), against ONE call of annotations.keypoint_labels_device for 16 and for 64 of those frames:
    wall time of the whole call (packing on the host, one upload, the launch, synchronised) and device events around the launch
    alone; and the largest distance between the two paths' labels on these frames.
(b) validate(folder) and one epoch of train_batches, frames/s with labels='host' against labels='device' at the same commit, same
    process, alternating.  labels='host' is the path as it was before the kernel existed, so this is the A/B against it.
    make_submit on the same folder stands beside validate(): the gap DESIGN.md 7 asks about.
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


def frames_64():
    import labels_ref as lr
    return lr.fixture_frames()[0] + lr.synthetic_frames(40)


def host_ms_per_frame(annots):
    from sncal_amd import annotations as an
    pts = [{c: [(p['x'], p['y']) for p in v] for c, v in a.items()} for a in annots]
    an.get_intersections(pts[0])
    per = []
    for p in pts:
        t0 = time.perf_counter()
        an.get_intersections(p)
        per.append((time.perf_counter() - t0) * 1e3)
    return per


def label_cells(dev, reps):
    import torch
    from sncal_amd import annotations as an
    annots = frames_64()
    per = host_ms_per_frame(annots)
    host = {'frames': len(per), 'mean_ms_per_frame': round(float(np.mean(per)), 3), 'median_ms_per_frame': round(float(np.median(per)), 3),
            'min_ms_per_frame': round(float(np.min(per)), 3), 'max_ms_per_frame': round(float(np.max(per)), 3)}
    # the two paths' labels on these frames
    _, _, _, labels, present = an.keypoint_labels_device(annots, device=dev, return_labels=True)
    labels, present = labels.cpu().numpy(), present.cpu().numpy().astype(bool)
    worst, same = 0.0, True
    for b, a in enumerate(annots):
        hl, _ = an.get_intersections({c: [(p['x'], p['y']) for p in v] for c, v in a.items()})
        same = same and [hl[i] is not None for i in range(57)] == list(present[b])
        for i in range(57):
            if hl[i] is not None and present[b, i]:
                worst = max(worst, float(np.hypot(labels[b, i, 0] - hl[i][0], labels[b, i, 1] - hl[i][1])))
    cells = []
    for B in (16, 64):
        batch = annots[:B]

        def call():
            return an.keypoint_labels_device(batch, device=dev)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        wall = [benchlib.wall(call)[0] * 1e3 for _ in range(reps)]
        points, offsets, pres = an.pack_annotations(batch)
        t0 = time.perf_counter()
        for _ in range(reps):
            an.pack_annotations(batch)
        pack_ms = (time.perf_counter() - t0) * 1e3 / reps
        ev, _ = benchlib.timed(call, reps)                        # device events: the upload and the launch, queued behind the host's packing
        host_ms = float(np.sum(per[:B]))
        c = {'frames': B, 'points': int(len(points)), 'status': 'measured', 'host_ms': round(host_ms, 2), 'device_call_wall': benchlib.stats(wall),
             'device_events': benchlib.stats(ev), 'pack_ms': round(pack_ms, 3),
             'speedup_wall_median': round(host_ms / benchlib.stats(wall)['median_ms'], 1)}
        print(json.dumps(c), flush=True)
        cells.append(c)
    return host, cells, {'max_label_distance_px': worst, 'presence_identical': bool(same), 'frames': len(annots)}


def pipeline_rates(dev, n_frames):
    import sncal_amd
    with tempfile.TemporaryDirectory(prefix='sncal_labels_', ignore_cleanup_errors=True) as tmp:
        folder = os.path.join(tmp, 'valid')
        source = benchlib.jpeg_folder(folder, n_frames)
        model = benchlib.keypoint_model(tmp)
        cal = sncal_amd.submit.default_calibrator()
        A, V, F = sncal_amd.augment, sncal_amd.validate, sncal_amd.frames

        def epoch(labels, bs):
            import random
            random.seed(1)
            np.random.seed(1)
            n = 0
            for b in F.train_batches(folder, bs, A.train_transform(), shuffle=True, seed=0, device=dev, margin=3.0, labels=labels):
                n += len(b['img_name'])
            return n
        rows = []
        for bs in (16, 64):
            row = {'batch_size': bs, 'frames': n_frames, 'status': 'measured'}
            runs = {'validate_host': lambda: V.validate(model, folder, cal, batch_size=bs, transform=A.test_transform(), labels='host'),
                    'validate_device': lambda: V.validate(model, folder, cal, batch_size=bs, transform=A.test_transform(), labels='device'),
                    'train_batches_host': lambda: epoch('host', bs), 'train_batches_device': lambda: epoch('device', bs),
                    'make_submit': lambda: sncal_amd.submit.make_submit(folder, model, cal, os.path.join(tmp, 'out'), batch_size=bs)}
            times = {k: [] for k in runs}
            for k, run in runs.items():
                run()                                                      # warm: workspaces, decoder, allocator, sample tables
            for _ in range(3):                                             # alternating
                for k, run in runs.items():
                    times[k].append(benchlib.wall(run)[0])
            for k, t in times.items():
                row[k + '_frames_per_s'] = round(n_frames / float(np.median(t)), 1)
                row[k + '_s'] = [round(x, 4) for x in t]
            rows.append(row)
            print(json.dumps(row), flush=True)
        return {'engine': model.nn_module.dtype_name, 'frames_source': source, 'rows': rows}


def write_md(rep, path):
    L = ['# Keypoint labels: the host path against one launch of the label kernel', '',
         f"Device: {rep['device']}.  Build: {rep['build']}.  Every figure below is **measured** by `tools/bench_labels.py` unless it says otherwise.", '',
         '## get_intersections per frame on the host, one device call per batch', '']
    h = rep.get('host')
    if h:
        L += [f"Host, one process, {h['frames']} frames (24 of tests/golden/annotations.json, 40 of synth.synthetic_annotation): "
              f"{h['mean_ms_per_frame']} ms per frame (median {h['median_ms_per_frame']}, {h['min_ms_per_frame']}-{h['max_ms_per_frame']}).", '']
    L += ['| frames | points | host ms (sum of its frames) | device call, wall median ms (p10-p90) | of which packing on the host ms | device events median ms | host / device wall |',
          '|---|---|---|---|---|---|---|']
    for c in rep.get('cells', []):
        w, e = c['device_call_wall'], c['device_events']
        L.append(f"| {c['frames']} | {c['points']} | {c['host_ms']} | {w['median_ms']} ({w['p10_ms']}-{w['p90_ms']}) | {c['pack_ms']} | {e['median_ms']} | "
                 f"{c['speedup_wall_median']}x |")
    L += ['', 'The device call is annotations.keypoint_labels_device: packing the annotations on the host, one upload, one launch (one '
          'wavefront per frame), synchronised for the wall figure.  Device events bracket the upload and the launch.', '']
    a = rep.get('agreement')
    if a:
        L += [f"Agreement on these {a['frames']} frames: presence {'identical' if a['presence_identical'] else 'DIFFERENT'}, largest label "
              f"distance {a['max_label_distance_px']:.2e} px (the tests' bound is 1e-5 px).", '']
    L += ["## validate(folder) and train_batches, labels='host' against labels='device'", '']
    p = rep.get('pipeline')
    if p:
        L += [f"Engine {p['engine']}; frames: {p['frames_source']}.  Same process, alternating, median of 3 after a warm run; frames/s.", '',
              '| batch | frames | validate host | validate device | train_batches host | train_batches device | make_submit |', '|---|---|---|---|---|---|---|']
        for r in p['rows']:
            L.append(f"| {r['batch_size']} | {r['frames']} | {r['validate_host_frames_per_s']} | {r['validate_device_frames_per_s']} | "
                     f"{r['train_batches_host_frames_per_s']} | {r['train_batches_device_frames_per_s']} | {r['make_submit_frames_per_s']} |")
        L += ['', "labels='host' is the path as it was before the label kernel, unchanged, so the first column of each pair is the parent's "
              'behaviour.  Both validate() columns run test_transform() (FixLRAmbiguous: a second get_intersections per frame on the host '
              'path, the kernel\'s flag on the device path); train_batches runs train_transform() and only delivers the batches (no network).']
    else:
        L.append(rep.get('pipeline_note') or 'not measured')
    benchlib.write_lines(L, path)


def main():
    ap = argparse.ArgumentParser()
    benchlib.add_common_args(ap, reps=16)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--skip-pipeline', action='store_true')
    a = ap.parse_args()
    import torch
    dev = torch.device('cuda:0')
    host, cells, agreement = label_cells(dev, a.reps)
    rep = {'device': torch.cuda.get_device_name(0), 'build': a.build, 'host': host, 'cells': cells, 'agreement': agreement}
    if a.skip_pipeline:
        rep['pipeline'], rep['pipeline_note'] = None, 'not measured (--skip-pipeline)'
    else:
        rep['pipeline'] = pipeline_rates(dev, a.frames)
    benchlib.write_report(rep, a.out, 'labels', write_md)


if __name__ == '__main__':
    main()
