"""The measurement method of the tools/bench_*.py report tools, owned once: reading a rocprofv3 kernel trace, naming a traced
template instantiation, the two timers and their statistics, the synthetic split with its two throw-away checkpoints, and the
arguments / trace / output plumbing every main() shares.  What is measured, the byte models, the grouping rules of each tool's
read_trace and the text of each report stay in the tool.

Only the standard library and numpy are imported here, so a tool's trace reader and report writer load on a machine with no GPU and
no libsncal.so; torch, bench and sncal_amd are imported inside the functions that need them.  Importing this module puts the
repository root on sys.path for them.
"""
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12          # bytes/s, the achievable HBM rate of the MI355X
TRACE_ERRORS = (KeyError, ValueError, OSError)          # what a trace in another layout raises in the readers below


# ---- rocprofv3 --kernel-trace --output-format csv

def trace_rows(trace_dir, *names):
    """The dispatch rows of every kernel-trace file under trace_dir whose Kernel_Name contains one of `names`, in start-time order."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if any(n in r.get('Kernel_Name', '') for n in names)]
    return sorted(rows, key=lambda r: int(r['Start_Timestamp']))


def duration_ms(row):
    return (int(row['End_Timestamp']) - int(row['Start_Timestamp'])) * 1e-6


def workgroups(row, axis):
    """Workgroups along 'X' / 'Y' / 'Z': the trace gives the grid in work-items.  A workgroup size that is absent, empty or 0 counts as 1."""
    return int(row[f'Grid_Size_{axis}']) // max(int(row.get(f'Workgroup_Size_{axis}', 1) or 1), 1)


def warm(ms):
    """Durations of one kernel in time order without the first (cold) call, when there is another."""
    return ms[1:] if len(ms) > 1 else ms


def call_stats(ms):
    ms = warm(ms)
    return {'median_ms': round(float(np.median(ms)), 4), 'min_ms': round(float(min(ms)), 4), 'max_ms': round(float(max(ms)), 4), 'calls': len(ms)}


def roof_share(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / HBM_ACHIEVABLE, 3)


def template_flags(base, kernel_name):
    """The boolean template arguments of `base<...>` in kernel_name, in order, integer arguments left out -> list of bool, or None
    when the name holds no instantiation of base.  The trace holds the name demangled (`base<4, true, false>`) or Itanium-mangled
    (`baseILi4ELb1ELb0EE`), depending on the profiler's settings."""
    m = re.search(re.escape(base) + r'<([^<>]*)>', kernel_name)
    if m:
        return [a.strip() == 'true' for a in m.group(1).split(',') if a.strip() in ('true', 'false')]
    m = re.search(re.escape(base) + r'I((?:L[a-z]\d+E)+)E', kernel_name)
    if m:
        return [v == '1' for t, v in re.findall(r'L([a-z])(\d+)E', m.group(1)) if t == 'b']
    return None


# ---- timers

def timed(fn, reps, other=None):
    """reps timings of fn in ms (device events), alternating with `other` when given -> (ms list, ms list of other)."""
    import torch
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


def wall(fn):
    """One call of fn between two synchronisations -> (seconds on the host's clock, fn's result)."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def peak_temp(fn):
    """Peak bytes fn allocates on the device beyond what was allocated before it."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    del r
    return torch.cuda.max_memory_allocated() - base


def stats(ms, digits=4, minmax=True, percentiles='index'):
    """Median and spread of repeated timings.  percentiles: 'index' (p10 / p90 are the sorted values at n // 10 and 9 n // 10),
    'linear' (np.percentile's interpolation) or None (no p10 / p90)."""
    a = np.sort(np.asarray(ms, dtype=np.float64))
    out = {'median_ms': round(float(np.median(a)), digits)}
    if minmax:
        out.update(min_ms=round(float(a[0]), digits), max_ms=round(float(a[-1]), digits))
    if percentiles:
        p10, p90 = (a[len(a) // 10], a[(9 * len(a)) // 10]) if percentiles == 'index' else np.percentile(a, (10, 90))
        out.update(p10_ms=round(float(p10), digits), p90_ms=round(float(p90), digits))
    out['reps'] = len(a)
    return out


# ---- the synthetic split and the two checkpoints

def jpeg_folder(path, n):
    """n frames + annotations.  Stamped synthetic frames encoded with Pillow when it is installed (baseline, 4:4:4, quality 98);
    otherwise the golden 960x540 JPEG, whose pixels mean nothing to the network (no keypoints, trivial solves)."""
    import sncal_amd
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


def _load(tmp, file, ck):
    import torch
    import sncal_amd
    path = os.path.join(tmp, file)
    torch.save(ck, path)
    return sncal_amd.load_model(path, device='cuda:0')


def keypoint_model(tmp):
    """hrnet_w48 with random-init weights that keep the designed signal path, through a checkpoint written into the caller's tmp."""
    import bench
    import sncal_amd
    return _load(tmp, 'model.pth', {
        'model_name': 'HRNetMetaModel',
        'params': {'nn_module': {'hrnet_config': sncal_amd.load_config('hrnet_w48'), 'num_refinement_stages': 0, 'num_heatmaps': 58},
                   'loss': {'num_refinement_stages': 0, 'stride': 2, 'sigma': 2.0, 'pred_size': [270, 480], 'num_keypoints': 57},
                   'prediction_transform': {'size': [540, 960]}, 'device': 'cuda:0'},
        'nn_state_dict': sncal_amd.synth.peaked_state_dict(bench.seeded_weights('hrnet_w48', seed=1), deep=True)})


def line_model(tmp):
    """line_hrnet_w48, the same way."""
    import bench
    import sncal_amd
    bare = {k: v for k, v in sncal_amd.load_config('line_hrnet_w48').items() if k not in ('head', 'upscale')}
    return _load(tmp, 'line.pth', {
        'model_name': 'EHMMetaModel',
        'params': {'nn_module': {'hrnet_config': bare, 'num_refinement_stages': 0, 'num_heatmaps': 23},
                   'loss': {'num_refinement_stages': 0, 'gmse_w': 1.0, 'awing_w': 1.0, 'sigma': 4},
                   'prediction_transform': {'scale': 4, 'sigma': 3}, 'device': 'cuda:0'},
        'nn_state_dict': sncal_amd.synth.line_deep_state_dict(bench.seeded_weights('line_hrnet_w48', seed=2))})


# ---- what every main() does

def add_common_args(ap, reps, trace_dir=False, kernel_only=False):
    if kernel_only:
        ap.add_argument('--kernel-only', action='store_true')
    if trace_dir:
        ap.add_argument('--trace-dir', default=None)
    ap.add_argument('--reps', type=int, default=reps)
    ap.add_argument('--build', default='unlabelled', help='label of the build the figures come from (written into the report)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))


def add_trace(rep, trace_dir, read, key='kernel_trace'):
    """rep[key] = read(trace_dir) when a trace directory is given.  A trace in another layout: say so, keep the rest of the report."""
    if trace_dir:
        try:
            rep[key] = read(trace_dir) or None
        except TRACE_ERRORS as e:
            rep[key], rep[key + '_note'] = None, f'not measured: the kernel trace could not be read ({e!r})'


def write_lines(lines, path):
    with open(path, 'w') as f:
        f.write('\n'.join(lines + ['']))


def write_report(rep, out, stem, write_md):
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, stem + '.json'), 'w') as f:
        json.dump(rep, f, indent=1)
    write_md(rep, os.path.join(out, stem + '.md'))
    print('wrote', os.path.join(out, stem + '.json'))
