"""Capture tests/golden/augment.npz from the imported reference (CPU): ColorAugment, GaussNoise, the keypoint model's composed
train_transform stages, the label transforms (flip_annot_names, Flip, FixLRAmbiguous) and the line model's flip_keypoints.

    python tools/make_golden_augment.py

The reference is imported with the stubs of tools/make_golden.py.  Two things are put in the place of third-party code:
  * the stub cv2 gets a `flip` that reverses the columns (cv2.flip(img, 1) is nothing else);
  * get_intersections' ellipse fit and homography are this build's, exactly as tools/make_golden.py does for annotations.json.
ToTensor is left out of the captured pipelines (torchvision is a stub): images are stored as the uint8 arrays that enter it.
Images are tiny; the file stays below the 256 KiB limit (about 227 KiB, most of it the label cases' JSON text).  It is written with fixed zip timestamps, so a second run gives the same bytes.
A candidate set that does not hold the label cases the tests need (see gen_labels) makes the tool fail instead of writing.
"""
import contextlib
import copy
import io
import json
import os
import random
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import make_golden as mg  # noqa: E402

mg.install_stubs()
sys.modules['cv2'].flip = lambda img, code: {1: lambda a: np.ascontiguousarray(a[:, ::-1])}[code](img)      # horizontal only
for _name in ('matplotlib', 'matplotlib.pyplot', 'tqdm'):                  # plotting / progress bars of the baseline scripts
    try:
        __import__(_name)
    except ImportError:
        sys.modules[_name] = types.ModuleType(_name)
        if _name == 'tqdm':
            sys.modules[_name].tqdm = lambda it, *a, **k: it

import augment_ref as ar  # noqa: E402
import sncal_amd  # noqa: E402
from sncal_amd import annotations as an  # noqa: E402
from sncal_amd import augment as mine  # noqa: E402


class Fit:
    def fit(self, X):
        q = an.fit_ellipse(np.asarray(X, dtype=np.float64))
        self.coefficients = list(q) if q is not None else []
        return self


sys.modules['ellipse'].LsqEllipse = Fit
sys.modules['cv2'].findHomography = lambda src, dst, method, thr: (an.homography_ransac(src, dst, thr), None)
import src.datatools.ellipse as rel  # noqa: E402
rel.LsqEllipse = Fit
import src.models.hrnet.transforms as rt  # noqa: E402
import src.models.line.transforms as rlt  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
SHAPES = [(10, 37, 3), (17, 64, 3), (70, 130, 3)]
DEFAULT = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2))


def as_bytes(obj):
    """JSON as a uint8 array (utf-8): a numpy string array would take four bytes per character."""
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def image(seed, shape, lo=0, hi=256):
    return np.random.Generator(np.random.PCG64(seed)).integers(lo, hi, shape, dtype=np.uint8)


def gen_colour(out):
    """name, seed, image, (brightness, color, contrast) ranges.  The two narrow-range images make both clips occur."""
    cases = [(f'{h}x{w}', 100 + i, image(10 + i, (h, w, c)), DEFAULT) for i, (h, w, c) in enumerate(SHAPES)]
    cases.append(('dark', 104, image(14, (12, 40, 3), 0, 13), ((0.8, 1.2), (0.8, 1.2), (1.5, 2.0))))
    cases.append(('bright', 105, image(15, (12, 40, 3), 243, 256), ((1.1, 1.3), (0.95, 1.05), (1.5, 2.0))))
    out['colour.names'] = np.array([c[0] for c in cases])
    for name, seed, img, (br, co, ct) in cases:
        np.random.seed(seed)
        got = rt.ColorAugment(brightness=br, color=co, contrast=ct)._img_aug(img.copy())
        rs = np.random.RandomState(seed)                                        # the same stream, the same calls: the recorded draws
        gain = rs.uniform(br[0], br[1]) * rs.uniform(co[0], co[1], 3)
        contrast = rs.uniform(ct[0], ct[1])
        ref_mean = ar.numpy_mean(img, gain)
        again, v = ar.colour(img, gain, contrast, mean=ref_mean)
        assert np.array_equal(again, got), name                                 # the draws are the reference's
        helper, vh = ar.colour(img, gain, contrast)
        near = np.abs(vh - np.rint(vh)) <= ar.RADIUS
        assert np.array_equal(helper[~near], got[~near]) and not near.any(), (name, int(near.sum()))       # the rule leaves out none
        if name == 'dark':
            assert (v < 0).any() and (got == 0).any()
        if name == 'bright':
            assert (v > 255).any() and (got == 255).any()
        assert got.dtype == np.uint8
        np.random.seed(seed)
        assert np.array_equal(rlt.ColorAugment(brightness=br, color=co, contrast=ct)._img_aug(img.copy()), got)  # the line model's copy
        out[f'colour.{name}.seed'] = np.array(seed)
        out[f'colour.{name}.ranges'] = np.array([br, co, ct], dtype=np.float64)
        out[f'colour.{name}.in'], out[f'colour.{name}.out'] = img, got
        out[f'colour.{name}.gain'], out[f'colour.{name}.contrast'] = gain, np.array(contrast)
        print(f'colour {name}: mean device - numpy {np.abs(ar.device_mean(img, gain) - ref_mean).max():.3g}, near-integer elements 0 of {img.size}')


def gen_noise(out):
    out['noise.names'] = np.array([f'{h}x{w}' for h, w, _ in SHAPES])
    for i, (h, w, c) in enumerate(SHAPES):
        name, seed, img = f'{h}x{w}', 200 + i, out[f'colour.{h}x{w}.in']                  # the colour case's input again
        np.random.seed(seed)
        got = rt.GaussNoise(30.0)({'image': img.copy()})['image']
        scale, n = ar.reference_normals(seed, img.shape, 30.0)
        assert np.array_equal(ar.noise(img, n), got), name
        assert (got == 0).any() and (got == 255).any()
        out[f'noise.{name}.seed'] = np.array(seed)
        out[f'noise.{name}.out'] = got
        print(f'noise {name}: scale {scale:.4f}')


class Recorder:
    """Wraps a reference transform: notes that it ran on the current sample."""

    def __init__(self, transform, flag, log):
        self.transform, self.flag, self.log = transform, flag, log

    def __call__(self, sample):
        self.log[-1]['flags'] |= self.flag
        return self.transform(sample)


def gen_composite(out, cands):
    """The reference's keypoint train_transform stages with the noise probability at 0, on 8 samples, python's and numpy's
    generators seeded once; the uniform draws are recorded by a wrapper around numpy.random.uniform."""
    names = ['0.main', '0.both', '0.both.mirrored', '1.both', '1.left.mirrored', '1.main', '1.both.mirrored', '2.right']
    log, draws = [], []
    pipeline = rt.ComposeTransform([rt.UseWithProb(Recorder(rt.ColorAugment(), ar.FLAG_COLOUR, log), 0.5),
                                    rt.UseWithProb(Recorder(rt.GaussNoise(30.0), ar.FLAG_NOISE, log), 0.0),
                                    rt.UseWithProb(Recorder(rt.Flip(), ar.FLAG_FLIP, log), 0.5), rt.FixLRAmbiguous()])
    uniform = np.random.uniform

    def recording(*a, **k):
        r = uniform(*a, **k)
        draws.append(np.atleast_1d(r).astype(np.float64))
        return r
    imgs = np.stack([image(30 + i, (18, 32, 3)) for i in range(len(names))])
    random.seed(5)
    np.random.seed(7)
    outs, annots_out, swapped = [], [], []
    np.random.uniform = recording
    try:
        for i, nm in enumerate(names):
            log.append({'flags': 0})
            n0 = len(draws)
            with contextlib.redirect_stdout(io.StringIO()):
                s = pipeline({'image': imgs[i].copy(), 'annot': copy.deepcopy(cands[nm]), 'swapped': False})
            d = draws[n0:]
            if log[-1]['flags'] & ar.FLAG_COLOUR:
                assert len(d) == 3 and d[0].size == 1 and d[1].size == 3 and d[2].size == 1
                log[-1]['gain'], log[-1]['contrast'] = (d[0][0] * d[1]).tolist(), float(d[2][0])
            else:
                assert len(d) == 0
                log[-1]['gain'], log[-1]['contrast'] = [1.0, 1.0, 1.0], 1.0
            outs.append(s['image'])
            annots_out.append(s['annot'])
            swapped.append(bool(s['swapped']))
    finally:
        np.random.uniform = uniform
    flags = [e['flags'] for e in log]
    assert any(f & ar.FLAG_COLOUR for f in flags) and any(f & ar.FLAG_FLIP for f in flags) and any(f == 0 for f in flags), flags
    assert any(swapped) and not all(swapped), swapped
    out['composite.seeds'] = np.array([5, 7])
    out['composite.in'], out['composite.out'] = imgs, np.stack(outs)
    out['composite.annot_in'] = as_bytes([cands[nm] for nm in names])
    out['composite.annot_out'] = as_bytes(annots_out)
    out['composite.swapped'] = np.array(swapped)
    out['composite.flags'] = np.array(flags)
    out['composite.gain'] = np.array([e['gain'] for e in log])
    out['composite.contrast'] = np.array([e['contrast'] for e in log])
    print('composite: flags', flags, 'swapped', swapped)


def gen_labels(out, cands):
    """flip_annot_names, Flip and FixLRAmbiguous on every candidate of seeds 0..2.  Required of the set: at least 4 annotations the
    reference swaps and 4 it does not, at least one decision by the medians branch and one by the side-count branch.
    The reference's FixLRAmbiguous returns only whether it swapped, so 'swapped' and the key order are the reference's, while
    'branch' is what this package's FixLRAmbiguous.decide reports (it restates the reference's control flow line by line and must
    agree on 'swapped' here): the branch condition on the set, and a test's comparison of the branch, rest on this build's logic."""
    names = [n for n in cands if int(n.split('.')[0]) < 3]
    fix, my_fix = rt.FixLRAmbiguous(), mine.FixLRAmbiguous()
    rec = []
    for nm in names:
        a = cands[nm]
        e = {'name': nm, 'in': a}
        r = rt.flip_annot_names(copy.deepcopy(a))
        assert all(r[k] == a[k0] for k, k0 in zip(r, a))
        e['flip_names'] = list(r)                                             # values unchanged, in this key order
        e['flip'] = rt.Flip()({'image': np.zeros((2, 2, 3), np.uint8), 'annot': copy.deepcopy(a)})['annot']
        with contextlib.redirect_stdout(io.StringIO()):
            s = fix({'annot': copy.deepcopy(a), 'swapped': False})
        assert all(s['annot'][k] == a[k0] for k, k0 in zip(s['annot'], a))
        e['fix_names'], e['swapped'] = list(s['annot']), bool(s['swapped'])
        swap, branch = my_fix.decide(a)
        assert swap == e['swapped'], nm
        e['branch'] = branch
        rec.append(e)
    n_swapped = sum(e['swapped'] for e in rec)
    branches = {e['branch'] for e in rec}
    if n_swapped < 4 or len(rec) - n_swapped < 4 or not {'medians', 'count'} <= branches:
        raise SystemExit(f'label set unusable: {n_swapped} swapped of {len(rec)}, branches {branches}')
    assert any(e['swapped'] and e['branch'] == 'medians' for e in rec) and any(e['swapped'] and e['branch'] == 'count' for e in rec)
    out['labels.cases'] = as_bytes(rec)
    for name in ('Side line top', 'Big rect. left bottom', 'Goal left post left ', 'Goal right post right', 'Middle line', 'Circle left'):
        assert mine.swap_top_bottom_names(name) == rt.swap_top_bottom_names(name) and mine.swap_posts_names(name) == rt.swap_posts_names(name)
    print(f'labels: {len(rec)} annotations, {n_swapped} swapped, branches {sorted(b for b in branches if b)}')


def gen_line_labels(out):
    rng = np.random.Generator(np.random.PCG64(61))
    rows = []
    for _ in range(4):
        kp = np.ones(23 * 6, dtype=np.float32) * -1
        for i in range(46):
            u = rng.uniform()
            if u < 0.6:
                kp[i * 3:i * 3 + 3] = (rng.uniform(0, 959), rng.uniform(0, 539), 1)
            elif u < 0.75:
                kp[i * 3:i * 3 + 3] = (rng.uniform(0, 959), rng.uniform(0, 539), 0)        # flag 0 with coordinates: not flipped
            elif u < 0.85:
                kp[i * 3:i * 3 + 3] = (-1, rng.uniform(0, 539), 1)                         # x == -1 with flag 1: not flipped
            else:
                kp[i * 3 + 2] = 0
        rows.append(kp)
    rows = np.stack(rows)
    out['line.in'] = rows
    out['line.w'] = np.array(960)
    out['line.out'] = np.stack([rlt.flip_keypoints(r.copy(), 960) for r in rows])
    assert not np.array_equal(out['line.in'], out['line.out'])


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    out = {}
    cands = dict(ar.candidate_annotations(sncal_amd))
    gen_colour(out)
    gen_noise(out)
    gen_composite(out, cands)
    gen_labels(out, cands)
    gen_line_labels(out)
    path = os.path.join(GOLD, 'augment.npz')
    write_npz(path, out)
    size = os.path.getsize(path)
    print(path, size, 'bytes')
    assert size < 256 * 1024


if __name__ == '__main__':
    main()
