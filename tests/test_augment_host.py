"""CPU: the host half of the train-time augmentation against the reference capture (tests/golden/augment.npz, written by
tools/make_golden_augment.py): the numpy restatement of the kernel's stages (tests/augment_ref.py), the parameter draws of a seeded
transform, every label transform, validate()'s opt-in transform, and the C entry point's argument checks.

Colour tolerance rule: every element equals the reference's uint8 EXACTLY, except elements whose fp64 pre-truncation value lies
within 2^-20 of an integer (the kernel's mean comes from exact integer sums, numpy's from a sum of rounded products: they differ by
parts in 1e12); at most ONE such element per case.  The fixture's seeds leave out none."""
import copy
import ctypes
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import augment_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'augment.npz'))


def unjson(a):
    return json.loads(a.tobytes().decode())


def check_colour(got, want, near, what):
    """The tolerance rule: exact outside `near`, and at most one element of `near` may differ."""
    diff = got != want
    assert not (diff & ~near).any(), (what, int((diff & ~near).sum()))
    assert int((diff & near).sum()) <= 1, (what, int((diff & near).sum()))
    return int((diff & near).sum())


def test_helper_matches_reference_colour(gold):
    for name in gold['colour.names']:
        img, gain, contrast = gold[f'colour.{name}.in'], gold[f'colour.{name}.gain'], float(gold[f'colour.{name}.contrast'])
        got, near = ar.augment(img, ar.FLAG_COLOUR, gain, contrast)
        assert check_colour(got, gold[f'colour.{name}.out'], near, name) == 0 and not near.any()      # the fixture's seeds leave out none
        assert np.abs(ar.device_mean(img, gain) - ar.numpy_mean(img, gain)).max() < 1e-10
        # the recorded draws are what the seeded generator gives in the reference's call order
        rs = np.random.RandomState(int(gold[f'colour.{name}.seed']))
        br, co, ct = gold[f'colour.{name}.ranges']
        assert np.array_equal(rs.uniform(br[0], br[1]) * rs.uniform(co[0], co[1], 3), gain) and rs.uniform(ct[0], ct[1]) == contrast
    assert (gold['colour.dark.out'] == 0).any() and (gold['colour.bright.out'] == 255).any()           # both clips occur


def test_helper_matches_reference_noise(gold):
    for name in gold['noise.names']:
        img = gold[f'colour.{name}.in']
        _, n = ar.reference_normals(int(gold[f'noise.{name}.seed']), img.shape)
        assert np.array_equal(ar.noise(img, n), gold[f'noise.{name}.out']), name


def composite_transform(A):
    """The fixture's pipeline: train_transform's stages with the noise probability at 0."""
    return A.ComposeTransform([A.UseWithProb(A.ColorAugment(), 0.5), A.UseWithProb(A.GaussNoise(30.0), 0.0), A.UseWithProb(A.Flip(), 0.5),
                               A.FixLRAmbiguous()])


def test_seeded_draws_and_labels_match_reference_composite(sncal, gold):
    A = sncal.augment
    annots = unjson(gold['composite.annot_in'])
    keep = copy.deepcopy(annots)
    random.seed(int(gold['composite.seeds'][0]))
    np.random.seed(int(gold['composite.seeds'][1]))
    params, samples = composite_transform(A).draw_batch(len(annots), 32, annots)
    assert [p.flags for p in params] == gold['composite.flags'].tolist()
    assert np.array_equal(np.array([list(p.gain) for p in params]), gold['composite.gain'])
    assert np.array_equal(np.array([p.contrast for p in params]), gold['composite.contrast'])
    want = unjson(gold['composite.annot_out'])
    for s, w, sw in zip(samples, want, gold['composite.swapped']):
        assert s.annot == w and list(s.annot) == list(w) and s.swapped == bool(sw)
    assert annots == keep                                                   # the caller's annotations are left as they were
    # the helper on the recorded draws gives the reference's images
    for i, p in enumerate(params):
        got, near = ar.augment(gold['composite.in'][i], p.flags, list(p.gain), p.contrast)
        assert check_colour(got, gold['composite.out'][i], near, i) == 0
    # the factories keep the reference's composition
    t = A.train_transform(prob=0.25)
    assert [type(x).__name__ for x in t.transforms] == ['UseWithProb', 'UseWithProb', 'UseWithProb', 'FixLRAmbiguous', 'ToTensor']
    assert [x.prob for x in t.transforms[:3]] == [0.25, 0.25, 0.5] and isinstance(t.transforms[2].transform, A.Flip)
    assert [type(x).__name__ for x in A.test_transform().transforms] == ['FixLRAmbiguous', 'ToTensor']
    lt = A.line_train_transform()
    assert isinstance(lt.transforms[2].transform, A.LineFlip) and [type(x).__name__ for x in A.line_test_transform().transforms] == ['ToTensor']


def test_noise_draws_follow_the_reference_order(sncal):
    """With noise on: the scale is np.random.uniform(0, sigma_sq) right after the colour draws, then one 64-bit seed."""
    A = sncal.augment
    random.seed(1)
    np.random.seed(2)
    params, _ = A.ComposeTransform([A.ColorAugment(), A.GaussNoise(30.0), A.ToTensor()]).draw_batch(2, 8)
    rs = np.random.RandomState(2)
    for p in params:
        gain = rs.uniform(0.8, 1.2) * rs.uniform(0.8, 1.2, 3)
        contrast = rs.uniform(0.8, 1.2)
        sigma = rs.uniform(0.0, 30.0)
        seed = int(rs.randint(0, 2 ** 64, dtype=np.uint64))
        assert (list(p.gain), p.contrast, p.noise_sigma, p.seed, p.flags) == (list(gain), contrast, sigma, seed, 3)
    with pytest.raises(sncal._lib.SncalError):                              # the kernel's stage order is fixed
        A.ComposeTransform([A.GaussNoise(), A.ColorAugment()]).draw_batch(1, 8)


def test_label_transforms_match_reference(sncal, gold):
    A = sncal.augment
    cases = unjson(gold['labels.cases'])
    fix = A.FixLRAmbiguous()
    assert sum(c['swapped'] for c in cases) >= 4 and sum(not c['swapped'] for c in cases) >= 4
    assert {'medians', 'count'} <= {c['branch'] for c in cases}
    for c in cases:
        a = c['in']
        keep = copy.deepcopy(a)
        got = A.flip_annot_names(a)
        assert list(got) == c['flip_names'] and all(got[k] is a[k0] for k, k0 in zip(got, a)), c['name']
        got = A.flip_annot(a)
        assert got == c['flip'] and list(got) == list(c['flip']), c['name']
        swap, branch = fix.decide(a)
        assert (swap, branch) == (c['swapped'], c['branch']), c['name']
        got = A.test_transform().labels(a)
        assert list(got) == c['fix_names'] and all(got[k] == a[k0] for k, k0 in zip(got, a)), c['name']
        assert a == keep
    assert A.swap_top_bottom_names('Big rect. left top') == 'Big rect. left bottom' and A.swap_top_bottom_names('Middle line') == 'Middle line'
    assert A.swap_posts_names('Goal left post left ') == 'Goal left post right' and A.swap_posts_names('Side line top') == 'Side line top'
    assert A.mirror_labels({'Side line left': 1, 'Circle central': 2}) == {'Side line right': 1, 'Circle central': 2}
    with pytest.raises(sncal._lib.SncalError):                              # an image transform is no label transform
        A.train_transform(prob=1.0).labels(cases[0]['in'])


def test_line_flip_keypoints_match_reference(sncal, gold):
    rows = gold['line.in'].copy()
    for r, want in zip(rows, gold['line.out']):
        out = sncal.augment.flip_keypoints(r, int(gold['line.w']))
        assert out is r and np.array_equal(out, want)                       # in place, as the reference
    x, flag = gold['line.in'].reshape(-1, 3)[:, 0], gold['line.in'].reshape(-1, 3)[:, 2]
    moved = gold['line.in'].reshape(-1, 3)[:, 0] != gold['line.out'].reshape(-1, 3)[:, 0]
    assert moved.any() and not moved[(flag == 0) | (x == -1)].any()
    assert ((flag == 0) & (x != -1)).any() and ((flag == 1) & (x == -1)).any()      # the fixture holds the two cases that stay


def test_validate_labels_with_and_without_the_transform(sncal, gold, tmp_path):
    """A split folder of the fixture's annotations: transform=None labels are what annot_to_keypoints and scale_points give on the
    files as they are (the labelling before this option existed); with test_transform() the frames the reference swaps differ,
    the others do not."""
    V, F, A = sncal.validate, sncal.frames, sncal.augment
    cases = unjson(gold['labels.cases'])[:10]
    for i, c in enumerate(cases):
        (tmp_path / f'{i:05d}.json').write_text(json.dumps(c['in']))
        (tmp_path / f'{i:05d}.jpg').write_bytes(b'\xff\xd8')
    names, annots = F.list_split(str(tmp_path))
    plain = F.labelled_batch(None, annots, names, 57, 2.0, (960, 540))
    for i, a in enumerate(annots):
        kp, mask = F.annot_to_keypoints(a, 57, 2.0)
        assert np.array_equal(plain['keypoints'][i].numpy(), kp) and np.array_equal(plain['mask'][i].numpy(), mask)
        assert plain['raw_annot'][i] == sncal.evaluate.scale_points(a, 960, 540)
    assert plain['img_name'] == names and plain['keypoints'].dtype.is_floating_point and tuple(plain['keypoints'].shape) == (len(cases), 171)
    t = A.test_transform()
    fixed = F.labelled_batch(None, [t.labels(a) for a in annots], names, 57, 2.0, (960, 540))
    swapped = [c['swapped'] for c in cases]
    assert any(swapped) and not all(swapped)
    for i, sw in enumerate(swapped):
        same = np.array_equal(plain['keypoints'][i].numpy(), fixed['keypoints'][i].numpy()) and plain['raw_annot'][i] == fixed['raw_annot'][i]
        assert same == (not sw), i
    with pytest.raises(sncal._lib.SncalError, match='folder form'):         # batches handed in carry their labels already
        V.validate(None, [], sncal.CameraCreator(sncal.PITCH_POINTS), transform=t)


def test_entry_point_validates_its_arguments_without_a_gpu(sncal):
    L = sncal._lib
    lib = L.lib()
    ERR_ARG, ERR_WS = -1, -4
    n = ctypes.c_size_t()
    assert lib.sncal_augment_workspace(4, 540, 960, ctypes.byref(n)) == 0 and n.value >= 4 * 3 * 8 and n.value % 16 == 0
    big = n.value
    assert lib.sncal_augment_workspace(4, 70, 130, ctypes.byref(n)) == 0 and 4 * 2 * 3 * 8 <= n.value <= big       # several workgroups per frame
    assert lib.sncal_augment_workspace(0, 540, 960, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.sncal_augment_workspace(4, 540, 960, None) == ERR_ARG
    assert lib.sncal_augment_workspace(4, 0, 960, ctypes.byref(n)) == ERR_ARG and lib.sncal_augment_workspace(4, 540, 0, ctypes.byref(n)) == ERR_ARG
    assert lib.sncal_augment_workspace(-1, 540, 960, ctypes.byref(n)) == ERR_ARG
    assert lib.sncal_augment_workspace(1, 40000, 40000, ctypes.byref(n)) == ERR_ARG and b'2^31' in lib.sncal_last_error()
    src, par, dst, ws = (ctypes.c_void_p(a) for a in (1 << 20, 2 << 20, 3 << 20, 4 << 20))      # dummy pointers; never dereferenced here
    B, H, W = 2, 17, 64
    lib.sncal_augment_workspace(B, H, W, ctypes.byref(n))
    assert lib.sncal_augment_u8(None, 0, H, W, None, None, None, None, None, 0, None) == 0      # B = 0 touches no pointer
    assert lib.sncal_augment_u8(None, B, H, W, par, None, dst, None, ws, n.value, None) == ERR_ARG and b'null' in lib.sncal_last_error()
    assert lib.sncal_augment_u8(src, B, H, W, None, None, dst, None, ws, n.value, None) == ERR_ARG
    assert lib.sncal_augment_u8(src, B, H, W, par, None, None, None, ws, n.value, None) == ERR_ARG and b'both outputs' in lib.sncal_last_error()
    assert lib.sncal_augment_u8(src, B, 0, W, par, None, dst, None, ws, n.value, None) == ERR_ARG
    assert lib.sncal_augment_u8(src, B, H, 0, par, None, dst, None, ws, n.value, None) == ERR_ARG
    assert lib.sncal_augment_u8(src, -1, H, W, par, None, dst, None, ws, n.value, None) == ERR_ARG
    nbytes = B * H * W * 3
    for d in (src.value, src.value + nbytes - 1, src.value - nbytes + 1):                     # dst inside, at the end, before the start
        assert lib.sncal_augment_u8(src, B, H, W, par, None, ctypes.c_void_p(d), None, ws, n.value, None) == ERR_ARG
        assert b'overlaps' in lib.sncal_last_error()
    assert lib.sncal_augment_u8(src, B, H, W, par, None, None, ctypes.c_void_p(src.value - 4 * nbytes + 4), ws, n.value, None) == ERR_ARG
    assert lib.sncal_augment_u8(src, B, H, W, par, None, dst, dst, ws, n.value, None) == ERR_ARG  # the two outputs on each other
    assert lib.sncal_augment_u8(src, B, H, W, par, ctypes.c_void_p(dst.value - 8 * nbytes + 8), dst, None, ws, n.value, None) == ERR_ARG
    assert b'd_noise overlaps' in lib.sncal_last_error()                                        # the normals end inside an output
    assert lib.sncal_augment_u8(src, B, H, W, par, None, dst, None, None, n.value, None) == ERR_ARG
    assert lib.sncal_augment_u8(src, B, H, W, par, None, dst, None, ctypes.c_void_p(ws.value + 8), n.value, None) == ERR_ARG
    assert lib.sncal_augment_u8(src, B, H, W, par, None, dst, None, ws, n.value - 1, None) == ERR_WS and b'need' in lib.sncal_last_error()
    if not __import__('torch').cuda.is_available():
        with pytest.raises(L.SncalError):                                   # no CPU path
            sncal.augment.train_transform()({'image': __import__('torch').zeros((1, 4, 4, 3), dtype=__import__('torch').uint8), 'annot': [{}]})


def test_struct_layout_matches_what_a_c_compiler_sees(sncal, tmp_path):
    L = sncal._lib
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    ct, cname = L.AugmentParams, 'sncal_augment_params'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "' + os.path.join(ROOT, 'include', 'sncal.h') + '"', 'int main(void) {',
             f'  printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));' for f in ct._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.check_call([gcc, str(tmp_path / 'layout.c'), '-o', str(tmp_path / 'layout')])
    seen = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / 'layout')]).decode().splitlines())
    assert int(seen[cname]) == ctypes.sizeof(ct) == 56
    for f in ct._fields_:
        assert int(seen[f[0]]) == getattr(ct, f[0]).offset, f[0]
