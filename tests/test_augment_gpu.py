"""GPU: sncal_augment_u8 (csrc/augment.hip) against the reference capture tests/golden/augment.npz and the numpy restatement
tests/augment_ref.py, and the host mirror end to end.

Colour tolerance rule: every element equals the reference's uint8 EXACTLY, except elements whose fp64 pre-truncation value (from
the helper) lies within 2^-20 of an integer; at most ONE such element per case.  Noise from a handed-in array, flip, ToTensor and
the path identity are exact.  The device generator is checked for what it promises (a frame's noise depends on its seed and its
source positions only) and for its distribution, with six-sigma bounds of the sampling distributions: for N samples of
out + 0.5 - 128 (out = floor(128 + sigma z), so out + 0.5 has the mean of 128 + sigma z and its variance plus 1/12) the mean has
standard deviation sigma / sqrt(N), the variance sigma^2 sqrt(2 / N), a lag-1 correlation 1 / sqrt(N), and chi-square over d
degrees of freedom has mean d and standard deviation sqrt(2 d).  The run is deterministic: it passes or fails for good."""
import ctypes
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import augment_ref as ar
from test_augment_host import check_colour, composite_transform, unjson

pytestmark = pytest.mark.gpu

COLOUR, NOISE, FLIP = ar.FLAG_COLOUR, ar.FLAG_NOISE, ar.FLAG_FLIP


def torch_to_tensor(u8, dims):
    """torch's (u8.permute -> float32).div(255), evaluated on the host where the reference's ToTensor runs: there div(255) is the
    correctly rounded fp32 division.  On the device torch turns a division by a Python scalar into a multiplication by
    float32(1 / 255), which rounds 126 of the 256 byte values differently; that is not what ToTensor gives a loader worker."""
    return u8.cpu().permute(*dims).to(torch.float32).div(255)


@pytest.fixture(scope='module')
def gold(gold_dir):
    return np.load(os.path.join(gold_dir, 'augment.npz'))


def params_of(sncal, rows):
    """rows: dicts with flags and optionally gain, contrast, sigma, seed."""
    p = (sncal._lib.AugmentParams * len(rows))()
    for i, r in enumerate(rows):
        g = r.get('gain', (1.0, 1.0, 1.0))
        p[i].gain[0], p[i].gain[1], p[i].gain[2] = float(g[0]), float(g[1]), float(g[2])
        p[i].contrast, p[i].noise_sigma, p[i].seed, p[i].flags = float(r.get('contrast', 1.0)), float(r.get('sigma', 0.0)), int(r.get('seed', 0)), r['flags']
    return p


def run(sncal, cuda, imgs, rows, noise=None, u8=True, chw=False):
    out = sncal.augment.augment_u8(torch.from_numpy(np.ascontiguousarray(imgs)).to(cuda), params_of(sncal, rows),
                                   noise=None if noise is None else torch.from_numpy(noise).to(cuda), want_u8=u8, want_chw=chw)
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def test_colour_matches_reference_with_mixed_flags(sncal, cuda, gold):
    """B = 3 of one fixture image: colour, untouched, colour + flip.  (70,130): a frame's sum spans several workgroups, and frames
    1 and 2 start off a 16-byte boundary."""
    for name in gold['colour.names']:
        img, want = gold[f'colour.{name}.in'], gold[f'colour.{name}.out']
        gc = dict(gain=gold[f'colour.{name}.gain'], contrast=float(gold[f'colour.{name}.contrast']))
        got, _ = run(sncal, cuda, np.stack([img] * 3), [dict(flags=COLOUR, **gc), dict(flags=0, **gc), dict(flags=COLOUR | FLIP, **gc)])
        _, near = ar.augment(img, COLOUR, gc['gain'], gc['contrast'])
        left_out = check_colour(got[0], want, near, name) + check_colour(got[2], ar.flip(want), ar.flip(near), name + ' flipped')
        print(f'colour {name}: elements left out by the tolerance rule: {left_out}')
        assert np.array_equal(got[1], img)


def test_colour_early_exit_of_the_sums_pass(sncal, cuda, gold):
    """Five frames, only frame 3 has the colour flag: the others' workgroups leave the sums kernel at once and the frames pass
    through; frame 3's mean is its own."""
    img, want = gold['colour.70x130.in'], gold['colour.70x130.out']
    gc = dict(gain=gold['colour.70x130.gain'], contrast=float(gold['colour.70x130.contrast']))
    others = [np.random.Generator(np.random.PCG64(50 + i)).integers(0, 256, img.shape, dtype=np.uint8) for i in range(4)]
    imgs = np.stack(others[:3] + [img] + others[3:])
    got, _ = run(sncal, cuda, imgs, [dict(flags=COLOUR if i == 3 else 0, **gc) for i in range(5)])
    _, near = ar.augment(img, COLOUR, gc['gain'], gc['contrast'])
    check_colour(got[3], want, near, 'frame 3')
    for i in (0, 1, 2, 4):
        assert np.array_equal(got[i], imgs[i]), i


def test_noise_from_the_reference_normals_is_exact(sncal, cuda, gold):
    for name in gold['noise.names']:
        img = gold[f'colour.{name}.in']
        _, n = ar.reference_normals(int(gold[f'noise.{name}.seed']), img.shape)
        other = np.random.Generator(np.random.PCG64(7)).normal(0, 40.0, img.shape)
        got, _ = run(sncal, cuda, np.stack([img] * 3), [dict(flags=NOISE), dict(flags=0), dict(flags=NOISE | FLIP)], noise=np.stack([n, other, n]))
        assert np.array_equal(got[0], gold[f'noise.{name}.out']), name
        assert np.array_equal(got[1], img)                                  # its noise array is not read
        assert np.array_equal(got[2], ar.flip(gold[f'noise.{name}.out'])), name      # the array is indexed in SOURCE coordinates


@pytest.mark.parametrize('shape', [(10, 37, 3), (17, 64, 3)])
def test_flip_is_an_exact_mirror_alone_and_combined(sncal, cuda, shape):
    rng = np.random.Generator(np.random.PCG64(shape[1]))
    imgs = rng.integers(0, 256, (4,) + shape, dtype=np.uint8)
    n = rng.normal(0, 25.0, imgs.shape)
    gc = dict(gain=(1.13, 0.91, 1.07), contrast=1.17)
    rows = [dict(flags=FLIP), dict(flags=FLIP | COLOUR, **gc), dict(flags=FLIP | NOISE), dict(flags=7, **gc)]
    got, chw = run(sncal, cuda, imgs, rows, noise=n, chw=True)
    for i, r in enumerate(rows):
        want, near = ar.augment(imgs[i], r['flags'], r.get('gain', (1, 1, 1)), r.get('contrast', 1.0), n[i])
        assert not near.any()                                               # own arithmetic on both sides: nothing to leave out
        assert np.array_equal(got[i], want), i
        assert np.array_equal(chw[i], ar.to_tensor(want)), i
    assert np.array_equal(got[0], imgs[0][:, ::-1])


def test_to_tensor_equals_torch_div(sncal, cuda):
    """Every byte value, both outputs together: fp32 CHW == torch's (u8.permute -> float32).div(255) bit for bit (torch_to_tensor), on the wide and
    the narrow path."""
    for W in (64, 37):
        img = np.arange(2 * 9 * W * 3, dtype=np.int64).reshape(2, 9, W, 3).astype(np.uint8)
        t = torch.from_numpy(img).to(cuda)
        u8, chw = sncal.augment.augment_u8(t, params_of(sncal, [dict(flags=0), dict(flags=FLIP)]), want_u8=True, want_chw=True)
        assert torch.equal(u8[0], t[0]) and torch.equal(u8[1], t[1].flip(1))
        want = torch_to_tensor(u8, (0, 3, 1, 2))
        assert torch.equal(chw.cpu(), want)
        assert np.array_equal(chw.cpu().numpy(), np.stack([ar.to_tensor(img[0]), ar.to_tensor(ar.flip(img[1]))]))
        assert set(np.unique(img)) == set(range(256))


def call(sncal, src, B, H, W, p, noise, dst, chw):
    L = sncal._lib
    n = ctypes.c_size_t()
    L.check(L.lib().sncal_augment_workspace(B, H, W, ctypes.byref(n)), 'sncal_augment_workspace')
    host = torch.from_numpy(np.frombuffer(p, dtype=np.uint8).copy())
    d_p = host.to(src.device)
    ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=src.device)
    L.check(L.lib().sncal_augment_u8(src.data_ptr(), B, H, W, d_p.data_ptr(), None if noise is None else noise.data_ptr(), dst.data_ptr(),
                                     chw.data_ptr(), ws.data_ptr(), ws.numel(), L.current_stream_ptr()), 'sncal_augment_u8')
    torch.cuda.synchronize()


def test_narrow_path_writes_the_bits_of_the_wide_path(sncal, cuda):
    """(2,17,64): the same frames from a base 3 bytes into a larger allocation (byte accesses) and aligned (16-byte accesses), all
    stages on, handed-in normals and the device generator: identical bits in both outputs."""
    B, H, W = 2, 17, 64
    rng = np.random.Generator(np.random.PCG64(17))
    img = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(cuda)
    noise = torch.from_numpy(rng.normal(0, 25.0, (B, H, W, 3))).to(cuda)
    p = params_of(sncal, [dict(flags=7, gain=(1.1, 0.9, 1.2), contrast=1.15, sigma=21.0, seed=11), dict(flags=3, gain=(0.85, 1.0, 1.1), contrast=0.9, sigma=9.0, seed=12)])
    n = img.numel()
    big_src, big_dst = torch.zeros(n + 64, dtype=torch.uint8, device=cuda), torch.zeros(n + 64, dtype=torch.uint8, device=cuda)
    big_src[3:3 + n] = img.reshape(-1)
    off_src, off_dst = big_src[3:3 + n], big_dst[3:3 + n]
    assert img.data_ptr() % 16 == 0 and off_src.data_ptr() % 16 == 3 and off_dst.data_ptr() % 16 == 3
    for nz in (noise, None):
        dst_a, chw_a = torch.zeros_like(img), torch.zeros((B, 3, H, W), dtype=torch.float32, device=cuda)
        call(sncal, img, B, H, W, p, nz, dst_a, chw_a)
        big_dst.zero_()
        chw_b = torch.zeros_like(chw_a)
        call(sncal, off_src, B, H, W, p, nz, off_dst, chw_b)
        assert torch.equal(off_dst.reshape(B, H, W, 3), dst_a) and torch.equal(chw_b, chw_a)
        assert int(big_dst[:3].sum()) == 0 and int(big_dst[3 + n:].sum()) == 0            # nothing written outside
        assert not torch.equal(dst_a, img)
        assert torch.equal(chw_a.cpu(), torch_to_tensor(dst_a, (0, 3, 1, 2)))


def test_device_noise_depends_on_seed_and_source_position_only(sncal, cuda):
    rng = np.random.Generator(np.random.PCG64(23))
    for shape in ((17, 64, 3), (10, 37, 3)):                                # wide and narrow
        imgs = rng.integers(40, 216, (4,) + shape, dtype=np.uint8)
        rows = [dict(flags=NOISE, sigma=12.0 + i, seed=1000 + i) for i in range(4)]
        a, _ = run(sncal, cuda, imgs, rows)
        b, _ = run(sncal, cuda, imgs, rows)
        assert np.array_equal(a, b)                                         # two runs, the same bits
        for k in range(4):                                                  # frame k of the batch == the frame alone
            alone, _ = run(sncal, cuda, imgs[k:k + 1], rows[k:k + 1])
            assert np.array_equal(alone[0], a[k]), k
        flipped, _ = run(sncal, cuda, imgs, [dict(r, flags=NOISE | FLIP) for r in rows])
        assert np.array_equal(flipped, a[:, :, ::-1])                       # flip on == mirror of flip off
        other, _ = run(sncal, cuda, imgs[:1], [dict(rows[0], seed=2000)])
        assert (other[0] != a[0]).mean() > 0.5                              # two seeds differ
        same_seed, _ = run(sncal, cuda, np.stack([imgs[0], imgs[0]]), [rows[0], rows[0]])
        assert np.array_equal(same_seed[0], same_seed[1])                   # and the place in the batch does not enter
        clear, _ = run(sncal, cuda, imgs, [dict(r, flags=0) for r in rows])
        assert np.array_equal(clear, imgs)                                  # flag clear: untouched
        assert (a != imgs).mean() > 0.5


def test_device_noise_distribution(sncal, cuda):
    H, W, sigma = 135, 240, 20.0
    img = np.full((1, H, W, 3), 128, dtype=np.uint8)
    out, _ = run(sncal, cuda, img, [dict(flags=NOISE, sigma=sigma, seed=0x5EED5EED1234)])
    out = out[0].astype(np.int64)
    N = out.size
    cdf = np.array([0.5 * (1.0 + math.erf((k - 128) / (sigma * math.sqrt(2.0)))) for k in range(257)])
    expect = N * np.diff(cdf)                                               # value k: N (Phi((k+1-128)/sigma) - Phi((k-128)/sigma))
    counts = np.bincount(out.reshape(-1), minlength=256)
    use = expect >= 5
    tail = float(expect[~use].sum())                                        # the bins left out of chi-square: a Poisson count of this mean
    assert counts[~use].sum() <= tail + 6 * math.sqrt(tail) + 1
    chi2 = float((((counts - expect) ** 2) / expect)[use].sum())
    d = int(use.sum()) - 1
    x = out + 0.5 - 128.0
    mean, var = float(x.mean()), float(x.var())
    z = (x - mean) / math.sqrt(var)
    lag = {'x': float((z[:, :-1] * z[:, 1:]).mean()), 'y': float((z[:-1] * z[1:]).mean()), 'channel': float((z[..., :-1] * z[..., 1:]).mean())}
    print(f'device noise: N {N}, chi2 {chi2:.1f} over {d} degrees of freedom (bound {d + 6 * math.sqrt(2 * d):.1f}), mean {mean:.4f} '
          f'(bound {6 * sigma / math.sqrt(N):.4f}), variance {var:.3f} (want {sigma ** 2 + 1 / 12:.3f} +- {6 * sigma ** 2 * math.sqrt(2 / N):.3f}), lag-1 {lag} '
          f'(bound {6 / math.sqrt(N):.4f})')
    assert chi2 <= d + 6 * math.sqrt(2 * d)
    assert abs(mean) <= 6 * sigma / math.sqrt(N)
    assert abs(var - (sigma ** 2 + 1 / 12)) <= 6 * sigma ** 2 * math.sqrt(2 / N)
    for k, v in lag.items():
        assert abs(v) <= 6 / math.sqrt(N), k


def test_train_transform_end_to_end_matches_reference(sncal, cuda, gold):
    """augment's classes on the composite fixture (noise probability 0), seeded like the capture: images and annotations equal the
    reference's; with ToTensor in the list the image is the fp32 CHW form of the same bytes."""
    A = sncal.augment
    annots = unjson(gold['composite.annot_in'])
    imgs = torch.from_numpy(gold['composite.in']).to(cuda)
    for to_tensor in (False, True):
        t = composite_transform(A)
        if to_tensor:
            t.transforms.append(A.ToTensor())
        random.seed(int(gold['composite.seeds'][0]))
        np.random.seed(int(gold['composite.seeds'][1]))
        out = t({'image': imgs, 'annot': annots})
        assert out['annot'] == unjson(gold['composite.annot_out']) and out['swapped'] == gold['composite.swapped'].tolist()
        assert out['flipped'] == [bool(f & FLIP) for f in gold['composite.flags']]
        got = out['image'].cpu().numpy()
        for i, want in enumerate(gold['composite.out']):
            _, near = ar.augment(gold['composite.in'][i], int(gold['composite.flags'][i]), gold['composite.gain'][i], float(gold['composite.contrast'][i]))
            if to_tensor:
                assert got.dtype == np.float32 and got.shape == (8, 3, 18, 32)
                ok = got[i] == ar.to_tensor(want)
                assert ok[~near.transpose(2, 0, 1)].all() and (~ok).sum() <= 1, i
            else:
                check_colour(got[i], want, near, i)
    # the line model's batch: frames and keypoints flipped together, classes kept
    kp = torch.from_numpy(gold['line.in'][:2].copy())
    out = A.ComposeTransform([A.LineFlip()])({'image': imgs[:2], 'keypoints': kp})
    assert torch.equal(out['image'], imgs[:2].flip(2))
    want = np.stack([A.flip_keypoints(r.copy(), 32) for r in gold['line.in'][:2]])
    assert np.array_equal(out['keypoints'].numpy(), want) and np.array_equal(kp.numpy(), gold['line.in'][:2])


def test_train_batches_over_a_split_folder(sncal, cuda, gold_dir, gold, tmp_path):
    """The golden 960x540 JPEG beside the fixture's annotations: shapes, order without shuffling, flipped frames carry flipped
    labels, and validate's folder batches with and without the label transform."""
    F, A = sncal.frames, sncal.augment
    full = np.load(os.path.join(gold_dir, 'jpeg_cases.npz'))['jpg.full'].tobytes()
    cases = unjson(gold['labels.cases'])[:5]
    for i, c in enumerate(cases):
        (tmp_path / f'{i:05d}.json').write_text(json.dumps(c['in']))
        (tmp_path / f'{i:05d}.jpg').write_bytes(full)
    dec = sncal.JpegDecoder(540, 960, max_batch=1, device=cuda)
    frame = dec.decode([full])[0].clone()
    dec.close()
    flips = A.ComposeTransform([A.UseWithProb(A.Flip(), 0.5), A.FixLRAmbiguous(), A.ToTensor()])
    random.seed(3)
    want_flip = [random.random() < 0.5 for _ in cases]
    assert any(want_flip) and not all(want_flip)
    random.seed(3)
    batches = list(F.train_batches(str(tmp_path), 2, flips, shuffle=False, device=cuda, margin=2.0))
    assert [b['img_name'] for b in batches] == [['00000.jpg', '00001.jpg'], ['00002.jpg', '00003.jpg'], ['00004.jpg']]
    plain = torch_to_tensor(frame, (2, 0, 1)).to(cuda)
    i = 0
    for b in batches:
        n = len(b['img_name'])
        assert tuple(b['image'].shape) == (n, 3, 540, 960) and b['image'].dtype == torch.float32 and b['image'].is_cuda
        assert tuple(b['keypoints'].shape) == (n, 171) and tuple(b['mask'].shape) == (n, 58) and len(b['raw_annot']) == n
        for j in range(n):
            a = cases[i]['in']
            if want_flip[i]:
                a = A.flip_annot(a)
            a = A.test_transform().labels(a)
            kp, mask = F.annot_to_keypoints(a, 57, 2.0)
            assert np.array_equal(b['keypoints'][j].numpy(), kp) and np.array_equal(b['mask'][j].numpy(), mask), i
            assert b['raw_annot'][j] == sncal.evaluate.scale_points(a, 960, 540)
            assert torch.equal(b['image'][j], plain.flip(2) if want_flip[i] else plain), i
            i += 1
    names = [n for b in F.train_batches(str(tmp_path), 2, A.ComposeTransform([]), shuffle=True, seed=4, device=cuda) for n in b['img_name']]
    again = [n for b in F.train_batches(str(tmp_path), 2, A.ComposeTransform([]), shuffle=True, seed=4, device=cuda) for n in b['img_name']]
    assert names == again and sorted(names) == [f'{k:05d}.jpg' for k in range(5)] and names != sorted(names)
    # validate's folder batches: transform=None is the labelling of the files as they are, test_transform() changes the swapped frames only
    none = list(F.folder_batches(str(tmp_path), 5, cuda, 57, 2.0, (960, 540), 0, []))[0]
    fixed = list(F.folder_batches(str(tmp_path), 5, cuda, 57, 2.0, (960, 540), 0, [], transform=A.test_transform()))[0]
    assert none['image'].dtype == torch.uint8 and torch.equal(none['image'], fixed['image']) and torch.equal(none['image'][0], frame)
    for k, c in enumerate(cases):
        kp, mask = F.annot_to_keypoints(c['in'], 57, 2.0)
        assert np.array_equal(none['keypoints'][k].numpy(), kp) and none['raw_annot'][k] == sncal.evaluate.scale_points(c['in'], 960, 540)
        assert torch.equal(none['keypoints'][k], fixed['keypoints'][k]) == (not c['swapped']), k
    assert any(c['swapped'] for c in cases) and not all(c['swapped'] for c in cases)
