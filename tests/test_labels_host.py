"""CPU: the host side of the device label path -- packing, the RANSAC sample tables, the generated kernel tables, the deferral of
FixLRAmbiguous, and labels='host' being today's labelled_batch."""
import importlib.util
import os
from unittest import mock

import numpy as np
import pytest
import torch

import sncal_amd
from sncal_amd import annotations as an
from sncal_amd import augment, frames

import labels_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_class_order():
    assert len(an.ANNOT_CLASSES) == 28 and len(set(an.ANNOT_CLASSES)) == 28
    assert set(an.ANNOT_CLASSES) == set(sncal_amd.evaluate.SYMMETRIC)            # every name mirror_labels knows, no other
    assert an.ANNOT_CLASSES[:3] == ('Circle central', 'Circle left', 'Circle right')


def test_pack_annotations_round_trips():
    t = np.linspace(0, 2 * np.pi, 300, endpoint=False)
    annots = [{},
              {'Middle line': [], 'Side line top': [{'x': 0.25, 'y': 0.5}]},
              {'Circle central': [{'x': 0.5 + 0.2 * np.cos(u), 'y': 0.5 + 0.1 * np.sin(u)} for u in t],
               'Goal left post left ': [(0.1, 0.2), (0.1, 0.3)], 'Line unknown': [(0.3, 0.3)]},
              {}]
    points, offsets, present = an.pack_annotations(annots)
    assert points.dtype == np.float64 and points.shape == (304, 2)
    assert offsets.dtype == np.int32 and offsets.shape == (4, 29) and present.dtype == np.int32 and present.shape == (4,)
    assert offsets[0, 0] == 0 and offsets[-1, -1] == 304 and (np.diff(offsets.reshape(-1)) >= 0).all()
    assert (offsets[1:, 0] == offsets[:-1, -1]).all()
    cid = {c: i for i, c in enumerate(an.ANNOT_CLASSES)}
    assert present[0] == 0 and present[3] == 0
    assert present[1] == (1 << cid['Middle line']) | (1 << cid['Side line top'])          # the empty class is a key all the same
    assert offsets[1, cid['Middle line'] + 1] - offsets[1, cid['Middle line']] == 0
    assert offsets[2, 1] - offsets[2, 0] == 300
    back = an.unpack_annotations(points, offsets, present)
    for a, b in zip(annots, back):
        assert set(a) == set(b)
        for k, v in a.items():
            assert b[k] == [((p['x'], p['y']) if isinstance(p, dict) else tuple(p)) for p in v]
    # an empty batch, and a name outside the class order
    p0, o0, m0 = an.pack_annotations([])
    assert p0.shape == (0, 2) and o0.shape == (0, 29) and m0.shape == (0,)
    with pytest.raises(KeyError):
        an.pack_annotations([{'Centre spot': [(0.5, 0.5)]}])


@pytest.mark.parametrize('n', [5, 6, 23, 53])
def test_ransac_samples_are_the_host_sequence(n):
    """Spy on the generator homography_ransac builds: the table holds the indices it draws, in order."""
    drawn = []
    real = np.random.Generator

    class Spy:
        def __init__(self, bitgen):
            self._g = real(bitgen)

        def choice(self, *a, **kw):
            drawn.append(self._g.choice(*a, **kw))
            return drawn[-1]
    rng = np.random.default_rng(n)
    src = rng.uniform(-50, 50, (n, 2))
    dst = src * 7.0 + 300.0 + rng.normal(0, 0.5, (n, 2))
    with mock.patch.object(an.np.random, 'Generator', Spy):
        assert an.homography_ransac(src, dst, 5.0) is not None
    table = an.ransac_samples(n)
    assert table.dtype == np.uint8 and table.shape == (200, 4) and len(drawn) == 200
    assert np.array_equal(table, np.stack(drawn))
    assert np.array_equal(an.sample_tables()[n], table) if n in (5, 53) else True


def test_kernel_tables_are_generated_from_the_python_tables():
    spec = importlib.util.spec_from_file_location('make_labels_tables', os.path.join(ROOT, 'tools', 'make_labels_tables.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert open(mod.path()).read() == mod.text()


def test_deferring_fix_lr():
    t, had = augment.test_transform().deferring_fix_lr()
    assert had and [type(x) for x in t.transforms] == [augment.ToTensor]
    t, had = augment.train_transform().deferring_fix_lr()
    assert had and not any(isinstance(x, augment.FixLRAmbiguous) for x in t.transforms) and len(t.transforms) == 4
    same = augment.ComposeTransform([augment.ToTensor()])
    assert same.deferring_fix_lr() == (same, False)
    full = augment.train_transform()
    full.deferring_fix_lr()
    assert any(isinstance(x, augment.FixLRAmbiguous) for x in full.transforms)              # the object itself is left alone
    for bad in ([augment.FixLRAmbiguous(), augment.UseWithProb(augment.Flip(), 0.5)], [augment.UseWithProb(augment.FixLRAmbiguous(), 0.5)],
                [augment.FixLRAmbiguous(threshold=5)], [augment.FixLRAmbiguous(), augment.FixLRAmbiguous()]):
        with pytest.raises(sncal_amd._lib.SncalError):
            augment.ComposeTransform(bad).deferring_fix_lr()


def test_labels_host_is_todays_labelled_batch():
    annots = lr.synthetic_frames(3) + [{}]
    names = [f'{i:05d}.jpg' for i in range(4)]
    image = torch.zeros((4, 2, 2, 3), dtype=torch.uint8)
    got = frames.labelled_batch(image, annots, names, 57, 3.0, (960, 540), labels='host')
    plain = frames.labelled_batch(image, annots, names, 57, 3.0, (960, 540))
    pairs = [frames.annot_to_keypoints(a, 57, 3.0) for a in annots]
    for out in (got, plain):
        assert out['keypoints'].dtype == torch.float32 and out['mask'].dtype == torch.int64 and not out['keypoints'].is_cuda
        assert out['keypoints'].numpy().tobytes() == np.stack([p[0] for p in pairs]).tobytes()
        assert np.array_equal(out['mask'].numpy(), np.stack([p[1] for p in pairs]))
        assert out['raw_annot'] == [sncal_amd.evaluate.scale_points(a, 960, 540) for a in annots] and out['img_name'] == names
    with pytest.raises(sncal_amd._lib.SncalError):
        frames.labelled_batch(image, annots, names, 57, 3.0, (960, 540), labels='gpu')
    with pytest.raises(sncal_amd._lib.SncalError):
        frames.labelled_batch(image, annots, names, 57, 3.0, (960, 540), labels='host', fix_lr=True)


def test_entry_point_validates_before_the_device():
    import ctypes
    lib = sncal_amd._lib.lib()
    n = ctypes.c_size_t(7)
    assert lib.sncal_keypoint_labels_workspace(64, 5000, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.sncal_keypoint_labels_workspace(-1, 0, ctypes.byref(n)) == -1
    one = ctypes.c_void_p(16)
    args = [one, 10, one, one, 1, 28, 960, 540, 1, 0.0, 57, 0, one, one, one, None, None, None, None, 0, None]

    def call(**kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.sncal_keypoint_labels(*a)
    assert call(_4=0) == 0                                                    # an empty batch touches nothing
    assert call(_5=27) == -1 and b'class order' in lib.sncal_last_error()
    assert call(_10=58) == -1 and call(_10=0) == -1
    assert call(_11=1) == -1 and b'd_swapped' in lib.sncal_last_error()      # the flag needs its output
    assert call(_11=2) == -1
    assert call(_12=None) == -1 and call(_15=one) == -1
