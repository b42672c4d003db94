"""OPTIONAL: the resize restatement (tests/resize_ref.py) and the kernel (sncal_resize_u8) against cv2.resize itself, byte for byte,
on the shapes of resize_ref.CASES with noise and ramp inputs.  Skipped wherever cv2 is not importable -- which includes the build
container and the GPU box: OpenCV parity of the resize stays UNPINNED until this file has run somewhere with a cv2 (the arithmetic
was restated from opencv 4.7's modules/imgproc/src/resize.cpp) and tests/golden/resize_cv2.npz is committed.

The expectations were written WITHOUT a cv2 at hand; a failure here is information about the restatement, not a broken build.

Both checks exist on the pattern of tests/test_solve_cv2_optional.py: unmarked for the restatement (the CPU run) and `gpu`-marked
for the kernel, so that whichever box first carries a cv2 runs them.  When the committed fixture is missing, the first run with a
cv2 WRITES it -- tests/golden/resize_cv2.npz -- so that one such run is enough to pin the restatement from then on.  The fixture
holds cv2's outputs for every case but the two whose result is 960x540 (kept out for their size: a committed file stays well under
1 MiB; those two are always computed by the cv2 at hand)."""
import os

import numpy as np
import pytest

cv2 = pytest.importorskip('cv2')

import resize_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 400 * 1024           # bytes of one case's output the fixture still holds

_WANT = None


def _key(case, kind):
    return '%dx%d-%dx%d.%s' % (case[:4] + (kind,))


def _cv2(case, kind):
    h, w, H, W, B = case
    src = ref.inputs(h, w, B)[kind]
    return np.stack([cv2.resize(f, (W, H)) for f in src])


def _want():
    """cv2.resize's outputs per (case, kind): the committed fixture where it holds them (pinned OpenCV), else the cv2 importable now."""
    global _WANT
    if _WANT is not None:
        return _WANT
    path = os.path.join(ROOT, 'tests', 'golden', 'resize_cv2.npz')
    have = dict(np.load(path)) if os.path.exists(path) else {}
    out, wrote = {}, {}
    for case in ref.CASES:
        for kind in ('noise', 'ramp'):
            k = _key(case, kind)
            out[k] = have[k] if k in have else _cv2(case, kind)
            if out[k].nbytes <= SMALL:
                wrote[k] = out[k]
    if not have:
        wrote['cv2_version'] = np.array(cv2.__version__)
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.savez_compressed(path, **wrote)
        except OSError:
            pass
    _WANT = out
    return out


def test_restatement_equals_cv2_resize_byte_for_byte():
    want = _want()
    for case in ref.CASES:
        h, w, H, W, B = case
        for kind, src in ref.inputs(h, w, B).items():
            got = ref.resize(src, (W, H))
            assert np.array_equal(got, want[_key(case, kind)]), (case, kind)


@pytest.mark.gpu
def test_kernel_equals_cv2_resize_byte_for_byte(sncal, cuda):
    import torch
    want = _want()
    for case in ref.CASES:
        h, w, H, W, B = case
        for kind, src in ref.inputs(h, w, B).items():
            got = sncal.resize.resize_u8(torch.from_numpy(src).to(cuda), (W, H)).cpu().numpy()
            assert np.array_equal(got, want[_key(case, kind)]), (case, kind)
