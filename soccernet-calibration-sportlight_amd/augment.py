"""Train-time augmentation on the device: the transforms of /root/reference/src/models/hrnet/transforms.py:16-221 and
/root/reference/src/models/line/transforms.py:10-190, same names and constructor arguments, over BATCHES.

    reference (one numpy sample in a loader worker)                   here (one batch, frames already on the device)
    ColorAugment, GaussNoise, Flip (image), ToTensor                  csrc/augment.hip: sncal_augment_u8, one launch per batch
    UseWithProb, ComposeTransform                                     the same draws, made on the host sample after sample
    Flip (labels), flip_annot_names, FixLRAmbiguous                   host, numpy only, over annotations.get_intersections
    line model: Flip = image flip + flip_keypoints + map flip         LineFlip: image flip + flip_keypoints; maps are not flipped,
                                                                      the flipped keypoints go to loss.create_keypoint_maps or to
                                                                      EHMLoss's rebuild form

A batch is {'image': (B,H,W,3) uint8 on the device (JpegDecoder's output), 'annot': list of B annotation dicts} for the keypoint
model, {'image', 'keypoints': (B, 3*pairs*2)} for the line model.  ComposeTransform.__call__ walks the samples in order and makes,
for each sample, the reference's draws with the same calls in the same order: random.random() per UseWithProb;
np.random.uniform for the brightness, then the three colours, then the contrast; np.random.uniform(0, sigma_sq) for the noise
scale.  Then ONE more draw the reference does not make: a 64-bit seed from np.random for the frame's device noise stream (the
reference draws H*W*3 normals from MT19937 there, which the device cannot replay: include/sncal.h).  So with the noise
probability at 0, a run seeded like the reference's (random.seed, np.random.seed) reproduces its parameter sequence and, through
the kernel, its images; with noise on, the two streams part at the first noisy sample: same distributions, other numbers.

The image comes back as uint8 (B,H,W,3), the input of forward_u8 -- or, with ToTensor in the list, as fp32 (B,3,H,W) in [0, 1].
The kernel applies colour, noise, flip in that order: a list that orders the image stages differently is refused.

Label transforms build NEW dicts: the reference's Flip writes x = 1 - x into the point dicts it was handed, i.e. into the
dataset's stored labels (transforms.py:129-131 on dataset.py:53-57); here the caller's annotation is left as it was.
"""
import ctypes
import random
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .annotations import get_intersections
from .evaluate import SYMMETRIC

FLAG_COLOUR, FLAG_NOISE, FLAG_FLIP = 1, 2, 4

# /root/reference/src/datatools/ellipse.py:160-185, restated: keypoint pairs whose line is perpendicular to the pitch's main axis,
# and the keypoints of the left / right half
PERP_LINES: List[Tuple[int, int]] = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (12, 13), (14, 15), (16, 17), (18, 19),
                                     (20, 21), (22, 23), (24, 25), (26, 27), (28, 29), (40, 41), (44, 45), (51, 52)]
POINTS_LEFT: List[int] = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 31, 33, 35, 37, 39, 43, 44, 45, 46, 47, 48, 49]
POINTS_RIGHT: List[int] = [16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 32, 34, 36, 38, 50, 51, 52, 53, 54, 55, 56]

# transforms.py:90-95 (the trailing blank of 'Goal left post left ' is SoccerNet's)
FLIP_POSTS = {'Goal left post right': 'Goal left post left ', 'Goal left post left ': 'Goal left post right',
              'Goal right post right': 'Goal right post left', 'Goal right post left': 'Goal right post right'}


# ---- label side (host) -----------------------------------------------------------------------------------------------
def mirror_labels(lines_dict: dict) -> dict:
    """baseline/evaluate_extremities.py:24-34 (baseline/evaluate_camera.py:11 and the reference's transforms import it from there):
    every class replaced by its point-symmetric class, values kept.  A class outside the table raises KeyError, as the reference's
    lookup in SoccerPitch.symetric_classes does."""
    return {SYMMETRIC[k]: v for k, v in lines_dict.items()}


def swap_top_bottom_names(line_name: str) -> str:
    """transforms.py:98-103."""
    x, y = 'top', 'bottom'
    if x in line_name or y in line_name:
        return y.join(part.replace(y, x) for part in line_name.split(x))
    return line_name


def swap_posts_names(line_name: str) -> str:
    """transforms.py:106-109."""
    return FLIP_POSTS.get(line_name, line_name)


def flip_annot_names(annot: dict, swap_top_bottom: bool = True, swap_posts: bool = True) -> dict:
    """transforms.py:112-119: the class names of a horizontally flipped frame."""
    annot = mirror_labels(annot)
    if swap_top_bottom:
        annot = {swap_top_bottom_names(k): v for k, v in annot.items()}
    if swap_posts:
        annot = {swap_posts_names(k): v for k, v in annot.items()}
    return annot


def flip_annot(annot: dict) -> dict:
    """Flip's label side (transforms.py:128-131): flipped names, x = 1.0 - x on every point; new point dicts."""
    return {k: [{**p, 'x': 1.0 - p['x']} for p in pts] for k, pts in flip_annot_names(annot).items()}


def flip_keypoints(x: np.ndarray, w: int) -> np.ndarray:
    """line/transforms.py:113-128, in place like the reference: x = w - x - 1 for rows [x, y, flag] with x != -1 and flag == 1.
    Mirrored, not fixed: the classes are NOT swapped, a left line stays a left line in the flipped frame."""
    for i in range(len(x) // 3):
        if x[i * 3] != -1 and x[i * 3 + 2] == 1:
            x[i * 3] = w - x[i * 3] - 1
    return x


def _decode_annot(annot: dict) -> dict:
    return {cls: [(p['x'], p['y']) for p in pts] for cls, pts in annot.items()}           # reader.decode_annot


class _Sample:
    """What the transforms of one ComposeTransform pass see of one sample: its parameter entry and its labels."""
    __slots__ = ('p', 'annot', 'keypoints', 'width', 'swapped', 'to_tensor', 'stage')

    def __init__(self, p, annot, keypoints, width):
        self.p, self.annot, self.keypoints, self.width = p, annot, keypoints, width
        self.swapped, self.to_tensor, self.stage = False, False, 0

    def image_stage(self, flag, name):
        if flag <= self.stage:
            raise _lib.SncalError(f'{name}: the kernel applies colour, noise, flip once each and in that order')
        self.stage = flag
        self.p.flags |= flag


class _Transform:
    """A transform used alone is a one-element ComposeTransform."""

    def draw(self, s: _Sample):
        raise NotImplementedError

    def __call__(self, batch: dict) -> dict:
        return ComposeTransform([self])(batch)


class ColorAugment(_Transform):
    def __init__(self, brightness: Tuple[float, float] = (0.8, 1.2), color: Tuple[float, float] = (0.8, 1.2),
                 contrast: Tuple[float, float] = (0.8, 1.2)):
        self.brightness, self.color, self.contrast = brightness, color, contrast

    def draw(self, s):
        s.image_stage(FLAG_COLOUR, 'ColorAugment')
        gain = np.random.uniform(self.brightness[0], self.brightness[1]) * np.random.uniform(self.color[0], self.color[1], 3)
        s.p.gain[0], s.p.gain[1], s.p.gain[2] = (float(g) for g in gain)
        s.p.contrast = float(np.random.uniform(self.contrast[0], self.contrast[1]))


class GaussNoise(_Transform):
    """sigma_sq is the reference's name for the upper end of the uniform draw of the noise SCALE (it is used as np.random.normal's
    standard deviation, transforms.py:51)."""

    def __init__(self, sigma_sq: float = 30.0):
        self.sigma_sq = sigma_sq

    def draw(self, s):
        s.image_stage(FLAG_NOISE, 'GaussNoise')
        s.p.noise_sigma = float(np.random.uniform(0.0, self.sigma_sq))
        s.p.seed = int(np.random.randint(0, 2 ** 64, dtype=np.uint64))


class Flip(_Transform):
    """Horizontal flip of the frame and of the keypoint model's annotation."""

    def draw(self, s):
        s.image_stage(FLAG_FLIP, 'Flip')
        if s.annot is None:
            raise _lib.SncalError("Flip needs the batch's 'annot' (the line model's flip is LineFlip)")
        s.annot = flip_annot(s.annot)


class LineFlip(_Transform):
    """The line model's Flip (line/transforms.py:131-139): frame and keypoints; 'keypoint_maps' are not flipped, build them from the
    flipped keypoints."""

    def draw(self, s):
        s.image_stage(FLAG_FLIP, 'LineFlip')
        if s.keypoints is None:
            raise _lib.SncalError("LineFlip needs the batch's 'keypoints'")
        flip_keypoints(s.keypoints, s.width)


class FixLRAmbiguous(_Transform):
    """transforms.py:136-186: where most annotated perpendicular lines run horizontally in the image (a camera behind a goal), left
    and right are decided by the image rows of the two halves' keypoints (medians), or by the count of left / right class names,
    and the names are mirrored when the annotation has them the other way round."""

    def __init__(self, threshold: float = 10, img_height: int = 540):
        self.threshold = threshold
        self.img_center = img_height / 2

    @staticmethod
    def _number_on_side(annot, side: str = 'left') -> int:
        return sum(side in name.split()[:3] for name in annot)

    def decide(self, annot: dict):
        """-> (swap, branch): branch is 'medians', 'count' or None (not a behind-the-goal view)."""
        n_left, n_right = self._number_on_side(annot, 'left'), self._number_on_side(annot, 'right')
        kpts, _ = get_intersections(_decode_annot(annot))
        n_horizontal = n_total = 0
        left_y, right_y = [], []
        for a, b in PERP_LINES:
            p1, p2 = kpts[a], kpts[b]
            if p1 is not None and p2 is not None:
                n_total += 1
                for i, p in ((a, p1), (b, p2)):
                    if i in POINTS_LEFT:
                        left_y.append(p[1])
                    elif i in POINTS_RIGHT:
                        right_y.append(p[1])
                dx, dy = abs(p1[0] - p2[0]), abs(p1[1] - p2[1])
                if dy < 1.0 or dx / dy > self.threshold:
                    n_horizontal += 1
        if n_total > 0 and n_horizontal / n_total >= 0.5:
            if left_y and right_y:
                return bool(np.median(left_y) < np.median(right_y)), 'medians'
            return n_right > n_left, 'count'
        return False, None

    def draw(self, s):
        if s.annot is None:
            raise _lib.SncalError("FixLRAmbiguous needs the batch's 'annot'")
        if self.decide(s.annot)[0]:
            s.annot = flip_annot_names(s.annot, swap_top_bottom=False, swap_posts=False)
            s.swapped = True


class ToTensor(_Transform):
    """Selects the fp32 (B,3,H,W) output, values / 255 (torchvision's ToTensor on a uint8 HWC image; the channel order stays)."""

    def draw(self, s):
        s.to_tensor = True


class UseWithProb(_Transform):
    def __init__(self, transform, prob: float = 0.5):
        self.transform, self.prob = transform, prob

    def draw(self, s):
        if random.random() < self.prob:
            self.transform.draw(s)


class ComposeTransform(_Transform):
    def __init__(self, transforms: Sequence[_Transform]):
        self.transforms = list(transforms)

    def draw(self, s):
        for t in self.transforms:
            t.draw(s)

    def draw_batch(self, B: int, width: int, annots: Optional[Sequence[dict]] = None, keypoints: Optional[np.ndarray] = None):
        """The host half, no GPU: -> (params, samples).  params is a ctypes array of B sncal_augment_params; samples[i] carries the
        transformed labels (.annot, .keypoints, .swapped) and .to_tensor."""
        params = (_lib.AugmentParams * max(B, 1))()
        samples = []
        for i in range(B):
            params[i].contrast = 1.0
            params[i].gain[0] = params[i].gain[1] = params[i].gain[2] = 1.0
            s = _Sample(params[i], annots[i] if annots is not None else None, keypoints[i] if keypoints is not None else None, width)
            self.draw(s)
            samples.append(s)
        return params, samples

    def deferring_fix_lr(self):
        """-> (a ComposeTransform without this list's FixLRAmbiguous, whether there was one): for callers that let the label kernel
        take the decision (sncal_keypoint_labels with SNCAL_LABELS_FIX_LR, validate.labelled_batch(labels='device', fix_lr=True)).
        This object is left as it is.  Refused where the kernel could not stand in: a FixLRAmbiguous under UseWithProb or in a
        nested list, one that is not the last label transform, or one with another threshold than the kernel's 10."""
        fix = [i for i, t in enumerate(self.transforms) if isinstance(t, FixLRAmbiguous)]
        for t in self.transforms:
            inner = t.transform if isinstance(t, UseWithProb) else t
            if isinstance(inner, ComposeTransform) or (inner is not t and isinstance(inner, FixLRAmbiguous)):
                raise _lib.SncalError('deferring_fix_lr: FixLRAmbiguous under UseWithProb or a nested list cannot be deferred')
        if not fix:
            return self, False
        if len(fix) > 1 or self.transforms[fix[0]].threshold != 10:
            raise _lib.SncalError('deferring_fix_lr: the label kernel applies one FixLRAmbiguous with threshold 10')
        for t in self.transforms[fix[0] + 1:]:
            if isinstance(t.transform if isinstance(t, UseWithProb) else t, (Flip, LineFlip)):
                raise _lib.SncalError('deferring_fix_lr: a flip after FixLRAmbiguous would have to run after the label kernel')
        return ComposeTransform([t for i, t in enumerate(self.transforms) if i != fix[0]]), True

    def labels(self, annot: dict) -> dict:
        """The label side alone, on one annotation (validate()'s transform=): a list that would change the image is refused."""
        params, (s,) = self.draw_batch(1, 0, [annot])
        if params[0].flags:
            raise _lib.SncalError('this transform changes the image: only label transforms (test_transform()) apply here')
        return s.annot

    def __call__(self, batch: dict) -> dict:
        import torch
        image = _lib.require_device(batch['image'], torch.uint8, "batch['image']")
        if image.dim() != 4 or image.shape[3] != 3:
            raise _lib.SncalError(f"batch['image'] {tuple(image.shape)} must be (B,H,W,3)")
        B, H, W = int(image.shape[0]), int(image.shape[1]), int(image.shape[2])
        annots, kp = batch.get('annot'), batch.get('keypoints')
        if annots is not None and len(annots) != B:
            raise _lib.SncalError(f"batch['annot'] holds {len(annots)} annotations for {B} frames")
        kp_np = None
        if kp is not None:
            kp_np = np.array(kp.cpu().numpy() if isinstance(kp, torch.Tensor) else kp)            # a copy: flip_keypoints writes in place
            if kp_np.ndim != 2 or kp_np.shape[0] != B:
                raise _lib.SncalError(f"batch['keypoints'] {kp_np.shape} must be (B, ...) with B = {B}")
        params, samples = self.draw_batch(B, W, annots, kp_np)
        to_tensor = any(s.to_tensor for s in samples) or (B == 0 and any(isinstance(t, ToTensor) for t in self.transforms))
        u8, chw = augment_u8(image, params, want_u8=not to_tensor, want_chw=to_tensor)
        out = dict(batch)
        out['image'] = chw if to_tensor else u8
        if annots is not None:
            out['annot'] = [s.annot for s in samples]
            out['swapped'] = [s.swapped for s in samples]
        if kp is not None:
            out['keypoints'] = torch.from_numpy(kp_np) if isinstance(kp, torch.Tensor) else kp_np
        out['flipped'] = [bool(p.flags & FLAG_FLIP) for p in params[:B]]
        return out


def augment_u8(image, params, noise=None, want_u8: bool = True, want_chw: bool = False):
    """sncal_augment_u8: image (B,H,W,3) uint8 on the device, params a ctypes array of B _lib.AugmentParams (host), noise
    (B,H,W,3) fp64 on the device or None (= the device generator) -> (uint8 (B,H,W,3) or None, fp32 (B,3,H,W) or None).
    Asynchronous on the current stream."""
    import torch
    image = _lib.require_device(image, torch.uint8, 'image')
    if image.dim() != 4 or image.shape[3] != 3:
        raise _lib.SncalError(f'image {tuple(image.shape)} must be (B,H,W,3)')
    B, H, W = int(image.shape[0]), int(image.shape[1]), int(image.shape[2])
    if len(params) < B:
        raise _lib.SncalError(f'{len(params)} parameter entries for {B} frames')
    if not (want_u8 or want_chw):
        raise _lib.SncalError('no output requested')
    if noise is not None:
        noise = _lib.require_device(noise, torch.float64, 'noise')
        if tuple(noise.shape) != tuple(image.shape):
            raise _lib.SncalError(f'noise {tuple(noise.shape)} must be shaped like the image {tuple(image.shape)}')
    dev = image.device
    ws = _lib.workspace('sncal_augment_workspace', B, max(H, 1), max(W, 1), device=dev)
    u8 = torch.empty_like(image) if want_u8 else None
    chw = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_chw else None
    if B == 0 or H == 0 or W == 0:
        return u8, chw
    host = torch.from_numpy(np.frombuffer(params, dtype=np.uint8, count=B * ctypes.sizeof(_lib.AugmentParams)).copy())
    _lib.launch('sncal_augment_u8', dev, image, B, H, W, host.to(dev), noise, u8, chw, ws, ws.numel())
    return u8, chw


def train_transform(brightness: Tuple[float, float] = (0.8, 1.2), color: Tuple[float, float] = (0.8, 1.2),
                    contrast: Tuple[float, float] = (0.8, 1.2), gauss_noise_sigma: float = 30.0, prob: float = 0.5):
    """transforms.py:199-213."""
    return ComposeTransform([UseWithProb(ColorAugment(brightness=brightness, color=color, contrast=contrast), prob),
                             UseWithProb(GaussNoise(gauss_noise_sigma), prob), UseWithProb(Flip(), 0.5), FixLRAmbiguous(), ToTensor()])


def test_transform():
    """transforms.py:216-221: what the reference's validation loader applies (validate.py:33, train.py:34)."""
    return ComposeTransform([FixLRAmbiguous(), ToTensor()])


test_transform.__test__ = False            # a factory with the reference's name, not a test


def line_train_transform(brightness: Tuple[float, float] = (0.8, 1.2), color: Tuple[float, float] = (0.8, 1.2),
                         contrast: Tuple[float, float] = (0.8, 1.2), gauss_noise_sigma: float = 30.0, prob: float = 0.5):
    """line/transforms.py:152-183."""
    return ComposeTransform([UseWithProb(ColorAugment(brightness=brightness, color=color, contrast=contrast), prob),
                             UseWithProb(GaussNoise(gauss_noise_sigma), prob), UseWithProb(LineFlip(), 0.5), ToTensor()])


def line_test_transform():
    """line/transforms.py:186-190."""
    return ComposeTransform([ToTensor()])
