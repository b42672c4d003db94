"""numpy fp64 restatement of the augmentation stages of csrc/augment.hip (written for this build; pinned to the reference's
ColorAugment / GaussNoise / Flip by tests/golden/augment.npz in tests/test_augment_host.py), and the fixture's candidate
annotations.  One frame at a time: img is (H,W,3) uint8."""
import numpy as np

FLAG_COLOUR, FLAG_NOISE, FLAG_FLIP = 1, 2, 4
RADIUS = 2.0 ** -20          # the colour tolerance rule: an element whose pre-truncation value lies this close to an integer may differ


def channel_sums(img):
    """The exact integer sums S_c."""
    return [int(s) for s in img.reshape(-1, 3).astype(np.int64).sum(axis=0)]


def device_mean(img, gain):
    """mean[c] = double(S_c) * gain[c] / double(H*W), the kernel's form."""
    npix = img.shape[0] * img.shape[1]
    return np.array([np.float64(s) * np.float64(g) / np.float64(npix) for s, g in zip(channel_sums(img), gain)])


def numpy_mean(img, gain):
    """The reference's form: numpy's fp64 mean of the rounded products."""
    return (img.astype(np.float64) * np.asarray(gain, dtype=np.float64)).mean(axis=(0, 1))


def colour(img, gain, contrast, mean=None):
    """-> (uint8 image, v): v is the fp64 value before clip and truncation."""
    p = img.astype(np.float64) * np.asarray(gain, dtype=np.float64)
    m = device_mean(img, gain) if mean is None else mean
    v = (p - m) * np.float64(contrast) + m
    return np.clip(v, 0.0, 255.0).astype(np.uint8), v


def noise(img, n):
    """n: (H,W,3) fp64 normals, already scaled."""
    return np.clip(img.astype(np.float64) + n, 0.0, 255.0).astype(np.uint8)


def reference_normals(seed, shape, sigma_sq=30.0):
    """What GaussNoise draws after np.random.seed(seed): (scale, the (H,W,3) array np.random.normal(0, scale, shape))."""
    rs = np.random.RandomState(seed)
    scale = rs.uniform(0.0, sigma_sq)
    return scale, rs.normal(0, scale, shape)


def flip(img):
    return np.ascontiguousarray(img[:, ::-1])


def to_tensor(img):
    return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0)


def augment(img, flags, gain=(1.0, 1.0, 1.0), contrast=1.0, n=None):
    """All three stages in the kernel's order -> (uint8 image, near): near marks the elements (in OUTPUT coordinates) the colour
    tolerance rule lets differ."""
    near = np.zeros(img.shape, dtype=bool)
    if flags & FLAG_COLOUR:
        img, v = colour(img, gain, contrast)
        near = np.abs(v - np.rint(v)) <= RADIUS
    if flags & FLAG_NOISE:
        img = noise(img, n)
    if flags & FLAG_FLIP:
        img, near = flip(img), flip(near)
    return img, near


def as_dicts(annot):
    return {c: [{'x': float(x), 'y': float(y)} for x, y in pts] for c, pts in annot.items()}


class TopDownView:
    """A stand-in for synth.random_camera's camera: the pitch seen from above with its main axis VERTICAL in the image (what a
    camera high behind a goal shows, without the perspective), so the lines across the pitch run horizontally -- the case
    FixLRAmbiguous exists for.  up = +1 puts the left half at the top of the image, -1 at the bottom; height lifts points with
    z != 0 sideways so that posts stay segments."""

    def __init__(self, scale, angle_deg, centre_x, up):
        self.scale, self.a, self.cx, self.up = scale, np.deg2rad(angle_deg), centre_x, up

    def project_points(self, w):
        w = np.asarray(w, dtype=np.float64)
        X, Y, Z = w[:, 0] - self.cx, w[:, 1], w[:, 2]
        u, v = self.up * (Y * np.cos(self.a) - X * np.sin(self.a)), self.up * (Y * np.sin(self.a) + X * np.cos(self.a))
        return np.c_[480.0 + self.scale * (u - 0.3 * Z), 270.0 + self.scale * (v + 0.3 * Z), np.ones(len(w))]


def candidate_annotations(sncal, seeds=range(8)):
    """[(name, annotation)] for the label fixtures: synth.synthetic_annotation under its own random cameras (main-camera views:
    FixLRAmbiguous leaves them) and under TopDownView -- both halves in view (the medians branch) or one half only (the
    side-count branch), the left half up or down, under the true names and under mirrored names."""
    from sncal_amd.evaluate import SYMMETRIC
    out = []
    for seed in seeds:
        out.append((f'{seed}.main', as_dicts(sncal.synth.synthetic_annotation(seed)[0])))
        for tag, scale, cx in (('both', 4.8, 0.0), ('left', 8.5, -27.0), ('right', 8.5, 27.0)):
            view = TopDownView(scale, (seed % 5 - 2) * 1.2, cx, 1 if seed % 2 == 0 else -1)
            keep = sncal.synth.random_camera
            sncal.synth.random_camera = lambda rng: view
            try:
                pts = sncal.synth.synthetic_annotation(1000 + seed)[0]
            finally:
                sncal.synth.random_camera = keep
            out.append((f'{seed}.{tag}', as_dicts(pts)))
            out.append((f'{seed}.{tag}.mirrored', as_dicts({SYMMETRIC[k]: v for k, v in pts.items()})))
    return out
