"""tests/golden/jpeg_reduced.npz: JPEG streams and the frames libjpeg-turbo's SCALED decode gives for them.

    python tools/make_golden_jpeg_reduced.py

The scaled decode is `scale_num / scale_denom = 1 / d` with every other default kept (JDCT_ISLOW, fancy upsampling): what
`cv2.imread(path, cv2.IMREAD_REDUCED_COLOR_2 / _4 / _8)` returns.  cv2 is not installed in the build image; Pillow drives the
same library: after `im.draft(mode, (w // d, h // d))` the decoder is configured with `(scale, draft) == (d, 0)` -- scale d and
draft mode OFF, so the DCT method and the upsampling stay the defaults.  Both facts are asserted for every case, so that neither a
plain smaller decode nor draft mode can become a golden.

    names                  case names, '<h>x<w>_<444|422|420|gray>_q<quality>_r<restart interval>'
    jpg.<name>             the stream
    bgr.<name>.d<d>        (ceil(h / d), ceil(w / d), 3) uint8 BGR for every denominator d in 2, 4, 8 with h // d >= 1 and w // d >= 1
    jpg.hd                 one 1920x1080 4:2:0 stream of a smooth seeded image
    bgr.hd.d<d>.rowsum     its row sums at d = 2, 4, 8
"""
import io
import os

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (33, 47), (37, 100), (20, 40), (64, 96)]      # (h, w)
QUALITIES = (95, 75, 40)
DENOMS = (2, 4, 8)


def test_image(h, w, seed):
    """What a broadcast frame has: smooth gradients, sharp white lines, saturated patches (range limiting, colour clamping), noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([40 + 30 * np.sin(xx / 37.0 + yy / 53.0), 130 + 60 * np.cos(xx / 29.0) * np.sin(yy / 41.0),
                    50 + (xx * 3 + yy * 5) % 97], -1).astype(np.float64)
    img += rng.normal(0, 5, img.shape)
    for k in range(4):
        img[np.abs(yy - (xx * (0.3 + 0.2 * k) + 5 * k)) < 1.2] = 255
    img[h // 3:h // 2, w // 4:w // 2] = [255, 0, 0]
    img[h // 2:h // 2 + max(1, h // 6), w // 2:w // 2 + max(1, w // 5)] = [0, 0, 255]
    img[: max(1, h // 8), : max(1, w // 8)] = 0
    return np.clip(img, 0, 255).astype(np.uint8)


def scaled_bgr(data: bytes, d: int) -> np.ndarray:
    """libjpeg-turbo's decode of `data` at 1 / d, BGR as cv2 returns it."""
    assert features.check_feature('libjpeg_turbo')
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    im.draft(im.mode, (w // d, h // d))
    assert im.decoderconfig == (d, 0), (im.decoderconfig, d)                 # (scale, draft): scale d, draft mode off
    assert im.size == (-(-w // d), -(-h // d)), (im.size, w, h, d)
    return np.ascontiguousarray(np.asarray(im.convert('RGB'))[..., ::-1])


def smooth_image(h: int, w: int, seed: int) -> np.ndarray:
    """A seeded low-frequency image: compresses to a small stream at full HD."""
    r = np.random.RandomState(seed)
    a = (r.rand(h // 120 + 2, w // 120 + 2, 3) * 255).astype(np.uint8)
    return np.asarray(Image.fromarray(a).resize((w, h), Image.BICUBIC))


def main():
    out, names, k = {}, [], 0
    for (h, w) in SIZES:
        for sub in ('444', '422', '420', 'gray'):
            for rs in (0, 3):
                q = QUALITIES[k % 3]
                im = Image.fromarray(test_image(h, w, 200 + k))
                kw = dict(quality=q)
                if sub == 'gray':
                    im = im.convert('L')
                else:
                    kw['subsampling'] = {'444': 0, '422': 1, '420': 2}[sub]
                if rs:
                    kw['restart_marker_blocks'] = rs
                b = io.BytesIO()
                im.save(b, 'JPEG', **kw)
                data = b.getvalue()
                name = f'{h}x{w}_{sub}_q{q}_r{rs}'
                names.append(name)
                out['jpg.' + name] = np.frombuffer(data, np.uint8)
                for d in DENOMS:
                    if w // d >= 1 and h // d >= 1:
                        out[f'bgr.{name}.d{d}'] = scaled_bgr(data, d)
                k += 1
    b = io.BytesIO()
    Image.fromarray(smooth_image(1080, 1920, 7)).save(b, 'JPEG', quality=60, subsampling=2)
    data = b.getvalue()
    out['jpg.hd'] = np.frombuffer(data, np.uint8)
    for d in DENOMS:
        out[f'bgr.hd.d{d}.rowsum'] = scaled_bgr(data, d).astype(np.int64).sum(axis=(1, 2))
    out['names'] = np.array(names)
    path = os.path.join(GOLD, 'jpeg_reduced.npz')
    np.savez_compressed(path, **out)
    print('jpeg_reduced ok:', len(names), 'streams,', sum(key.startswith('bgr.') for key in out) - 3, 'reduced frames, 1080p stream',
          len(data), 'bytes, file', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
