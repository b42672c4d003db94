#!/usr/bin/env python3
"""Capture tests/golden/hrnet_w48x4.npz from the imported reference (CPU): the keypoint network at `upscale: 4`.

    python tools/make_golden_upscale4.py

In the manner of tools/make_golden.py::gen_hrnet (same stubs): the reference's HRNetHeatmap on the packaged hrnet_w48x4 config at full
depth, seeded_state_dict(cfg, 70, 1.5), seeded_input(1, H, W, 71) at 64x96 (head 64x96) and 70x102 (stem 35x51, head 72x104: the head is
not twice the stem).  Asserts max |reference - oracle| < 1e-4 and stores, per size (keys '<H>x<W>.<name>'):

    decode                     the reference's HRNetPredictionTransform((540, 960)) of its own output
    maxp, checksum, abs_checksum
    out_strided                out[:, :, ::4, ::4]
    full, full_channels        the full maps of every 8th channel and of the background channel

Seed 70 at gain 1.5 was chosen with the oracle so that an engine inside the suite's 2e-4 bound cannot move a decode index: for every
keypoint channel the top two entries of the column-maxima and of the row-maxima vectors differ by more than 1e-3 in log-probability
(measured 1.17e-3 at 64x96, 2.19e-3 at 70x102; of seeds 70..109 at gains 1.5 and 4.0 only 70 and 75 at gain 1.5 pass at both sizes).
The tool asserts that gap on the reference's own output and fails otherwise.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
CFG, SEED, GAIN = 'hrnet_w48x4', 70, 1.5
SIZES = ((64, 96), (70, 102))
MIN_GAP = 1e-3
# The arrays above are 688 KB of float32 for the two sizes; log-probabilities do not compress (zlib keeps 87 %, byte planes of
# x-deltas 67 %), and the suite compares them at 2e-4, so they stay exact float32.  The bound only guards against growth.
MAX_BYTES = 640 * 1000


def decode_gap(logp):
    """Smallest difference between the two largest entries of the column-maxima and of the row-maxima vector over the keypoint
    channels of (B,C,h,w) log-probabilities: what a perturbation has to exceed to move an index of the decode."""
    kp = logp[:, :-1]
    gap = np.inf
    for v in (kp.max(axis=2), kp.max(axis=3)):            # (B,C-1,w) column maxima, (B,C-1,h) row maxima
        s = np.sort(v, axis=-1)
        gap = min(gap, float((s[..., -1] - s[..., -2]).min()))
    return gap


def main():
    mg.install_stubs()
    from oracle import hrnet_ref as hr, decode as od
    from src.models.hrnet.model import HRNetHeatmap
    from src.models.hrnet.transforms import HRNetPredictionTransform
    cfg = hr.load_config(CFG)
    assert cfg['upscale'] == 4
    torch.manual_seed(0)
    net = HRNetHeatmap(mg.ref_cfg(cfg), num_refinement_stages=0, num_heatmaps=cfg['num_classes'])
    sd = hr.seeded_state_dict(cfg, SEED, GAIN)
    net.load_state_dict(sd, strict=True)
    net.eval()
    out = {'seed': np.array(SEED), 'head_gain': np.array(GAIN), 'sizes': np.array(SIZES)}
    for H, W in SIZES:
        x = hr.seeded_input(1, H, W, SEED + 1)
        with torch.no_grad():
            ref = net(x)[-1]
        err = (ref - hr.forward(sd, x, cfg)).abs().max().item()
        assert err < 1e-4, err
        refn = ref.numpy()
        gap = decode_gap(refn)
        assert gap >= MIN_GAP, (H, W, gap)
        dec = HRNetPredictionTransform((540, 960))(ref).numpy()
        assert np.array_equal(dec[..., :2], od.keypoint_decode(refn, (540, 960))[..., :2])
        chans = sorted(set(range(0, refn.shape[1], 8)) | {refn.shape[1] - 1})
        k = f'{H}x{W}.'
        out[k + 'decode'] = dec
        out[k + 'maxp'] = np.exp(refn).max(axis=(2, 3))
        out[k + 'checksum'] = np.array(mg.checksum(refn))
        out[k + 'abs_checksum'] = np.array(mg.checksum(np.abs(refn)))
        out[k + 'out_strided'] = refn[:, :, ::4, ::4].copy()
        out[k + 'full_channels'] = np.array(chans)
        out[k + 'full'] = refn[:, chans].copy()
        out[k + 'gap'] = np.array(gap)
        print(f'{CFG} {H}x{W} ok: head {refn.shape[2]}x{refn.shape[3]}, max|ref-oracle| = {err:.3g}, decode gap {gap:.3g}, '
              f'logp range {refn.min():.2f} .. {refn.max():.2f}')
    path = os.path.join(GOLD, CFG + '.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, 'bytes')
    assert size < MAX_BYTES, size


if __name__ == '__main__':
    main()
