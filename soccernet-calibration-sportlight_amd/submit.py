"""Harness counterpart of /root/reference/src/utils/make_submit.py:42-75: image directory ->
`camera_<frame>.json` files + completeness, with every stage of the loop on the GPU path.

    reference loop (per batch of 8)                      here (per batch, default 64)
    cv2.imread + ToTensor + torch.stack   :62-63          JpegDecoder.decode (host Huffman, device IDCT/colour) -> uint8 BGR
    model.predict(tensor).cpu().numpy()   :64             CalibrationPipeline.submit: forward + decode on the main stream,
    16-process pool, CameraCreator per row :65-69          one batched solve on a side stream (overlaps the next batch)
    json.dump(cam.to_json_parameters())   :36-37          interop.save_cameras, written while the next batch runs

    python -m sncal_amd.submit --img-dir DIR --model model.pth --save-dir OUT [--lines-file lines.pkl] [--reduce 2] [--resize 960 540]

--reduce 2 / 4 / 8 (make_submit(..., reduce=)) is the loop whose imread carries cv2.IMREAD_REDUCED_COLOR_2 / _4 / _8: libjpeg's
scaled decode, so that 1920x1080 footage reaches a network trained at 960x540 at the size it was trained for.
--resize W H (make_submit(..., resize=(W, H))) is the loop with a cv2.resize(img, (W, H)) behind its imread, on the device
(resize.resize_u8): 1280x720 footage, or any other size, into that network.  It composes with --reduce.
"""
import argparse
import os
from typing import List, Optional

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')      # see pipeline.py: streams must not alias on a hardware queue

import torch  # noqa: E402

from . import _lib
from .frames import decode_dropping, read_probed, skipper
from .interop import save_cameras
from .jpeg import JpegDecoder, check_reduce
from .metamodel import load_model
from .pipeline import CalibrationPipeline
from .pitch import PITCH_POINTS
from .prediction import CameraCreator, camera_from_record
from .resize import add_resize_argument, check_size, parsed_resize, resize_u8


def default_calibrator(lines_file: Optional[str] = None) -> CameraCreator:
    """The CameraCreator make_submit.py:45-50 builds."""
    return CameraCreator(PITCH_POINTS, conf_thresh=0.5, conf_threshs=[0.5, 0.35, 0.2], algorithm='iterative_voter',
                         lines_file=lines_file, max_rmse=55.0, max_rmse_rel=5.0, min_points=5, min_focal_length=10.0,
                         min_points_per_plane=6, min_points_for_refinement=6, reliable_thresh=57)


def run_frame_size(img_dir: str, img_names: List[str], sample: int = 32):
    """(H, W) of the run: the most frequent size among the first `sample` files whose headers the decoder accepts.  One odd file at
    the head of os.listdir's order (a thumbnail, a progressive or damaged stream) therefore neither ends the run nor makes every
    other frame a size mismatch.  Raises when no file of the sample can be probed."""
    sizes = {}
    for n in img_names[:sample]:
        try:
            info = read_probed(img_dir, n)[1]
        except (_lib.SncalError, OSError):
            continue
        key = (info['height'], info['width'])
        sizes[key] = sizes.get(key, 0) + 1
    if not sizes:
        raise _lib.SncalError(f'{img_dir}: none of the first {min(sample, len(img_names))} files is a JPEG the device decoder accepts '
                              '(baseline sequential Huffman, no EXIF rotation)')
    return max(sizes.items(), key=lambda kv: kv[1])[0]


def make_submit(img_dir: str, model, calibrator: CameraCreator, save_dir: str, batch_size: int = 64,
                decoder_threads: int = 0, img_names: Optional[List[str]] = None, max_skip_fraction: float = 0.5, reduce: int = 1,
                resize=None) -> dict:
    """The directory loop on a non-blocking stream of its own (JPEG decode, network, result copies), never on the legacy null
    stream: the condition for the pipeline's CU-masked solve streams (pipeline.py).  See _make_submit for the loop itself.

    reduce=2 / 4 / 8: the frames are decoded at that fraction of their size (libjpeg's scaled decode, what the reference's loop
    computes when its imread carries cv2.IMREAD_REDUCED_COLOR_2 / _4 / _8 -- not cv2.resize).  The run's size vote and the
    per-file size check stay on the SOURCE size; the network, the pipeline and the calibrator see the reduced frames, and the
    cameras written are in the pixels of the DECODED frame, exactly as in that reference loop.  A caller who wants them in
    source pixels rescales them with Camera.scale_resolution.

    resize=(W, H): every decoded frame (at 1 / reduce when given) is brought to W x H by resize.resize_u8, cv2.resize's INTER_LINEAR,
    one more launch per batch between the decoder and the network; the cameras are in the pixels of the RESIZED frame.  The size
    vote and the double-buffered loop stay on one source size: frames of another size are skipped as without it."""
    check_reduce(reduce)                                                            # refuses a bad denominator before anything runs
    if resize is not None:
        resize = check_size(resize)
    own = torch.cuda.Stream(device=model.nn_module.device)
    with torch.cuda.stream(own):
        res = _make_submit(img_dir, model, calibrator, save_dir, batch_size, decoder_threads, img_names, max_skip_fraction, reduce,
                           resize)
    own.synchronize()
    return res


def _make_submit(img_dir: str, model, calibrator: CameraCreator, save_dir: str, batch_size: int = 64,
                 decoder_threads: int = 0, img_names: Optional[List[str]] = None, max_skip_fraction: float = 0.5,
                 reduce: int = 1, resize=None) -> dict:
    """Returns {'frames', 'written', 'completeness', 'skipped'} (make_submit.py:72 prints the completeness).  Files the device
    decoder cannot take are skipped with a warning; when more than `max_skip_fraction` of the run was skipped the function
    raises instead of returning a near-empty result that looks like a bad model."""
    os.makedirs(save_dir, exist_ok=True)
    if img_names is None:
        img_names = [n for n in os.listdir(img_dir) if n.endswith('.jpg')]          # make_submit.py:56
    total = len(img_names)
    if total == 0:
        return {'frames': 0, 'written': 0, 'completeness': 0.0, 'skipped': []}
    H, W = run_frame_size(img_dir, img_names)
    net = model.nn_module
    pt = model.prediction_transform
    pipe = CalibrationPipeline(net, calibrator, decode_size=(pt.H, pt.W))
    dec = JpegDecoder(H, W, max_batch=batch_size, threads=decoder_threads, device=net.device, reduce=reduce)     # H, W: the source size
    frames = [torch.empty((batch_size, dec.out_height, dec.out_width, 3), dtype=torch.uint8, device=net.device) for _ in range(2)]
    # resize: the decoder's frames are resized into buffers of their own, two again (batch k + 1 is resized while batch k's solve reads)
    sized = None if resize is None else [torch.empty((batch_size, resize[1], resize[0], 3), dtype=torch.uint8, device=net.device)
                                         for _ in range(2)]
    pending = []                                                                    # (names, records, event)
    written = 0
    skipped = []                                                                    # frames the device decoder cannot take
    skip = skipper(skipped)

    def drain(keep: int):
        nonlocal written
        while len(pending) > keep:
            names, rec, ev = pending.pop(0)
            ev.synchronize()
            cams = [camera_from_record(r, calibrator.img_size) for r in calibrator.records(rec)]
            written += save_cameras(cams, names, save_dir)

    for k, i in enumerate(range(0, total, batch_size)):
        files = []
        for n in img_names[i:i + batch_size]:
            # a file the device decoder does not handle (progressive, arithmetic-coded, CMYK, another size than the first frame's, damaged)
            # is skipped with a warning and simply gets no camera file -- what the reference's loop does for a frame without a
            # camera -- instead of ending the run (cv2.imread would decode some of these: decode them elsewhere and upload uint8 frames)
            try:                                    # SncalError only: a file that cannot be read (OSError) ends the run
                blob, fi = read_probed(img_dir, n)
                if (fi['height'], fi['width']) != (H, W):
                    raise _lib.SncalError(f"{fi['width']}x{fi['height']} where the run's frames are {W}x{H}")
            except _lib.SncalError as e:
                skip(n, e)
                continue
            files.append((n, blob))
        if not files:
            continue
        kept, x = decode_dropping(dec, files, skip, out=frames[k & 1])
        if not kept:
            continue
        names = [files[p][0] for p in kept]
        if sized is not None:
            x = resize_u8(x, resize, out=sized[k & 1][:len(names)])
        out = pipe.submit(x, names=names)
        pending.append((names, out[1], pipe.last_done))
        drain(1)                                                                    # write batch k-1 while batch k runs
    drain(0)
    pipe.join()
    pipe.check_range()                                                              # the split-fp16 engine's range flag: raises if any batch left the fp16 range
    dec.close()
    if len(skipped) > max_skip_fraction * total:
        raise _lib.SncalError(f'{len(skipped)} of {total} frames were skipped (first: {skipped[0]}): more than the allowed fraction '
                              f'{max_skip_fraction:g}; decode these frames elsewhere and feed uint8 tensors to the pipeline')
    return {'frames': total, 'written': written, 'completeness': written / total, 'skipped': skipped}


def parser():
    ap = argparse.ArgumentParser(description='Camera calibration of a directory of frames (make_submit.py counterpart)')
    ap.add_argument('--img-dir', required=True)
    ap.add_argument('--model', required=True, help='argus checkpoint of the keypoint model (model_name/params/nn_state_dict)')
    ap.add_argument('--save-dir', required=True)
    ap.add_argument('--lines-file', default=None, help='lines pickle of export_line_result.py (optional)')
    ap.add_argument('--batch-size', type=int, default=64)
    ap.add_argument('--reduce', type=int, default=1, choices=[1, 2, 4, 8],
                    help="decode the frames at 1/N of their size (libjpeg's scaled decode = cv2.IMREAD_REDUCED_COLOR_N): 2 takes "
                         '1920x1080 footage into a 960x540 network; the cameras are in the pixels of the decoded frame')
    add_resize_argument(ap)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--dtype', default=None, choices=['fp16x3', 'bf16x3', 'fp32', 'bf16', 'fp8'],
                    help='default: the fp32-class engine of the build (fp16x3: split-fp16 products, fp32 accumulation -- the exact engine\'s '
                         'keypoint indices on every measured frame); fp32: the reference\'s own arithmetic on the fp32 MFMA, 2.8x slower; '
                         'bf16 / fp8: throughput modes, keypoints may move by one cell on near-ties')
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    resize = parsed_resize(a)
    if not torch.cuda.is_available():
        raise _lib.SncalError('no GPU visible: this package has no CPU path')
    model = load_model(a.model, loss=None, optimizer=None, device=a.device, dtype=a.dtype)
    res = make_submit(a.img_dir, model, default_calibrator(a.lines_file), a.save_dir, batch_size=a.batch_size, reduce=a.reduce,
                      resize=resize)
    print(f"Completeness: {res['completeness']:.2f}")
    return res


if __name__ == '__main__':
    main()
