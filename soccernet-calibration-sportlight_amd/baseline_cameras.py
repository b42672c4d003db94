"""Cameras from line extremities: the dev-kit's baseline of the calibration task (baseline/baseline_cameras.py).

    reference                                                      here
    normalization_transform                         :13-41         normalization_transform (host, numpy)
    estimate_homography_from_line_correspondences   :44-106        estimate_homography_from_line_correspondences (host, numpy)
    __main__: candidates, line matches, homography, :174-246       frame_flow / cameras_from_extremities on the host;
      Camera.from_homography, the nearest-candidate                csrc/linecam.hip (sncal_baseline_cameras) for a batch in one launch:
      matches, Camera.refine_camera                                line_cameras()
    __main__: the folder loop                       :150-251       baseline_cameras() and the command line

    python -m sncal_amd.baseline_cameras -s DATASET -p PREDICTIONS [--split valid] [--resolution_width 960] [--resolution_height 540]
    python -m sncal_amd.baseline_cameras --line-model line.pth --img-dir DIR --save-dir OUT [--reduce N]

Declared properties:
  * a class with fewer than two points is skipped (the reference raises IndexError); in the peaks form a class is kept only when
    both of its slots pass the threshold;
  * order: the host functions walk a dict in its own key order, as the reference does; the packed form and the device walk the
    classes in ANNOT_CLASSES order.  Order moves last bits (the sums of the normalisation, the SVD), except that ties of the
    nearest-candidate choice go to the first candidate;
  * pixels are x * W, y * H (:188-189), while export_extremities divides by (W - 1, H - 1): the baseline reads every point
    stretched by 1 / (W - 1), a property it inherits from the file convention;
  * the refinement is this project's LM (sncal_pnp_refine_lm's schedule, cap and stop): unpinned against OpenCV, as everywhere.
"""
import argparse
import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .annotations import ANNOT_CLASSES, pack_annotations
from .camera import Camera
from .evaluate import LINE_EXTREMITIES
from .frames import decoded_batches
from .lines import LINE_CLS
from .pitch import PITCH_POINTS, PITCH_POINTS_TO_INTERSECTON
from .resize import add_resize_argument, parsed_resize

IGNORED = 'Circle central'
STATUS_NONE, STATUS_HOMOGRAPHY, STATUS_REFINED = 0, 1, 2       # SNCAL_LINECAM_*
MATCH_MAX_PX = 100.0

# ---- the pitch tables of the method (csrc/linecam_tables.inc is written from these by tools/make_linecam_tables.py) ------------
LINE_ENDS: Dict[str, tuple] = {name: (a, b) for name, a, b in LINE_EXTREMITIES}             # SoccerPitch.line_extremities_keys
END_POINTS: List[str] = sorted({p for ends in LINE_ENDS.values() for p in ends}, key=PITCH_POINTS_TO_INTERSECTON.get)
END_INDEX = {name: i for i, name in enumerate(END_POINTS)}


def on_lawn(name: str) -> bool:
    """get_2d_homogeneous_line's condition (soccerpitch.py:519-521): a line of the lawn plane."""
    return name in LINE_ENDS and 'post' not in name and 'crossbar' not in name and 'Circle' not in name


def pitch_line(name: str) -> Optional[np.ndarray]:
    """get_2d_homogeneous_line (soccerpitch.py:512-528)."""
    if not on_lawn(name):
        return None
    a, b = (PITCH_POINTS[k] for k in LINE_ENDS[name])
    return np.cross(np.array([a[0], a[1], 1.]), np.array([b[0], b[1], 1.]))


# ---- the reference's functions, restated ------------------------------------------------------------------------------------

def normalization_transform(points) -> np.ndarray:
    """:13-41: the similarity that centres the cloud and brings its mean distance to the centre to sqrt(2); the mean distance is
    the running mean d += (d_i - d) / n, in the cloud's order.  A cloud of mean distance <= 0 keeps scale 1."""
    pts = np.asarray(points, dtype=np.float64)
    cx, cy = np.mean(pts, axis=0)[:2]
    d = 0.
    for n, p in enumerate(pts, 1):
        x, y = p[0] - cx, p[1] - cy
        d += (np.sqrt(x * x + y * y) - d) / n
    s = 1. if d <= 0. else np.sqrt(2) / d
    return np.array([[s, 0., -s * cx], [0., s, -s * cy], [0., 0., 1.]])


def line_system(lines, T1=np.eye(3), T2=np.eye(3)) -> np.ndarray:
    """:53-84: the (2L, 9) system of L (pitch line, image line) pairs, each line mapped by inv(T)^T."""
    A = np.zeros((len(lines) * 2, 9))
    T1it, T2it = np.linalg.inv(T1).T, np.linalg.inv(T2).T
    for i, (src, dst) in enumerate(lines):
        u, v, w = T1it @ src
        x, y, z = T2it @ dst
        A[2 * i] = (0, x * w, -x * v, 0, y * w, -v * y, 0, z * w, -v * z)
        A[2 * i + 1] = (x * w, 0, -x * u, y * w, 0, -u * y, z * w, 0, -u * z)
    return A


def estimate_homography_from_line_correspondences(lines, T1=np.eye(3), T2=np.eye(3)):
    """:44-106 -> (success, H).  The right singular vector is the one at index min(2L, 9) - 1 of the singular values sorted
    descending, walking up past exact zeros (:87-97): with exactly four lines that is the vector of the SMALLEST OF EIGHT singular
    values, not the null vector of the 8 x 9 system.  Kept as it is."""
    try:
        _, s, vh = np.linalg.svd(line_system(lines, T1, T2))
    except np.linalg.LinAlgError:
        return False, np.eye(3)
    for i in range(s.shape[0] - 1, -1, -1):
        if s[i] > 0:
            H = np.linalg.inv(T2) @ vh[i].reshape(3, 3) @ T1
            with np.errstate(all='ignore'):
                return True, H / H[2, 2]
    return False, np.eye(3)


def frame_flow(prediction: dict, img_size=(960, 540)) -> dict:
    """:174-236 for one frame's {class: [{'x', 'y'} or (x, y), ...]} (normalised), up to the refinement -> {'status' 0 / 1,
    'n_lines', 'T1', 'T2', 'H', 'camera' (Camera or None), 'slots' {end point name: class id * 2 + end of the chosen candidate},
    'matches' [(3-D point, 2-D point)], 'points' (the end points in their order of first appearance)}."""
    W, H = img_size
    cid = {c: i for i, c in enumerate(ANNOT_CLASSES)}
    line_matches, candidates, src_pts = [], {}, []
    for name, pts in prediction.items():
        if name == IGNORED or 'unknown' in name or len(pts) < 2:
            continue
        ends = LINE_ENDS[name]
        xy = [((p['x'], p['y']) if isinstance(p, dict) else (p[0], p[1])) for p in pts[:2]]
        p1, p2 = (np.array([x * W, y * H, 1.]) for x, y in xy)
        src_pts.extend([p1, p2])
        for end in ends:
            candidates.setdefault(end, []).extend([(p1, cid[name] * 2), (p2, cid[name] * 2 + 1)])
        with np.errstate(all='ignore'):
            line = np.cross(p1, p2)
            if not np.isfinite(np.sum(line)):
                continue
        if on_lawn(name):
            line_matches.append((pitch_line(name), line))
    out = {'status': STATUS_NONE, 'n_lines': len(line_matches), 'T1': None, 'T2': None, 'H': None, 'camera': None, 'slots': {},
           'matches': [], 'points': list(candidates)}
    if len(line_matches) < 4:
        return out
    with np.errstate(all='ignore'):
        out['T1'] = normalization_transform([PITCH_POINTS[k][:2] for k in candidates])
        out['T2'] = normalization_transform(src_pts)
        ok, Hm = estimate_homography_from_line_correspondences(line_matches, out['T1'], out['T2'])
    if not ok:
        return out
    out['H'] = Hm
    cam = Camera(W, H)
    with np.errstate(all='ignore'):
        if not cam.from_homography(Hm):
            return out
        out['status'], out['camera'] = STATUS_HOMOGRAPHY, cam
        for k, cands in candidates.items():
            q = cam.project_point(PITCH_POINTS[k])
            if 0 < q[0] < W and 0 < q[1] < H:
                dist = np.array([np.sqrt((q[0] - c[0]) ** 2 + (q[1] - c[1]) ** 2) for c, _ in cands])
                sel = int(np.argmin(dist))                       # the first of equal distances; a NaN distance wins and fails the test below
                if dist[sel] < MATCH_MAX_PX:
                    out['slots'][k] = cands[sel][1]
                    out['matches'].append((PITCH_POINTS[k], cands[sel][0][:2]))
    return out


def cameras_from_extremities(predictions: Sequence[dict], img_size=(960, 540), refine: bool = True) -> List[Optional[Camera]]:
    """:174-246 per frame: a Camera or None.  With more than 3 matches the camera is refined through Camera.refine_camera (the
    device LM of one frame); refine=False stops after from_homography and needs no GPU."""
    cams = []
    for pred in predictions:
        r = frame_flow(pred, img_size)
        if r['camera'] is not None and refine and len(r['matches']) > 3:
            r['camera'].refine_camera(r['matches'])
        cams.append(r['camera'])
    return cams


# ---- the device call -------------------------------------------------------------------------------------------------------

def line_cameras(peaks=None, pred_annots=None, img_size=(960, 540), refine: bool = True, scale: float = 4, p_threshold: float = 0.2,
                 device='cuda:0'):
    """sncal_baseline_cameras for a batch -> (cameras (B, sizeof(sncal_camera)) uint8, status (B,) int32, H (B,9) float64, n_lines (B,)
    int32, slots (B, len(END_POINTS)) int32), on the device; asynchronous on the current stream.
    peaks        (B,C,2,3) fp32 on the GPU, rows [x, y, p] (C <= 23 channels in LINE_CLS order): a class is kept when both slots have
                 p >= p_threshold; pixel = float32(x * scale), read as the extremities_<id>.json of export_extremities would give it
    pred_annots  the other form: predictions as normalised dicts (the extremities_<id>.json files) or pack_annotations' tuple
    status 0 = no camera, 1 = from the homography, 2 = refined; slots[b, e] = class id * 2 + end of the candidate matched to
    END_POINTS[e], or -1."""
    import ctypes
    import torch
    if (peaks is None) == (pred_annots is None):
        raise _lib.SncalError('line_cameras takes exactly one of peaks= and pred_annots=')
    if peaks is not None:
        peaks = _lib.require_device(peaks, torch.float32, 'peaks')
        if peaks.dim() != 4 or tuple(peaks.shape[2:]) != (2, 3):
            raise _lib.SncalError(f'peaks {tuple(peaks.shape)} must be (B,C,2,3): two slots [x, y, p] per channel')
        B, dev, parts = peaks.shape[0], peaks.device, []
    else:
        p_pts, p_off, _ = pred_annots if isinstance(pred_annots, tuple) else pack_annotations(pred_annots)
        B, dev, parts = len(p_off), torch.device(device), [p_pts, p_off]
    rec = ctypes.sizeof(_lib.Camera)
    cams = torch.zeros((B, rec), dtype=torch.uint8, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    Hm = torch.zeros((B, 9), dtype=torch.float64, device=dev)
    n_lines = torch.zeros(B, dtype=torch.int32, device=dev)
    slots = torch.full((B, len(END_POINTS)), -1, dtype=torch.int32, device=dev)
    if B or peaks is not None:
        if peaks is not None:
            args = (peaks, peaks.shape[1], float(scale), float(p_threshold), None, 0, None)      # an empty batch's peaks go as NULL
        else:
            d_in, ptr = _lib.upload(parts, dev, pinned=True)                                 # one upload, pinned: extremity_counts' reason
            args = (None, 0, float(scale), float(p_threshold), ptr[0], len(p_pts), ptr[1])
        _lib.launch('sncal_baseline_cameras', dev, *args, B, len(ANNOT_CLASSES), int(img_size[0]), int(img_size[1]), int(bool(refine)),
                    cams, status, Hm, n_lines, slots, len(END_POINTS))
    return cams, status, Hm, n_lines, slots


def records_to_cameras(cams, status, img_size=(960, 540)) -> List[Optional[Camera]]:
    """line_cameras' records (device or host) -> a Camera per frame, None where the status is 0."""
    raw = cams.cpu().numpy() if hasattr(cams, 'cpu') else np.asarray(cams)
    st = status.cpu().numpy() if hasattr(status, 'cpu') else np.asarray(status)
    out = []
    for b in range(len(st)):
        if st[b] == STATUS_NONE:
            out.append(None)
            continue
        r = _lib.Camera.from_buffer_copy(raw[b].tobytes())
        cam = Camera(img_size[0], img_size[1])
        cam._set_intrinsics(np.float64(r.fx), np.float64(r.fy), (r.cx, r.cy))
        cam.rotation = np.array(r.rotation, dtype=np.float64).reshape(3, 3)
        cam.position = np.array(r.position, dtype=np.float64)
        out.append(cam)
    return out


# ---- folders -----------------------------------------------------------------------------------------------------------------

def baseline_cameras(soccernet_dir: str, prediction_dir: str, split: str = 'valid', resolution=(960, 540), batch_size: int = 256,
                     device='cuda:0') -> int:
    """The reference's command line (:150-251), batched: for the frames of soccernet_dir/split/per_match_info.json that have a
    prediction_dir/split/extremities_<id>.json, the cameras of sncal_baseline_cameras, written as camera_<id>.json beside the
    predictions through interop.save_cameras -> files written."""
    from .interop import save_cameras
    dataset_dir = os.path.join(soccernet_dir, split)
    if not os.path.exists(dataset_dir):
        raise _lib.SncalError(f'{dataset_dir}: invalid dataset path')
    with open(os.path.join(dataset_dir, 'per_match_info.json'), 'r') as f:
        match_info = json.load(f)
    names, preds, written = [], [], 0

    def flush():
        nonlocal written
        if names:
            cams, status = line_cameras(pred_annots=preds, img_size=resolution, device=device)[:2]
            written += save_cameras(records_to_cameras(cams, status, resolution), names, os.path.join(prediction_dir, split))
            names.clear(), preds.clear()
    for match in match_info:
        for frame in match_info[match]:
            index = frame.split('.')[0]
            path = os.path.join(prediction_dir, split, f'extremities_{index}.json')
            if not os.path.exists(path):
                continue
            with open(path, 'r') as f:
                pred = json.load(f)
            preds.append(pred)
            names.append(index + '.jpg')
            if len(names) == batch_size:
                flush()
    flush()
    return written


def line_model_cameras(img_dir: str, model, save_dir: str, batch_size: int = 64, conf_threshold: float = 0.2, decoder_threads: int = 0,
                       reduce: int = 1, collect: Optional[list] = None, resize=None) -> int:
    """One pass over the .jpg files of img_dir: JPEG decode -> line network -> two-peak decode -> sncal_baseline_cameras on the decoded
    peaks where they lie (no host round trip between the decode and the cameras) -> camera_<id>.json in save_dir -> files written.
    collect: a list that receives (names, peaks, records, status) per batch, on the device.
    resize=(W, H): every frame is brought to W x H after the decode (resize.resize_u8: the cv2.resize of baseline/dataloader.py:62 and
    detect_extremities.py:237), frames of any size, mixed sizes included (frames.decoded_batches); the cameras are in its pixels."""
    from .interop import save_cameras
    names = sorted(f for f in os.listdir(img_dir) if f.endswith('.jpg'))
    skipped: List[str] = []
    frames = decoded_batches(img_dir, names, batch_size, model.device, decoder_threads, skipped, reduce=reduce, resize=resize)
    written = 0
    try:
        for keep, image in frames:
            peaks = model.predict(image).contiguous()
            size = (image.shape[2], image.shape[1])
            cams, status = line_cameras(peaks=peaks, img_size=size, scale=1, p_threshold=conf_threshold)[:2]
            kept = [names[j] for j in keep]
            if collect is not None:
                collect.append((kept, peaks, cams, status))
            written += save_cameras(records_to_cameras(cams, status, size), kept, save_dir)
    finally:
        frames.close()
    return written


def parser():
    ap = argparse.ArgumentParser(description='Baseline for camera parameters extraction (baseline_cameras.py counterpart)')
    ap.add_argument('-s', '--soccernet', default='./annotations', type=str, help='Path to the SoccerNet-V3 dataset folder')
    ap.add_argument('-p', '--prediction', default='./results_bis', required=False, type=str, help='Path to the prediction folder')
    ap.add_argument('--split', required=False, type=str, default='valid', help='Select the split of data')
    ap.add_argument('--resolution_width', required=False, type=int, default=960, help='width resolution of the images')
    ap.add_argument('--resolution_height', required=False, type=int, default=540, help='height resolution of the images')
    ap.add_argument('--line-model', type=str, default=None, help='line checkpoint: the one-pass form (with --img-dir and --save-dir)')
    ap.add_argument('--img-dir', type=str, default=None, help='folder of .jpg frames for the one-pass form')
    ap.add_argument('--save-dir', type=str, default=None, help='where the one-pass form writes camera_<id>.json')
    ap.add_argument('--reduce', type=int, default=1, help='decode the frames at 1/N of their size (1, 2, 4, 8)')
    add_resize_argument(ap)
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    resize = parsed_resize(a)
    if a.line_model is not None:
        if not (a.img_dir and a.save_dir):
            ap.error('--line-model needs --img-dir and --save-dir')
        from .metamodel import load_model
        n = line_model_cameras(a.img_dir, load_model(a.line_model), a.save_dir, reduce=a.reduce, resize=resize)
    else:
        n = baseline_cameras(a.soccernet, a.prediction, split=a.split, resolution=(a.resolution_width, a.resolution_height))
    print(f'{n} cameras written')
    return n


if __name__ == '__main__':
    main()
