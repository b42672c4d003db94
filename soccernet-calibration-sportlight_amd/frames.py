"""The input side: the JPEG files of a folder -> batches of uint8 BGR frames (and label dicts) on the device."""
import json
import os
import warnings
from typing import Callable, Iterator, List, Sequence

import numpy as np
import torch

from . import _lib
from .annotations import get_extreme_points, get_intersections, keypoint_labels_device, line_keypoints, sort_anno
from .augment import flip_annot_names
from .evaluate import scale_points
from .jpeg import JpegDecoder, check_reduce, probe, reduced_size
from .resize import check_size, resize_u8


def annot_to_keypoints(annot: dict, num_keypoints: int = 57, margin: float = 0.0):
    """HRNetDataset._annot2keypoints (dataset.py:73-87): SoccerNet annotation {class: [{'x', 'y'}, ...]} (normalised) ->
    (keypoints (3*num_keypoints,) float32 [x, y, 1] or [-1, -1, 0], mask (num_keypoints + 1,) int64)."""
    points = {cls: [(p['x'], p['y']) for p in pts] for cls, pts in annot.items()}           # reader.decode_annot
    kpts, missing = get_intersections(points, margin=margin)
    keypoints = np.ones(num_keypoints * 3, dtype=np.float32) * -1
    for i in range(num_keypoints):
        if kpts[i] is not None:
            keypoints[i * 3], keypoints[i * 3 + 1], keypoints[i * 3 + 2] = kpts[i][0], kpts[i][1], 1
        else:
            keypoints[i * 3 + 2] = 0
    mask = np.ones(num_keypoints + 1, dtype=np.int64)
    for i in missing:
        mask[i] = 0
    return keypoints, mask


def _annotated(folder: str) -> Iterator[tuple]:
    """(image name, annotation dict) of every .json of a split folder whose .jpg exists, sorted; names containing 'info' skipped."""
    for fname in sorted(os.listdir(folder)):
        if 'info' in fname or not fname.endswith('.json'):
            continue
        img = fname.replace('.json', '.jpg')
        if os.path.exists(os.path.join(folder, img)):
            with open(os.path.join(folder, fname), 'r') as f:
                yield img, json.load(f)


def list_split(folder: str):
    """dataset.py:41-50: (image names, annotation dicts) of a SoccerNet split folder, sorted; names containing 'info' skipped."""
    pairs = list(_annotated(folder))
    return [img for img, _ in pairs], [annot for _, annot in pairs]


MAX_SOURCE_SIZES = 4        # decoders a run with resize= keeps, one per distinct source size


def resize_plan(height: int, width: int, reduce: int = 1, resize=None):
    """Size bookkeeping of one height x width file (host only) -> ((h, w) it is decoded at, (H, W) of the frame yielded): decoded at
    1 / reduce (libjpeg rounds up), then brought to resize=(W, H) -- cv2.imread(path, IMREAD_REDUCED_COLOR_n) followed by
    cv2.resize(img, (W, H)).  resize=None: yielded as decoded."""
    dec = reduced_size(height, width, reduce)
    if resize is None:
        return dec, dec
    W, H = check_size(resize)
    return dec, (H, W)


def skipper(skipped: List[str]) -> Callable:
    """skip(name, why) of a run: the file is named in `skipped` and in a warning."""
    def skip(name, why):
        warnings.warn(f'{name}: skipped ({why})')
        skipped.append(name)
    return skip


def read_probed(folder: str, name: str):
    """-> (the file's bytes, jpeg.probe's dict of them).  Raises what open() and probe raise: the caller's except decides."""
    with open(os.path.join(folder, name), 'rb') as f:
        blob = f.read()
    return blob, probe(blob)


def decode_dropping(dec: JpegDecoder, files: Sequence[tuple], skip: Callable, out: torch.Tensor = None):
    """files [(name, blob), ...] of dec's size -> (positions in `files` kept, their frames decoded as ONE batch), ([], None) when
    every file was bad.  out: the buffer the decoder writes to (its first rows are returned); None: the decoder allocates."""
    into = (lambda n: None) if out is None else (lambda n: out[:n])
    kept = list(range(len(files)))
    try:
        return kept, dec.decode([b for _, b in files], into(len(files)))
    except _lib.SncalError:                             # a stream damaged behind its headers: find it, drop it, decode the rest
        kept = []
    for p, (name, blob) in enumerate(files):
        try:
            dec.decode([blob], into(1))
            kept.append(p)
        except _lib.SncalError as e:
            skip(name, e)
    if not kept:
        return [], None
    return kept, dec.decode([files[p][1] for p in kept], into(len(kept)))


def decoded_batches(folder: str, names: Sequence[str], batch_size: int, device, decoder_threads: int, skipped: List[str],
                    frame_size=None, reduce: int = 1, resize=None) -> Iterator[tuple]:
    """(indices into `names`, (n,H,W,3) uint8 BGR frames on the device) per batch of the JPEG files `names` of `folder`.  A file
    the decoder cannot take, or whose size is not the run's (frame_size (H, W), or the first frame's when None), is left out of
    its batch and named in `skipped`; a batch left empty is not yielded.
    reduce=2 / 4 / 8: the files are decoded at that fraction (JpegDecoder(reduce=): libjpeg's scaled decode, cv2.imread's
    IMREAD_REDUCED_COLOR flags).  frame_size stays the size of the frames YIELDED: a file is taken when its reduced size equals it.
    resize=(W, H): every decoded frame is brought to W x H by resize.resize_u8 (cv2.resize's INTER_LINEAR; after the reduced decode
    when reduce is given too), so files of ANY size are taken, mixed sizes included: one decoder per distinct source size, at most
    MAX_SOURCE_SIZES in a run -- a file of a further size is skipped and named like any other refusal.  A batch's files are decoded
    per size group and resized into their rows of the one batch yielded, in file order.  frame_size, when given, must be (H, W)."""
    check_reduce(reduce)
    size = None if frame_size is None else tuple(frame_size)
    if resize is not None:
        W, H = check_size(resize)
        if size is not None and size != (H, W):
            raise _lib.SncalError(f'resize={W}x{H} where frame_size asks for frames of {size[1]}x{size[0]}')
    decs = {}                   # source (height, width) -> its decoder, in order of first appearance; without resize there is ONE
    skip = skipper(skipped)

    def admit(fi):
        """The key in `decs` of a file that is taken (its decoder built when it is the first of its size); SncalError otherwise."""
        nonlocal size
        key = (fi['height'], fi['width'])
        if resize is None:
            got = reduced_size(key[0], key[1], reduce)
            if size is None:
                size = got
            if got != size:
                raise _lib.SncalError(f"{fi['width']}x{fi['height']}" + (f' (1/{reduce}: {got[1]}x{got[0]})' if reduce != 1 else '') +
                                      f" where the run's frames are {size[1]}x{size[0]}")
            if decs and key not in decs:                # sizes that round up to the same frame
                (h, w), = decs
                raise _lib.SncalError(f"{fi['width']}x{fi['height']} where the run's source frames are {w}x{h}")
        elif key not in decs and len(decs) >= MAX_SOURCE_SIZES:
            raise _lib.SncalError(f"{fi['width']}x{fi['height']}: source size number {MAX_SOURCE_SIZES + 1} of a run that keeps a "
                                  f'decoder for {MAX_SOURCE_SIZES} (' + ', '.join(f'{w}x{h}' for h, w in decs) + ')')
        if key not in decs:                             # a decoder is built for the SOURCE size of the first frame taken at it
            decs[key] = JpegDecoder(key[0], key[1], max_batch=batch_size, threads=decoder_threads, device=device, reduce=reduce)
        return key

    try:
        for i in range(0, len(names), batch_size):
            groups = {}                                 # key in decs -> [(index into names, blob)], file order inside a group
            for j in range(i, min(i + batch_size, len(names))):
                try:
                    blob, fi = read_probed(folder, names[j])
                    key = admit(fi)
                except (_lib.SncalError, OSError) as e:
                    skip(names[j], e)
                    continue
                groups.setdefault(key, []).append((j, blob))
            decoded = []                                # (indices, frames at the decoded size) per size group with a file left
            for key, files in groups.items():
                kept, image = decode_dropping(decs[key], [(names[j], blob) for j, blob in files], skip)
                if kept:
                    decoded.append(([files[p][0] for p in kept], image))
            if not decoded:
                continue
            if resize is None:                          # one group: its decoded tensor is the batch
                yield decoded[0]
                continue
            keep = sorted(j for js, _ in decoded for j in js)
            row = {j: r for r, j in enumerate(keep)}
            out = torch.empty((len(keep), H, W, 3), dtype=torch.uint8, device=device)
            for js, image in decoded:
                r0 = row[js[0]]
                if [row[j] for j in js] == list(range(r0, r0 + len(js))):      # a run of rows: resized where it belongs
                    resize_u8(image, (W, H), out=out[r0:r0 + len(js)])
                else:
                    out[torch.tensor([row[j] for j in js], device=out.device)] = resize_u8(image, (W, H))
            yield keep, out
    finally:                                            # also when the consumer stops early or raises: generator.close() lands here
        for dec in decs.values():
            dec.close()


def _label_mode(labels: str, transform):
    """labels='host' | 'device' -> (the transform to run on the host, whether the label kernel takes FixLRAmbiguous' decision)."""
    if labels not in ('host', 'device'):
        raise _lib.SncalError(f"labels={labels!r}: 'host' or 'device'")
    if labels == 'host' or transform is None:
        return transform, False
    if not hasattr(transform, 'deferring_fix_lr'):
        raise _lib.SncalError("labels='device' takes an augment.ComposeTransform (its FixLRAmbiguous moves into the label kernel)")
    return transform.deferring_fix_lr()


def folder_batches(folder: str, batch_size: int, device, num_keypoints: int, margin: float, img_size, decoder_threads: int,
                   skipped: List[str], transform=None, labels: str = 'host', reduce: int = 1, resize=None) -> Iterator[dict]:
    """The batch dicts of a split folder, frames decoded on the device as uint8 BGR (at 1 / reduce, then brought to resize=(W, H):
    see decoded_batches; the labels are normalised coordinates and do not change).  A file the decoder cannot take is left out
    of its batch and named in `skipped`.  transform: None, or the label transform of the reference's validation loader
    (augment.test_transform(): FixLRAmbiguous), applied to each annotation before scale_points and annot_to_keypoints as
    HRNetDataset.__getitem__ does (dataset.py:60-64).  labels: see labelled_batch."""
    names, annots = list_split(folder)
    transform, fix_lr = _label_mode(labels, transform)
    if transform is not None:
        annots = [transform.labels(a) for a in annots]
    frames = decoded_batches(folder, names, batch_size, device, decoder_threads, skipped, reduce=reduce, resize=resize)
    try:
        for keep, image in frames:
            yield labelled_batch(image, [annots[j] for j in keep], [names[j] for j in keep], num_keypoints, margin, img_size,
                                 labels=labels, fix_lr=fix_lr)
    finally:
        frames.close()


def labelled_batch(image, annots: Sequence[dict], names: Sequence[str], num_keypoints: int, margin: float, img_size,
                   labels: str = 'host', fix_lr: bool = False) -> dict:
    """The reference's batch dict (dataset.py:52-71 + custom_collate) from frames and their (already transformed) annotations.
    labels='host': annot_to_keypoints per frame, 'keypoints' and 'mask' on the host.  labels='device': one launch of the label kernel
    for the batch (annotations.keypoint_labels_device), 'keypoints' and 'mask' on the image's device; with fix_lr the kernel also
    takes FixLRAmbiguous' decision -- the annotations then come in WITHOUT that transform applied (ComposeTransform.deferring_fix_lr)
    -- and the host renames the swapped frames' annotations for 'raw_annot' from one copy of B bytes."""
    if labels == 'host':
        if fix_lr:
            raise _lib.SncalError("fix_lr is the label kernel's: with labels='host' FixLRAmbiguous runs in the transform")
        pairs = [annot_to_keypoints(a, num_keypoints, margin) for a in annots]
        keypoints = torch.from_numpy(np.stack([p[0] for p in pairs]))
        mask = torch.from_numpy(np.stack([p[1] for p in pairs]))
    elif labels == 'device':
        keypoints, mask, swapped = keypoint_labels_device(annots, margin=margin, num_keypoints=num_keypoints, fix_lr=fix_lr,
                                                          device=image.device)
        if fix_lr:
            annots = [flip_annot_names(a, swap_top_bottom=False, swap_posts=False) if s else a
                      for a, s in zip(annots, swapped.cpu().tolist())]
    else:
        raise _lib.SncalError(f"labels={labels!r}: 'host' or 'device'")
    return {'image': image,
            'keypoints': keypoints,
            'mask': mask,
            'raw_annot': [scale_points(a, img_size[0], img_size[1]) for a in annots],
            'img_name': list(names)}


def train_batches(folder: str, batch_size: int, transform, shuffle: bool = True, seed=None, device='cuda:0', num_keypoints: int = 57,
                  margin: float = 0.0, img_size=(960, 540), decoder_threads: int = 0, skipped: List[str] = None,
                  labels: str = 'host', reduce: int = 1, resize=None) -> Iterator[dict]:
    """One epoch of the reference's TRAINING batches (train.py:31-33: HRNetDataset with train_transform under a shuffling loader)
    of a split folder: {'image', 'keypoints', 'mask', 'raw_annot', 'img_name'}.  Frames are decoded and augmented on the device
    (augment.train_transform: 'image' is fp32 (B,3,H,W) with ToTensor in the list, uint8 (B,H,W,3) without); the labels come from
    the transformed annotations.  shuffle draws the epoch's order from numpy.random.RandomState(seed) -- a generator of its own, so
    the transform's draws from random / numpy.random are those of a run without shuffling.  A file the decoder cannot take is
    left out of its batch and named in `skipped` (when a list is given); the last batch may be short, as the reference's is.
    labels: see labelled_batch; with 'device' the transform's FixLRAmbiguous is carried out by the label kernel (it draws nothing,
    so the other transforms' draws are those of labels='host').  reduce, resize: the frames are decoded at 1 / reduce and
    brought to resize=(W, H) (decoded_batches) before the transform sees them."""
    names, annots = list_split(folder)
    order = np.random.RandomState(seed).permutation(len(names)) if shuffle else np.arange(len(names))
    names, annots = [names[j] for j in order], [annots[j] for j in order]
    transform, fix_lr = _label_mode(labels, transform)
    frames = decoded_batches(folder, names, batch_size, device, decoder_threads, skipped if skipped is not None else [], reduce=reduce,
                             resize=resize)
    try:
        for keep, image in frames:
            out = transform({'image': image, 'annot': [annots[j] for j in keep]})
            yield labelled_batch(out['image'], out['annot'], [names[j] for j in keep], num_keypoints, margin, img_size,
                                 labels=labels, fix_lr=fix_lr)
    finally:
        frames.close()


def list_line_split(folder: str, input_size=(960, 540), annots: bool = False):
    """EHMDataset.__init__ (line/dataset.py:54-67): (image names, labels) of the frames whose annotation sort_anno finds usable;
    labels are get_extreme_points' dicts.  Sorted by name (the reference takes os.listdir's order).  annots=True: a third list, the
    kept frames' annotations as they are on disk ({class: [{'x', 'y'}, ...]}, what the extremity metric scores against)."""
    names, labels, raw = [], [], []
    for img, annot in _annotated(folder):
        points = {cls: [(p['x'], p['y']) for p in pts] for cls, pts in annot.items()}           # reader.decode_annot
        res, usable = sort_anno(points, img_size=input_size)
        if usable:
            names.append(img)
            labels.append(get_extreme_points(res, img_size=input_size))
            raw.append(annot)
    return (names, labels, raw) if annots else (names, labels)


def line_folder_batches(folder: str, batch_size: int, device, num_keypoint_pairs: int, input_size, decoder_threads: int,
                        skipped: List[str], reduce: int = 1, annots: bool = False, resize=None) -> Iterator[dict]:
    """The line model's batch dicts {'image', 'keypoints', 'line_para', 'img_name'} of a split folder (no 'keypoint_maps': the
    loss rebuilds them); with annots=True also 'annot', the frames' annotations as they are on disk.  A frame is taken when its size
    at 1 / reduce is input_size (W, H): a 1920x1080 split goes into the 960x540 network with reduce=2.  That is libjpeg's scaled decode (cv2.imread's IMREAD_REDUCED_COLOR_2), NOT the cv2.resize of
    line/dataset.py:73 -- a declared deviation; a frame of any other size is skipped.
    resize=input_size IS that cv2.resize (resize.resize_u8, after the decode at 1 / reduce): frames of any size are taken, mixed
    sizes included (decoded_batches)."""
    names, labels, *raw = list_line_split(folder, input_size, annots=annots)
    frames = decoded_batches(folder, names, batch_size, device, decoder_threads, skipped, frame_size=(input_size[1], input_size[0]),
                             reduce=reduce, resize=resize)
    try:
        for keep, image in frames:
            pairs = [line_keypoints(labels[j], num_keypoint_pairs) for j in keep]
            batch = {'image': image,
                     'keypoints': torch.from_numpy(np.stack([p[0] for p in pairs])),
                     'line_para': torch.tensor([p[1] for p in pairs], dtype=torch.float64),
                     'img_name': [names[j] for j in keep]}
            if annots:
                batch['annot'] = [raw[0][j] for j in keep]
            yield batch
    finally:
        frames.close()
