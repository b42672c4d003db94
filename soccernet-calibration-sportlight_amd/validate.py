"""Score a checkpoint: counterpart of /root/reference/src/models/hrnet/validate.py (val_config.yaml, optimize_valid.yaml) with
every stage on the GPU path.

    reference (argus Model.validate over get_loader)              here
    cv2.imread + ToTensor, get_intersections   dataset.py:52-87   JpegDecoder -> uint8 BGR frames; annotations.get_intersections
    model.val_step: forward, HRNetLoss, decode metamodel.py:59-86 HRNetMetaModel.val_step: one forward (heatmap + keypoints), fused loss
    L2metric                                   metrics.py:14-94   metrics.L2metric, accumulators on the device
    EvalAImetric: 16-process pool per frame    metrics.py:97-229  metrics.EvalAImetric: batched solve + batched evaluation
    Loss metric (argus)                                           mean of the step losses weighted by step size (see validate())

    python -m sncal_amd.validate --data DIR --model model.pth [--lines-file lines.pkl] [--batch-size 16] [--reduce 2]

The line model (line/train_config.yaml: val_loss and the monitored val_acc) is scored by validate_line():
    EHMDataset listing, sort_anno, extreme points  line/dataset.py:54-92   list_line_split, annotations.line_keypoints
    model.val_step: forward, EHMLoss, decode       line/metamodel.py:51-71 EHMMetaModel.val_step: one forward, fused loss, target rebuilt
    AccMetric                                      line/metrics.py:20-137  metrics.AccMetric: counts on the device

    python -m sncal_amd.validate --line --data DIR --model line.pth [--batch-size 8] [--reduce 2]

--reduce 2 / 4 / 8 decodes the split's frames at that fraction (libjpeg's scaled decode = cv2.imread's IMREAD_REDUCED_COLOR flags, not
cv2.resize): a 1920x1080 split scored by a 960x540 checkpoint.
--resize W H brings every frame to W x H after the decode with cv2.resize's bilinear shrink on the device (resize.resize_u8: the
cv2.resize of line/dataset.py:73): a 1280x720 split, or one of mixed sizes, scored by a 960x540 checkpoint.  It composes with --reduce.
"""
import argparse
import json
import os
import warnings
from typing import Dict, Iterable, Iterator, List, Sequence, Union

import numpy as np
import torch

from . import _lib
from .annotations import get_extreme_points, get_intersections, keypoint_labels_device, line_keypoints, sort_anno
from .evaluate import scale_points
from .jpeg import JpegDecoder, check_reduce, probe, reduced_size
from .lines import LINE_CLS
from .metrics import AccMetric, EvalAImetric, EvalAISweep, ExtremityMetric, L2metric
from .prediction import CameraCreator, parse_range
from .resize import check_size, resize_u8


class _State:
    def __init__(self, phase='val'):
        self.phase = phase
        self.metrics = {}


class ValidationResult(dict):
    """The metrics dict; .frames = frames seen, .skipped = names of the frames that could not be decoded (counted as missed)."""
    frames = 0
    skipped: List[str] = []
    params: Dict[str, float] = {}           # validate(sweep=): the grid point this result belongs to
    extremities: Dict[float, dict] = None   # validate_line(extremities=): ExtremityMetric.compute()'s dict per threshold


class SweepResults(list):
    """validate(sweep=)'s ValidationResults in grid order (max_rmse outermost); .best = index of the first maximum of val_evalai."""
    best = 0


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


def list_split(folder: str):
    """dataset.py:41-50: (image names, annotation dicts) of a SoccerNet split folder, sorted; names containing 'info' skipped."""
    names, annots = [], []
    for fname in sorted(os.listdir(folder)):
        if 'info' in fname or not fname.endswith('.json'):
            continue
        img = fname.replace('.json', '.jpg')
        if os.path.exists(os.path.join(folder, img)):
            with open(os.path.join(folder, fname), 'r') as f:
                annots.append(json.load(f))
            names.append(img)
    return names, annots


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


def _resized_batches(folder, names, batch_size, device, decoder_threads, skipped, frame_size, reduce, resize):
    """decoded_batches with resize=(W, H): any source size is taken, one JpegDecoder per distinct size (MAX_SOURCE_SIZES at most)."""
    W, H = check_size(resize)
    if frame_size is not None and tuple(frame_size) != (H, W):
        raise _lib.SncalError(f'resize={W}x{H} where frame_size asks for frames of {frame_size[1]}x{frame_size[0]}')
    decs = {}                                           # source (height, width) -> its decoder, in order of first appearance

    def skip(name, why):
        warnings.warn(f'{name}: skipped ({why})')
        skipped.append(name)

    try:
        for i in range(0, len(names), batch_size):
            groups = {}                                 # source size -> [(index into names, blob)], file order inside a group
            for j in range(i, min(i + batch_size, len(names))):
                try:
                    with open(os.path.join(folder, names[j]), 'rb') as f:
                        blob = f.read()
                    fi = probe(blob)
                    key = (fi['height'], fi['width'])
                    if key not in decs:
                        if len(decs) >= MAX_SOURCE_SIZES:
                            raise _lib.SncalError(f"{fi['width']}x{fi['height']}: source size number {MAX_SOURCE_SIZES + 1} of a run that keeps a "
                                                  f'decoder for {MAX_SOURCE_SIZES} (' + ', '.join(f'{w}x{h}' for h, w in decs) + ')')
                        decs[key] = JpegDecoder(key[0], key[1], max_batch=batch_size, threads=decoder_threads, device=device, reduce=reduce)
                except (_lib.SncalError, OSError) as e:
                    skip(names[j], e)
                    continue
                groups.setdefault(key, []).append((j, blob))
            decoded = []                                # (indices, frames at the decoded size) per size group
            for key, files in groups.items():
                dec = decs[key]
                try:
                    image = dec.decode([b for _, b in files])
                except _lib.SncalError:                 # a stream damaged behind its headers: find it, drop it, decode the rest
                    good = []
                    for j, blob in files:
                        try:
                            dec.decode([blob])
                            good.append((j, blob))
                        except _lib.SncalError as e:
                            skip(names[j], e)
                    if not good:
                        continue
                    files = good
                    image = dec.decode([b for _, b in files])
                decoded.append(([j for j, _ in files], image))
            keep = sorted(j for js, _ in decoded for j in js)
            if not keep:
                continue
            row = {j: r for r, j in enumerate(keep)}
            out = torch.empty((len(keep), H, W, 3), dtype=torch.uint8, device=device)
            for js, image in decoded:
                r0 = row[js[0]]
                if [row[j] for j in js] == list(range(r0, r0 + len(js))):      # a run of rows: resized where it belongs
                    resize_u8(image, (W, H), out=out[r0:r0 + len(js)])
                else:
                    out[torch.tensor([row[j] for j in js], device=out.device)] = resize_u8(image, (W, H))
            yield keep, out
    finally:
        for dec in decs.values():
            dec.close()


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
    if resize is not None:
        yield from _resized_batches(folder, names, batch_size, device, decoder_threads, skipped, frame_size, reduce, resize)
        return
    dec, size = None, frame_size

    def skip(name, why):
        warnings.warn(f'{name}: skipped ({why})')
        skipped.append(name)

    try:
        for i in range(0, len(names), batch_size):
            keep, blobs = [], []
            for j in range(i, min(i + batch_size, len(names))):
                try:
                    with open(os.path.join(folder, names[j]), 'rb') as f:
                        blob = f.read()
                    fi = probe(blob)
                    got = reduced_size(fi['height'], fi['width'], reduce)
                    if size is None:
                        size = got
                    if got != tuple(size):
                        raise _lib.SncalError(f"{fi['width']}x{fi['height']}" + (f' (1/{reduce}: {got[1]}x{got[0]})' if reduce != 1 else '') +
                                              f" where the run's frames are {size[1]}x{size[0]}")
                    if dec is not None and (fi['height'], fi['width']) != (dec.height, dec.width):      # sizes that round up to the same frame
                        raise _lib.SncalError(f"{fi['width']}x{fi['height']} where the run's source frames are {dec.width}x{dec.height}")
                    if dec is None:         # the decoder is built for the SOURCE size of the first frame taken
                        dec = JpegDecoder(fi['height'], fi['width'], max_batch=batch_size, threads=decoder_threads, device=device, reduce=reduce)
                except (_lib.SncalError, OSError) as e:
                    skip(names[j], e)
                    continue
                keep.append(j)
                blobs.append(blob)
            if not keep:
                continue
            try:
                image = dec.decode(blobs)
            except _lib.SncalError:                         # a stream damaged behind its headers: find it, drop it, decode the rest
                good = []
                for j, blob in zip(keep, blobs):
                    try:
                        dec.decode([blob])
                        good.append((j, blob))
                    except _lib.SncalError as e:
                        skip(names[j], e)
                if not good:
                    continue
                keep, blobs = [j for j, _ in good], [b for _, b in good]
                image = dec.decode(blobs)
            yield keep, image
    finally:                                            # also when the consumer stops early or raises: generator.close() lands here
        if dec is not None:
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
            from .augment import flip_annot_names
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
    for fname in sorted(os.listdir(folder)):
        if 'info' in fname or not fname.endswith('.json'):
            continue
        img = fname.replace('.json', '.jpg')
        if not os.path.exists(os.path.join(folder, img)):
            continue
        with open(os.path.join(folder, fname), 'r') as f:
            annot = json.load(f)
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


def validate(model, data: Union[str, Iterable[dict]], camera: Union[CameraCreator, Sequence[CameraCreator]], batch_size: int = 16,
             loss=None, decoder_threads: int = 0, conf_threshold: float = 0.5, pckhs_thres: Sequence[float] = (2.0, 5.0, 10.0, 50.0),
             threshold: int = 5, img_size=(960, 540), transform=None, labels: str = 'host', reduce: int = 1, sweep: Dict[str, Sequence[float]] = None,
             resize=None):
    """-> {'val_loss', 'val_l2', 'val_precision', 'val_recall', 'val_pcks-2.0', ..., 'val_l2_reprojection', 'val_completeness',
    'val_eval_precision', 'val_eval_recall', 'val_eval_accuracy', 'val_evalai'} as floats (a ValidationResult).

    data    a SoccerNet split folder (NNNNN.jpg + NNNNN.json) or any iterable of the batch dicts the reference's loader yields
            ({'image', 'keypoints', 'mask', 'raw_annot', 'img_name'}; batch_size then is whatever the iterable delivers)
    camera  a CameraCreator, or a LIST of them: the network, the loss and L2metric run once per batch, only solve + evaluation run
            per calibrator, and a list of results comes back, one per calibrator -- the trials of optimize_valid.yaml without
            running the network once per trial
    loss    an HRNetLoss; default: the model's own (params['loss'] of the checkpoint)
    transform  folder form only.  None: the annotations as they are on disk.  augment.test_transform(): what the reference's
            validation loader applies (validate.py:33, train.py:34) -- FixLRAmbiguous mirrors the class names of a behind-the-goal
            frame annotated the other way round, so val_loss and the keypoint metrics of such frames are taken against the
            keypoints the reference takes them against
    labels  folder form only.  'host': annotations.get_intersections per frame; 'device': one launch of the label kernel per batch,
            the transform's FixLRAmbiguous included
    reduce  folder form only.  2 / 4 / 8: the frames are decoded at that fraction of their size (libjpeg's scaled decode, what
            cv2.imread returns with IMREAD_REDUCED_COLOR_2 / _4 / _8; not cv2.resize), so that a 1920x1080 split is scored by a
            network trained at 960x540.  img_size stays the size the metrics work in; the labels are normalised and do not change
    resize  folder form only.  (W, H): every frame is brought to that size after the decode (at 1 / reduce when given) by
            resize.resize_u8, cv2.resize's INTER_LINEAR on the device; frames of any size are taken, mixed sizes included
            (decoded_batches).  img_size is in the resized frame's units
    sweep   {'max_rmse': [...], 'max_rmse_rel': [...]}: the search space of optimize_valid.yaml in ONE pass.  camera then is one
            CameraCreator ('iterative_voter' or 'voter'; its own max_rmse / max_rmse_rel are not read): every batch is solved once
            and each distinct camera evaluated once (metrics.EvalAISweep), and a SweepResults comes back: one ValidationResult per
            point of the cartesian product, max_rmse outermost, each with .params, equal key by key to validate(..., [one
            calibrator per grid point]); .best is the first maximum of val_evalai.  val_loss and the keypoint metrics are computed
            once.  conf_thresh(s), min_points* and reliable_thresh change the solves themselves: they stay the caller's loop

    val_loss is the mean of the step losses weighted by step size.  This is the one definition here NOT taken from the reference:
    it is computed by pytorch-argus' Loss metric there, whose source is not part of the reference tree.
    A frame the decoder refuses (folder form) gets no prediction: it is left out of val_loss and the keypoint metrics and counted
    as a missed frame by the camera metrics, as a frame without a camera is.  The host waits for the GPU once, at the end."""
    if transform is not None and not isinstance(data, (str, os.PathLike)):
        raise _lib.SncalError('transform applies to the folder form: batches handed in carry their labels already')
    if labels != 'host' and not isinstance(data, (str, os.PathLike)):
        raise _lib.SncalError('labels applies to the folder form: batches handed in carry their labels already')
    if reduce != 1 and not isinstance(data, (str, os.PathLike)):
        raise _lib.SncalError('reduce applies to the folder form: batches handed in carry their frames already')
    if resize is not None and not isinstance(data, (str, os.PathLike)):
        raise _lib.SncalError('resize applies to the folder form: batches handed in carry their frames already')
    if sweep is not None:
        if isinstance(camera, (list, tuple)):
            raise _lib.SncalError('sweep takes ONE CameraCreator: the grid replaces the list of calibrators')
        if set(sweep) != {'max_rmse', 'max_rmse_rel'}:
            raise _lib.SncalError(f"sweep={{'max_rmse': [...], 'max_rmse_rel': [...]}}, not keys {sorted(sweep)}")
    cams = list(camera) if isinstance(camera, (list, tuple)) else [camera]
    own_loss = model.loss
    if loss is not None:
        model.loss = loss                      # for this call only: restored below
    batches = None
    try:
        loss_fn = model._loss()
        nk = loss_fn.num_keypoints
        l2 = L2metric(num_keypoints=nk, conf_threshold=conf_threshold, pckhs_thres=pckhs_thres)
        if sweep is not None:
            evals = [EvalAISweep(camera, sweep['max_rmse'], sweep['max_rmse_rel'], threshold=threshold, img_size=img_size)]
        else:
            evals = [EvalAImetric(c, threshold=threshold, img_size=img_size) for c in cams]
        skipped: List[str] = []
        if isinstance(data, (str, os.PathLike)):
            batches = folder_batches(os.fspath(data), batch_size, model.device, nk, float(loss_fn.sigma), img_size, decoder_threads, skipped,
                                     transform=transform, labels=labels, reduce=reduce, resize=resize)
        loss_sum = torch.zeros((), dtype=torch.float64, device=model.device)
        frames = 0
        for batch in (batches if batches is not None else data):
            out = model.val_step(batch)
            B = out['prediction'].shape[0]
            frames += B
            loss_sum = loss_sum + out['loss'].to(torch.float64) * B
            l2.update(out)
            for ev in evals:
                ev.update(out)
        model.check_range()
    finally:
        if batches is not None:
            batches.close()                    # ends the generator: its finally closes the decoder, also after an exception mid-epoch
        if loss is not None:
            model.loss = own_loss
    val_loss = float(loss_sum.item()) / frames if frames else float('nan')
    results = SweepResults() if sweep is not None else []
    for ev in evals:
        ev.add_missed(len(skipped))
        for g in (range(len(ev)) if sweep is not None else [None]):
            state = _State('val')
            state.metrics['val_loss'] = val_loss
            l2.epoch_complete(state)
            if g is None:
                ev.epoch_complete(state)
            else:
                ev.epoch_complete(state, g)
            res = ValidationResult({k: float(v) for k, v in state.metrics.items()})
            res.frames, res.skipped = ev.total_frames, list(skipped)          # the camera metric's own count: scored + skipped
            if g is not None:
                res.params = ev.params(g)
            results.append(res)
    if sweep is not None:
        scores = [r['val_evalai'] for r in results]
        results.best = scores.index(max(scores))
        return results
    return results if isinstance(camera, (list, tuple)) else results[0]


def validate_line(model, data: Union[str, Iterable[dict]], batch_size: int = 8, loss=None, conf_threshold: float = 0.2,
                  decoder_threads: int = 0, input_size=(960, 540), reduce: int = 1, extremities: Sequence[float] = None, resize=None):
    """Score a line-model checkpoint (EHMMetaModel) -> {'val_loss', 'val_acc'} as floats (a ValidationResult): the two numbers
    line/train_config.yaml logs and monitors.

    data    a SoccerNet split folder (NNNNN.jpg + NNNNN.json; frames whose annotation the reference's sort_anno rejects are
            dropped, as its dataset drops them) whose frames are input_size once decoded at 1 / reduce, or any iterable of the batch dicts the reference's loader
            yields ({'image', 'keypoints', 'line_para', ['keypoint_maps']}; batch_size then is whatever the iterable delivers)
    loss    an EHMLoss; default: the model's own (params['loss'] of the checkpoint)
    reduce  folder form only.  A 1920x1080 split is taken with reduce=2: libjpeg's scaled decode (cv2.imread with
            IMREAD_REDUCED_COLOR_2), which is NOT the cv2.resize of line/dataset.py:73 -- a declared deviation.
            The labels are normalised coordinates and do not change; a frame whose reduced size is not input_size is skipped
    resize  folder form only.  input_size again, as (W, H): every frame is brought to it after the decode (at 1 / reduce when given)
            by resize.resize_u8 -- the cv2.resize of line/dataset.py:73 -- so frames of any size are scored, mixed sizes included
    extremities  None (default): the two keys above, nothing else runs.  A tuple of pixel thresholds, e.g. (5, 10, 20): the
            dev-kit's extremity metric (baseline/evaluate_extremities.py; metrics.ExtremityMetric, one more launch per batch) on the
            decoded peaks with p >= conf_threshold, against each frame's RAW annotation scaled to input_size: the keys
            'val_ext_acc@t', 'val_ext_precision@t', 'val_ext_recall@t', the means over the frames, are added, and the per-class table and
            error lists are left in .extremities.  The folder form reads the annotations itself; in the iterable form every batch
            dict must carry 'annot', the B annotations {class: [{'x', 'y'}, ...]} in normalised coordinates (SncalError otherwise).
            The frames sort_anno drops are not scored here, as they are not in val_acc, and neither is a frame the decoder
            refuses: the dev-kit's scorer run over the folders (extremities.evaluate_extremities) scores every annotation file

    val_loss is the mean of the step losses weighted by step size, as in validate(); val_acc is AccMetric's value (the plain mean
    of the per-batch a@20 * 1.15, so it depends on batch_size, as in the reference).  A frame the decoder refuses (folder form) is
    left out and named in .skipped.  The host waits for the GPU once, at the end."""
    if reduce != 1 and not isinstance(data, (str, os.PathLike)):
        raise _lib.SncalError('reduce applies to the folder form: batches handed in carry their frames already')
    if resize is not None and not isinstance(data, (str, os.PathLike)):
        raise _lib.SncalError('resize applies to the folder form: batches handed in carry their frames already')
    own_loss = model.loss
    if loss is not None:
        model.loss = loss                      # for this call only: restored below
    batches = None
    try:
        model._loss()
        acc = AccMetric(num_keypoints=len(LINE_CLS), conf_threshold=conf_threshold)
        # the prediction transform has applied its scale: the peaks are pixels already
        ext = None if extremities is None else ExtremityMetric(extremities, conf_threshold=conf_threshold, scale=1, img_size=input_size)
        skipped: List[str] = []
        if isinstance(data, (str, os.PathLike)):
            batches = line_folder_batches(os.fspath(data), batch_size, model.device, acc.num_keypoints, input_size, decoder_threads, skipped,
                                          reduce=reduce, annots=ext is not None, resize=resize)
        loss_sum = torch.zeros((), dtype=torch.float64, device=model.device)
        frames = 0
        for batch in (batches if batches is not None else data):
            if ext is not None and 'annot' not in batch:
                raise _lib.SncalError("validate_line(extremities=...): every batch dict must carry 'annot', the frames' raw annotations")
            out = model.val_step(batch)
            acc.num_keypoints = out['prediction'].shape[1]          # the channel count is the network's
            B = out['prediction'].shape[0]
            frames += B
            loss_sum = loss_sum + out['loss'].to(torch.float64) * B
            acc.update(out)
            if ext is not None:
                ext.update({'prediction': out['prediction'], 'annot': batch['annot']})
        model.check_range()
    finally:
        if batches is not None:
            batches.close()
        if loss is not None:
            model.loss = own_loss
    state = _State('val')
    state.metrics['val_loss'] = float(loss_sum.item()) / frames if frames else float('nan')
    acc.epoch_complete(state)
    detail = None
    if ext is not None:
        detail = ext.compute()
        ext.epoch_complete(state, detail)
    res = ValidationResult({k: float(v) for k, v in state.metrics.items()})
    if detail is not None:
        res.extremities = detail
    res.frames, res.skipped = frames + len(skipped), list(skipped)
    return res


def add_resize_argument(ap):
    """--resize W H, shared by the validate, submit and baseline_cameras command lines; parsed_resize() reads it back."""
    ap.add_argument('--resize', type=int, nargs=2, default=None, metavar=('W', 'H'),
                    help="bring every frame to W x H after the decode (cv2.resize's bilinear shrink, on the device): frames of any "
                         'size, mixed sizes included, e.g. --resize 960 540 for a 1280x720 folder; composes with --reduce')


def parsed_resize(a):
    """The resize= keyword of a parsed command line: None, or (W, H)."""
    return None if a.resize is None else check_size(tuple(a.resize), '--resize')


def parser():
    ap = argparse.ArgumentParser(description='Validate a keypoint checkpoint on a SoccerNet split (validate.py counterpart)')
    ap.add_argument('--line', action='store_true', help='the checkpoint is the line model (EHMMetaModel): val_loss and val_acc')
    ap.add_argument('--data', required=True, help='split folder: NNNNN.jpg + NNNNN.json')
    ap.add_argument('--model', required=True, help='argus checkpoint of the keypoint model (model_name/params/nn_state_dict)')
    ap.add_argument('--lines-file', default=None, help='lines pickle of export_line_result.py (optional)')
    ap.add_argument('--batch-size', type=int, default=None, help='default 16, with --line 8')
    ap.add_argument('--reduce', type=int, default=1, choices=[1, 2, 4, 8],
                    help="decode the frames at 1/N of their size (libjpeg's scaled decode = cv2.IMREAD_REDUCED_COLOR_N)")
    add_resize_argument(ap)
    ap.add_argument('--sweep-max-rmse', default=None, metavar='START:STOP:STEP',
                    help="sweep camera.max_rmse over Hydra's range(start, stop, step), stop excluded (optimize_valid.yaml: 10:70:4); one solve per batch")
    ap.add_argument('--sweep-max-rmse-rel', default=None, metavar='START:STOP:STEP', help='the same for camera.max_rmse_rel (optimize_valid.yaml: 4:16:2)')
    ap.add_argument('--extremities', default=None, metavar='T[,T...]',
                    help="with --line: also the dev-kit's extremity metric at these pixel thresholds, e.g. 5,10,20")
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--dtype', default=None, choices=['fp16x3', 'bf16x3', 'fp32', 'bf16', 'fp8'])
    return ap


def main(argv=None):
    from .metamodel import load_model
    from .submit import default_calibrator
    ap = parser()
    a = ap.parse_args(argv)
    resize = parsed_resize(a)
    sweep = None
    if a.sweep_max_rmse is not None or a.sweep_max_rmse_rel is not None:
        if a.line:
            ap.error('--sweep-max-rmse / --sweep-max-rmse-rel are the keypoint model\'s: the line model has no calibrator')
        cal = default_calibrator(None)             # an axis that is not swept keeps the calibrator's value
        sweep = {'max_rmse': parse_range(a.sweep_max_rmse) if a.sweep_max_rmse is not None else [cal.max_rmse],
                 'max_rmse_rel': parse_range(a.sweep_max_rmse_rel) if a.sweep_max_rmse_rel is not None else [cal.max_rmse_rel]}
    ext = None
    if a.extremities is not None:
        if not a.line:
            ap.error("--extremities is the line model's metric: it goes with --line")
        ext = tuple(float(t) for t in a.extremities.split(','))
    if not torch.cuda.is_available():
        raise _lib.SncalError('no GPU visible: this package has no CPU path')
    model = load_model(a.model, device=a.device, dtype=a.dtype)
    if a.line:
        res = validate_line(model, a.data, batch_size=a.batch_size or 8, reduce=a.reduce, extremities=ext, resize=resize)
    else:
        res = validate(model, a.data, default_calibrator(a.lines_file), batch_size=a.batch_size or 16, reduce=a.reduce, sweep=sweep,
                       resize=resize)
    if sweep is not None:
        print(f"{'max_rmse':>10} {'max_rmse_rel':>12} {'completeness':>12} {'accuracy':>10} {'evalai':>10}")
        for r in res:
            print(f"{r.params['max_rmse']:>10g} {r.params['max_rmse_rel']:>12g} {r['val_completeness']:>12.6f} {r['val_eval_accuracy']:>10.6f} "
                  f"{r['val_evalai']:>10.6f}")
        best = res[res.best]
        print(f"best: max_rmse={best.params['max_rmse']:g} max_rmse_rel={best.params['max_rmse_rel']:g} val_evalai={best['val_evalai']:.6f}")
        res = best
    for k, v in res.items():
        print(f'{k}: {v:.6f}')
    if res.skipped:
        print(f'skipped: {len(res.skipped)} of {res.frames} frames')
    return res


if __name__ == '__main__':
    main()
