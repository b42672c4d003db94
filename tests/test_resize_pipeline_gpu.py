"""GPU: resize=(W, H) through the folder entry points.  JPEGs written by Pillow at 96x128, 72x96 and 192x256 (H x W) in one
temporary folder: decoded_batches takes them all, in file order, each row the resize_u8 of that file decoded alone; a fifth source
size is skipped and named; resize=None keeps the single-size rule; reduce composes; validate_line, make_submit and the one-pass
baseline_cameras form score / write every frame of a folder none of whose frames has the network's size.
A stream damaged behind its headers is dropped from its batch (without resize) or its size group (with it) and the rest is decoded
again; a consumer that stops early closes every decoder."""
import io
import json
import os

import numpy as np
import pytest
import torch

import validate_line_ref as vr
from oracle import hrnet_ref as hr
from oracle import jpeg as oj

pytestmark = pytest.mark.gpu

Image = pytest.importorskip('PIL.Image')

SIZES = [(96, 128), (72, 96), (192, 256)]                   # H x W of the files
MORE = [(64, 80), (40, 56)]                                 # a fourth and a fifth size


def _jpeg(h, w, seed):
    """A baseline JPEG (4:2:0, quality 90) of a smooth h x w picture with some texture."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.stack([127 + 100 * np.sin(x / (5.0 + c) + seed) * np.cos(y / (7.0 - c)) + rng.uniform(-20, 20, (h, w)) for c in range(3)], -1)
    b = io.BytesIO()
    Image.fromarray(np.clip(rgb, 0, 255).astype(np.uint8)).save(b, 'JPEG', quality=90, subsampling=2)
    return b.getvalue()


def _folder(path, sizes):
    """One file per entry of `sizes`, named in order -> (names, blobs)."""
    names, blobs = [], []
    for i, (h, w) in enumerate(sizes):
        names.append(f'{i:05d}.jpg')
        blobs.append(_jpeg(h, w, i))
        (path / names[-1]).write_bytes(blobs[-1])
    return names, blobs


def _alone(sncal, cuda, blob, hw, size, reduce=1):
    """One file decoded by a decoder of its own (at 1 / reduce), then resize_u8 -> (H,W,3) on the device."""
    dec = sncal.JpegDecoder(hw[0], hw[1], max_batch=1, device=cuda, reduce=reduce)
    try:
        return sncal.resize.resize_u8(dec.decode([blob]), size)[0]
    finally:
        dec.close()


def test_mixed_sizes_come_out_in_file_order_each_resized_alone(sncal, cuda, tmp_path):
    order = [0, 1, 0, 2, 2, 1, 0]                           # batches of 4: groups interleave in the first, are runs in the second
    sizes = [SIZES[k] for k in order]
    names, blobs = _folder(tmp_path, sizes)
    skipped, seen = [], []
    for keep, image in sncal.frames.decoded_batches(str(tmp_path), names, 4, cuda, 0, skipped, frame_size=(54, 72), resize=(72, 54)):
        assert image.shape == (len(keep), 54, 72, 3) and image.dtype == torch.uint8 and image.is_contiguous()
        for r, j in enumerate(keep):
            assert torch.equal(image[r], _alone(sncal, cuda, blobs[j], sizes[j], (72, 54))), names[j]
        seen += keep
    assert seen == list(range(len(names))) and skipped == []
    # frame_size may be left out: the frames yielded are resize's
    got = [img.shape for _, img in sncal.frames.decoded_batches(str(tmp_path), names, 8, cuda, 0, [], resize=(72, 54))]
    assert got == [(7, 54, 72, 3)]


def test_a_fifth_source_size_is_skipped_and_named(sncal, cuda, tmp_path):
    sizes = [SIZES[0], SIZES[1], SIZES[2], MORE[0], MORE[1], SIZES[1], MORE[1], MORE[0]]
    names, blobs = _folder(tmp_path, sizes)
    skipped, seen = [], []
    with pytest.warns(UserWarning, match='source size number 5'):
        for keep, image in sncal.frames.decoded_batches(str(tmp_path), names, 3, cuda, 0, skipped, resize=(72, 54)):
            for r, j in enumerate(keep):
                assert torch.equal(image[r], _alone(sncal, cuda, blobs[j], sizes[j], (72, 54))), names[j]
            seen += keep
    assert skipped == [names[4], names[6]] and seen == [0, 1, 2, 3, 5, 7]


def test_without_resize_the_first_size_wins_as_before(sncal, cuda, tmp_path):
    sizes = [SIZES[0], SIZES[1], SIZES[0], SIZES[2]]
    names, blobs = _folder(tmp_path, sizes)
    skipped, seen = [], []
    with pytest.warns(UserWarning, match="96x72 where the run's frames are 128x96"):
        for keep, image in sncal.frames.decoded_batches(str(tmp_path), names, 4, cuda, 0, skipped, resize=None):
            assert image.shape == (len(keep), 96, 128, 3)
            seen += keep
    assert seen == [0, 2] and skipped == [names[1], names[3]]
    skipped = []
    with pytest.warns(UserWarning, match='skipped'):
        assert list(sncal.frames.decoded_batches(str(tmp_path), names, 4, cuda, 0, skipped, frame_size=(54, 72))) == []
    assert skipped == names


def test_reduce_then_resize_equals_the_reduced_decode_resized(sncal, cuda, tmp_path):
    sizes = [SIZES[2], SIZES[0], (97, 129)]                 # the last one: libjpeg rounds the halved size up
    names, blobs = _folder(tmp_path, sizes)
    (keep, image), = sncal.frames.decoded_batches(str(tmp_path), names, 4, cuda, 0, [], reduce=2, resize=(72, 54))
    assert keep == [0, 1, 2] and image.shape == (3, 54, 72, 3)
    for j in keep:
        assert sncal.frames.resize_plan(sizes[j][0], sizes[j][1], 2, (72, 54))[1] == (54, 72)
        assert torch.equal(image[j], _alone(sncal, cuda, blobs[j], sizes[j], (72, 54), reduce=2)), names[j]
    # the 192x256 file at 1/2 is 96x128: the same frame as the decoder's own reduced output brought to 72x54
    dec = sncal.JpegDecoder(192, 256, max_batch=1, device=cuda, reduce=2)
    half = dec.decode([blobs[0]])
    dec.close()
    assert half.shape == (1, 96, 128, 3) and torch.equal(image[0], sncal.resize.resize_u8(half, (72, 54))[0])


def _damage(sncal, cuda, path, blob, hw):
    """Overwrite the file with its stream damaged behind the headers, the way tests/test_jpeg_gpu.py damages one: 128 bytes at offset
    200 of the entropy-coded segment become 1024 one-bits, and no Huffman code of the tables is that long.  The headers still probe;
    the oracle and the decoder's host entropy stage (before any launch) refuse the stream."""
    sos = blob.find(b'\xff\xda')
    assert sos > 0 and blob.count(b'\xff\xda') == 1
    start = sos + 2 + ((blob[sos + 2] << 8) | blob[sos + 3])             # first byte of the entropy-coded segment
    assert len(blob) - start > 328
    cut = blob[:start + 200] + b'\xff\x00' * 64 + blob[start + 328:]
    fi = sncal.jpeg.probe(cut)
    assert (fi['height'], fi['width']) == hw
    with pytest.raises(oj.JpegError, match='bad Huffman code'):
        oj.decode_bgr(cut)
    dec = sncal.JpegDecoder(hw[0], hw[1], max_batch=1, device=cuda)
    try:
        with pytest.raises(sncal._lib.SncalError):
            dec.decode([cut])
    finally:
        dec.close()
    path.write_bytes(cut)


def _skip_warnings(record):
    return [str(w.message) for w in record if 'skipped' in str(w.message)]


def test_a_stream_damaged_behind_its_headers_is_dropped_from_its_batch_without_resize(sncal, cuda, tmp_path):
    """The batch decode fails, every file of the batch is decoded alone, the bad one is skipped and named, the rest decoded again as one
    batch: the rule make_submit is pinned to (tests/test_jpeg_gpu.py), here in decoded_batches."""
    sizes = [SIZES[0]] * 5
    names, blobs = _folder(tmp_path, sizes)
    _damage(sncal, cuda, tmp_path / names[2], blobs[2], sizes[2])
    skipped, keeps = [], []
    with pytest.warns(UserWarning) as record:
        for keep, image in sncal.frames.decoded_batches(str(tmp_path), names, 4, cuda, 0, skipped):
            assert image.shape == (len(keep), 96, 128, 3) and image.dtype == torch.uint8 and image.is_contiguous()
            dec = sncal.JpegDecoder(96, 128, max_batch=1, device=cuda)
            for r, j in enumerate(keep):
                assert torch.equal(image[r], dec.decode([blobs[j]])[0]), names[j]
            dec.close()
            keeps.append(keep)
    assert keeps == [[0, 1, 3], [4]] and skipped == [names[2]]
    said = _skip_warnings(record)
    assert len(said) == 1 and said[0].startswith(f'{names[2]}: skipped (')


def test_a_stream_damaged_behind_its_headers_is_dropped_from_its_size_group_with_resize(sncal, cuda, tmp_path):
    sizes = [SIZES[k] for k in (0, 1, 0, 1, 2)]
    names, blobs = _folder(tmp_path, sizes)
    _damage(sncal, cuda, tmp_path / names[3], blobs[3], sizes[3])       # the second 72x96 file
    skipped, keeps = [], []
    with pytest.warns(UserWarning) as record:
        for keep, image in sncal.frames.decoded_batches(str(tmp_path), names, 4, cuda, 0, skipped, resize=(72, 54)):
            assert image.shape == (len(keep), 54, 72, 3) and image.is_contiguous()
            for r, j in enumerate(keep):
                assert torch.equal(image[r], _alone(sncal, cuda, blobs[j], sizes[j], (72, 54))), names[j]
            keeps.append(keep)
    assert keeps == [[0, 1, 2], [4]] and skipped == [names[3]]
    said = _skip_warnings(record)
    assert len(said) == 1 and said[0].startswith(f'{names[3]}: skipped (')


def test_a_size_group_or_a_batch_left_empty_by_damaged_streams(sncal, cuda, tmp_path):
    """A group whose only file is damaged yields nothing and the batch's other groups their rows; a batch with nothing left is not yielded."""
    sizes = [SIZES[k] for k in (0, 1, 0, 1)]
    names, blobs = _folder(tmp_path, sizes)
    for j in (1, 3):
        _damage(sncal, cuda, tmp_path / names[j], blobs[j], sizes[j])
    skipped = []
    with pytest.warns(UserWarning, match='skipped'):
        got = list(sncal.frames.decoded_batches(str(tmp_path), names, 3, cuda, 0, skipped, resize=(72, 54)))
    assert [keep for keep, _ in got] == [[0, 2]] and skipped == [names[1], names[3]]
    for r, j in enumerate(got[0][0]):
        assert torch.equal(got[0][1][r], _alone(sncal, cuda, blobs[j], sizes[j], (72, 54))), names[j]
    # without resize: files 0 and 2 are the run's size, 1 and 3 are refused for theirs; then 2 is damaged too and its batch is empty
    _damage(sncal, cuda, tmp_path / names[2], blobs[2], sizes[2])
    skipped = []
    with pytest.warns(UserWarning, match='skipped'):
        got = list(sncal.frames.decoded_batches(str(tmp_path), names, 2, cuda, 0, skipped))
    assert [keep for keep, _ in got] == [[0]] and skipped == [names[1], names[3], names[2]]     # 3 at its probe, 2 at its decode


def test_a_consumer_that_stops_early_closes_every_decoder(sncal, cuda, tmp_path, monkeypatch):
    sizes = [SIZES[k] for k in (0, 1, 0, 1)]
    names, _ = _folder(tmp_path, sizes)
    closed = []                 # (source size, handle afterwards) per close() that found a handle: __del__ calls close() again.  No decoder
    close = sncal.JpegDecoder.close    # is kept here: one whose last reference the patched function held would be finalised while the patch is undone

    def counted(self):
        held = bool(self._h)
        close(self)
        if held:
            closed.append(((self.height, self.width), self._h))
    monkeypatch.setattr(sncal.JpegDecoder, 'close', counted)
    frames = sncal.frames.decoded_batches(str(tmp_path), names, 2, cuda, 0, [], resize=(72, 54))
    keep, image = next(frames)
    assert keep == [0, 1] and image.shape == (2, 54, 72, 3) and closed == []
    frames.close()
    assert sorted(closed) == sorted((size, None) for size in SIZES[:2])


def _line_model(sncal, gold_dir, tmp):
    g = np.load(os.path.join(gold_dir, 'line_w18_64x96.npz'))
    cfg = hr.load_config('line_hrnet_w18')
    bare = {k: v for k, v in cfg.items() if k not in ('head', 'upscale')}
    ck = {'model_name': 'EHMMetaModel',
          'params': {'nn_module': {'hrnet_config': bare, 'num_refinement_stages': 0, 'num_heatmaps': 23},
                     'loss': {'num_refinement_stages': 0, 'gmse_w': 1.0, 'awing_w': 1.0, 'sigma': 4},
                     'prediction_transform': {'scale': 4, 'sigma': 6}, 'device': 'cuda:0'},
          'nn_state_dict': hr.seeded_state_dict(cfg, int(g['seed']), float(g['head_gain']))}
    path = str(tmp / 'line.pth')
    torch.save(ck, path)
    return sncal.load_model(path, loss=None, optimizer=None, device='cuda:0', dtype='fp32')


def test_validate_line_scores_every_frame_of_a_folder_of_other_sizes(sncal, cuda, gold_dir, tmp_path):
    """input_size 96x64 (the W18 line golden's), files at 128x96, 96x72 and 256x192: without resize every frame is skipped, with it
    every frame is scored, and the result equals the steps composed by hand on line_folder_batches' frames."""
    model = _line_model(sncal, gold_dir, tmp_path)
    folder = tmp_path / 'split'
    folder.mkdir()
    usable = [c for c in vr.label_cases(np.load(os.path.join(gold_dir, 'validate_line.npz'))) if c['usable']][:5]
    sizes = [SIZES[k] for k in (0, 1, 2, 1, 0)]
    names, blobs = _folder(folder, sizes)
    for n, case in zip(names, usable):
        with open(folder / n.replace('.jpg', '.json'), 'w') as f:
            json.dump({cls: [{'x': x, 'y': y} for x, y in pts] for cls, pts in case['points'].items()}, f)
    listed, _ = sncal.frames.list_line_split(str(folder), (96, 64))
    assert listed == names
    with pytest.warns(UserWarning, match='skipped'):
        before = sncal.validate.validate_line(model, str(folder), batch_size=2, input_size=(96, 64))
    assert before.skipped == names and before.frames == 5 and np.isnan(before['val_loss'])
    res = sncal.validate.validate_line(model, str(folder), batch_size=2, input_size=(96, 64), resize=(96, 64))
    assert res.skipped == [] and res.frames == 5 and np.isfinite(res['val_loss']) and 0.0 <= res['val_acc'] <= 1.15
    acc = sncal.AccMetric(num_keypoints=23, conf_threshold=0.2)
    total, frames = 0.0, 0
    for b in sncal.frames.line_folder_batches(str(folder), 2, cuda, 23, (96, 64), 0, [], resize=(96, 64)):
        assert b['image'].shape[1:] == (64, 96, 3)
        for r, n in enumerate(b['img_name']):
            j = names.index(n)
            assert torch.equal(b['image'][r], _alone(sncal, cuda, blobs[j], sizes[j], (96, 64)))
        out = model.val_step(b)
        acc.update(out)
        total += float(out['loss'].double()) * len(b['img_name'])
        frames += len(b['img_name'])
    assert frames == 5 and res['val_acc'] == acc.compute() and abs(res['val_loss'] - total / frames) <= 1e-12 * abs(res['val_loss'])
    # a resize that is not the network's input size is refused; batches handed in carry their frames already
    with pytest.raises(sncal._lib.SncalError, match='frame_size'):
        sncal.validate.validate_line(model, str(folder), batch_size=2, input_size=(96, 64), resize=(72, 54))
    with pytest.raises(sncal._lib.SncalError, match='folder form'):
        sncal.validate.validate_line(model, [], resize=(96, 64))
    # the one-pass cameras form sees the same frames: every file reaches the network at 96x64
    collect = []
    sncal.baseline_cameras.line_model_cameras(str(folder), model, str(tmp_path / 'cams'), batch_size=8, resize=(96, 64), collect=collect)
    assert [c[0] for c in collect] == [names] and collect[0][1].shape[0] == 5


def test_make_submit_resizes_between_the_decoder_and_the_network(sncal, cuda, tmp_path, monkeypatch):
    cfg = hr.load_config('hrnet_w18')
    ck = {'model_name': 'HRNetMetaModel',
          'params': {'nn_module': {'hrnet_config': cfg, 'num_refinement_stages': 0, 'num_heatmaps': 58},
                     'prediction_transform': {'size': [64, 96]}, 'device': 'cuda:0'},
          'nn_state_dict': hr.seeded_state_dict(cfg, 3, 4.0)}
    path = str(tmp_path / 'model.pth')
    torch.save(ck, path)
    model = sncal.load_model(path, loss=None, optimizer=None, device='cuda:0', dtype='fp32')
    img_dir = tmp_path / 'imgs'
    img_dir.mkdir()
    sizes = [SIZES[0], SIZES[0], SIZES[1], SIZES[0], SIZES[0]]          # the vote is 128x96: the 96x72 file is skipped, as without resize
    names, blobs = _folder(img_dir, sizes)
    fed = []
    submit = sncal.pipeline.CalibrationPipeline.submit

    def spy(self, x, *a, **kw):
        fed.append((list(kw.get('names', [])), x.clone()))
        return submit(self, x, *a, **kw)
    monkeypatch.setattr(sncal.pipeline.CalibrationPipeline, 'submit', spy)
    with pytest.warns(UserWarning, match='skipped'):
        res = sncal.submit.make_submit(str(img_dir), model, sncal.submit.default_calibrator(), str(tmp_path / 'out'), batch_size=2,
                                       img_names=names, resize=(96, 64))
    assert res['frames'] == 5 and res['skipped'] == [names[2]]
    assert [n for ns, _ in fed for n in ns] == [names[0], names[1], names[3], names[4]]
    for ns, x in fed:
        assert x.shape == (len(ns), 64, 96, 3)
        for r, n in enumerate(ns):
            j = names.index(n)
            assert torch.equal(x[r], _alone(sncal, cuda, blobs[j], sizes[j], (96, 64))), n
    with pytest.raises(sncal._lib.SncalError):
        sncal.submit.make_submit(str(img_dir), model, sncal.submit.default_calibrator(), str(tmp_path / 'out2'), resize=(96,))
