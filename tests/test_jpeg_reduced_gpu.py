"""GPU: libjpeg's scaled decode on the device (JpegDecoder(reduce=2 / 4 / 8) = cv2.imread's IMREAD_REDUCED_COLOR_2 / _4 / _8) against
libjpeg-turbo's own frames (tests/golden/jpeg_reduced.npz) and the numpy restatement (tests/jpeg_reduced_ref.py).  Integer
arithmetic end to end: equality is the criterion everywhere."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import hrnet_ref as hr

import jpeg_reduced_ref as rr

pytestmark = pytest.mark.gpu


def _full_cases(gold_dir):
    g = np.load(os.path.join(gold_dir, 'jpeg_cases.npz'))
    return g, [str(n) for n in g['names']]


@pytest.fixture(scope='module')
def hd(gold_dir):
    """The 1080p stream and the restatement's frames for it, computed once."""
    g, _, _ = rr.cases(gold_dir)
    data = g['jpg.hd'].tobytes()
    return g, data, {d: rr.decode_bgr(data, d) for d in (2, 4, 8)}


def test_reduced_frames_equal_libjpeg_turbo_bit_exact(sncal, cuda, gold_dir):
    """Every golden stream x denominator.  The streams of one source size share a batch, so one launch mixes 4:4:4 / 4:2:2 / 4:2:0 /
    grey (block sizes 8, 4, 2, 1 side by side) and restart intervals; three calls use both staging slots; the last call fills a
    tensor of the caller's."""
    g, names, denoms = rr.cases(gold_dir)
    by_size = {}
    for n in names:
        by_size.setdefault(n.split('_')[0], []).append(n)
    checked = 0
    for size, group in by_size.items():
        h, w = (int(v) for v in size.split('x'))
        blobs = [g['jpg.' + n].tobytes() for n in group]
        for d in denoms[group[0]]:
            dec = sncal.JpegDecoder(h, w, max_batch=len(group), threads=4, device=cuda, reduce=d)
            assert (dec.reduce, dec.out_height, dec.out_width) == (d, -(-h // d), -(-w // d))
            first = dec.decode(blobs)
            dec.decode(blobs[::-1])
            mine = torch.full((len(group), dec.out_height, dec.out_width, 3), 7, dtype=torch.uint8, device=cuda)
            assert dec.decode(blobs, out=mine) is mine
            for out in (first.cpu().numpy(), mine.cpu().numpy()):
                for i, n in enumerate(group):
                    assert np.array_equal(out[i], g[f'bgr.{n}.d{d}']), (n, d)
                    checked += 1
            dec.close()
    assert checked == 2 * 184


def test_scale_one_is_todays_decoder(sncal, cuda, gold_dir):
    """reduce=1 and sncal_jpeg_create_scaled(..., 1, ...) give the bytes sncal_jpeg_create's decoder gives."""
    L = sncal._lib
    g, names = _full_cases(gold_dir)
    for size in ('29x37', '100x130', '1x1'):
        group = [n for n in names if n.split('_')[0] == size]
        h, w = (int(v) for v in size.split('x'))
        blobs = [g['jpg.' + n].tobytes() for n in group]
        B = len(blobs)
        dec = sncal.JpegDecoder(h, w, max_batch=B, threads=2, device=cuda, reduce=1)
        assert (dec.out_height, dec.out_width) == (h, w)
        got = dec.decode(blobs).cpu().numpy()
        dec.close()
        ptrs = (ctypes.c_char_p * B)(*blobs)
        lens = (ctypes.c_size_t * B)(*[len(b) for b in blobs])
        raw = []
        for create in (lambda out: L.lib().sncal_jpeg_create(B, h, w, 2, out), lambda out: L.lib().sncal_jpeg_create_scaled(B, h, w, 1, 2, out)):
            hnd = ctypes.c_void_p()
            L.check(create(ctypes.byref(hnd)), 'create')
            oh, ow = ctypes.c_int(), ctypes.c_int()
            L.check(L.lib().sncal_jpeg_output_size(hnd, ctypes.byref(oh), ctypes.byref(ow)), 'sncal_jpeg_output_size')
            assert (oh.value, ow.value) == (h, w)
            t = torch.zeros((B, h, w, 3), dtype=torch.uint8, device=cuda)
            L.check(L.lib().sncal_jpeg_decode(hnd, ptrs, lens, B, t.data_ptr(), L.current_stream_ptr()), 'sncal_jpeg_decode')
            raw.append(t.cpu().numpy())
            L.lib().sncal_jpeg_destroy(hnd)
        assert np.array_equal(raw[0], raw[1]) and np.array_equal(got, raw[0])
        for i, n in enumerate(group):
            assert np.array_equal(got[i], g['bgr.' + n]), n


def test_1080p_reduced_matches_row_sums_and_the_restatement(sncal, cuda, hd):
    g, data, want = hd
    for d in (2, 4, 8):
        dec = sncal.JpegDecoder(1080, 1920, max_batch=2, threads=2, device=cuda, reduce=d)
        got = dec.decode([data, data]).cpu().numpy()
        dec.close()
        assert got.shape == (2, 1080 // d, 1920 // d, 3)
        assert np.array_equal(got[0].astype(np.int64).sum(axis=(1, 2)), g[f'bgr.hd.d{d}.rowsum']), d
        assert np.array_equal(got[0], want[d]) and np.array_equal(got[1], want[d]), d


def test_1080p_at_half_size_feeds_the_540p_network(sncal, cuda, hd):
    """1920x1080 -> reduce=2 -> sncal_hrnet_forward_u8: the keypoints of the same pixels passed through ToTensor on the host."""
    _, data, want = hd
    dec = sncal.JpegDecoder(1080, 1920, max_batch=1, threads=1, device=cuda, reduce=2)
    out = dec.decode([data])
    assert np.array_equal(out[0].cpu().numpy(), want[2])
    net = sncal.HRNetHeatmap('hrnet_w18', dtype='fp32', device=cuda)
    net.load_state_dict(hr.seeded_state_dict(hr.load_config('hrnet_w18'), 3, 4.0))
    _, k_u8 = net.forward(out, want_heat=False, decode_size=(540, 960))
    x = torch.from_numpy(np.ascontiguousarray(want[2][None])).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)   # ToTensor, on the host
    _, k_f = net.forward(x.to(cuda), want_heat=False, decode_size=(540, 960))
    assert torch.equal(k_u8, k_f)
    dec.close()


def test_refusals_name_the_frame_and_leave_the_decoder_usable(sncal, cuda, gold_dir):
    g, names, _ = rr.cases(gold_dir)
    full, _ = _full_cases(gold_dir)
    n64 = [n for n in names if n.startswith('64x96_420_') and n.endswith('_r0')][0]
    n33 = [n for n in names if n.startswith('33x47_420_') and n.endswith('_r0')][0]
    good, other = g['jpg.' + n64].tobytes(), g['jpg.' + n33].tobytes()
    with pytest.raises(sncal._lib.SncalError, match='reduce'):
        sncal.JpegDecoder(64, 96, device=cuda, reduce=3)
    dec = sncal.JpegDecoder(64, 96, max_batch=4, device=cuda, reduce=2)
    with pytest.raises(sncal._lib.SncalError, match='frame 1.*47x33'):          # the SOURCE size is what is compared
        dec.decode([good, other])
    with pytest.raises(sncal._lib.SncalError, match='frame 2.*SOF2'):
        dec.decode([good, good, full['jpg.progressive'].tobytes()])
    with pytest.raises(sncal._lib.SncalError, match=r'out must be \(1,32,48,3\)'):
        dec.decode([good], out=torch.empty((1, 64, 96, 3), dtype=torch.uint8, device=cuda))
    assert dec.decode([]).shape == (0, 32, 48, 3)
    assert np.array_equal(dec.decode([good])[0].cpu().numpy(), g[f'bgr.{n64}.d2'])
    dec.close()


def test_folder_batches_decode_at_the_reduced_size(sncal, cuda, gold_dir, tmp_path):
    """decoded_batches(..., reduce=2): the reduced frames of the files of the run's size, the odd file named in `skipped`."""
    g, names, _ = rr.cases(gold_dir)
    group = [n for n in names if n.startswith('37x100_')]
    odd = [n for n in names if n.startswith('20x40_')][0]
    files = []
    for k, n in enumerate(group[:3] + [odd] + group[3:]):
        files.append(f'{k:05d}.jpg')
        (tmp_path / files[-1]).write_bytes(g['jpg.' + n].tobytes())
    order = group[:3] + [None] + group[3:]
    skipped = []
    with pytest.warns(UserWarning, match='00003.jpg: skipped'):
        got = list(sncal.frames.decoded_batches(str(tmp_path), files, 4, cuda, 2, skipped, reduce=2))
    assert skipped == ['00003.jpg']
    assert [keep for keep, _ in got] == [[0, 1, 2], [4, 5, 6, 7], [8]]
    for keep, image in got:
        assert image.shape == (len(keep), 19, 50, 3)
        for j, frame in zip(keep, image.cpu().numpy()):
            assert np.array_equal(frame, g[f'bgr.{order[j]}.d2']), order[j]
    # frame_size is the size of the frames yielded: the same folder at another size takes nothing
    skipped = []
    with pytest.warns(UserWarning, match='skipped'):
        assert list(sncal.frames.decoded_batches(str(tmp_path), files[:2], 4, cuda, 2, skipped, frame_size=(37, 100), reduce=2)) == []
    assert skipped == files[:2]


def test_make_submit_reduce_runs_the_half_size_loop(sncal, cuda, gold_dir, tmp_path):
    """make_submit(..., reduce=2): five 960x540 files through a 480x270 network write exactly the camera files model.predict and
    solve_batch give for the restatement's 480x270 frames (the loop whose imread carries cv2.IMREAD_REDUCED_COLOR_2)."""
    g, _ = _full_cases(gold_dir)
    full = g['jpg.full'].tobytes()
    img_dir, save_dir = tmp_path / 'imgs', tmp_path / 'out'
    img_dir.mkdir()
    names = [f'{i:05d}.jpg' for i in range(5)]
    for n in names:
        (img_dir / n).write_bytes(full)
    cfg = hr.load_config('hrnet_w18')
    ck = {'model_name': 'HRNetMetaModel',
          'params': {'nn_module': {'hrnet_config': cfg, 'num_refinement_stages': 0, 'num_heatmaps': 58},
                     'prediction_transform': {'size': [270, 480]}, 'device': 'cuda:0'},
          'nn_state_dict': hr.seeded_state_dict(cfg, 3, 4.0)}
    path = str(tmp_path / 'model.pth')
    torch.save(ck, path)
    model = sncal.load_model(path, loss=None, optimizer=None, device='cuda:0', dtype='fp32')
    cal = sncal.submit.default_calibrator()
    with pytest.raises(sncal._lib.SncalError, match='reduce'):
        sncal.submit.make_submit(str(img_dir), model, cal, str(save_dir), reduce=3)
    res = sncal.submit.make_submit(str(img_dir), model, cal, str(save_dir), batch_size=2, decoder_threads=2, reduce=2)
    assert res['frames'] == 5 and res['skipped'] == [] and 0.0 <= res['completeness'] <= 1.0
    half = rr.decode_bgr(full, 2)
    assert half.shape == (270, 480, 3)
    x = torch.from_numpy(np.ascontiguousarray(half)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    pred = model.predict(torch.stack([x] * 5))
    cams = cal.solve_batch(pred.cpu().numpy(), names)
    want = sorted('camera_' + n.replace('.jpg', '.json') for n, c in zip(names, cams) if c is not None)
    assert sorted(os.listdir(save_dir)) == want and res['written'] == len(want)
