"""CameraCreator -- host mirror of /root/reference/src/models/hrnet/prediction.py:44-437.

Same constructor (pitch, img_size, conf_thresh, algorithm, lines_file, **kwargs -> attributes), same
``__call__(pred (57,3) float32, name) -> Optional[Camera]`` that never raises, same five algorithm names,
picklable (it holds only python data, so it can be shipped to worker processes exactly like the reference's
at make_submit.py:53-54,69).  The solve itself -- every heuristic of the reference's voters -- runs on the
GPU: one wavefront per frame in sncal_calibrate (kernels and entry points: csrc/solve.hip; the control flow
of this file: csrc/solve_flow.hpp).  ``solve_batch`` is the batched entry the frame pipeline uses; ``__call__`` is the one-frame form of it.
"""
import ctypes
import os
import pickle
from typing import Dict, Optional, Tuple

import numpy as np

from . import _lib
from .camera import Camera
from .lines import lines_to_keypoints, keypoints_to_array, line_eq_intersection  # noqa: F401
from .pitch import PITCH_POINTS, INTERSECTON_TO_PITCH_POINTS, IMG_SIZE, top_gates, point_sets, keep_points  # noqa: F401

ALGORITHMS = {'iterative_voter': 0, 'original_voter': 1, 'voter': 2, 'opencv_calibration': 3,
              'opencv_calibration_multiplane': 4}
STATUS_NAMES = {0: None, 1: 'original_voter', 2: 'original_voter_hom', 3: 'camera_rel', 4: 'camera_acc',
                5: 'cam_all', 6: 'cam_ground', 7: 'voter_hom'}


def swap_z_y(point_3d):
    point_3d = point_3d.copy()
    point_3d[0] = point_3d[1]
    point_3d[1] = point_3d[2]
    point_3d[2] = 0.0
    return point_3d


def good_camera(mtx, pos):
    return bool(10 <= mtx[0, 0] <= 20000 and -250 < pos[0] < 250 and -250 < pos[1] < 250 and -100 < pos[2] < 0)


def is_good_camera(cam: Camera):
    return good_camera(cam.calibration, cam.position)


def camera_from_record(rec, img_size=IMG_SIZE) -> Optional[Camera]:
    """sncal_camera (ctypes) -> Camera with the attribute values the reference leaves behind."""
    if rec.status == 0:
        return None
    cam = Camera(*img_size)
    cam.position = np.array(rec.position[:], dtype=np.float64)
    cam.rotation = np.array(rec.rotation[:], dtype=np.float64).reshape(3, 3)
    cam.calibration = np.array([[rec.fx, 0.0, rec.cx], [0.0, rec.fy, rec.cy], [0.0, 0.0, 1.0]])
    cam.xfocal_length = np.float64(rec.fx)
    cam.yfocal_length = np.float64(rec.fy)
    cam.principal_point = (img_size[0] / 2.0, img_size[1] / 2.0)
    cam.rmse = float(rec.rmse)
    cam.source = STATUS_NAMES.get(rec.status, str(rec.status))
    cam.n_points = int(rec.n_points)          # size of the matched-point set rmse is the mean over (sncal_camera.n_points)
    return cam


SWEEP_MAX_GRID = 4096          # sncal_calibrate_sweep's bound on n_grid


def sweep_grid(max_rmse, max_rmse_rel) -> np.ndarray:
    """(n_grid,2) float64 rows [max_rmse, max_rmse_rel]: the cartesian product of the two value lists, max_rmse outermost."""
    a = np.asarray(list(max_rmse), dtype=np.float64).reshape(-1)
    r = np.asarray(list(max_rmse_rel), dtype=np.float64).reshape(-1)
    if not (1 <= len(a) * len(r) <= SWEEP_MAX_GRID):
        raise _lib.SncalError(f'a sweep holds 1..{SWEEP_MAX_GRID} grid points, not {len(a)} x {len(r)}')
    return np.ascontiguousarray(np.stack([np.repeat(a, len(r)), np.tile(r, len(a))], axis=1))


def parse_range(text: str):
    """'start:stop:step' -> the values of Hydra's range(start, stop, step): stop excluded; ints stay ints.  'start:stop' steps by 1."""
    parts = text.split(':')
    if len(parts) not in (2, 3) or not all(p.strip() for p in parts):
        raise ValueError(f'{text!r}: start:stop[:step]')
    nums = [float(p) if any(c in p for c in '.eEn') else int(p) for p in parts]
    start, stop, step = nums[0], nums[1], nums[2] if len(nums) == 3 else 1
    if step == 0 or not all(np.isfinite(v) for v in (start, stop, step)):
        raise ValueError(f'{text!r}: the step is zero or a bound is not finite')
    n = max(0, int(np.ceil((stop - start) / step)))
    return [start + i * step for i in range(n)]


class CameraCreator:
    def __init__(self, pitch: Dict[str, np.ndarray] = None, img_size: Tuple[int, int] = (960, 540),
                 conf_thresh: float = 0.2, algorithm: str = 'opencv_calibration', lines_file=None, **kwargs):
        assert algorithm in ALGORITHMS, f'Should be one of: {list(ALGORITHMS.keys())}'
        self.algorithm_name = algorithm
        self.conf_thresh = conf_thresh
        self.pitch = pitch if pitch is not None else PITCH_POINTS
        # A pitch dict that differs from the template is REFUSED, on purpose.  The reference reads `self.pitch` in some places
        # (prediction.py:149, 200, 240, 381: the calibration views of opencv_calibration(_multiplane) and original_voter) and the
        # module-level PITCH_POINTS in others (:465 get_matched_points -> every refine_camera / projection_rmse, :505, :534, :582: the
        # homography camera and all of voter's subset cameras), so with another pitch its voters calibrate against one template and
        # refine / score against another.  make_submit.py:45 passes PITCH_POINTS itself; reproducing that inconsistency would serve nobody.
        for i, name in INTERSECTON_TO_PITCH_POINTS.items():
            if name in self.pitch and not np.allclose(self.pitch[name], PITCH_POINTS[name], atol=1e-9):
                raise ValueError(f'pitch point {name} differs from the built-in 105x68 m template (the reference itself mixes '
                                 'self.pitch with its module-level PITCH_POINTS: see the comment above)')
        self.img_size = tuple(img_size)
        self.lines_data = self._line_keypoints(lines_file) if lines_file is not None else {}
        # defaults of the kwargs make_submit.py:45-50 passes
        self.conf_threshs = [0.5, 0.35, 0.2]
        self.max_rmse, self.max_rmse_rel = 55.0, 5.0
        self.min_points, self.min_focal_length = 5, 10.0
        self.min_points_per_plane, self.min_points_for_refinement, self.reliable_thresh = 6, 6, 57
        # build-side switch (no reference counterpart): 'opencv' = the minimisers follow OpenCV's own LM schedules (default),
        # 'converged' = every minimiser runs to convergence (sncal_voter_cfg.lm_schedule)
        self.lm_schedule = 'opencv'
        self.refine_max_iters = 20000        # the reference's own criterion (camera.py:116); see sncal_voter_cfg.refine_max_iters
        for key, value in kwargs.items():
            setattr(self, key, value)
        self.stat = {'n': 0, 'frames_4': 0, 'frames_4_6': 0, 'frames_bad_cam': 0}

    @staticmethod
    def _line_keypoints(lines_file) -> Dict[str, Dict[int, Tuple[float, float]]]:
        """The line model's pickle (export_line_result.py:188-201) -> per image the keypoints its line pairs intersect in; images
        without any are left out (prediction.py:105-124)."""
        assert os.path.exists(lines_file), f'{lines_file} does not exist'
        with open(lines_file, 'rb') as f:
            per_image = pickle.load(f)
        joined = ((name, lines_to_keypoints(rec['lines'][0])) for name, rec in per_image.items())
        return {name: pts for name, pts in joined if pts}

    # ---- C ABI plumbing -------------------------------------------------------------------------------
    def _cfg(self):
        c = _lib.VoterCfg()
        c.algorithm = ALGORITHMS[self.algorithm_name]
        c.conf_thresh = float(self.conf_thresh)
        ths = list(self.conf_threshs)
        if len(ths) > _lib.MAX_CONF_THRESHS:       # the reference loops over any number (prediction.py:245-257); make_submit.py passes 3
            raise _lib.SncalError(f'conf_threshs holds {len(ths)} thresholds; sncal_voter_cfg carries at most {_lib.MAX_CONF_THRESHS}')
        c.n_conf_threshs = len(ths)
        for i, t in enumerate(ths):
            c.conf_threshs[i] = float(t)
        c.max_rmse, c.max_rmse_rel = float(self.max_rmse), float(self.max_rmse_rel)
        c.min_points, c.min_points_per_plane = int(self.min_points), int(self.min_points_per_plane)
        c.min_points_for_refinement, c.reliable_thresh = int(self.min_points_for_refinement), int(self.reliable_thresh)
        c.min_focal_length = float(self.min_focal_length)
        c.img_w, c.img_h = int(self.img_size[0]), int(self.img_size[1])
        if self.lm_schedule not in ('opencv', 'converged'):
            raise _lib.SncalError(f"lm_schedule must be 'opencv' or 'converged', not {self.lm_schedule!r}")
        c.lm_schedule = 0 if self.lm_schedule == 'opencv' else 1
        c.refine_max_iters = int(self.refine_max_iters)
        return c

    def line_points_array(self, names):
        """(B,30,3) float32 [x, y, valid] from the ingested lines file, or None if no frame has any."""
        if not self.lines_data or names is None:
            return None
        arr = np.zeros((len(names), 30, 3), dtype=np.float32)
        hit = False
        for b, n in enumerate(names):
            if n is not None and n in self.lines_data:
                arr[b] = keypoints_to_array(self.lines_data[n])
                hit = True
        return arr if hit else None

    def solve_device(self, d_kpts, d_line_pts=None, out=None):
        """Batched solve on device tensors: d_kpts (B,57,3) float32 cuda -> uint8 cuda tensor of B sncal_camera
        records (asynchronous on the current stream).  The solve's scratch is a workspace tensor of this call
        (sncal_calibrate_workspace / sncal_calibrate_ws: the library allocates nothing), taken from torch's caching allocator on the
        current stream -- stream-ordered reuse, no hipMalloc in steady state, no host wait for another stream's solves."""
        import torch
        _lib.require_device(d_kpts, torch.float32, 'kpts')
        B = d_kpts.shape[0]
        if tuple(d_kpts.shape[1:]) != (57, 3):
            raise _lib.SncalError('kpts must be (B,57,3)')
        if d_line_pts is not None:
            _lib.require_device(d_line_pts, torch.float32, 'line_pts')
        if out is None:
            out = torch.empty((B, ctypes.sizeof(_lib.Camera)), dtype=torch.uint8, device=d_kpts.device)
        cfg = self._cfg()
        ws = _lib.workspace('sncal_calibrate_workspace', B, ctypes.byref(cfg), device=d_kpts.device)
        _lib.launch('sncal_calibrate_ws', d_kpts.device, d_kpts, d_line_pts, B, ctypes.byref(cfg), out, ws, ws.numel())
        return out

    def sweep_slots(self) -> int:
        """S of sweep_device: the first pass's camera and five per voter threshold."""
        if self.algorithm_name not in ('iterative_voter', 'voter'):
            raise _lib.SncalError(f'{self.algorithm_name} never reads max_rmse / max_rmse_rel: there is nothing to sweep '
                                  "(algorithm 'iterative_voter' or 'voter')")
        return 1 + 5 * (len(self.conf_threshs) if self.algorithm_name == 'iterative_voter' else 1)

    def sweep_device(self, d_kpts, d_line_pts, max_rmse, max_rmse_rel):
        """ONE batched solve for every (max_rmse, max_rmse_rel) of the cartesian product, max_rmse outermost (sweep_grid): the two
        parameters only choose among the cameras a solve produces (sncal_calibrate_sweep).  -> (outcomes (B,S,sizeof(sncal_camera))
        uint8, choice (n_grid,B) int32), both on the device: outcomes[b, choice[g, b]] is the record solve_device returns for frame b
        with grid point g's values (choice -1: no camera, the all-zero record).  This creator's own max_rmse / max_rmse_rel are not
        read.  Asynchronous on the current stream."""
        import torch
        _lib.require_device(d_kpts, torch.float32, 'kpts')
        B = d_kpts.shape[0]
        if tuple(d_kpts.shape[1:]) != (57, 3):
            raise _lib.SncalError('kpts must be (B,57,3)')
        if d_line_pts is not None:
            _lib.require_device(d_line_pts, torch.float32, 'line_pts')
        S = self.sweep_slots()
        grid = sweep_grid(max_rmse, max_rmse_rel)
        cfg = self._cfg()
        ws = _lib.workspace('sncal_calibrate_sweep_workspace', B, ctypes.byref(cfg), len(grid), device=d_kpts.device)
        d_grid = torch.from_numpy(grid).to(d_kpts.device)
        outcomes = torch.empty((B, S, ctypes.sizeof(_lib.Camera)), dtype=torch.uint8, device=d_kpts.device)
        choice = torch.empty((len(grid), B), dtype=torch.int32, device=d_kpts.device)
        _lib.launch('sncal_calibrate_sweep', d_kpts.device, d_kpts, d_line_pts, B, ctypes.byref(cfg), d_grid, len(grid), outcomes, choice,
                    ws, ws.numel())
        return outcomes, choice

    @staticmethod
    def records(out_tensor):
        """uint8 device tensor from solve_device -> ctypes array of sncal_camera (synchronises)."""
        host = out_tensor.cpu().numpy().tobytes()
        n = len(host) // ctypes.sizeof(_lib.Camera)
        return (_lib.Camera * n).from_buffer_copy(host)

    def solve_batch(self, preds, names=None):
        """preds (B,57,3) float32 (numpy or torch, any device) -> list of Optional[Camera]."""
        import torch
        if not torch.cuda.is_available():
            raise _lib.SncalError('CameraCreator needs a GPU (libsncal.so has no CPU path)')
        t = preds if isinstance(preds, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(preds, dtype=np.float32))
        if not t.is_cuda:
            t = t.to('cuda')
        t = t.contiguous().float()
        lp = self.line_points_array(names)
        d_lp = torch.from_numpy(lp).to(t.device) if lp is not None else None
        recs = self.records(self.solve_device(t, d_lp))
        return [camera_from_record(r, self.img_size) for r in recs]

    def __call__(self, pred, name: Optional[str] = None) -> Optional[Camera]:
        cam = None
        try:
            cam = self.solve_batch(np.asarray(pred, dtype=np.float32)[None], [name])[0]
        except Exception as e:      # the reference's firewall (prediction.py:130-136)
            print(f'Camera initialization exc: {e}')
        return cam

    def _get_points_from_lines(self, name=None):
        if self.lines_data is not None and name is not None and name in self.lines_data:
            return self.lines_data[name]
        return {}


def get_matched_points(camera_points):
    return [(PITCH_POINTS[INTERSECTON_TO_PITCH_POINTS[i]], camera_points[i]) for i in camera_points]
