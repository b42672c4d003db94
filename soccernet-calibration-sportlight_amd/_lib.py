"""ctypes binding of libsncal.so (the C ABI declared in include/sncal.h).

There is NO fallback: if the library is missing or a symbol cannot be resolved, importing the product
path raises.  PyTorch is used by the callers only for device memory and streams.
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SNCAL_LIB_PATH') or os.path.join(_PKG, 'libsncal.so')     # override: A/B runs of two builds

c_float_p = ctypes.POINTER(ctypes.c_float)
c_double_p = ctypes.POINTER(ctypes.c_double)
c_int_p = ctypes.POINTER(ctypes.c_int)
vp = ctypes.c_void_p


class HRNetDesc(ctypes.Structure):
    """sncal_hrnet_desc."""
    _fields_ = [('num_classes', ctypes.c_int), ('stem_width', ctypes.c_int), ('upscale', ctypes.c_int),
                ('head_softmax', ctypes.c_int), ('stage1_blocks', ctypes.c_int),
                ('stage1_channels', ctypes.c_int), ('num_modules', ctypes.c_int * 3),
                ('num_branches', ctypes.c_int * 3), ('num_blocks', ctypes.c_int * 3),
                ('num_channels', (ctypes.c_int * 4) * 3)]


class KernelStat(ctypes.Structure):
    """sncal_kernel_stat."""
    _fields_ = [('kernel', ctypes.c_char * 96), ('flops', ctypes.c_double), ('bytes', ctypes.c_double),
                ('ms', ctypes.c_double), ('launches', ctypes.c_int)]


class PlanOp(ctypes.Structure):
    """sncal_plan_op."""
    _fields_ = [('type', ctypes.c_int), ('active', ctypes.c_int), ('conv', ctypes.c_int), ('name', ctypes.c_char * 96),
                ('cin', ctypes.c_int), ('cout', ctypes.c_int), ('ksize', ctypes.c_int), ('stride', ctypes.c_int),
                ('col_off', ctypes.c_int), ('in_', ctypes.c_int), ('res', ctypes.c_int), ('out', ctypes.c_int),
                ('base', ctypes.c_int), ('src', ctypes.c_int * 4), ('nsrc', ctypes.c_int), ('head_direct', ctypes.c_int),
                ('head_src', ctypes.c_int * 5), ('head_nsrc', ctypes.c_int), ('head_fold', ctypes.c_int * 3),
                ('head_nfold', ctypes.c_int), ('relu', ctypes.c_int), ('out_coff', ctypes.c_int), ('out_f32', ctypes.c_int),
                ('fp8', ctypes.c_int), ('kernel', ctypes.c_char * 96), ('res_twin', ctypes.c_int), ('launch', ctypes.c_int),
                ('writes_out', ctypes.c_int), ('writes_twin', ctypes.c_int), ('prep_in', ctypes.c_int)]


class PlanTensor(ctypes.Structure):
    """sncal_plan_tensor."""
    _fields_ = [('C', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int), ('dtype', ctypes.c_int), ('twin', ctypes.c_int),
                ('alive', ctypes.c_int), ('scale', ctypes.c_float), ('bytes', ctypes.c_size_t), ('sub_batch', ctypes.c_int),
                ('offset', ctypes.c_size_t), ('first', ctypes.c_int), ('last', ctypes.c_int)]


class Camera(ctypes.Structure):
    """sncal_camera."""
    _fields_ = [('position', ctypes.c_double * 3), ('rotation', ctypes.c_double * 9),
                ('fx', ctypes.c_double), ('fy', ctypes.c_double), ('cx', ctypes.c_double),
                ('cy', ctypes.c_double), ('rmse', ctypes.c_double), ('status', ctypes.c_int32),
                ('n_points', ctypes.c_int32)]


MAX_CONF_THRESHS = 16          # SNCAL_MAX_CONF_THRESHS


class VoterCfg(ctypes.Structure):
    """sncal_voter_cfg."""
    _fields_ = [('algorithm', ctypes.c_int), ('n_conf_threshs', ctypes.c_int), ('conf_thresh', ctypes.c_double),
                ('conf_threshs', ctypes.c_double * MAX_CONF_THRESHS),
                ('max_rmse', ctypes.c_double), ('max_rmse_rel', ctypes.c_double),
                ('min_points', ctypes.c_int), ('min_points_per_plane', ctypes.c_int),
                ('min_points_for_refinement', ctypes.c_int), ('reliable_thresh', ctypes.c_int),
                ('min_focal_length', ctypes.c_double), ('img_w', ctypes.c_int), ('img_h', ctypes.c_int),
                ('lm_schedule', ctypes.c_int), ('refine_max_iters', ctypes.c_int)]


class JpegInfo(ctypes.Structure):
    """sncal_jpeg_info."""
    _fields_ = [('width', ctypes.c_int32), ('height', ctypes.c_int32), ('components', ctypes.c_int32),
                ('h_samp', ctypes.c_int32), ('v_samp', ctypes.c_int32), ('restart_interval', ctypes.c_int32),
                ('blocks', ctypes.c_int32 * 3)]


class AugmentParams(ctypes.Structure):
    """sncal_augment_params."""
    _fields_ = [('gain', ctypes.c_double * 3), ('contrast', ctypes.c_double), ('noise_sigma', ctypes.c_double),
                ('seed', ctypes.c_uint64), ('flags', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]


# name -> (restype, argtypes); must list every function include/sncal.h declares
SIGNATURES = {
    'sncal_version': (ctypes.c_int, []),
    'sncal_last_error': (ctypes.c_char_p, []),
    'sncal_x3_name': (ctypes.c_char_p, []),
    'sncal_heatmap_decode': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, vp, vp]),
    'sncal_line_decode': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_float, ctypes.c_float, vp, vp]),
    'sncal_hrnet_create': (ctypes.c_int, [ctypes.POINTER(HRNetDesc), ctypes.c_int, ctypes.POINTER(vp)]),
    'sncal_hrnet_destroy': (None, [vp]),
    'sncal_hrnet_num_convs': (ctypes.c_int, [vp]),
    'sncal_hrnet_conv_info': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p,
                                             ctypes.c_int, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p]),
    'sncal_hrnet_set_conv': (ctypes.c_int, [vp, ctypes.c_int, vp, vp, vp]),
    'sncal_hrnet_finalize': (ctypes.c_int, [vp]),
    'sncal_hrnet_set_equalize': (ctypes.c_int, [vp, ctypes.c_int]),
    'sncal_hrnet_equalize': (ctypes.c_int, [vp, c_int_p]),
    'sncal_hrnet_get_conv': (ctypes.c_int, [vp, ctypes.c_int, vp, vp, vp]),
    'sncal_hrnet_range_status': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), ctypes.c_int, vp]),
    'sncal_hrnet_output_size': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, c_int_p, c_int_p]),
    'sncal_hrnet_workspace': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_size_t)]),
    'sncal_hrnet_forward': (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp,
                                           ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]),
    'sncal_evaluate_cameras': (ctypes.c_int, [vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int,
                                              ctypes.c_double, ctypes.c_int, ctypes.c_int, vp, vp]),
    'sncal_evaluate_cameras_detail': (ctypes.c_int, [vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int,
                                                     ctypes.c_double, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]),
    'sncal_lines_to_points': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_float, ctypes.c_double, vp, vp]),
    'sncal_hrnet_forward_u8': (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp,
                                              ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]),
    'sncal_hrnet_set_profiling': (ctypes.c_int, [vp, ctypes.c_int]),
    'sncal_hrnet_calibrate_fp8': (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]),
    'sncal_hrnet_calibrate_fp8_workspace': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    'sncal_hrnet_set_fp8_layers': (ctypes.c_int, [vp, ctypes.c_char_p]),
    'sncal_hrnet_plan_num_ops': (ctypes.c_int, [vp]),
    'sncal_hrnet_plan_num_tensors': (ctypes.c_int, [vp]),
    'sncal_hrnet_plan_op': (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(PlanOp)]),
    'sncal_hrnet_plan_tensor': (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(PlanTensor)]),
    'sncal_hrnet_plan_tap': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp]),
    'sncal_hrnet_get_profile': (ctypes.c_int, [vp, ctypes.POINTER(KernelStat), ctypes.c_int, c_int_p]),
    'sncal_pnp_refine_lm': (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int,
                                           ctypes.c_double, vp]),
    'sncal_solve_pnp': (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]),
    'sncal_jpeg_probe': (ctypes.c_int, [vp, ctypes.c_size_t, ctypes.POINTER(JpegInfo)]),
    'sncal_jpeg_entropy_decode': (ctypes.c_int, [vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.POINTER(JpegInfo)]),
    'sncal_jpeg_create': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]),
    'sncal_jpeg_create_scaled': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(vp)]),
    'sncal_jpeg_output_size': (ctypes.c_int, [vp, c_int_p, c_int_p]),
    'sncal_jpeg_scaled_layout': (ctypes.c_int, [ctypes.POINTER(JpegInfo), ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                                                ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                ctypes.POINTER(ctypes.c_int32)]),
    'sncal_jpeg_destroy': (None, [vp]),
    'sncal_jpeg_decode': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t),
                                         ctypes.c_int, vp, vp]),
    'sncal_create_target': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int, vp, vp]),
    'sncal_heatmap_loss_workspace': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.POINTER(ctypes.c_size_t)]),
    'sncal_heatmap_loss': (ctypes.c_int, [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                          ctypes.c_float, ctypes.c_int, vp, vp, ctypes.c_size_t, vp]),
    'sncal_heatmap_loss_grad': (ctypes.c_int, [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                               ctypes.c_float, ctypes.c_int, c_double_p, vp, vp, vp, ctypes.c_size_t, vp]),
    'sncal_line_target': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                         vp, vp]),
    'sncal_line_loss_workspace': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_size_t)]),
    'sncal_line_loss': (ctypes.c_int, [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_float, ctypes.c_int, vp, vp, ctypes.c_size_t, vp]),
    'sncal_ehm_loss_grad': (ctypes.c_int, [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                            ctypes.c_float, ctypes.c_float, ctypes.c_int, c_double_p, vp, vp, vp, ctypes.c_size_t, vp]),
    'sncal_line_acc_counts': (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, c_float_p, ctypes.c_int, vp, vp]),
    'sncal_augment_workspace': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    'sncal_augment_u8': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]),
    'sncal_keypoint_labels_workspace': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    'sncal_keypoint_labels': (ctypes.c_int, [vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_uint, vp, vp, vp, vp, vp, vp, vp,
                                             ctypes.c_size_t, vp]),
    'sncal_extremity_counts': (ctypes.c_int, [vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_float, ctypes.c_float, vp, ctypes.c_int, vp,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, vp, vp, vp,
                                              vp]),
    'sncal_baseline_cameras': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_float, ctypes.c_float, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int, vp]),
    'sncal_resize_tables': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                                           ctypes.POINTER(ctypes.c_int16)]),
    'sncal_resize_u8': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp]),
    'sncal_calibrate': (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.POINTER(VoterCfg), vp, vp]),
    'sncal_calibrate_workspace': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(VoterCfg), ctypes.POINTER(ctypes.c_size_t)]),
    'sncal_calibrate_ws': (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.POINTER(VoterCfg), vp, vp, ctypes.c_size_t, vp]),
    'sncal_calibrate_sweep_workspace': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(VoterCfg), ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    'sncal_calibrate_sweep': (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.POINTER(VoterCfg), vp, ctypes.c_int, vp, vp, vp, ctypes.c_size_t, vp]),
    'sncal_evaluate_outcomes': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int,
                                               ctypes.c_double, ctypes.c_int, ctypes.c_int, vp, vp]),
    'sncal_sweep_fold': (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]),
    'sncal_shutdown': (ctypes.c_int, []),
    'sncal_stream_create_cu_mask': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(vp)]),
    'sncal_stream_destroy': (ctypes.c_int, [vp]),
}

_lib = None
MISSING = []


class SncalError(RuntimeError):
    pass


def lib():
    """Load libsncal.so once; raise loudly if it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SncalError(f'{LIB_PATH} is missing: build it with __graft_entry__.build() '
                             '(hipcc --offload-arch=gfx950); this package has no CPU fallback')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError:          # calling it later raises; tests/test_abi.py requires none
                MISSING.append(name)
                continue
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


class SncalRangeError(SncalError):
    """SNCAL_ERR_RANGE: the fp16x3 engine met a folded weight (load_state_dict) or an activation (range_status) that fp16 hi + lo
    halves do not represent; the reference's fp32 predict() has no such limit -- use dtype='fp32'."""


ERR_RANGE = -6


def check(status, what=''):
    if status != 0:
        msg = lib().sncal_last_error().decode(errors='replace')
        raise (SncalRangeError if status == ERR_RANGE else SncalError)(f'{what} failed with status {status}: {msg}')


def current_stream_ptr():
    """hipStream_t of torch's current stream as an integer (0 = default stream)."""
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def call(name, *args, device=None):
    """check(lib().<name>(*args), name).  A tensor (anything with data_ptr) goes as its address -- NULL for an empty one -- and None
    and everything else as they are.  device: make it current around a host call that needs it (the launches use launch())."""
    fn = getattr(lib(), name)
    args = [a.data_ptr() if hasattr(a, 'data_ptr') else a for a in args]
    if device is None:
        return check(fn(*args), name)
    import torch
    with torch.cuda.device(device):
        check(fn(*args), name)


def launch(name, device, *args):
    """call() with `device` current and torch's current stream on it as the last argument: where include/sncal.h puts every
    `void* stream` (tests/test_lib_call_host.py holds the header to that)."""
    import torch
    with torch.cuda.device(device):
        call(name, *args, current_stream_ptr())


def workspace_bytes(query_name, *dims):
    """The size_t a sncal_*_workspace query writes through its last argument."""
    n = ctypes.c_size_t()
    call(query_name, *dims, ctypes.byref(n))
    return n.value


def workspace(query_name, *dims, device):
    """uint8 scratch of the size the query names, at least 16 bytes so that an empty batch still has an address."""
    import torch
    return torch.empty(max(workspace_bytes(query_name, *dims), 16), dtype=torch.uint8, device=device)


def pack_parts(parts):
    """Host arrays -> (flat uint8 array holding them one after the other, their byte offsets).  Every part starts at a multiple
    of 8 bytes, in whatever order they come, so each can be read on the device as the type it has."""
    import numpy as np
    offsets = [0]
    for p in parts:
        offsets.append(offsets[-1] + -(-p.nbytes // 8) * 8)
    flat = np.zeros(offsets.pop(), np.uint8)
    for at, p in zip(offsets, parts):
        flat[at:at + p.nbytes] = np.ascontiguousarray(p).reshape(-1).view(np.uint8)
    return flat, offsets


def upload(parts, device, pinned=False):
    """pack_parts in one copy to the device -> (the device tensor, which the caller keeps alive until the launch is queued, [device
    address of each part]).  pinned: from page-locked memory and without waiting; a copy from pageable memory holds the host
    until the stream has drained."""
    import torch
    flat, offsets = pack_parts(parts)
    host = torch.from_numpy(flat)
    d = host.pin_memory().to(device, non_blocking=True) if pinned else host.to(device)
    return d, [d.data_ptr() + at for at in offsets]


def require_device(t, dtype, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SncalError(f'{name} must be a tensor on the GPU (libsncal has no CPU path)')
    if t.dtype != dtype:
        raise SncalError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise SncalError(f'{name} must be contiguous')
    return t
