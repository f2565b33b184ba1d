"""ctypes binding of libnaf_hip.so (C ABI: include/naf_hip.h).

Replaces the pybind11 module `_hash_encoder` of the reference (src/encoder/hashencoder/src/bindings.cpp:5-8,
loaded by backend.py:6-16).  There is deliberately NO fallback: if the library is missing or a call fails the
caller gets a RuntimeError -- the product path never routes through a CPU implementation.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import build as _build

F32, F16, BF16 = 0, 1, 2
LAYOUT_LBC, LAYOUT_BLC = 0, 1
MLP_PARAMS = 4225
SCATTER_AUTO, SCATTER_ATOMIC, SCATTER_BINNED = 0, 1, 2
CFG_PER_LEVEL_LAUNCHES = 1
CFG_EXPLICIT_DEPTHS = 2
CFG_LEVELS_INTERLEAVED = 4
CFG_FORWARD_FUSED = 8
CFG_FUSED_STORE_FEATURES = 16
CFG_ENCODE_TWO_GATHERS = 32
CFG_ENCODE_WINDOWS = 64
CFG_BACKWARD_ONE_WAVE_PER_SIMD = 128
CFG_ENCODE_LEVEL_MAJOR = 256
CFG_ENCODE_GROUPS_2 = 512
CFG_ENCODE_GROUPS_4 = 1024
CFG_SCATTER_PAIR12 = 2048
CFG_TEST_TINY_BLOCKS = 4096
CFG_LEVELS_GATHER_PASS = 32768
CFG_MLP_TWO_KERNELS = 65536          # diagnostics: the MLP forward / backward pair instead of mlp16_train_kernel on small bf16 steps
CFG_MIN_BUCKETS_SHIFT = 13          # bits 13-14: at least 64 << value row buckets per level in the binned scatter
GRAD_INPUTS_NONE, GRAD_INPUTS_EXACT, GRAD_INPUTS_REFERENCE = 0, 1, 2

_DTYPE_CODE = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
_lib = None


class RenderCfg(ctypes.Structure):
    """struct naf_render_cfg (include/naf_hip.h)."""
    _fields_ = [
        ("n_samples", ctypes.c_uint32), ("perturb", ctypes.c_int32), ("bound", ctypes.c_float),
        ("L", ctypes.c_uint32), ("C", ctypes.c_uint32), ("H", ctypes.c_uint32),
        ("table_dtype", ctypes.c_int32), ("mlp_precision", ctypes.c_int32), ("last_activation", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("ray_index_base", ctypes.c_uint32), ("log2_hashmap_size", ctypes.c_uint32),
        ("scatter_mode", ctypes.c_int32), ("flags", ctypes.c_uint32),
    ]


MAX_GRAD_BUCKETS = 16


class GradBuckets(ctypes.Structure):
    """struct naf_grad_buckets (include/naf_hip.h): level ranges + the hipEvent_t recorded when each is final."""
    _fields_ = [
        ("n_buckets", ctypes.c_uint32), ("level_begin", ctypes.c_uint32 * MAX_GRAD_BUCKETS),
        ("level_end", ctypes.c_uint32 * MAX_GRAD_BUCKETS), ("ready", ctypes.c_void_p * MAX_GRAD_BUCKETS),
        ("mlp_ready", ctypes.c_void_p),
    ]


MAX_DRAW_SEGMENTS = 16


class TableAdam(ctypes.Structure):
    """struct naf_table_adam (include/naf_hip.h): the table's Adam state for naf_render_train_adam."""
    _fields_ = [
        ("param", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p), ("param_lp", ctypes.c_void_p),
        ("lp_dtype", ctypes.c_int32), ("n", ctypes.c_uint64), ("lr", ctypes.c_float), ("beta1", ctypes.c_float),
        ("beta2", ctypes.c_float), ("eps", ctypes.c_float), ("step", ctypes.c_uint32), ("grad_scale", ctypes.c_float),
        ("mlp_param", ctypes.c_void_p), ("mlp_exp_avg", ctypes.c_void_p), ("mlp_exp_avg_sq", ctypes.c_void_p),
    ]


class ScanDraw(ctypes.Structure):
    """struct naf_scan_draw (include/naf_hip.h): valid-pixel lists of the projections a step draws from."""
    _fields_ = [
        ("n_segments", ctypes.c_uint32), ("rays_per_segment", ctypes.c_uint32),
        ("valid", ctypes.c_void_p * MAX_DRAW_SEGMENTS), ("n_valid", ctypes.c_uint32 * MAX_DRAW_SEGMENTS),
    ]


class Detector(ctypes.Structure):
    """struct naf_detector (include/naf_hip.h): the detector of a scan, as every entry point that makes its rays takes it."""
    _fields_ = [
        ("det_w", ctypes.c_uint32), ("det_h", ctypes.c_uint32), ("du", ctypes.c_float), ("dv", ctypes.c_float), ("ou", ctypes.c_float),
        ("ov", ctypes.c_float), ("DSD", ctypes.c_float), ("near", ctypes.c_float), ("far", ctypes.c_float), ("parallel", ctypes.c_int32),
    ]


class NextDraw(ctypes.Structure):
    """struct naf_next_draw (include/naf_hip.h): the arguments of naf_draw_scan_rays for the NEXT step's pixels."""
    _fields_ = [
        ("draw", ScanDraw), ("poses", ctypes.c_void_p), ("projections", ctypes.c_void_p), ("pixels", ctypes.c_void_p),
        ("target", ctypes.c_void_p), ("rays", ctypes.c_void_p),
        ("first_draw", ctypes.c_uint32), ("n_draws", ctypes.c_uint32), ("n_projections", ctypes.c_uint32), ("det", Detector),
        ("seed", ctypes.c_uint64),
    ]


# name -> (restype, argtypes); mirrors include/naf_hip.h one to one (checked by tests/test_abi_symbols.py)
_vp, _u32, _u64, _i32, _f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_float
_det, _u32x3, _f32x3 = ctypes.POINTER(Detector), ctypes.POINTER(ctypes.c_uint32 * 3), ctypes.POINTER(ctypes.c_float * 3)
SIGNATURES = {
    "naf_last_error": (ctypes.c_char_p, []),
    "naf_abi_version": (_i32, []),
    "naf_profile_enable": (_i32, [_i32]),
    "naf_profile_collect": (_i32, [ctypes.c_char_p, ctypes.c_size_t]),
    "naf_hash_encode_forward": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _i32, _vp, _i32, _i32, _vp]),
    "naf_hash_encode_backward": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _i32, _vp, _vp, _i32, _i32, _vp]),
    "naf_hash_encode_workspace_bytes": (ctypes.c_size_t, [_u32, _u32, _u32, _u32, _u32, _i32]),
    "naf_hash_encode_backward_ws": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _i32, _vp, _vp, _i32, _i32, _u32, _vp,
                                           ctypes.c_size_t, _vp]),
    "naf_sample_rays": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _i32, _f32, _u64, _u32, _vp]),
    "naf_fine_depths": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _i32, _i32, _u64, _u32, _vp, _vp]),
    "naf_draw_scan_rays": (_i32, [ctypes.POINTER(ScanDraw), _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _det, _u64, _vp]),
    "naf_generate_rays": (_i32, [_vp, _vp, ctypes.c_int64, _vp, _u64, _u32, _det, _vp]),
    "naf_integrate_forward": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp]),
    "naf_integrate_backward": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp]),
    "naf_scatter_overflow_count": (_i32, [ctypes.POINTER(RenderCfg), _u64, _vp, ctypes.POINTER(ctypes.c_uint32)]),
    "naf_scatter_overflow_levels": (_i32, [ctypes.POINTER(RenderCfg), _u64, _vp, ctypes.POINTER(ctypes.c_uint32 * 32)]),
    "naf_render_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(RenderCfg), _u64]),
    "naf_forward_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(RenderCfg), _u64]),
    "naf_render_forward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _vp, _vp]),
    "naf_render_forward_samples": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _vp, _vp]),
    "naf_render_backward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _vp, _i32, _vp]),
    "naf_render_train": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _vp, _vp]),
    "naf_render_train_bucketed": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _vp,
                                         ctypes.POINTER(GradBuckets), _vp]),
    "naf_render_train_adam": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _vp,
                                     ctypes.POINTER(TableAdam), _vp]),
    "naf_render_train_adam_draw": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _vp,
                                          ctypes.POINTER(TableAdam), ctypes.POINTER(NextDraw), _vp]),
    "naf_levels_encode": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, ctypes.POINTER(RenderCfg), _u32, _u32, _vp]),
    "naf_levels_field_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _vp, _vp, _vp]),
    "naf_levels_scatter": (_i32, [_vp, _vp, _vp, ctypes.c_size_t, _u32, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _u32, _u32, _vp,
                                  ctypes.POINTER(TableAdam), ctypes.POINTER(ctypes.c_int), _vp]),
    "naf_field_forward": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, ctypes.POINTER(RenderCfg), _vp, _vp]),
    "naf_field_forward_grid": (_i32, [ctypes.POINTER(ctypes.c_double * 3), ctypes.POINTER(ctypes.c_double * 3), _u32x3, _vp, _vp, _vp, _vp,
                                      ctypes.POINTER(RenderCfg), _vp, ctypes.c_size_t, _vp]),
    "naf_adam_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _u64, _f32, _f32, _f32, _f32, _u32, _f32, _i32, _vp]),
    "naf_normalize_inputs": (_i32, [_vp, _u64, _f32, _vp, _vp, _vp]),
    "naf_project_rays": (_i32, [_vp, _u32, _u32, _u32, _f32x3, _vp, _u64, _f32, _vp, _vp]),
    "naf_project_scan": (_i32, [_vp, _u32x3, _f32x3, _vp, _u32, _det, _f32, _vp, _vp]),
    "naf_project_rays_siddon": (_i32, [_vp, _u32, _u32, _u32, _f32x3, _vp, _u64, _vp, _vp]),
    "naf_project_scan_siddon": (_i32, [_vp, _u32x3, _f32x3, _vp, _u32, _det, _vp, _vp]),
    "naf_backproject_rays": (_i32, [_vp, _vp, _u64, _u32, _u32, _u32, _f32x3, _f32, _vp, _vp]),
    "naf_backproject_scan": (_i32, [_vp, _u32x3, _f32x3, _vp, _u32, _det, _f32, _vp, _vp]),
    "naf_backproject_rays_siddon": (_i32, [_vp, _vp, _u64, _u32, _u32, _u32, _f32x3, _vp, _vp]),
    "naf_backproject_scan_siddon": (_i32, [_vp, _u32x3, _f32x3, _vp, _u32, _det, _vp, _vp]),
    "naf_filter_rows": (_i32, [_vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "naf_filter_rows_views": (_i32, [_vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "naf_sart_residual_scan": (_i32, [_vp, _u32x3, _f32x3, _vp, _u32, _det, _f32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "naf_sart_backproject_scan": (_i32, [_vp, _vp, _u32, _u32, _u32x3, _f32x3, _vp, _det, _f32, _vp, _vp, _vp]),
    "naf_sart_update": (_i32, [_vp, _vp, _vp, _u64, _f32, _i32, _i32, _i32, _vp]),
    "naf_sart_residual_scan_siddon": (_i32, [_vp, _u32x3, _f32x3, _vp, _u32, _det, _vp, _u32, _vp, _vp, _vp, _vp]),
    "naf_sart_backproject_scan_siddon": (_i32, [_vp, _vp, _u32, _u32, _u32x3, _f32x3, _vp, _det, _vp, _vp, _vp]),
    "naf_backproject_scan_gather": (_i32, [_vp, _vp, _u32, _u32, _u32x3, _f32x3, _vp, _det, _f32, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "naf_ssim_3d_workspace_bytes": (ctypes.c_size_t, [_u32, _u32, _u32]),
    "naf_ssim_3d": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, ctypes.c_size_t, _vp]),
    "naf_resize_volume_workspace_bytes": (ctypes.c_size_t, [_u32x3, _u32x3]),
    "naf_resize_volume": (_i32, [_vp, _u32x3, _f32, _f32, _vp, _u32x3, _vp, _vp, ctypes.c_size_t, _vp]),
    "naf_tv_workspace_bytes": (ctypes.c_size_t, [_u32, _u32, _u32]),
    "naf_tv_gradient": (_i32, [_vp, _u32, _u32, _u32, _f32, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "naf_tv_descent": (_i32, [_vp, _vp, _u32, _u32, _u32, _f32, _u32, _f32, _vp, _vp, ctypes.c_size_t, _vp]),
    "naf_tv_prox_step": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _f32, _f32, _i32, _vp]),
    "naf_tv_prox_primal": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _f32, _i32, _vp]),
    "naf_cgls_workspace_bytes": (ctypes.c_size_t, [_u64, _u32]),
    "naf_cgls_wdot": (_i32, [_vp, _vp, _u64, _u32, _u32, _vp, ctypes.c_size_t, _vp]),
    "naf_cgls_residual_step": (_i32, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _vp, ctypes.c_size_t, _vp]),
    "naf_cgls_direction_step": (_i32, [_vp, _vp, _vp, _u64, _u32, _u32, _vp, ctypes.c_size_t, _vp]),
    "naf_volume_sample_points": (_i32, [_vp, _u32, _u32, _u32, _f32x3, _vp, _u64, _vp, _vp]),
    "naf_volume_draw_sample": (_i32, [_vp, _u32x3, _f32x3, _f32x3, _f32x3, _u64, _u32, _u32, _vp, _vp, _vp]),
    "naf_align_scores_workspace_bytes": (ctypes.c_size_t, [_u32, _u32, _u32, _u32, _u32]),
    "naf_align_shift_scores": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, ctypes.c_size_t, _vp, _vp]),
    "naf_align_peak": (_i32, [_vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "naf_align_shift_views": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp]),
    "naf_stripe_workspace_bytes": (ctypes.c_size_t, [_u32, _u32, _u32, _u32]),
    "naf_stripe_remove_sorting": (_i32, [_vp, _u32, _u32, _u32, _u32, _vp, ctypes.c_size_t, _vp, _vp]),
    "naf_frames_condition": (_i32, [_vp, _i32, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _f32, _u32, _vp, _vp, _vp]),
    "naf_inpaint_rows": (_i32, [_vp, _vp, _vp, _f32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "naf_center_slices": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _i32, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _vp, _vp]),
    "naf_center_metrics_workspace_bytes": (ctypes.c_size_t, [_u32, _u32, _u32]),
    "naf_center_metrics": (_i32, [_vp, _u32, _u32, _u32, _f32, _f32, _f32, _vp, _vp, ctypes.c_size_t, _vp]),
    "naf_center_slices_tilted": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32,
                                        _vp, _vp]),
}


def library_path():
    return _build.LIB_PATH


def lib():
    """Load (once) the prebuilt in-tree library; raise loudly if it is absent or incomplete."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            # a fresh checkout has sources only (*.so is git-ignored): compile them now if the ROCm toolchain is here;
            # there is no other way to run -- no CPU fallback exists for the NAF hot path
            try:
                _build.build_library()
            except Exception as e:
                raise RuntimeError(
                    f"{path} not found and could not be built ({e}).  Build it with "
                    "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950).  "
                    "There is no CPU fallback for the NAF hot path.") from e
        handle = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().naf_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libnaf_hip {what} failed ({rc}): {msg}")


def dtype_code(dt):
    try:
        return _DTYPE_CODE[dt]
    except KeyError:
        raise RuntimeError(f"libnaf_hip: unsupported dtype {dt}") from None


def ptr(t):
    """Device pointer of a tensor that must already live on the GPU and be contiguous (hashencoder.cu:17-18)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libnaf_hip: tensor must be a CUDA/HIP tensor (no CPU path)")
    if not t.is_contiguous():
        raise RuntimeError("libnaf_hip: tensor must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def check_volume(t, who, name="volume"):
    """A volume argument of the library: a contiguous float32 [n1, n2, n3] CUDA/HIP tensor (no CPU path)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a CUDA/HIP tensor (no CPU path)")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be float32, got {t.dtype}")
    if t.dim() != 3:
        raise ValueError(f"{who}: {name} must be [n1, n2, n3], got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")


def check_stack(t, shape, like, who, name):
    """A stack of views or another array argument: a contiguous float32 CUDA/HIP tensor of `shape`, on `like`'s device if given."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a CUDA/HIP tensor (no CPU path)")
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    if like is not None and t.device != like.device:
        raise ValueError(f"{who}: {name} must be on the device of the other arguments")


def check_rays(rays, like, who, whose):
    """Rays of the library: a float32 [n, 8] CUDA/HIP tensor on the device of `like` (named `whose` in the message) -> n."""
    if not isinstance(rays, torch.Tensor) or not rays.is_cuda or rays.device != like.device:
        raise RuntimeError(f"{who}: rays must be a CUDA/HIP tensor on the {whose} device")
    if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError(f"{who}: rays must be float32 [n, 8], got {rays.dtype} {tuple(rays.shape)}")
    return rays.shape[0]


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def profile_enable(on=True):
    check(lib().naf_profile_enable(int(on)), "profile_enable")


def profile_collect():
    """-> {kernel: (launches, total_ms)} for everything launched since profile_enable(True)."""
    buf = ctypes.create_string_buffer(1 << 16)
    check(lib().naf_profile_collect(buf, len(buf)), "profile_collect")
    out = {}
    for line in buf.value.decode().splitlines():
        name, count, ms = line.rsplit(" ", 2)
        out[name] = (int(count), float(ms))
    return out
