"""ctypes binding of lib/libnof.so (the C ABI in include/nof.h).

This is the product's only route to the GPU: there is no CPU fallback.  If the shared
library is missing or fails to load, ``lib()`` raises — loudly — instead of degrading.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("NOF_LIB") or os.path.join(_PKG, "lib", "libnof.so")  # NOF_LIB: diagnostic builds

NOF_MAX_LEVELS = 4
NOF_NUM_TIMERS = 8
TIMER_NAMES = ("pack", "sample", "mlp_fwd", "render_fwd", "render_bwd", "mlp_bwd", "wgrad", "wgrad_reduce")
STATUS = {0: "NOF_OK", 1: "NOF_ERR_INVALID_ARG", 2: "NOF_ERR_HIP", 3: "NOF_ERR_RCCL", 4: "NOF_ERR_OOM",
          5: "NOF_ERR_UNSUPPORTED"}


class NofError(RuntimeError):
    def __init__(self, status: int, where: str, msg: str):
        super().__init__(f"{where}: {STATUS.get(status, status)}: {msg}")
        self.status = status


NOF_PRECISION_F32, NOF_PRECISION_F32_SPLIT, NOF_PRECISION_F16X2, NOF_PRECISION_F32_F16SPLIT, NOF_PRECISION_F16 = 0, 1, 2, 3, 4
NOF_PRECISION_F16_PRODUCTS = 5  # the any-shape path's fp16-product mode (every network)
# the training drivers' --precision names
PRECISION_NAMES = {"f32": NOF_PRECISION_F32, "split": NOF_PRECISION_F32_SPLIT, "f16x2": NOF_PRECISION_F16X2,
                   "f16split": NOF_PRECISION_F32_F16SPLIT, "f16": NOF_PRECISION_F16,
                   "f16p": NOF_PRECISION_F16_PRODUCTS}


class nof_config(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("max_rays", C.c_int32), ("num_levels", C.c_int32),
        ("num_samples", C.c_int32 * NOF_MAX_LEVELS),
        ("net_depth", C.c_int32), ("net_width", C.c_int32),
        ("net_depth_condition", C.c_int32), ("net_width_condition", C.c_int32),
        ("skip_layer", C.c_int32), ("min_deg_point", C.c_int32), ("max_deg_point", C.c_int32),
        ("deg_view", C.c_int32), ("randomized", C.c_int32), ("white_bkgd", C.c_int32),
        ("resample_padding", C.c_float), ("coarse_loss_mult", C.c_float),
        ("seed", C.c_uint64), ("stream", C.c_void_p), ("precision", C.c_int32), ("grad_buckets", C.c_int32),
        ("lindisp", C.c_int32), ("ray_shape", C.c_int32),
        ("density_bias", C.c_float), ("rgb_padding", C.c_float),
        ("stop_level_grad", C.c_int32),
    ]

    # include/nof.h appends `float distortion_loss_mult` after stop_level_grad.  The struct is 8-byte aligned (seed,
    # stream) and ended 4 bytes short of a multiple of 8, so the new field takes what were its tail padding bytes
    # and sizeof(nof_config) is what it was (lib() checks it against nof_config_size()).  The field list above is
    # left ending at stop_level_grad (CPU tests of earlier options pin that name as its last entry); the new field
    # is a property at its offset instead, read and set like any other (default_config(distortion_loss_mult=x)).
    @property
    def distortion_loss_mult(self) -> float:
        return C.c_float.from_buffer(self, _DIST_MULT_OFFSET).value

    @distortion_loss_mult.setter
    def distortion_loss_mult(self, value: float) -> None:
        C.c_float.from_buffer(self, _DIST_MULT_OFFSET).value = value


_DIST_MULT_OFFSET = nof_config.stop_level_grad.offset + C.sizeof(C.c_int32)
assert _DIST_MULT_OFFSET + C.sizeof(C.c_float) <= C.sizeof(nof_config), "nof_config: no room for distortion_loss_mult"


class nof_model_ext(C.Structure):
    _fields_ = [("size", C.c_uint32), ("appearance_views", C.c_int32), ("appearance_dim", C.c_int32)]


class nof_level_view(C.Structure):
    _fields_ = [("n", C.c_int32), ("samples", C.c_int32)] + [
        (k, C.c_void_p) for k in ("t", "weights", "comp_rgb", "density", "rgb", "density_grad", "rgb_grad")]


class nof_mlp_debug(C.Structure):
    _fields_ = [("M", C.c_int32)] + [(k, C.c_void_p) for k in
                                     ("act_in", "act_h", "act_h9", "masks", "zhead", "delta", "delta9x")] + \
        [("generic", C.c_int32), ("gen_h", C.c_void_p), ("gen_hc", C.c_void_p)]


class nof_gemm_src(C.Structure):
    _fields_ = [("p", C.c_void_p), ("si", C.c_int64), ("sk", C.c_int64), ("idiv", C.c_int32)]


class nof_gemm_args(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("K1", C.c_int32), ("K2", C.c_int32),
                ("A1", nof_gemm_src), ("A2", nof_gemm_src), ("B1", nof_gemm_src), ("B2", nof_gemm_src),
                ("bias", C.c_void_p), ("relu", C.c_int32), ("G", C.c_void_p), ("gi", C.c_int64), ("gj", C.c_int64),
                ("C", C.c_void_p), ("ci", C.c_int64), ("cj", C.c_int64), ("kchunk", C.c_int32),
                ("slab_stride", C.c_int64), ("rowsum", C.c_void_p), ("scale_amax", C.c_void_p),
                ("scale_src", C.c_int32), ("ksplit", C.c_int32)]


class nof_render_out(C.Structure):
    _fields_ = [("num_levels", C.c_int32), ("comp_rgb", C.c_void_p * NOF_MAX_LEVELS),
                ("distance", C.c_void_p * NOF_MAX_LEVELS), ("acc", C.c_void_p * NOF_MAX_LEVELS)]


class nof_batch(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(k, C.c_void_p) for k in (
        "origins", "directions", "viewdirs", "radii", "nears", "fars", "loss_mults", "pixels", "record_index")]


class nof_step_stats(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("weight_l2", "grad_norm", "grad_abs_max", "grad_norm_clipped",
                                         "clip_scale")] + [("iteration", C.c_int32)]


class nof_view_out(C.Structure):
    _fields_ = [("rgb", C.c_void_p * NOF_MAX_LEVELS), ("distance", C.c_void_p), ("acc", C.c_void_p)]


class nof_view_metrics(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("num_levels", C.c_int32),
                ("mse", C.c_double * NOF_MAX_LEVELS), ("psnr", C.c_float * NOF_MAX_LEVELS), ("ssim", C.c_float)]


NOF_VIEW_SSIM = 1

OUTPUT_GRAD_FN = C.CFUNCTYPE(C.c_uint64, C.c_void_p, C.c_uint64, C.c_int32, C.c_float, C.c_uint64)
GRAD_BUCKET_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64))
NOF_GRAD_ACCUMULATE, NOF_GRAD_PUBLISH, NOF_GRAD_BUCKETS = 1, 2, 2
NOF_NUMERIC_FORWARD, NOF_NUMERIC_DELTA = 1, 2

P = C.c_void_p
F = C.c_float
I32 = C.c_int32
U32 = C.c_uint32
U64 = C.c_uint64
PP = C.POINTER(C.POINTER(C.c_float))

# name -> argtypes (restype nof_status = int32 unless listed in _RESTYPE)
SIGNATURES = {
    "nof_config_default": [C.POINTER(nof_config)],
    "nof_last_error": [],
    "nof_version": [],
    "nof_config_size": [],
    "nof_mipnerf_create": [C.POINTER(nof_config), C.POINTER(P)],
    "nof_mipnerf_create_ex": [C.POINTER(nof_config), C.POINTER(nof_model_ext), C.POINTER(P)],
    "nof_mipnerf_appearance": [P, C.POINTER(P), C.POINTER(P), C.POINTER(I32), C.POINTER(I32)],
    "nof_mipnerf_set_ray_views": [P, P],
    "nof_mipnerf_set_render_appearance": [P, I32],
    "nof_mipnerf_destroy": [P],
    "nof_mipnerf_get_gradient": [P, I32, P, P, P, P, P, P, OUTPUT_GRAD_FN, P, C.POINTER(PP)],
    "nof_mipnerf_get_gradient_device": [P, I32, P, P, P, P, P, P, P, F, C.POINTER(PP)],
    "nof_mipnerf_get_gradient_device_ex": [P, I32, P, P, P, P, P, P, P, F, U32, C.POINTER(PP)],
    "nof_mipnerf_set_grad_buckets": [P, GRAD_BUCKET_FN, P],
    "nof_grad_bucket_spans": [I32, C.POINTER(I32), I32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                              C.POINTER(I32)],
    "nof_mipnerf_layer_sizes": [P, C.POINTER(I32), I32, C.POINTER(I32)],
    "nof_mipnerf_mlp": [P, C.POINTER(P)],
    "nof_mipnerf_set_rng": [P, U64, U32, U32],
    "nof_mipnerf_get_rng": [P, C.POINTER(U64), C.POINTER(U32), C.POINTER(U32)],
    "nof_mipnerf_level_view": [P, I32, C.POINTER(nof_level_view)],
    "nof_mipnerf_cross_view": [P, I32, C.POINTER(P), C.POINTER(P)],
    "nof_mipnerf_set_ray_grad": [P, I32],
    "nof_mipnerf_ray_grad": [P, C.POINTER(P), C.POINTER(P)],
    "nof_mipnerf_loss": [P, C.POINTER(F)],
    "nof_mipnerf_distortion_loss": [P, C.POINTER(F)],
    "nof_mipnerf_set_interlevel_loss": [P, F],
    "nof_mipnerf_set_contraction": [P, I32],
    "nof_mipnerf_get_contraction": [P, P],
    "nof_mipnerf_set_step_fusion": [P, U32],
    "nof_mipnerf_interlevel_loss": [P, C.POINTER(F)],
    "nof_mipnerf_numeric_status": [P, C.POINTER(U32), I32],
    "nof_device_checks": [C.POINTER(U32), I32],
    "nof_device_checks_selftest": [],
    "nof_mipnerf_render_device": [P, I32, P, P, P, P, P, I32, I32, C.POINTER(nof_render_out)],
    "nof_image_metrics": [P, P, I32, I32, F, C.POINTER(F), C.POINTER(F), P],
    "nof_dataset_open": [C.c_char_p, I32, C.POINTER(P)],
    "nof_dataset_open_streaming": [C.c_char_p, I32, C.c_int64, C.POINTER(P)],
    "nof_dataset_is_streaming": [P, C.POINTER(I32)],
    "nof_dataset_from_host": [P, C.c_int64, I32, C.POINTER(P)],
    "nof_dataset_count": [P, C.POINTER(C.c_int64)],
    "nof_dataset_next": [P, I32, U64, U32, U32, P, C.POINTER(nof_batch), C.POINTER(F)],
    "nof_dataset_destroy": [P],
    "nof_generate_rays": [P, I32, I32, I32, F, F, F, I32, P, P, P],
    "nof_dataset_generate": [P, I32, I32, I32, F, F, F, I32, P, I32, C.POINTER(P)],
    "nof_multiscale_layout": [I32, I32, F, I32, I32, I32, C.POINTER(I32), C.POINTER(I32), C.POINTER(F),
                              C.POINTER(F), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "nof_dataset_from_images": [P, I32, I32, I32, F, F, F, I32, P, I32, I32, I32, C.POINTER(P)],
    "nof_dataset_materialize": [P, P, P],
    "nof_dataset_scene_info": [P, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32), C.POINTER(I32), C.POINTER(I32)],
    "nof_dataset_render_view": [P, P, I32, P, I32, U32, C.POINTER(nof_view_out), C.POINTER(nof_view_metrics)],
    "nof_dataset_pose_grad": [P, I32, P, P, P, I32, P],
    "nof_dataset_batch_views": [P, I32, P, P],
    "nof_dataset_get_poses": [P, P],
    "nof_dataset_set_poses": [P, P],
    "nof_recenter_poses": [P, I32],
    "nof_dp_unique_id": [P],
    "nof_dp_init_rank": [P, I32, I32, I32, C.POINTER(P)],
    "nof_dp_init_rank_timeout": [P, I32, I32, I32, I32, C.POINTER(P)],
    "nof_dp_attach": [P, P, P],
    "nof_dp_wait": [P, I32],
    "nof_dp_step_end": [P, I32],
    "nof_dp_abort": [P],
    "nof_dp_init_all": [I32, C.POINTER(I32), C.POINTER(P)],
    "nof_dp_allreduce": [P, P, C.c_int64, P],
    "nof_dp_allreduce_grads": [P, P, P],
    "nof_dp_allreduce_grads_all": [I32, C.POINTER(P), C.POINTER(P), C.POINTER(P)],
    "nof_dp_destroy": [P],
    "nof_dp_init_loopback": [I32, I32, C.POINTER(P)],
    "nof_dp_train_step": [I32, C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P), I32, I32, U64, I32, F,
                          C.POINTER(F)],
    "nof_checkpoint_save": [C.c_char_p, P, P],
    "nof_checkpoint_load": [C.c_char_p, P, P],
    "nof_mipnerf_enable_timing": [P, I32],
    "nof_mipnerf_enable_timing_mask": [P, C.c_uint32],
    "nof_mipnerf_read_timing": [P, C.POINTER(F), C.POINTER(I32), I32],
    "nof_mlp_get_output": [P, P, P, I32, I32, I32, C.POINTER(U64), C.POINTER(U64)],
    "nof_mlp_get_gradient": [P, P, P, I32, C.POINTER(PP)],
    "nof_mlp_get_gradient_ex": [P, P, P, I32, U32, C.POINTER(PP)],
    "nof_mlp_params": [P, C.POINTER(PP)],
    "nof_mlp_grads": [P, C.POINTER(PP)],
    "nof_mlp_flat_params": [P, C.POINTER(P), C.POINTER(C.c_int64)],
    "nof_mlp_flat_grads": [P, C.POINTER(P), C.POINTER(C.c_int64)],
    "nof_mlp_layer_sizes": [P, C.POINTER(I32), I32, C.POINTER(I32)],
    "nof_mlp_debug_view": [P, I32, C.POINTER(nof_mlp_debug)],
    "nof_mlp_gen_dispatch": [P, I32, C.POINTER(U32), I32, C.POINTER(I32)],
    "nof_gen_dispatch_name": [I32, C.POINTER(C.c_char_p)],
    "nof_mlp_gen_dispatch_h": [P, I32, C.POINTER(U32), I32, C.POINTER(I32)],
    "nof_gen_dispatch_h_name": [I32, C.POINTER(C.c_char_p)],
    "nof_adam_create": [C.POINTER(I32), I32, C.POINTER(nof_config), C.POINTER(P)],
    "nof_adam_step": [P, PP, PP, F],
    "nof_adam_iteration": [P, C.POINTER(I32)],
    "nof_adam_destroy": [P],
    "nof_adam_set_options": [P, F, F, F, I32],
    "nof_adam_get_options": [P, C.POINTER(F), C.POINTER(F), C.POINTER(F), C.POINTER(I32)],
    "nof_adam_stats": [P, C.POINTER(nof_step_stats)],
    "nof_adam_moments": [P, C.POINTER(P), C.POINTER(P), C.POINTER(C.c_int64)],
    "nof_gradcalc_create": [I32, C.POINTER(nof_config), C.POINTER(P)],
    "nof_gradcalc_output_gradient": [P, U64, P, I32, U64, F, I32, C.POINTER(U64)],
    "nof_gradcalc_destroy": [P],
    "nof_retrieve_output": [U64, I32, P],
    "nof_lr_decay": [I32, F, F, I32, I32, F],
    "nof_device_count": [C.POINTER(I32)],
    "nof_set_device": [I32],
    "nof_malloc": [C.POINTER(P), C.c_size_t],
    "nof_free": [P],
    "nof_memcpy_h2d": [P, P, C.c_size_t],
    "nof_memcpy_d2h": [P, P, C.c_size_t],
    "nof_memcpy_d2d": [P, P, C.c_size_t, P],
    "nof_memset": [P, C.c_int, C.c_size_t],
    "nof_stream_sync": [P],
    "nof_kernel_sample_stratified": [I32, I32, P, P, I32, U64, U32, U32, U32, P, P],
    "nof_kernel_sample_stratified_ex": [I32, I32, P, P, I32, U64, U32, U32, U32, P, P, I32],
    "nof_kernel_sample_pdf": [I32, I32, P, P, I32, F, I32, U64, U32, U32, U32, P, P, P],
    "nof_kernel_cast": [I32, I32, P, P, P, P, P, P, P],
    "nof_kernel_cast_ex": [I32, I32, P, P, P, P, P, P, P, I32],
    "nof_kernel_cast_contract": [I32, I32, P, P, P, P, P, P, P, I32, I32],
    "nof_kernel_encode": [I32, I32, P, P, P, P, P, P],
    "nof_kernel_render": [I32, I32, P, P, P, P, I32, P, P, P],
    "nof_kernel_render_grad": [I32, I32, P, P, P, P, I32, P, P, P, P, F, F, P, P, P],
    "nof_kernel_render_grad_ex": [I32, I32, P, P, P, P, I32, P, P, P, P, F, F, P, P, P, P, P],
    "nof_kernel_render_grad_dist": [I32, I32, P, P, P, P, I32, P, P, P, P, F, F, P, P, P, P, P, P, I32, F, P, P],
    "nof_kernel_interlevel": [I32, I32, P, P, I32, P, P, P, F, F, I32, P, P, P],
    "nof_kernel_sample_pdf_grad": [I32, I32, P, P, I32, F, I32, U64, U32, U32, U32, P, P, P, P],
    "nof_kernel_encode_grad": [I32, I32, P, P, P, P, I32, I32, I32, P, P, P, P],
    "nof_kernel_ray_grad": [I32, I32, P, P, P, P, I32, I32, I32, P, P, P, P, I32, P, P, I32, P, P, P],
    "nof_kernel_encode_grad_ex": [I32, I32, P, P, P, P, I32, I32, I32, P, P, P, P, I32],
    "nof_kernel_ray_grad_ex": [I32, I32, P, P, P, P, I32, I32, I32, P, P, P, P, I32, P, P, I32, P, P, P, I32],
    "nof_kernel_adam": [C.c_int64, P, P, P, P, F, I32, P],
    "nof_kernel_gemm_h": [C.POINTER(nof_gemm_args), P],
    "nof_kernel_appearance_gather": [I32, I32, I32, I32, P, P, P, I32, P, P],
    "nof_kernel_appearance_grad": [I32, I32, I32, P, P, P, I32, P],
}
_RESTYPE = {"nof_config_default": None, "nof_last_error": C.c_char_p, "nof_version": C.c_char_p,
            "nof_config_size": C.c_size_t,
            "nof_lr_decay": C.c_float}

_lib = None


def lib():
    """Load libnof.so (raises if absent: the product never falls back to a CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"HIP extension missing: {LIB_PATH}. Build it with `python -c "
                               f"'import __graft_entry__ as g; g.build()'` or `make -C nerf-or-nothing_amd`.")
        # torch first when it is installed: its bundled libamdhip64 carries the soname
        # libamdhip64.so.7 that libnof.so needs, so the library binds to the HIP runtime already in
        # the process.  Loaded the other way round, torch's libraries (which name the file
        # libamdhip64.so) bring in a second HIP + HSA runtime, and whichever initialises second finds
        # no device.  Without torch (a C# / plain-ctypes host) libnof.so loads the system runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass

        L = C.CDLL(LIB_PATH)
        diag = bool(os.environ.get("NOF_LIB"))  # a diagnostic build of an older tree may lack newer entry points
        for name, args in SIGNATURES.items():
            if diag and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = _RESTYPE.get(name, C.c_int32)
        if diag and (not hasattr(L, "nof_config_size") or L.nof_config_size() < C.sizeof(nof_config)):
            pass  # an older build reads its own (shorter, prefix-identical) nof_config
        elif L.nof_config_size() != C.sizeof(nof_config):  # the struct this binding passes must be the library's
            raise RuntimeError(f"nof_config: the library expects {L.nof_config_size()} bytes, this binding "
                               f"passes {C.sizeof(nof_config)} (include/nof.h and nof/_lib.py disagree)")
        _lib = L
    return _lib


def check(status: int, where: str):
    if status != 0:
        msg = lib().nof_last_error()
        raise NofError(status, where, msg.decode() if msg else "")


def call(name: str, *args):
    st = getattr(lib(), name)(*args)
    check(st, name)
    return st


def default_config(**overrides) -> nof_config:
    cfg = nof_config()
    lib().nof_config_default(C.byref(cfg))
    for k, v in overrides.items():
        if k == "num_samples":
            for i, s in enumerate(v):
                cfg.num_samples[i] = s
            cfg.num_levels = len(v)
        else:
            setattr(cfg, k, v)
    return cfg
