"""Python mirror of the reference's host API (namespace AcceleratedNeRFUtils) over the C ABI.

Same class and method names as the C++/CLI classes the C# driver binds
(Program.cs:24-26,42,51-60): ``AcceleratedMipNeRF``, ``AcceleratedMLP``,
``AcceleratedAdamOptimizer``, ``AcceleratedGradientCalculator``, ``OutputRetriever``.
Device pointers cross this boundary as Python ints (the reference's uint64_t / float*),
exactly as they cross it in the reference; ``device_tensor`` wraps one in a torch view
(torch is used only for device memory and streams).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import call, lib

# include/nof.h NOF_STEP_FUSION_* (AcceleratedMipNeRF.set_step_fusion)
STEP_FUSION_BWD_PAIR = 1
STEP_FUSION_VIEW_TABLES = 2
STEP_FUSION_ALL = 3


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(x) -> int:
    """int device pointer from an int or a torch tensor."""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    return int(x.data_ptr())


def device_tensor(ptr: int, shape, dtype="float32", device=None):
    """Zero-copy torch view of library-owned device memory (borrowed: do not keep past the owner)."""
    import torch

    typestr = {"float32": "<f4", "int32": "<i4"}[dtype]
    n = int(np.prod(shape))

    class _View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 3}

    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.as_tensor(_View(), device=dev).view(*shape)


def to_numpy(ptr: int, shape, dtype=np.float32) -> np.ndarray:
    out = np.empty(shape, dtype)
    call("nof_memcpy_d2h", out.ctypes.data, C.c_void_p(ptr), out.nbytes)
    return out


def _ptr_list(pp, count) -> list[int]:
    return [C.cast(pp[i], C.c_void_p).value or 0 for i in range(count)]


def gen_dispatch_names() -> list[str]:
    """The any-shape path's kernel variants in the order of the dispatch tally (host only, no GPU)."""
    out, name = [], C.c_char_p()
    while lib().nof_gen_dispatch_name(len(out), C.byref(name)) == 0:
        out.append(name.value.decode())
    return out


def gen_dispatch_h_names() -> list[str]:
    """The fp16-product GEMM variants (NOF_PRECISION_F16_PRODUCTS, k_gemm_h) in the order of their tally."""
    out, name = [], C.c_char_p()
    while lib().nof_gen_dispatch_h_name(len(out), C.byref(name)) == 0:
        out.append(name.value.decode())
    return out


def kernel_gemm_h(stream=None, **fields) -> None:
    """One k_gemm_h product (include/nof.h nof_kernel_gemm_h).  fields: nof_gemm_args members; A1 / A2 / B1 / B2
    as (pointer or tensor, si, sk[, idiv]) tuples, the other pointers as device pointers or tensors."""
    a = L.nof_gemm_args()
    a.ksplit = 1
    for k, v in fields.items():
        if k in ("A1", "A2", "B1", "B2"):
            src = getattr(a, k)
            src.p, src.si, src.sk = _ptr(v[0]), int(v[1]), int(v[2])
            src.idiv = int(v[3]) if len(v) > 3 else 1
        elif k in ("bias", "G", "C", "rowsum", "scale_amax"):
            setattr(a, k, None if v is None else _ptr(v))
        else:
            setattr(a, k, int(v))
    call("nof_kernel_gemm_h", C.byref(a), stream)


def kernel_interlevel(n, samples_prop, t_prop, w_prop, samples_tgt, t_tgt, w_tgt, loss_mults, loss_mult_sum, mult,
                      w_grad, rays=None, accumulate=False, stream=None) -> None:
    """One k_interlevel launch (include/nof.h nof_kernel_interlevel): device pointers or tensors; w_grad
    [n, samples_prop] is overwritten, or added to with accumulate; rays ([n], optional) receives the per-ray term."""
    call("nof_kernel_interlevel", int(n), int(samples_prop), _ptr(t_prop), _ptr(w_prop), int(samples_tgt),
         _ptr(t_tgt), _ptr(w_tgt), _ptr(loss_mults), float(loss_mult_sum), float(mult), int(bool(accumulate)),
         _ptr(w_grad), _ptr(rays) or None, stream)


class AcceleratedMLP:
    """Borrowed view of the MLP owned by an AcceleratedMipNeRF (AcceleratedMLP.h:7-45)."""

    NUM_TENSORS = 22  # the reference network's [W0..W10, b0..b10]; any-shape networks: 2 (D + Dc + 2)

    def __init__(self, handle, owner):
        self._h = handle
        self._owner = owner  # keeps the owning AcceleratedMipNeRF alive
        self.num_tensors = len(self.get_layer_sizes())

    def get_layer_sizes(self) -> list[int]:
        out = (C.c_int32 * 64)()
        cnt = C.c_int32()
        call("nof_mlp_layer_sizes", self._h, out, 64, C.byref(cnt))
        return list(out[: cnt.value])

    def get_output(self, enc_pos, enc_dir, level: int, n_rays: int, samples: int):
        """MLPcpp:214-255 -> (density_ptr, rgb_ptr)."""
        d, r = C.c_uint64(), C.c_uint64()
        call("nof_mlp_get_output", self._h, _ptr(enc_pos), _ptr(enc_dir), level, n_rays, samples, C.byref(d),
             C.byref(r))
        return d.value, r.value

    def get_gradient(self, color_gradient, density_gradient, level: int, flags: int | None = None) -> list[int]:
        """MLPcpp:256-321 -> 2L device gradient pointers (22 for the reference network; flags: NOF_GRAD_* bits)."""
        pp = L.PP()
        if flags is None:
            call("nof_mlp_get_gradient", self._h, _ptr(color_gradient), _ptr(density_gradient), level, C.byref(pp))
        else:
            call("nof_mlp_get_gradient_ex", self._h, _ptr(color_gradient), _ptr(density_gradient), level, flags,
                 C.byref(pp))
        return _ptr_list(pp, self.num_tensors)

    @property
    def allParams(self) -> list[int]:
        pp = L.PP()
        call("nof_mlp_params", self._h, C.byref(pp))
        return _ptr_list(pp, self.num_tensors)

    @property
    def allGradients(self) -> list[int]:
        pp = L.PP()
        call("nof_mlp_grads", self._h, C.byref(pp))
        return _ptr_list(pp, self.num_tensors)

    def debug_view(self, level: int) -> dict:
        d = L.nof_mlp_debug()
        call("nof_mlp_debug_view", self._h, level, C.byref(d))
        return {k: getattr(d, k) for k in ("M", "act_in", "act_h", "act_h9", "masks", "zhead", "delta", "delta9x",
                                           "generic", "gen_h", "gen_hc")}

    def gen_dispatch(self, clear: bool = False) -> dict:
        """Launches per kernel variant of the any-shape path since creation or the last clear
        (name -> count, every variant listed; all zero for a fused network)."""
        names = gen_dispatch_names()
        counts = (C.c_uint32 * len(names))()
        n = C.c_int32()
        call("nof_mlp_gen_dispatch", self._h, int(bool(clear)), counts, len(names), C.byref(n))
        if n.value != len(names):
            raise RuntimeError(f"nof_mlp_gen_dispatch: {n.value} variants, {len(names)} names")
        return {k: int(counts[i]) for i, k in enumerate(names)}

    def gen_dispatch_h(self, clear: bool = False) -> dict:
        """gen_dispatch for the fp16-product GEMMs of NOF_PRECISION_F16_PRODUCTS (name -> count; all zero in
        every other mode)."""
        names = gen_dispatch_h_names()
        counts = (C.c_uint32 * len(names))()
        n = C.c_int32()
        call("nof_mlp_gen_dispatch_h", self._h, int(bool(clear)), counts, len(names), C.byref(n))
        if n.value != len(names):
            raise RuntimeError(f"nof_mlp_gen_dispatch_h: {n.value} variants, {len(names)} names")
        return {k: int(counts[i]) for i, k in enumerate(names)}

    def relu_masks(self, level: int) -> np.ndarray:
        """Decode the forward's packed ReLU bits -> uint8 [M, 8*256 + 128] (h0..h7, h9); any-shape
        networks: the stored activations > 0 -> [M, D*W + Dc*Wc] (the oracle's relu_mask order)."""
        dv = self.debug_view(level)
        M = dv["M"]
        if dv["generic"]:
            c = self._owner.config
            D, W, Dc, Wc = c.net_depth, c.net_width, c.net_depth_condition, c.net_width_condition
            h = to_numpy(dv["gen_h"], (D, M, W)).transpose(1, 0, 2).reshape(M, D * W)
            hc = to_numpy(dv["gen_hc"], (Dc, M, Wc)).transpose(1, 0, 2).reshape(M, Dc * Wc)
            return (np.concatenate([h, hc], axis=1) > 0).astype(np.uint8)
        nb = M // 32
        out = np.zeros((M, 8 * 256 + 128), np.uint8)
        if self._owner.config.precision == 4:  # F16 (mlp_h32.h): [lane][4 words], two 16-bit shift registers
            raw = to_numpy(dv["masks"], (nb, 9, 64, 4), np.uint32)
            lane = np.arange(64)
            x, h = lane & 31, lane >> 5
            rows = np.arange(nb)[:, None] * 32 + x[None, :]
            for slot in range(9):
                base = slot * 256
                for t in range(8 if slot < 8 else 4):
                    for r in range(16):
                        f = 32 * t + 8 * (r >> 2) + 4 * h + (r & 3)  # [64]
                        k = 8 * (t & 1) + (r >> 1)  # packed dword shifted in k-th: bit 15 - k of its half
                        bit = (raw[:, slot, :, t >> 1] >> np.uint32(16 * (r & 1) + 15 - k)) & np.uint32(1)
                        out[rows, base + f[None, :]] = bit.astype(np.uint8)
            return out
        if self._owner.config.precision in (0, 2, 3):  # 16x16 kernels (mlp16.h): [half][lane][uint2]
            raw = to_numpy(dv["masks"], (nb, 9, 2, 64, 2), np.uint32)
            lane = np.arange(64)
            j, g = lane & 15, lane >> 4
            for slot in range(9):
                base = slot * 256
                for t in range(16 if slot < 8 else 8):
                    for r in range(4):
                        f = 16 * t + 4 * g + r  # [64]
                        bit = (raw[:, slot, :, :, t >> 3] >> np.uint32(31 - ((t & 7) * 4 + r))) & np.uint32(1)
                        rows = np.arange(nb)[:, None, None] * 32 + 16 * np.arange(2)[None, :, None] + j[None, None, :]
                        out[rows, base + f[None, None, :]] = bit.astype(np.uint8)
            return out
        raw = to_numpy(dv["masks"], (nb, 9, 64, 4), np.uint32)
        lane = np.arange(64)
        j, h = lane & 31, lane >> 5
        for slot in range(9):
            ntile = 8 if slot < 8 else 4
            base = slot * 256
            for ot in range(ntile):
                for r in range(16):
                    f = ot * 32 + 8 * (r >> 2) + 4 * h + (r & 3)  # [64]
                    bit = (raw[:, slot, :, ot >> 1] >> np.uint32(31 - ((ot & 1) * 16 + r))) & np.uint32(1)  # [nb, 64]
                    rows = (np.arange(nb)[:, None] * 32 + j[None, :])
                    out[rows, base + f[None, :]] = bit.astype(np.uint8)
        return out

    def flat_params(self):
        p, n = C.c_void_p(), C.c_int64()
        call("nof_mlp_flat_params", self._h, C.byref(p), C.byref(n))
        return p.value, n.value

    def flat_grads(self):
        p, n = C.c_void_p(), C.c_int64()
        call("nof_mlp_flat_grads", self._h, C.byref(p), C.byref(n))
        return p.value, n.value


class AcceleratedMipNeRF:
    """AcceleratedMipNeRF.h:10-41 (ctor MNcpp:7-50, GetGradient MNcpp:52-144)."""

    def __init__(self, config: L.nof_config | None = None, appearance_views: int = 0, appearance_dim: int = 0,
                 **overrides):
        """appearance_views = V, appearance_dim = G > 0: per-view appearance embeddings (include/nof.h
        nof_mipnerf_create_ex): a zero-initialised table [V, G] outside the parameter arena, one row per training
        image, feeds the view layer; any-shape path only (a fused 8x256 model raises NofError(NOF_ERR_UNSUPPORTED))."""
        self.config = config if config is not None else L.default_config(**overrides)
        self._hook_errors = []
        self._bucket_cb = None
        h = C.c_void_p()
        if appearance_views or appearance_dim:
            ext = L.nof_model_ext(C.sizeof(L.nof_model_ext), int(appearance_views), int(appearance_dim))
            call("nof_mipnerf_create_ex", C.byref(self.config), C.byref(ext), C.byref(h))
        else:
            call("nof_mipnerf_create", C.byref(self.config), C.byref(h))
        self._h = h
        m = C.c_void_p()
        call("nof_mipnerf_mlp", self._h, C.byref(m))
        self.mlp = AcceleratedMLP(m, self)

    def close(self):
        if getattr(self, "_h", None):
            lib().nof_mipnerf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def GetGradient(self, origins, directions, radii, nears, fars, loss_multipliers, get_output_gradient):
        """Host arrays + callback(dev_comp_rgb, level, loss_mult_sum, dev_loss_mults) -> dev dL/dC ptr."""
        arrs = [_f32(a) for a in (origins, directions, radii, nears, fars, loss_multipliers)]
        n = arrs[2].shape[0]
        err = []

        def tramp(user, comp, level, msum, lm):
            try:
                return int(get_output_gradient(comp, level, msum, lm))
            except Exception as e:  # never unwind through C
                err.append(e)
                return 0

        cb = L.OUTPUT_GRAD_FN(tramp)
        pp = L.PP()
        st = lib().nof_mipnerf_get_gradient(self._h, n, *[a.ctypes.data for a in arrs], cb, None, C.byref(pp))
        if err:
            raise err[0]
        L.check(st, "nof_mipnerf_get_gradient")
        return _ptr_list(pp, self.mlp.num_tensors)

    def get_gradient_device(self, n, origins, directions, radii, nears, fars, loss_mults, pixels, loss_mult_sum,
                            accumulate: bool = False, publish: bool = True):
        """All inputs device-resident (ints or torch tensors); loss gradient fused into the integrator.
        accumulate: add onto the gradient arena (micro-batching); publish: this call completes the
        step's gradient (fires the bucket hook, if one is set)."""
        pp = L.PP()
        self._hook_errors = []
        args = (self._h, n, _ptr(origins), _ptr(directions), _ptr(radii), _ptr(nears), _ptr(fars), _ptr(loss_mults),
                _ptr(pixels), float(loss_mult_sum))
        if not accumulate and publish:
            st = lib().nof_mipnerf_get_gradient_device(*args, C.byref(pp))
        else:
            flags = (L.NOF_GRAD_ACCUMULATE if accumulate else 0) | (L.NOF_GRAD_PUBLISH if publish else 0)
            st = lib().nof_mipnerf_get_gradient_device_ex(*args, flags, C.byref(pp))
        if self._hook_errors:
            raise self._hook_errors[0]
        L.check(st, "nof_mipnerf_get_gradient_device")
        return _ptr_list(pp, self.mlp.num_tensors)

    def set_grad_buckets(self, fn):
        """fn(bucket, [(offset, count), ...]) is called during every publishing get_gradient call once
        the bucket's gradient values are enqueued on the model's stream (include/nof.h); None removes it."""
        if fn is None:
            self._bucket_cb = None
            call("nof_mipnerf_set_grad_buckets", self._h, L.GRAD_BUCKET_FN(), None)
            return

        def tramp(user, bucket, nspans, offs, cnts):
            try:
                fn(int(bucket), [(int(offs[i]), int(cnts[i])) for i in range(nspans)])
            except Exception as e:  # never unwind through C; re-raised after the call
                self._hook_errors.append(e)

        self._bucket_cb = L.GRAD_BUCKET_FN(tramp)  # keep the thunk alive while installed
        call("nof_mipnerf_set_grad_buckets", self._h, self._bucket_cb, None)

    def GetLayerSizes(self) -> list[int]:
        out = (C.c_int32 * 64)()
        cnt = C.c_int32()
        call("nof_mipnerf_layer_sizes", self._h, out, 64, C.byref(cnt))
        return list(out[: cnt.value])

    def set_rng(self, seed: int, step: int, ray_base: int = 0):
        call("nof_mipnerf_set_rng", self._h, seed, step, ray_base)

    def get_rng(self):
        s, st, rb = C.c_uint64(), C.c_uint32(), C.c_uint32()
        call("nof_mipnerf_get_rng", self._h, C.byref(s), C.byref(st), C.byref(rb))
        return s.value, st.value, rb.value

    def level_view(self, level: int) -> dict:
        v = L.nof_level_view()
        call("nof_mipnerf_level_view", self._h, level, C.byref(v))
        n, S = v.n, v.samples
        shapes = {"t": (n, S + 1), "weights": (n, S), "comp_rgb": (n, 3), "density": (n, S), "rgb": (n, S, 3),
                  "density_grad": (n, S), "rgb_grad": (n, S, 3)}
        return {k: (getattr(v, k), shp) for k, shp in shapes.items()}

    def level_numpy(self, level: int) -> dict:
        return {k: to_numpy(p, shp) for k, (p, shp) in self.level_view(level).items()}

    def cross_numpy(self, level: int) -> dict:
        """stop_level_grad = 0: the last step's cross-level terms of `level` (include/nof.h
        nof_mipnerf_cross_view): "w_grad" [n, S] = dL/dw from the next level's resampler, "t_grad" [n, S + 1] =
        dL/dt; None where the level has none (the last level / level 0, or stop_level_grad = 1).  With
        set_interlevel_loss(mult > 0) "w_grad" also holds that loss's dL/dw, at either stop_level_grad."""
        v = L.nof_level_view()
        call("nof_mipnerf_level_view", self._h, level, C.byref(v))
        q, dt = C.c_void_p(), C.c_void_p()
        call("nof_mipnerf_cross_view", self._h, level, C.byref(q), C.byref(dt))
        return {"w_grad": to_numpy(q.value, (v.n, v.samples)) if q.value else None,
                "t_grad": to_numpy(dt.value, (v.n, v.samples + 1)) if dt.value else None}

    def set_ray_grad(self, on: bool = True) -> None:
        """Every later step also leaves dL/d origins, dL/d directions of its rays (include/nof.h
        nof_mipnerf_set_ray_grad; any-shape path only: a fused 8x256 model raises NofError(NOF_ERR_UNSUPPORTED))."""
        call("nof_mipnerf_set_ray_grad", self._h, int(bool(on)))

    def ray_grad(self):
        """The last step's (dL/do, dL/dd) as borrowed device pointers, each [n, 3] (to_numpy / device_tensor)."""
        o, d = C.c_void_p(), C.c_void_p()
        call("nof_mipnerf_ray_grad", self._h, C.byref(o), C.byref(d))
        return o.value, d.value

    def loss(self) -> float:
        out = C.c_float()
        call("nof_mipnerf_loss", self._h, C.byref(out))
        return out.value

    def distortion_loss(self) -> float:
        """The distortion term of the last gradient step, lambda_d sum_r mu_r L_r / sum mu (the model's
        distortion_loss_mult= keyword, include/nof.h nof_config.distortion_loss_mult); 0.0 with the option off.
        loss() stays the photometric loss."""
        out = C.c_float()
        call("nof_mipnerf_distortion_loss", self._h, C.byref(out))
        return out.value

    def set_interlevel_loss(self, mult: float) -> None:
        """The interlevel (proposal) loss of mip-NeRF 360 times `mult` on every level but the last, whose (t, w) is
        the stop-gradient target (include/nof.h nof_mipnerf_set_interlevel_loss); 0 switches it off.  Every
        precision mode and both settings of stop_level_grad."""
        call("nof_mipnerf_set_interlevel_loss", self._h, float(mult))

    def interlevel_loss(self) -> float:
        """The interlevel term of the last gradient step, summed over the coarser levels and the rays; 0.0 with the
        option off.  loss() stays the photometric loss."""
        out = C.c_float()
        call("nof_mipnerf_interlevel_loss", self._h, C.byref(out))
        return out.value

    def set_contraction(self, mode=1) -> None:
        """Scene contraction for unbounded scenes (include/nof.h nof_mipnerf_set_contraction): 1 / True
        (NOF_CONTRACT_SPHERE) maps every sample's Gaussian into the ball of radius 2 before it is encoded, in the
        training step, render_device and RayDataset.render_view; 0 / False switches it off.  Cameras are expected
        inside the unit ball.  A hyper-parameter (checkpoints do not hold it); any-shape path only: a fused 8x256
        model raises NofError(NOF_ERR_UNSUPPORTED)."""
        call("nof_mipnerf_set_contraction", self._h, int(mode))

    def set_step_fusion(self, flags: int = STEP_FUSION_ALL) -> None:
        """Diagnostic (include/nof.h nof_mipnerf_set_step_fusion): STEP_FUSION_* bit flags, all on by default;
        a cleared bit runs that part of the fused 8x256 training step the unfused way.  Results are bit for bit
        the same at every setting."""
        call("nof_mipnerf_set_step_fusion", self._h, int(flags))

    def contraction(self) -> int:
        """The contraction mode in force (0 = none, 1 = sphere)."""
        out = C.c_int32()
        call("nof_mipnerf_get_contraction", self._h, C.byref(out))
        return out.value

    def appearance(self):
        """(table_ptr, grad_ptr, V, G): borrowed device pointers to the appearance table E and its gradient dE, each
        [V, G] (to_numpy / device_tensor).  The caller owns the update: an AcceleratedAdamOptimizer([V * G]) steps
        ([table_ptr], [grad_ptr]).  A model without appearance raises NofError(NOF_ERR_INVALID_ARG)."""
        t, g, V, G = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
        call("nof_mipnerf_appearance", self._h, C.byref(t), C.byref(g), C.byref(V), C.byref(G))
        return t.value, g.value, V.value, G.value

    def set_ray_views(self, view_ids) -> None:
        """The view ids ([n] int32, a device pointer or tensor the caller keeps alive) of the rays of the next
        gradient step or render_device; that call resets them (None clears them now)."""
        call("nof_mipnerf_set_ray_views", self._h, _ptr(view_ids) or None)

    def set_render_appearance(self, view: int = -1) -> None:
        """The view whose embedding calls without per-ray ids use (render_device without ids,
        RayDataset.render_view, AcceleratedMLP.get_output); -1 (the default): the zero vector."""
        call("nof_mipnerf_set_render_appearance", self._h, int(view))

    def numeric_status(self, clear: bool = True) -> int:
        """NOF_NUMERIC_* bits (non-finite forward outputs / output gradients) since the last clear."""
        out = C.c_uint32()
        call("nof_mipnerf_numeric_status", self._h, C.byref(out), int(clear))
        return out.value

    def render_device(self, n, origins, directions, radii, nears, fars, randomized=False, white_bkgd=None):
        """MipNerfModel.Call (MNcs:36-97): forward-only two-level render of device-resident rays.
        Returns [{"comp_rgb": (ptr, (n, 3)), "distance": (ptr, (n,)), "acc": (ptr, (n,))}] per level."""
        out = L.nof_render_out()
        white = self.config.white_bkgd if white_bkgd is None else int(white_bkgd)
        call("nof_mipnerf_render_device", self._h, n, _ptr(origins), _ptr(directions), _ptr(radii), _ptr(nears),
             _ptr(fars), int(randomized), white, C.byref(out))
        return [{"comp_rgb": (out.comp_rgb[l], (n, 3)), "distance": (out.distance[l], (n,)),
                 "acc": (out.acc[l], (n,))} for l in range(out.num_levels)]

    def render_rays(self, rays: dict, randomized=False, chunk=None, device=None) -> list[dict]:
        """Render host rays (synth/record dict of numpy arrays) in chunks of max_rays; numpy results
        per level: comp_rgb [N, 3], distance [N], acc [N]."""
        import torch

        dev = device or torch.device("cuda", self.config.device)
        N = rays["o"].shape[0]
        chunk = min(chunk or self.config.max_rays, self.config.max_rays)
        keys = ("o", "d", "radius", "near", "far")
        outs = None
        for b in range(0, N, chunk):
            e = min(N, b + chunk)
            t = {k: torch.from_numpy(np.ascontiguousarray(rays[k][b:e], dtype=np.float32)).to(dev) for k in keys}
            lv = self.render_device(e - b, t["o"], t["d"], t["radius"], t["near"], t["far"], randomized)
            torch.cuda.synchronize(dev)
            res = [{k: to_numpy(p, shp) for k, (p, shp) in L_.items()} for L_ in lv]
            if outs is None:
                outs = [{k: [] for k in r} for r in res]
            for o, r in zip(outs, res):
                for k, v in r.items():
                    o[k].append(v)
        return [{k: np.concatenate(v) for k, v in o.items()} for o in outs]

    def enable_timing(self, on: bool = True, timers=None):
        """hipEvent timing of every kernel class, or only of the named ones (L.TIMER_NAMES)."""
        if timers is None:
            call("nof_mipnerf_enable_timing", self._h, int(on))
        else:
            mask = sum(1 << L.TIMER_NAMES.index(t) for t in timers) if on else 0
            call("nof_mipnerf_enable_timing_mask", self._h, C.c_uint32(mask))

    def read_timing(self) -> dict:
        ms = (C.c_float * L.NOF_NUM_TIMERS)()
        cnt = (C.c_int32 * L.NOF_NUM_TIMERS)()
        call("nof_mipnerf_read_timing", self._h, ms, cnt, L.NOF_NUM_TIMERS)
        return {name: (ms[i], cnt[i]) for i, name in enumerate(L.TIMER_NAMES)}


class AcceleratedAdamOptimizer:
    """AcceleratedAdamOptimizer.h:5-20; step = one fused launch over flat arenas.

    grad_max_norm, grad_max_val, weight_decay_mult (Config.GradMaxNorm / GradMaxVal / WeightDecayMult,
    TrainState.cs:58-59,70; 0 = off) and stats (gather the step statistics alone): include/nof.h
    nof_adam_set_options.  With any of them set a step gathers the record that stats() returns."""

    def __init__(self, layer_sizes, config: L.nof_config | None = None, grad_max_norm: float = 0.0,
                 grad_max_val: float = 0.0, weight_decay_mult: float = 0.0, stats: bool = False):
        self.config = config if config is not None else L.default_config()
        arr = (C.c_int32 * len(layer_sizes))(*layer_sizes)
        self.n = len(layer_sizes)
        h = C.c_void_p()
        call("nof_adam_create", arr, len(layer_sizes), C.byref(self.config), C.byref(h))
        self._h = h
        if grad_max_norm or grad_max_val or weight_decay_mult or stats:  # a NaN is truthy: refused below
            self.set_options(grad_max_norm, grad_max_val, weight_decay_mult, stats)

    def set_options(self, grad_max_norm: float = 0.0, grad_max_val: float = 0.0, weight_decay_mult: float = 0.0,
                    stats: bool = False):
        """Negative or NaN values raise NofError (NOF_ERR_INVALID_ARG) and leave the options as they were."""
        call("nof_adam_set_options", self._h, float(grad_max_norm), float(grad_max_val), float(weight_decay_mult),
             int(bool(stats)))

    def get_options(self) -> dict:
        n, v, w, s = C.c_float(), C.c_float(), C.c_float(), C.c_int32()
        call("nof_adam_get_options", self._h, C.byref(n), C.byref(v), C.byref(w), C.byref(s))
        return {"grad_max_norm": n.value, "grad_max_val": v.value, "weight_decay_mult": w.value,
                "stats": bool(s.value)}

    def stats(self) -> dict:
        """The last step's record (StatsUtil.cs:13,16-18 + clip_scale, iteration); synchronises the stream.
        NofError when no step has gathered statistics."""
        st = L.nof_step_stats()
        call("nof_adam_stats", self._h, C.byref(st))
        return {k: getattr(st, k) for k, _ in L.nof_step_stats._fields_}

    def step(self, params, grads, learning_rate: float):
        pa = (C.POINTER(C.c_float) * self.n)(*[C.cast(C.c_void_p(p), C.POINTER(C.c_float)) for p in params])
        ga = (C.POINTER(C.c_float) * self.n)(*[C.cast(C.c_void_p(g), C.POINTER(C.c_float)) for g in grads])
        call("nof_adam_step", self._h, pa, ga, float(learning_rate))

    def moments(self):
        """(m_ptr, v_ptr, count): the first and second moments, device pointers borrowed from the optimizer."""
        m, v, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        call("nof_adam_moments", self._h, C.byref(m), C.byref(v), C.byref(n))
        return m.value or 0, v.value or 0, n.value

    @property
    def iteration(self) -> int:
        it = C.c_int32()
        call("nof_adam_iteration", self._h, C.byref(it))
        return it.value

    def close(self):
        if getattr(self, "_h", None):
            lib().nof_adam_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AcceleratedGradientCalculator:
    """AcceleratedGradientCalculator.h:8-17 (D15 fixed: pixels uploaded, one buffer per level)."""

    def __init__(self, batch_size: int, config: L.nof_config | None = None):
        self.config = config if config is not None else L.default_config()
        h = C.c_void_p()
        call("nof_gradcalc_create", batch_size, C.byref(self.config), C.byref(h))
        self._h = h

    def get_output_gradient(self, input_ptr, pixels, loss_mults, loss_mult_sum: float, level: int) -> int:
        px = _f32(pixels)
        out = C.c_uint64()
        call("nof_gradcalc_output_gradient", self._h, _ptr(input_ptr), px.ctypes.data, px.shape[0], _ptr(loss_mults),
             float(loss_mult_sum), level, C.byref(out))
        return out.value

    def close(self):
        if getattr(self, "_h", None):
            lib().nof_gradcalc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OutputRetriever:
    @staticmethod
    def RetrieveOutput(dev_output: int, size: int) -> np.ndarray:
        """OutputRetriever.cpp:6-14 -> float32 [size, 3]."""
        out = np.empty((size, 3), np.float32)
        call("nof_retrieve_output", C.c_uint64(dev_output), size, out.ctypes.data)
        return out


class RayDataset:
    """BinDataset (BinDataset.cs:10-53) resident in HBM: 64-byte records, batches gathered on the
    device with Philox-drawn record indices (with replacement)."""

    FIELDS = {"o": ("origins", 3), "d": ("directions", 3), "viewdir": ("viewdirs", 3), "radius": ("radii", 1),
              "near": ("nears", 1), "far": ("fars", 1), "lossmult": ("loss_mults", 1), "pix": ("pixels", 3)}

    def __init__(self, path=None, records=None, device: int = 0, generate: dict | None = None,
                 max_resident: int | None = None, scene: dict | None = None):
        """path: record file (max_resident: HBM-resident iff at most that many records, else streamed
        from the file per batch); records: host [N, 16] array; generate: dict(poses [V, 12], width,
        height, focal, near, far, ndc=False, images=device tensor [V, H, W, 3] or None) -> rays made on
        the GPU; scene: the same dict plus num_scales=1 and multiscale_loss=True -> image-backed: poses
        and an image pyramid stay in HBM and each batch's rays are made in its gather, at num_scales
        resolutions (multiscale_layout)."""
        h = C.c_void_p()
        if scene is not None:
            g = dict(scene)
            poses = np.ascontiguousarray(g["poses"], dtype=np.float32).reshape(-1, 12)
            img = g.get("images")
            call("nof_dataset_from_images", poses.ctypes.data, poses.shape[0], int(g["width"]), int(g["height"]),
                 float(g["focal"]), float(g["near"]), float(g["far"]), int(bool(g.get("ndc", False))),
                 _ptr(img) if img is not None else None, int(g.get("num_scales", 1)),
                 int(not g.get("multiscale_loss", True)), device, C.byref(h))
        elif generate is not None:
            g = dict(generate)
            poses = np.ascontiguousarray(g["poses"], dtype=np.float32).reshape(-1, 12)
            img = g.get("images")
            call("nof_dataset_generate", poses.ctypes.data, poses.shape[0], int(g["width"]), int(g["height"]),
                 float(g["focal"]), float(g["near"]), float(g["far"]), int(bool(g.get("ndc", False))),
                 _ptr(img) if img is not None else None, device, C.byref(h))
        elif path is not None and max_resident is not None:
            call("nof_dataset_open_streaming", str(path).encode(), device, int(max_resident), C.byref(h))
        elif path is not None:
            call("nof_dataset_open", str(path).encode(), device, C.byref(h))
        else:
            rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 16)
            call("nof_dataset_from_host", rec.ctypes.data, rec.shape[0], device, C.byref(h))
        self._h = h
        self._device = device

    def __len__(self):
        n = C.c_int64()
        call("nof_dataset_count", self._h, C.byref(n))
        return n.value

    @property
    def streaming(self) -> bool:
        s = C.c_int32()
        call("nof_dataset_is_streaming", self._h, C.byref(s))
        return bool(s.value)

    def next(self, n: int, seed: int, step: int, ray_base: int = 0, stream=None, with_sum: bool = True):
        """Device SoA batch {key: (ptr, shape)} (+ 'record_index') and the loss-mult sum (or None)."""
        b = L.nof_batch()
        msum = C.c_float()
        call("nof_dataset_next", self._h, n, seed, step, ray_base, stream, C.byref(b),
             C.byref(msum) if with_sum else None)
        out = {k: (getattr(b, f), (n, w) if w > 1 else (n,)) for k, (f, w) in self.FIELDS.items()}
        out["record_index"] = (b.record_index, (n,))
        return out, (msum.value if with_sum else None)

    def materialize(self, stream=None):
        """Every record in order -> device tensor [count, 16] (torch): generated for an image-backed
        dataset, copied for a resident one; a streaming dataset raises NofError(NOF_ERR_UNSUPPORTED)."""
        import torch

        out = torch.empty((len(self), 16), dtype=torch.float32, device=torch.device("cuda", self._device))
        call("nof_dataset_materialize", self._h, out.data_ptr(), stream)
        torch.cuda.synchronize(self._device)
        return out

    def scene_info(self) -> dict:
        """An image-backed dataset's shape: num_views, num_scales, width / height per scale, has_images
        (any other dataset raises NofError(NOF_ERR_UNSUPPORTED))."""
        V, S, has = C.c_int32(), C.c_int32(), C.c_int32()
        w, h = (C.c_int32 * 4)(), (C.c_int32 * 4)()
        call("nof_dataset_scene_info", self._h, C.byref(V), C.byref(S), w, h, C.byref(has))
        return dict(num_views=V.value, num_scales=S.value, width=list(w[: S.value]), height=list(h[: S.value]),
                    has_images=bool(has.value))

    def render_view(self, model: "AcceleratedMipNeRF", view=None, pose=None, scale: int = 0, ssim: bool = True,
                    score=None, outputs=None) -> dict:
        """One whole view at `scale`, rendered on the device in chunks of the model's max_rays (include/nof.h
        nof_dataset_render_view): view = a view of the scene, or pose = 12 floats (rotation row-major, then
        translation) for a novel one.  Returns torch device tensors {"rgb": [per level [H, W, 3]],
        "distance": [H, W], "acc": [H, W]} (last level), enqueued on the model's stream; outputs: None = all of
        them, else the names to produce among "rgb" (every level), "rgb<level>", "distance", "acc" (the others
        are None).  score (default: a view of a scene with images) adds "mse", "psnr" (per level against the
        image the dataset keeps) and "ssim" (last level; None unless ssim), and synchronises."""
        import torch

        if (view is None) == (pose is None):
            raise ValueError("render_view takes a view or a pose")
        info = self.scene_info()
        if score is None:
            score = pose is None and info["has_images"]
        ok = 0 <= scale < info["num_scales"]  # a scale out of range: empty buffers, the library refuses the call
        W, H, L_ = info["width"][scale] if ok else 0, info["height"][scale] if ok else 0, model.config.num_levels
        dev = torch.device("cuda", self._device)
        want = None if outputs is None else set(outputs)

        def buf(name, shape, level=None):
            if want is not None and name not in want and (level is None or f"{name}{level}" not in want):
                return None
            return torch.empty(shape, dtype=torch.float32, device=dev)

        res = {"rgb": [buf("rgb", (H, W, 3), l) for l in range(L_)], "distance": buf("distance", (H, W)),
               "acc": buf("acc", (H, W)), "width": W, "height": H}
        out = L.nof_view_out()
        for l, t in enumerate(res["rgb"]):
            out.rgb[l] = _ptr(t) or None
        out.distance, out.acc = _ptr(res["distance"]) or None, _ptr(res["acc"]) or None
        host_pose = None
        if pose is not None:
            host_pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(12)
        m = L.nof_view_metrics()
        call("nof_dataset_render_view", self._h, model._h, -1 if view is None else int(view),
             host_pose.ctypes.data if host_pose is not None else None, int(scale),
             L.NOF_VIEW_SSIM if (score and ssim) else 0, C.byref(out), C.byref(m) if score else None)
        if score:
            res.update(mse=list(m.mse[:L_]), psnr=list(m.psnr[:L_]), ssim=m.ssim if ssim else None)
        return res

    def pose_grad(self, o_grad, d_grad, n: int, out=None, accumulate: bool = False, stream=None):
        """Camera refinement (include/nof.h nof_dataset_pose_grad): the gradients [n, 3] of the LAST next() batch's
        rays (AcceleratedMipNeRF.ray_grad()) summed per view -> torch device tensor [V, 12] (rotation row-major,
        then translation), enqueued on `stream`; out: a tensor to write (accumulate: to add to).  An NDC scene or a
        record dataset raises NofError(NOF_ERR_UNSUPPORTED)."""
        import torch

        if out is None:
            if accumulate:
                raise ValueError("accumulate needs the tensor to add to (out)")
            out = torch.zeros((self.scene_info()["num_views"], 12), dtype=torch.float32,
                              device=torch.device("cuda", self._device))
        call("nof_dataset_pose_grad", self._h, int(n), _ptr(o_grad), _ptr(d_grad), out.data_ptr(), int(accumulate),
             stream)
        return out

    def batch_views(self, n: int, out=None, stream=None):
        """The view of every ray of the LAST next() batch -> torch device tensor [n] int32 (include/nof.h
        nof_dataset_batch_views), enqueued on `stream`: the ids AcceleratedMipNeRF.set_ray_views takes.  A record
        dataset raises NofError(NOF_ERR_UNSUPPORTED)."""
        import torch

        if out is None:
            out = torch.empty((int(n),), dtype=torch.int32, device=torch.device("cuda", self._device))
        call("nof_dataset_batch_views", self._h, int(n), out.data_ptr(), stream)
        return out

    def poses(self) -> np.ndarray:
        """The image-backed dataset's pose table [V, 12] (host copy)."""
        P = np.empty((self.scene_info()["num_views"], 12), np.float32)
        call("nof_dataset_get_poses", self._h, P.ctypes.data)
        return P

    def set_poses(self, P) -> None:
        """Replace the pose table ([V, 12]: rotation row-major, then translation): the next batch and render_view use it."""
        P = np.ascontiguousarray(P, dtype=np.float32)
        if P.size != 12 * self.scene_info()["num_views"]:
            raise ValueError("set_poses takes every view's pose: [V, 12]")
        call("nof_dataset_set_poses", self._h, P.ctypes.data)

    def close(self):
        if getattr(self, "_h", None):
            lib().nof_dataset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def generate_rays(poses, width, height, focal, near, far, ndc=False, images=None, out=None, stream=None):
    """Dataset.GenerateRays on the GPU -> device records tensor [V*H*W, 16] (torch)."""
    import torch

    poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 12)
    n = poses.shape[0] * int(width) * int(height)
    if out is None:
        out = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    call("nof_generate_rays", poses.ctypes.data, poses.shape[0], int(width), int(height), float(focal), float(near),
         float(far), int(bool(ndc)), _ptr(images) if images is not None else None, out.data_ptr(), stream)
    return out


def multiscale_layout(width, height, focal, num_scales=1, multiscale_loss=True, num_views=1) -> dict:
    """The record layout of a multiscale scene (host only): per scale the width, height, focal length,
    loss multiplier and first record, and the record count.  scale, view, y, x of record i:
    s = the last scale with first[s] <= i, then divmod of i - first[s] by width[s] * height[s] and width[s]."""
    S = int(num_scales)
    w, h, first = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_int64 * 4)()
    f, lm, count = (C.c_float * 4)(), (C.c_float * 4)(), C.c_int64()
    call("nof_multiscale_layout", int(width), int(height), float(focal), S, int(not multiscale_loss), int(num_views),
         w, h, f, lm, first, C.byref(count))
    return dict(width=list(w[:S]), height=list(h[:S]), focal=list(f[:S]), lossmult=list(lm[:S]),
                first=list(first[:S]), count=count.value)


def recenter_poses(poses) -> np.ndarray:
    """LLFFDataset.RecenterPoses (Dataset.cs:309-319) on host poses [V, 12] (returns a copy)."""
    p = np.array(poses, dtype=np.float32).reshape(-1, 12).copy()
    call("nof_recenter_poses", p.ctypes.data, p.shape[0])
    return p


def save_checkpoint(path, model: "AcceleratedMipNeRF", adam: "AcceleratedAdamOptimizer"):
    """Parameters, Adam moments/step and Philox state -> checksummed file (atomic rename)."""
    call("nof_checkpoint_save", str(path).encode(), model._h, adam._h)


def load_checkpoint(path, model: "AcceleratedMipNeRF", adam: "AcceleratedAdamOptimizer"):
    call("nof_checkpoint_load", str(path).encode(), model._h, adam._h)


def image_metrics(img0, img1, max_val=1.0, stream=None) -> tuple[float, float]:
    """(PSNR, SSIM) of two [H, W, 3] images on the GPU (MipHelpers.cs:672, 685-736).  Accepts
    device tensors, or numpy arrays (copied to the current device)."""
    import torch

    def dev(x):
        if isinstance(x, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        return x.contiguous()

    a, b = dev(img0), dev(img1)
    H, W = int(a.shape[0]), int(a.shape[1])
    assert tuple(a.shape) == (H, W, 3) and tuple(b.shape) == (H, W, 3), "images must be [H, W, 3]"
    psnr, ssim = C.c_float(), C.c_float()
    call("nof_image_metrics", a.data_ptr(), b.data_ptr(), W, H, float(max_val), C.byref(psnr), C.byref(ssim),
         stream)
    return psnr.value, ssim.value


def device_checks(clear: bool = True) -> int:
    """NOF_CHECK_* bits failed inside the kernels on the current device since the last clear
    (synchronises).  Only a checked build (lib/libnof_check.so, `make check`, selected with NOF_LIB)
    has the checks; the product library raises NofError(NOF_ERR_UNSUPPORTED)."""
    out = C.c_uint32()
    call("nof_device_checks", C.byref(out), int(clear))
    return out.value


def device_checks_selftest() -> None:
    """Fail NOF_CHECK_SELFTEST on purpose (checked build only)."""
    call("nof_device_checks_selftest")


def learning_rate_decay(step, lr_init=5e-4, lr_final=5e-6, max_steps=1000000, lr_delay_steps=2500,
                        lr_delay_mult=0.01) -> float:
    """MathHelpers.LearningRateDecay (MipHelpers.cs:758-773); defaults = TrainState.cs:54-58."""
    return float(lib().nof_lr_decay(step, lr_init, lr_final, max_steps, lr_delay_steps, lr_delay_mult))


def grad_bucket_spans(layer_sizes, bucket: int) -> list[tuple[int, int]]:
    """(offset, count) spans of the flat gradient arena that gradient bucket `bucket` covers."""
    sz = (C.c_int32 * len(layer_sizes))(*layer_sizes)
    off, cnt, ns = (C.c_int64 * 4)(), (C.c_int64 * 4)(), C.c_int32()
    call("nof_grad_bucket_spans", bucket, sz, len(layer_sizes), off, cnt, C.byref(ns))
    return [(off[i], cnt[i]) for i in range(ns.value)]


def device_count() -> int:
    c = C.c_int32()
    call("nof_device_count", C.byref(c))
    return c.value
