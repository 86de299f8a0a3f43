"""GPU parity of the per-view appearance embeddings (nof_mipnerf_create_ex) against the fp64 autograd
reference tests/appearance_ref.py (pinned by finite differences in tests/test_appearance_cpu.py).

Bounds.  Gather kernel: bitwise the numpy concatenation.  Gradient kernel: against the fp64 sum of the same fp32 terms,
(n - 1) 2^-24 sum |terms| per element (n - 1 fp32 additions, each within half an ulp of a partial sum no larger than
sum |terms|); an empty view exactly 0.  Whole step, F32: every parameter gradient tensor, dE, (stop_level_grad = 0)
dL/dt of the levels above 0 and, with ray gradients, dL/do and dL/dd <= max(1e-5, 4 x e_off), e_off the worst
parameter-gradient tensor error of the same shape, rays and seeds with G = 0 against the existing reference
(tests/contraction_ref.py), the floor DESIGN.md 6i uses.  F16_PRODUCTS (ReLU decisions adopted): max(2e-3, 4 x e_off).
DESIGN.md 6j has the measured figures.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_l2
from test_appearance_cpu import CONTRACTED_CASE, RAY_SEED, VIEWS, table, view_ids
from test_gpu_crosslevel import RAY_BASE, REF8, SEED, STEP, TINY, _dev, _gpu_index, _grads, _model, _params, _step
from test_gpu_raygrad import DS_SEED, DS_STEP, FOCAL, H, NP, SCALES, V, W, _batch, _ray_grads, _scene
from test_raygen import _poses

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-or-nothing_amd")
TOL = 1e-5
F16P_TOL = 2e-3
f32 = np.float32


def _h2d(ptr, a):
    import nof

    a = np.ascontiguousarray(a)
    nof._lib.call("nof_memcpy_h2d", C.c_void_p(ptr), a.ctypes.data, a.nbytes)


# ---- the two kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 4, 7, 32])
@pytest.mark.parametrize("Vd", [15, 27])
def test_kernel_gather(gpu, Vd, G):
    import torch
    import nof

    n, Vw = 5, 3
    rng = np.random.default_rng(Vd * 100 + G)
    ed = rng.standard_normal((n, Vd)).astype(f32)
    E = rng.standard_normal((Vw, G)).astype(f32)
    ids = np.array([1, -1, 1, Vw, 2], np.int32)  # a repeat, and the two ids just outside the table
    d_ed, d_E, d_ids = _dev(ed, gpu), _dev(E, gpu), _dev(ids, gpu)

    def run(idp, const):
        out = torch.full((n, Vd + G), 7.0, device=gpu)
        nof._lib.call("nof_kernel_appearance_gather", n, Vd, G, Vw, d_ed.data_ptr(), d_E.data_ptr(), idp, const,
                      out.data_ptr(), None)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    rows = np.where(((ids >= 0) & (ids < Vw))[:, None], E[np.clip(ids, 0, Vw - 1)], f32(0))
    want = np.concatenate([ed, rows], 1)
    assert np.array_equal(run(d_ids.data_ptr(), 0).view(np.int32), want.view(np.int32))
    assert np.all(want[1, Vd:] == 0) and np.all(want[3, Vd:] == 0)
    # no ids: the constant view, or the zero vector
    assert np.array_equal(run(None, 1), np.concatenate([ed, np.tile(E[1], (n, 1))], 1))
    assert np.array_equal(run(None, -1), np.concatenate([ed, np.zeros((n, G), f32)], 1))


@pytest.mark.parametrize("G", [1, 7, 32])
@pytest.mark.parametrize("n", [37, 300])
def test_kernel_grad(gpu, n, G):
    import torch
    import nof

    Vw = 4
    rng = np.random.default_rng(n + G)
    ids = rng.choice([0, 1, 3], size=n).astype(np.int32)  # view 2 draws no ray
    ids[n // 2] = -1
    assert all(np.sum(ids == v) > 1 for v in (0, 1, 3))
    dapp = rng.standard_normal((n, G)).astype(f32)
    d_ids, d_app = _dev(ids, gpu), _dev(dapp, gpu)

    def run(out, acc):
        nof._lib.call("nof_kernel_appearance_grad", n, G, Vw, d_ids.data_ptr(), d_app.data_ptr(), out.data_ptr(), acc,
                      None)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    got = run(torch.full((Vw, G), 7.0, device=gpu), 0)
    worst = 0.0
    for v in range(Vw):
        terms = dapp[ids == v].astype(np.float64)
        ref, mag = terms.sum(0), np.abs(terms).sum(0)
        bound = (n - 1) * 2.0 ** -24 * mag
        err = np.abs(got[v] - ref)
        assert np.all(err <= bound), (v, err.max(), bound.min())
        worst = max(worst, float(np.max(err / np.maximum(mag, 1e-30))))
    print(f"k_appearance_grad n={n} G={G}: worst |err| / sum |terms| {worst:.2e}")
    assert np.all(got[2] == 0)  # the empty view: exactly 0
    # accumulate on the same input: exactly twice, the empty row's sentinel untouched
    buf = _dev(got.copy(), gpu)
    buf[2] = 5.0
    twice = run(buf, 1)
    assert np.array_equal(twice[[0, 1, 3]], 2 * got[[0, 1, 3]]) and np.all(twice[2] == 5.0)
    # run to run
    assert np.array_equal(run(torch.full((Vw, G), 7.0, device=gpu), 0).view(np.int32), got.view(np.int32))


# ---- the model ---------------------------------------------------------------------------------------------------
def _app_model(spec, n, samples, dim, precision=0, views=VIEWS, **kw):
    return _model(spec, n, samples, precision, appearance_views=views if dim else 0, appearance_dim=dim, **kw)


def _table(m):
    import nof

    t, g, Vw, G = m.appearance()
    return nof.to_numpy(t, (Vw, G)), nof.to_numpy(g, (Vw, G))


@pytest.mark.parametrize("spec,G", [(TINY, 4), (TINY, 7), (REF8, 8)])
def test_layout_is_the_widened_view_layer(gpu, spec, G):
    import appearance_ref as A
    import torch_ref as R

    D, W_, Dc, Wc, skip, lo, hi, dv = spec
    m = _app_model(spec, 4, (64, 64), G, stop_level_grad=0)
    want = R.glorot(A.net(spec, G), SEED)
    assert np.array_equal(_params(m).view(np.int32), want.astype(f32).view(np.int32))
    sizes = m.GetLayerSizes()
    base = _model(spec, 4, (64, 64), stop_level_grad=0)
    sizes0 = base.GetLayerSizes()
    Vd = 3 * (2 * dv + 1)
    assert sizes[D + 1] == Wc * (W_ + Vd + G) and sizes0[D + 1] == Wc * (W_ + Vd)
    assert [a for i, a in enumerate(sizes) if i != D + 1] == [a for i, a in enumerate(sizes0) if i != D + 1]
    assert m.mlp.get_layer_sizes() == sizes
    E, dE = _table(m)
    assert E.shape == (VIEWS, G) and not np.any(E) and not np.any(dE)  # zero-initialised
    m.close(); base.close()


def _run(gpu, spec, n, samples, stop, dim, precision=0, adopt=False, E=None, ray_grad=False, contraction=0, post=None,
         rays=None, **kw):
    import nof
    from nof import synth

    r = synth.blender_rays(n, seed=RAY_SEED) if rays is None else rays
    m = _app_model(spec, n, samples, dim, precision, stop_level_grad=stop, **kw)
    if ray_grad:
        m.set_ray_grad(True)
    if contraction:
        m.set_contraction(1)
    if post:
        post(m)
    ids = None
    if dim:
        if E is not None:
            _h2d(m.appearance()[0], E)
        ids = _dev(view_ids(n), gpu)
        m.set_ray_views(ids)
    _step(m, r, gpu)
    L = len(samples)
    out = dict(G=_grads(m), params=_params(m), lv=[m.level_numpy(l) for l in range(L)], rays=r,
               masks={l: m.mlp.relu_masks(l) for l in range(L)} if adopt else None,
               cross=[m.cross_numpy(l) for l in range(L)])
    if dim:
        out["E"], out["dE"] = _table(m)
    if ray_grad:
        out["o_grad"], out["d_grad"] = _ray_grads(m, n)
    m.close()
    return out


def _reference(gpu, out, spec, samples, stop, dim, contraction, **kw):
    import appearance_ref as A
    import contraction_ref as CR
    from test_gpu_crosslevel import _net

    D, W_, Dc, Wc, skip, lo, hi, dv = spec
    lv = out["lv"]
    n = out["rays"]["o"].shape[0]
    common = dict(samples=samples, min_deg=lo, max_deg=hi, deg_view=dv, seed=SEED, step_idx=STEP, ray_base=RAY_BASE,
                  cylinder=bool(kw.get("ray_shape", 0)), idx=_gpu_index(lv, samples, gpu),
                  t_value={l: lv[l]["t"] for l in range(1, len(samples))}, relu=out["masks"], detach=bool(stop),
                  contraction=bool(contraction))
    if not dim:  # the existing reference
        return CR.step(out["params"], out["rays"], net=_net(spec), **common), _net(spec)
    net = A.net(spec, dim)
    return A.step(out["params"], out["E"], view_ids(n), out["rays"], net=net, **common), net


def _param_errors(G, ref, net):
    import crosslevel_ref as X

    return {name: rel_l2(G[o:o + s], ref["grads"][o:o + s]) for name, o, s in X.tensors(net)}


def _check_step(gpu, spec, n, samples, stop, dim, precision=0, adopt=False, tol=TOL, ray_grad=False, contraction=0, **kw):
    opt = dict(precision=precision, adopt=adopt, ray_grad=ray_grad, contraction=contraction, **kw)
    off = _run(gpu, spec, n, samples, stop, 0, **opt)
    ref0, net0 = _reference(gpu, off, spec, samples, stop, 0, contraction, **kw)
    e_off = max(_param_errors(off["G"], ref0, net0).values())
    on = _run(gpu, spec, n, samples, stop, dim, E=table(dim), **opt)
    assert np.array_equal(on["E"], table(dim))  # the borrowed pointer is the table the step read
    ref, net = _reference(gpu, on, spec, samples, stop, dim, contraction, **kw)
    bound = max(tol, 4 * e_off)
    errs = _param_errors(on["G"], ref, net)
    errs["dE"] = rel_l2(on["dE"], ref["e_grad"])
    if ray_grad:
        errs["dL/do"], errs["dL/dd"] = rel_l2(on["o_grad"], ref["o_grad"]), rel_l2(on["d_grad"], ref["d_grad"])
    for l in range(1, len(samples)):
        got = on["cross"][l]["t_grad"]
        assert (got is None) == bool(stop) and (ref["t_grad"][l] is None) == bool(stop)
        if got is not None:
            errs[f"dL/dt^{l}"] = rel_l2(got, ref["t_grad"][l])
    worst = max(errs, key=errs.get)
    print(f"{spec} {n} x {samples} G={dim} stop {stop} precision {precision} ray_grad {ray_grad} contraction "
          f"{contraction}: worst {worst} {errs[worst]:.2e} (bound {bound:.2e}, e_off {e_off:.2e}); params "
          f"{max(v for k, v in errs.items() if k[0] != 'd'):.2e} "
          + " ".join(f"{k} {v:.2e}" for k, v in errs.items() if k[0] == "d"))
    bad = {k: v for k, v in errs.items() if not v <= bound}
    assert not bad, (bad, bound)
    return on, ref


@pytest.mark.parametrize("stop", [1, 0])
def test_step_f32_tiny_two_levels(gpu, stop):
    _check_step(gpu, TINY, 5, (64, 128), stop, 4)


@pytest.mark.parametrize("stop", [1, 0])
def test_step_f32_tiny_three_levels(gpu, stop):
    _check_step(gpu, TINY, 3, (64, 64, 64), stop, 7)


def test_step_f32_reference_network(gpu):
    """8x256 in NOF_PRECISION_F32 with stop_level_grad = 0: the F32 route to the any-shape path"""
    _check_step(gpu, REF8, 3, (64, 64), 0, 8)


@pytest.mark.parametrize("stop", [1, 0])
def test_step_f32_ray_gradients_and_contraction(gpu, stop):
    """dL/do and dL/dd too.  The three-level case: contracted, the two-level case's density-bias gradient (one number)
    cancels to 1 / 26 of its terms in the fp64 reference itself (tests/test_appearance_cpu.py CONTRACTED_CASE); measured
    there on an MI355X: every other tensor, dE, dL/do and dL/dd within 1e-5, that number at 2.2e-5"""
    n, samples, dim = CONTRACTED_CASE
    _check_step(gpu, TINY, n, samples, stop, dim, ray_grad=True, contraction=1)


@pytest.mark.parametrize("stop", [1, 0])
def test_step_f16_products(gpu, stop):
    _check_step(gpu, TINY, 3, (64, 64, 64), stop, 7, precision=5, adopt=True, tol=F16P_TOL)


def test_the_term_is_there(gpu):
    """RAY_SEED (tests/test_appearance_cpu.py) was chosen from the reference alone: there the reference's dE is more
    than 100 x the bound next to the view layer's weight gradient.  Here: the same holds of the reference at the GPU's
    parameters, and the GPU gradient with the table differs from the one with E = 0 by more than 100 x the bound."""
    n, samples, dim = 5, (64, 128), 4
    on, ref = _check_step(gpu, TINY, n, samples, 1, dim)
    import appearance_ref as A
    import crosslevel_ref as X

    name, o, s = [t for t in X.tensors(A.net(TINY, dim)) if t[0] == f"W{TINY[0] + 1}"][0]
    r_e = float(np.linalg.norm(ref["e_grad"]) / np.linalg.norm(ref["grads"][o:o + s]))
    zero = _run(gpu, TINY, n, samples, 1, dim, E=np.zeros((VIEWS, dim), f32))
    r_p = rel_l2(zero["G"], on["G"])
    print(f"|dE| / |dW_view| (reference) {r_e:.2e}; GPU gradient, E vs 0: {r_p:.2e}")
    assert r_e > 100 * TOL and r_p > 100 * TOL
    assert np.any(zero["dE"])  # a zero table still has a gradient


def test_micro_batching_doubles_the_table_gradient(gpu):
    from nof import synth

    n, samples, dim = 5, (64, 128), 4
    r = synth.blender_rays(n, seed=RAY_SEED)
    for stop in (1, 0):
        m = _app_model(TINY, n, samples, dim, stop_level_grad=stop)
        _h2d(m.appearance()[0], table(dim))
        ids = _dev(view_ids(n), gpu)
        got = []
        for acc in (False, True):
            m.set_rng(SEED, STEP, RAY_BASE)
            m.set_ray_views(ids)
            _step(m, r, gpu, accumulate=acc)
            got.append(_table(m)[1].copy())
        assert np.any(got[0]) and np.array_equal(got[1], 2 * got[0]), stop
        m.close()


@pytest.mark.parametrize("stop", [1, 0])
def test_deterministic_and_callback(gpu, stop):
    """two runs with the losses, lindisp and contraction on: the same bits; the callback entry: the device entry's"""
    import torch
    import nof
    from nof import synth

    n, samples, dim = 8, (64, 64, 64), 7
    r = synth.blender_rays(n, seed=5)
    kw = dict(lindisp=1, distortion_loss_mult=0.01)
    post = lambda m: m.set_interlevel_loss(0.5)
    runs = [_run(gpu, TINY, n, samples, stop, dim, E=table(dim), ray_grad=True, contraction=1, rays=r, post=post, **kw)
            for _ in range(2)]
    for k in ("G", "dE", "o_grad", "d_grad"):
        assert np.array_equal(runs[0][k].view(np.int32), runs[1][k].view(np.int32)), k
    assert np.any(runs[0]["dE"]) and np.all(np.isfinite(runs[0]["dE"])) and np.all(np.isfinite(runs[0]["G"]))
    b = _app_model(TINY, n, samples, dim, stop_level_grad=stop, **kw)
    b.set_ray_grad(True)
    b.set_contraction(1)
    post(b)
    _h2d(b.appearance()[0], table(dim))
    ids = _dev(view_ids(n), gpu)
    b.set_ray_views(ids)
    gc = nof.AcceleratedGradientCalculator(n, b.config)
    b.GetGradient(r["o"], r["d"], r["radius"], r["near"], r["far"], r["lossmult"],
                  lambda comp, level, msum, lm: gc.get_output_gradient(comp, r["pix"], lm, msum, level))
    torch.cuda.synchronize()
    assert np.array_equal(_table(b)[1].view(np.int32), runs[0]["dE"].view(np.int32))
    assert np.array_equal(_grads(b), runs[0]["G"])
    gc.close(); b.close()


def test_option_off_is_the_parent_bitwise(gpu):
    """create_ex(ext = NULL) and create_ex(dim = 0): gradients and both dispatch tallies of nof_mipnerf_create, a 4x128
    model, 64 rays x (64, 64)"""
    import nof
    from nof import synth
    from test_gpu_generic import SPECS

    n, samples = 64, (64, 64)
    r = synth.blender_rays(n, seed=23)
    D, W_, Dc, Wc, skip, lo, hi, dv = SPECS["configs0_4x128"]
    cfg = nof.default_config(seed=SEED, max_rays=n, num_samples=samples, net_depth=D, net_width=W_,
                             net_depth_condition=Dc, net_width_condition=Wc, skip_layer=skip, min_deg_point=lo,
                             max_deg_point=hi, deg_view=dv)
    got = []
    for how in ("create", "null", "dim0"):
        if how == "create":
            m = nof.AcceleratedMipNeRF(cfg)
        else:  # through the C entry point, then the Python object around the handle
            ext = nof._lib.nof_model_ext(12, 5, 0)
            h = C.c_void_p()
            nof._lib.call("nof_mipnerf_create_ex", C.byref(cfg), None if how == "null" else C.byref(ext), C.byref(h))
            m = nof.AcceleratedMipNeRF.__new__(nof.AcceleratedMipNeRF)
            m.config, m._hook_errors, m._bucket_cb, m._h = cfg, [], None, h
            mh = C.c_void_p()
            nof._lib.call("nof_mipnerf_mlp", h, C.byref(mh))
            m.mlp = nof.api.AcceleratedMLP(mh, m)
            with pytest.raises(nof._lib.NofError) as e:
                m.appearance()
            assert e.value.status == 1
        m.set_rng(SEED, STEP, RAY_BASE)
        _step(m, r, gpu)
        got.append((_grads(m), dict(m.mlp.gen_dispatch()), dict(m.mlp.gen_dispatch_h())))
        m.close()
    for g in got[1:]:
        assert np.array_equal(g[0].view(np.int32), got[0][0].view(np.int32)) and g[1] == got[0][1] and g[2] == got[0][2]
    assert np.any(got[0][0]) and any(got[0][1].values())


def test_dispatch_tally_has_no_new_entry(gpu):
    """an appearance model's launches land in the existing variants: the name lists are the parent's, and the step of a
    G > 0 model tallies the same variant set as G = 0"""
    from nof import synth

    n, samples = 5, (64, 128)
    r = synth.blender_rays(n, seed=RAY_SEED)
    names = []
    for dim in (0, 4):
        m = _app_model(TINY, n, samples, dim)
        if dim:
            ids = _dev(view_ids(n), gpu)
            m.set_ray_views(ids)
        _step(m, r, gpu)
        names.append({k for k, c in m.mlp.gen_dispatch().items() if c})
        m.close()
    assert names[0] == names[1]


def test_missing_ids_are_refused_and_the_object_stays_usable(gpu):
    import nof
    from nof import synth

    n, samples, dim = 5, (64, 128), 4
    r = synth.blender_rays(n, seed=RAY_SEED)
    m = _app_model(TINY, n, samples, dim)
    with pytest.raises(nof._lib.NofError) as e:
        _step(m, r, gpu)
    assert e.value.status == 1 and "ray views" in str(e.value)
    ids = _dev(view_ids(n), gpu)
    m.set_ray_views(ids)
    _step(m, r, gpu)
    assert np.any(_grads(m)) and np.all(np.isfinite(_grads(m)))
    with pytest.raises(nof._lib.NofError) as e:  # the ids held for that one step
        _step(m, r, gpu)
    assert e.value.status == 1
    for bad in (-2, VIEWS):
        with pytest.raises(nof._lib.NofError) as e:
            m.set_render_appearance(bad)
        assert e.value.status == 1
    m.close()
    plain = _model(TINY, n, samples)
    for call in (lambda: plain.appearance(), lambda: plain.set_ray_views(ids), lambda: plain.set_render_appearance(0)):
        with pytest.raises(nof._lib.NofError) as e:
            call()
        assert e.value.status == 1
    plain.close()


# ---- rendering ---------------------------------------------------------------------------------------------------
def test_render_device(gpu):
    import torch
    import nof
    from nof import synth

    n, samples, dim = 8, (64, 64), 4
    r = synth.blender_rays(n, seed=9)
    d = {k: _dev(v, gpu) for k, v in r.items()}
    m = _app_model(TINY, n, samples, dim, randomized=0)
    _h2d(m.appearance()[0], table(dim))
    ids = _dev(view_ids(n), gpu)
    m.set_ray_views(ids)
    _step(m, r, gpu)
    trained = [m.level_numpy(l)["comp_rgb"].copy() for l in range(2)]

    def render(with_ids):
        if with_ids:
            m.set_ray_views(ids)
        out = m.render_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], randomized=False)
        torch.cuda.synchronize()
        return [nof.to_numpy(*o["comp_rgb"]).copy() for o in out]

    with_ids, without = render(True), render(False)  # (the second call: the first reset the ids)
    for l in range(2):
        assert rel_l2(with_ids[l], trained[l]) == 0.0, l
        assert rel_l2(without[l], with_ids[l]) > 100 * TOL, l
    _h2d(m.appearance()[0], np.zeros((VIEWS, dim), f32))
    zeroed = render(True)
    for l in range(2):
        assert np.array_equal(zeroed[l].view(np.int32), without[l].view(np.int32)), l
    m.close()


def test_render_view_uses_the_constant_view(gpu):
    """nof_dataset_render_view after set_render_appearance(v): bitwise render_device with ids all v on the
    materialised records; a 4-view 40 x 24 scene"""
    import torch
    import nof
    from test_gpu_render_view import _host, _rays, _same, _slice

    dim, chunk, v = 4, 80, 2
    images = np.random.default_rng(17).random((V, H, W, 3), dtype=f32)
    scene = dict(poses=_poses(V, seed=1), width=W, height=H, focal=FOCAL, near=2.0, far=6.0, ndc=False,
                 images=torch.from_numpy(images).to(gpu), num_scales=1)
    ds = nof.RayDataset(scene=scene)
    rec = _slice(ds.materialize().cpu().numpy(), nof.multiscale_layout(W, H, FOCAL, 1, True, V), 1, 0)
    m = nof.AcceleratedMipNeRF(seed=5, max_rays=chunk, num_samples=(64, 64), net_depth=2, net_width=64,
                               net_depth_condition=1, net_width_condition=32, appearance_views=V, appearance_dim=dim)
    _h2d(m.appearance()[0], (0.5 * np.random.default_rng(2).standard_normal((V, dim))).astype(f32))
    ids = torch.full((chunk,), v, dtype=torch.int32, device=gpu)
    want = [[], []]
    for p0 in range(0, len(rec), chunk):
        q = {k: _dev(a, gpu) for k, a in _rays(rec[p0:p0 + chunk]).items()}
        k = len(q["radius"])
        m.set_ray_views(ids)
        out = m.render_device(k, q["o"], q["d"], q["radius"], q["near"], q["far"], randomized=False)
        torch.cuda.synchronize()
        for l, o in enumerate(out):
            want[l].append(nof.to_numpy(*o["comp_rgb"]).copy())
    want = [np.concatenate(x) for x in want]
    neutral = _host(ds.render_view(m, view=1, scale=0, score=False))[0]
    m.set_render_appearance(v)
    got = _host(ds.render_view(m, view=1, scale=0, score=False))[0]
    for l in range(2):
        assert _same(got[l].reshape(-1, 3), want[l]), l
        assert not np.array_equal(neutral[l], got[l]), l
    m.close(); ds.close()


def test_batch_views(gpu):
    """nof_dataset_batch_views equals the host decode of record_index through nof_multiscale_layout: 37 rays, 2 scales"""
    import torch
    import nof

    ds = nof.RayDataset(scene=_scene(gpu))
    b, msum, rays, idx = _batch(ds, NP)
    lay = nof.multiscale_layout(W, H, FOCAL, SCALES, True, V)
    want = np.zeros(NP, np.int32)
    for r, i in enumerate(idx):
        s = max(k for k in range(SCALES) if lay["first"][k] <= i)
        want[r] = (int(i) - lay["first"][s]) // (lay["width"][s] * lay["height"][s])
    got = ds.batch_views(NP)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert np.any(idx >= lay["first"][1]) and np.any(idx < lay["first"][1]) and len(set(want)) > 1
    assert np.array_equal(ds.batch_views(5).cpu().numpy(), want[:5])
    with pytest.raises(nof._lib.NofError) as e:
        ds.batch_views(NP + 1)
    assert e.value.status == 1
    ds.close()
    from nof import synth

    rec = nof.RayDataset(records=synth.pack_records(synth.blender_rays(64, seed=1)))
    rec.next(8, 1, 1)
    with pytest.raises(nof._lib.NofError) as e:
        rec.batch_views(8)
    assert e.value.status == 5
    rec.close()


# ---- data parallel, checked build, driver ------------------------------------------------------------------------
def test_dp_train_step_refuses_an_appearance_model(gpu):
    import nof
    from nof import synth

    n = 8
    m = _app_model(TINY, n, (64, 64), 4)
    adam = nof.AcceleratedAdamOptimizer(m.GetLayerSizes(), m.config)
    ds = nof.RayDataset(records=synth.pack_records(synth.blender_rays(64, seed=1)))
    ms, ad, dd = (C.c_void_p * 1)(m._h), (C.c_void_p * 1)(adam._h), (C.c_void_p * 1)(ds._h)
    st = nof.lib().nof_dp_train_step(1, None, ms, ad, dd, n, 0, 1, 1, 1e-3, None)
    assert st == 5 and b"appearance" in nof.lib().nof_last_error()
    ds.close(); adam.close(); m.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import nof
from nof import synth
assert nof._lib.LIB_PATH.endswith("libnof_check.so"), nof._lib.LIB_PATH
assert nof.device_checks(clear=True) == 0
n = 8
r = synth.blender_rays(n, seed=3)
d = {k: torch.from_numpy(v).cuda() for k, v in r.items()}
ids = torch.from_numpy((np.arange(n) % 3).astype(np.int32)).cuda()
for prec, stop in ((0, 1), (0, 0), (5, 1)):
    m = nof.AcceleratedMipNeRF(seed=5, max_rays=n, num_samples=(64, 128), precision=prec, stop_level_grad=stop,
                               net_depth=3, net_width=32, net_width_condition=16, skip_layer=2, max_deg_point=4, deg_view=2,
                               appearance_views=3, appearance_dim=7)
    m.set_ray_views(ids)
    m.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"], float(n))
    m.render_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"])
    torch.cuda.synchronize()
    bits = nof.device_checks(clear=True)
    assert bits == 0, f"precision {prec}: failed checks {bits:#x}"
    t, g, V, G = m.appearance()
    dE = nof.to_numpy(g, (V, G))
    assert np.all(np.isfinite(dE)) and np.any(dE)
    m.close()
print("OK")
"""


def test_checked_build_runs_clean(gpu):
    lib = os.path.join(PKG, "lib", "libnof_check.so")
    assert os.path.exists(lib), "build it with: make -C nerf-or-nothing_amd check"
    out = subprocess.run([sys.executable, "-c", CHILD, PKG], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, NOF_LIB=lib))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_driver_trains_with_appearance(gpu, tmp_path):
    """python -m nof.train --scene ... --appearance-dim 4 --precision f16p: the loss falls, appearance.npy is [V, 4]
    and non-zero; a fused precision and a record dataset are refused before any step, with the library's message"""
    rng = np.random.default_rng(3)
    base = np.array([0.2, 0.5, 0.3], f32)
    gain = np.linspace(0.6, 1.4, V, dtype=f32)[:, None, None, None]
    images = ((base + 0.05 * rng.random((V, H, W, 3), dtype=f32)) * gain).astype(f32)
    npz = tmp_path / "scene.npz"
    np.savez(npz, poses=_poses(V, seed=1), images=images, focal=FOCAL, near=2.0, far=6.0)
    tail = ["--appearance-dim", "4", "--batch", "64"]
    common = [sys.executable, "-m", "nof.train", "--scene", str(npz)] + tail
    cmd = common + ["--precision", "f16p", "--samples", "64", "64", "--net-depth", "3", "--net-width", "32",
                    "--net-width-condition", "16", "--steps", "30", "--print-every", "1", "--lr-init", "5e-3",
                    "--lr-delay-steps", "0", "--appearance-lr", "1e-2", "--ckpt-dir", str(tmp_path)]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"Step \d+/1000000, Loss: (\S+)", out.stdout)]
    print("losses", losses[0], losses[-1])
    assert len(losses) == 30 and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    E = np.load(tmp_path / "appearance.npy")
    assert E.shape == (V, 4) and E.dtype == np.float32 and np.all(np.isfinite(E)) and np.any(E)
    bad = subprocess.run(common + ["--steps", "1"], capture_output=True, text=True, timeout=300, env=env,
                         cwd=str(tmp_path))
    assert bad.returncode != 0 and "any-shape" in bad.stderr and "Step" not in bad.stdout
    bad = subprocess.run([sys.executable, "-m", "nof.train", "--synthetic", "256", "--precision", "f16p", "--steps", "1"]
                         + tail, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert bad.returncode != 0 and "image-backed" in bad.stderr and "Step" not in bad.stdout
