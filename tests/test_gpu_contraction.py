"""GPU parity of the scene contraction (nof_mipnerf_set_contraction) against tests/contraction_ref.py (pinned
on the CPU by tests/test_contraction_cpu.py).

Bounds.  Forward kernel: bitwise contract32 of the fp32 cast (torch_ref.cast, which k_cast reproduces bit for bit), and
element-wise |got - ref| <= 1e-5 |ref| against the fp64 map of the same fp32 Gaussians (the map's own error: the cast's
mean d t + o cancels where a ray crosses a coordinate plane, which is not this feature's arithmetic).  Adjoint kernels:
rel L2 <= 1e-5 per output against fp64 autograd, the project's fp32 parity bound.  Whole step, F32: every parameter
gradient tensor, dL/do, dL/dd and (stop_level_grad = 0) dL/dt of the levels above 0 <= max(1e-5, 4 x e_off), e_off the
worst parameter-gradient tensor error of the same model and rays with the contraction off against the same reference
without the map (the parent's arithmetic; the factor 4 as in test_gpu_crosslevel.py / test_gpu_raygrad.py).
F16_PRODUCTS (ReLU decisions adopted): max(2e-3, 4 x e_off).  DESIGN.md 6i has the measured figures.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_l2
from test_gpu_crosslevel import RAY_BASE, REF8, SEED, STEP, TINY, _dev, _gpu_index, _grads, _model, _net, _params, _step
from test_gpu_raygrad import FOCAL, H, V, W, _ray_grads
from test_raygen import _poses
from test_raygrad_cpu import RAY_SEED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-or-nothing_amd")
TOL = 1e-5
F16P_TOL = 2e-3
f32 = np.float32


# ---- kernel entry points -----------------------------------------------------------------------------------------
def _kernel_rays(S, seed, geometric=False):
    from nof import synth

    n = 5
    r = synth.blender_rays(n, seed=6)  # |o| ~ 4, near / far 2 / 6
    rng = np.random.default_rng(seed)
    if geometric:
        t = np.tile(np.geomspace(2.0, 2e3, S + 1), (n, 1)).astype(f32)
    else:
        t = np.sort(2.0 + 4.0 * rng.random((n, S + 1)), axis=1).astype(f32)
    return n, r, t, rng


def _branches(mean):
    """the share of the samples outside the unit ball, by the kernel's own fp32 test"""
    n2 = (mean[..., 0] * mean[..., 0] + mean[..., 1] * mean[..., 1]) + mean[..., 2] * mean[..., 2]
    return float(np.mean(n2 > f32(1)))


def _cast(gpu, n, S, t, r, ray_shape, contraction, name="nof_kernel_cast_contract"):
    import torch
    import nof

    dv = {k: _dev(v, gpu) for k, v in dict(t=t, o=r["o"], d=r["d"], radius=r["radius"]).items()}
    mean, cov = torch.full((n, S, 3), 7.0, device=gpu), torch.full((n, S, 3), 7.0, device=gpu)
    args = [n, S, dv["t"].data_ptr(), dv["o"].data_ptr(), dv["d"].data_ptr(), dv["radius"].data_ptr(), mean.data_ptr(),
            cov.data_ptr(), None, ray_shape]
    nof._lib.call(name, *args, *([contraction] if name == "nof_kernel_cast_contract" else []))
    torch.cuda.synchronize()
    return mean, cov, dv


@pytest.mark.parametrize("geometric", [False, True])
@pytest.mark.parametrize("ray_shape", [0, 1])
def test_kernel_cast_contract(gpu, ray_shape, geometric):
    import torch
    import contraction_ref as CR
    import torch_ref as R

    S = 64
    n, r, t, _ = _kernel_rays(S, 100 + ray_shape, geometric)
    mean, cov, _ = _cast(gpu, n, S, t, r, ray_shape, 1)
    m32, v32 = R.cast(t, r["o"], r["d"], r["radius"], bool(ray_shape))
    out = _branches(m32)
    print(f"cast_contract ray_shape {ray_shape} geometric {geometric}: {100 * out:.0f} % of the samples outside the ball")
    if geometric:
        assert out >= 0.1 and np.linalg.norm(m32, axis=-1).max() > 1e3
    else:
        assert 0.1 <= out <= 0.9  # each branch holds at least 10 % of the samples
    wm, wv = CR.contract32(m32, v32)
    gm, gv = mean.cpu().numpy(), cov.cpu().numpy()
    assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32)) and np.array_equal(gv.view(np.uint32), wv.view(np.uint32))
    rm, rv = CR.contract(torch.from_numpy(m32.astype(np.float64)), torch.from_numpy(v32.astype(np.float64)))
    for got, ref, name in ((gm, rm.numpy(), "mean"), (gv, rv.numpy(), "cov")):
        err = np.abs(got.astype(np.float64) - ref)
        print(f"  {name}: worst element-wise relative error {np.max(err / np.maximum(np.abs(ref), 1e-300)):.2e}")
        assert np.all(err <= TOL * np.abs(ref)), name
    assert np.all(np.linalg.norm(gm.astype(np.float64), axis=-1) < 2.0)
    # contraction 0: nof_kernel_cast_ex, bit for bit
    a = _cast(gpu, n, S, t, r, ray_shape, 0)
    b = _cast(gpu, n, S, t, r, ray_shape, 0, name="nof_kernel_cast_ex")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(a[0].cpu().numpy(), m32) and not torch.equal(a[0], mean)


@pytest.mark.parametrize("ray_shape", [0, 1])
@pytest.mark.parametrize("max_deg", [4, 16])  # P = 24: half of a sample's 8 threads idle; P = 96
@pytest.mark.parametrize("S", [64, 128])  # two and four 32-sample passes
def test_kernel_adjoints_match_autograd(gpu, S, max_deg, ray_shape):
    import torch
    import nof
    import contraction_ref as CR
    import crosslevel_ref as X
    import raygrad_ref as G

    P, dv_deg = 6 * max_deg, 4
    n, r, t, rng = _kernel_rays(S, 1000 * S + 10 * max_deg + ray_shape)
    sigma = rng.gamma(1.0, 2.0, (n, S)).astype(f32)
    rgb = rng.random((n, S, 3), dtype=f32)
    gC = rng.standard_normal((n, 3)).astype(f32)
    genc = rng.standard_normal((n * S, P)).astype(f32)
    genc *= np.repeat(f32(2.0) ** -np.arange(max_deg, dtype=f32), 6)[None, :]  # (as test_gpu_raygrad.py)
    gdir = rng.standard_normal((n, 27)).astype(f32)
    mean, cov, dv = _cast(gpu, n, S, t, r, ray_shape, 1)
    out = _branches(_cast(gpu, n, S, t, r, ray_shape, 0)[0].cpu().numpy())
    assert 0.1 <= out <= 0.9
    dv["sigma"] = _dev(sigma, gpu)
    ep96, ed = torch.zeros((n * S, 96), device=gpu), torch.zeros((n, 27), device=gpu)
    nof._lib.call("nof_kernel_encode", n, S, mean.data_ptr(), cov.data_ptr(), dv["d"].data_ptr(), ep96.data_ptr(),
                  ed.data_ptr(), None)
    enc = ep96[:, :P].contiguous()
    # the reference: cast -> contraction -> IPE; the integrator and the view PE for the ray gradients
    T = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=g)
    t64, o64, d64, s64 = T(t, True), T(r["o"], True), T(r["d"], True), T(sigma, True)
    m64, c64 = G.cast(t64, o64, d64, r["radius"], bool(ray_shape))
    m64, c64 = CR.contract(m64, c64, snap=True)
    f = X.ipe(m64, c64, 0, max_deg)
    assert rel_l2(enc.cpu().numpy().reshape(n, S, P), f.detach().numpy()) <= 1e-6
    L_enc = (f * T(genc.reshape(n, S, P))).sum()
    dt_ref = torch.autograd.grad(L_enc, t64, retain_graph=True)[0].numpy()
    Cr, _ = G.render(s64, T(rgb), T(t), d64)
    Lr = (Cr * T(gC)).sum()
    dsig = torch.autograd.grad(Lr, s64, retain_graph=True)[0].numpy().astype(f32)
    (Lr + L_enc + (G.dir_pe(d64, dv_deg) * T(gdir)).sum()).backward()
    dg, ds, dd = _dev(genc, gpu), _dev(dsig, gpu), _dev(gdir, gpu)

    def encode_grad(name, *tail):
        tg = torch.full((n, S + 1), 7.0, device=gpu)
        nof._lib.call(name, n, S, dv["t"].data_ptr(), dv["o"].data_ptr(), dv["d"].data_ptr(), dv["radius"].data_ptr(),
                      ray_shape, 0, max_deg, enc.data_ptr(), dg.data_ptr(), tg.data_ptr(), None, *tail)
        torch.cuda.synchronize()
        return tg

    def ray_grad(name, *tail):
        og, dgr = torch.full((n, 3), 7.0, device=gpu), torch.full((n, 3), 7.0, device=gpu)
        nof._lib.call(name, n, S, dv["t"].data_ptr(), dv["o"].data_ptr(), dv["d"].data_ptr(), dv["radius"].data_ptr(),
                      ray_shape, 0, max_deg, enc.data_ptr(), dg.data_ptr(), dv["sigma"].data_ptr(), ds.data_ptr(), dv_deg,
                      ed.data_ptr(), dd.data_ptr(), 0, og.data_ptr(), dgr.data_ptr(), None, *tail)
        torch.cuda.synchronize()
        return og, dgr

    tg = encode_grad("nof_kernel_encode_grad_ex", 1)
    og, dgr = ray_grad("nof_kernel_ray_grad_ex", 1)
    e_t = rel_l2(tg.cpu().numpy(), dt_ref)
    e_o, e_d = rel_l2(og.cpu().numpy(), o64.grad.numpy()), rel_l2(dgr.cpu().numpy(), d64.grad.numpy())
    print(f"contracted adjoints S={S} PE (0, {max_deg}) ray_shape {ray_shape}: dt {e_t:.2e} do {e_o:.2e} dd {e_d:.2e}")
    assert e_t <= TOL and e_o <= TOL and e_d <= TOL, (e_t, e_o, e_d)
    # contraction 0: the entry points they extend, bit for bit; and the map's adjoint is there
    tg0, tg_old = encode_grad("nof_kernel_encode_grad_ex", 0), encode_grad("nof_kernel_encode_grad")
    (og0, dg0), (og_old, dg_old) = ray_grad("nof_kernel_ray_grad_ex", 0), ray_grad("nof_kernel_ray_grad")
    assert torch.equal(tg0, tg_old) and torch.equal(og0, og_old) and torch.equal(dg0, dg_old)
    for on, off, name in ((tg, tg0, "dt"), (og, og0, "do"), (dgr, dg0, "dd")):
        assert rel_l2(on.cpu().numpy(), off.cpu().numpy()) > 100 * TOL, name


# ---- whole step --------------------------------------------------------------------------------------------------
def _run(gpu, spec, n, samples, stop, precision=0, adopt=False, contraction=1, ray_grad=True, rays=None, post=None, **kw):
    from nof import synth

    r = synth.blender_rays(n, seed=RAY_SEED) if rays is None else rays
    m = _model(spec, n, samples, precision, stop_level_grad=stop, **kw)
    if ray_grad:
        m.set_ray_grad(True)
    if contraction:
        m.set_contraction(contraction)
    if post:
        post(m)
    assert m.contraction() == contraction
    _step(m, r, gpu)
    L = len(samples)
    out = dict(G=_grads(m), params=_params(m), lv=[m.level_numpy(l) for l in range(L)],
               masks={l: m.mlp.relu_masks(l) for l in range(L)} if adopt else None, rays=r,
               cross=[m.cross_numpy(l) for l in range(L)])
    if ray_grad:
        out["o_grad"], out["d_grad"] = _ray_grads(m, n)
    m.close()
    return out


def _reference(gpu, out, spec, samples, stop, contraction, **kw):
    import contraction_ref as CR

    D, W_, Dc, Wc, skip, lo, hi, dv = spec
    lv = out["lv"]
    return CR.step(out["params"], out["rays"], net=_net(spec), samples=samples, min_deg=lo, max_deg=hi, deg_view=dv,
                   seed=SEED, step_idx=STEP, ray_base=RAY_BASE, cylinder=bool(kw.get("ray_shape", 0)),
                   idx=_gpu_index(lv, samples, gpu), t_value={l: lv[l]["t"] for l in range(1, len(samples))},
                   relu=out["masks"], detach=bool(stop), contraction=bool(contraction))


def _param_errors(G, ref, spec):
    import crosslevel_ref as X

    return {name: rel_l2(G[o:o + s], ref["grads"][o:o + s]) for name, o, s in X.tensors(_net(spec))}


def _check_step(gpu, spec, n, samples, stop, precision=0, adopt=False, tol=TOL, **kw):
    off = _run(gpu, spec, n, samples, stop, precision, adopt, contraction=0, **kw)
    e_off = max(_param_errors(off["G"], _reference(gpu, off, spec, samples, stop, 0, **kw), spec).values())
    on = _run(gpu, spec, n, samples, stop, precision, adopt, contraction=1, **kw)
    ref = _reference(gpu, on, spec, samples, stop, 1, **kw)
    bound = max(tol, 4 * e_off)
    errs = _param_errors(on["G"], ref, spec)
    errs["dL/do"], errs["dL/dd"] = rel_l2(on["o_grad"], ref["o_grad"]), rel_l2(on["d_grad"], ref["d_grad"])
    for l in range(1, len(samples)):
        got = on["cross"][l]["t_grad"]
        assert (got is None) == bool(stop) and (ref["t_grad"][l] is None) == bool(stop)
        if got is not None:
            errs[f"dL/dt^{l}"] = rel_l2(got, ref["t_grad"][l])
    outside = [_branches(CRm) for CRm in _uncontracted_means(on, kw)]
    worst = max(errs, key=errs.get)
    print(f"{spec} {n} x {samples} stop {stop} precision {precision} {kw}: worst {worst} {errs[worst]:.2e} "
          f"(bound {bound:.2e}, e_off {e_off:.2e}); params {max(v for k, v in errs.items() if k[0] != 'd'):.2e} "
          + " ".join(f"{k} {v:.2e}" for k, v in errs.items() if k[0] == "d")
          + f"; outside the ball per level {[round(x, 2) for x in outside]}")
    assert min(outside) > 0.1 and max(outside) < 0.95  # both branches are exercised
    bad = {k: v for k, v in errs.items() if not v <= bound}
    assert not bad, (bad, bound)
    assert rel_l2(on["G"], off["G"]) > 100 * TOL  # the option changes the step
    return errs, bound


def _uncontracted_means(out, kw):
    import torch_ref as R

    r = out["rays"]
    return [R.cast(lv["t"], r["o"], r["d"], r["radius"], bool(kw.get("ray_shape", 0)))[0] for lv in out["lv"]]


@pytest.mark.parametrize("stop", [1, 0])
@pytest.mark.parametrize("ray_shape", [0, 1])
def test_step_f32_tiny_two_levels(gpu, ray_shape, stop):
    _check_step(gpu, TINY, 5, (64, 128), stop, ray_shape=ray_shape)


@pytest.mark.parametrize("stop", [1, 0])
def test_step_f32_tiny_three_levels(gpu, stop):
    _check_step(gpu, TINY, 3, (64, 64, 64), stop)


def test_step_f32_reference_network(gpu):
    """8x256 in NOF_PRECISION_F32 with stop_level_grad = 0: the F32 route to the any-shape path"""
    _check_step(gpu, REF8, 3, (64, 64), 0)


@pytest.mark.parametrize("spec,n,samples,stop", [(TINY, 3, (64, 64, 64), 0), (TINY, 3, (64, 64, 64), 1),
                                                 (REF8, 3, (64, 64), 1)])
def test_step_f16_products(gpu, spec, n, samples, stop):
    _check_step(gpu, spec, n, samples, stop, precision=5, adopt=True, tol=F16P_TOL)


# ---- unchanged behaviour, determinism, paths ---------------------------------------------------------------------
def test_option_off_is_the_parent_bitwise(gpu):
    """never switched on, and switched on then off: configs0_4x128's gradient and dispatch tally (test_gpu_generic's)"""
    from nof import synth
    from test_gpu_generic import DISPATCH, SPECS

    n, samples = 8, (64, 128)
    r = synth.blender_rays(n, seed=23)
    got = []
    for toggle in (False, True):
        m = _model(SPECS["configs0_4x128"], n, samples)
        if toggle:
            m.set_contraction(1)
            m.set_contraction(0)
        _step(m, r, gpu)
        tally = {k for k, c in m.mlp.gen_dispatch().items() if c}
        assert tally == set(DISPATCH["configs0_4x128"]), sorted(tally ^ set(DISPATCH["configs0_4x128"]))
        got.append((_grads(m), dict(m.mlp.gen_dispatch())))
        m.close()
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    # switched on: the same launches (the option adds none to the tally)
    m = _model(SPECS["configs0_4x128"], n, samples)
    m.set_contraction(1)
    _step(m, r, gpu)
    assert dict(m.mlp.gen_dispatch()) == got[0][1] and not np.array_equal(_grads(m), got[0][0])
    m.close()


def test_option_on_changes_the_encoding_only(gpu):
    """one model, off then on: level 0's t (stratified, before any cast) is bitwise the same and the only one; every
    comp_rgb differs"""
    from nof import synth

    n, samples = 3, (64, 64, 64)
    r = synth.blender_rays(n, seed=RAY_SEED)
    m = _model(TINY, n, samples)
    lv = {}
    for mode in (0, 1):
        m.set_contraction(mode)
        m.set_rng(SEED, STEP, RAY_BASE)
        _step(m, r, gpu)
        lv[mode] = [{k: v.copy() for k, v in m.level_numpy(l).items()} for l in range(3)]
    m.close()
    assert np.array_equal(lv[0][0]["t"], lv[1][0]["t"])
    for l in range(3):
        assert not np.array_equal(lv[0][l]["comp_rgb"], lv[1][l]["comp_rgb"]), l
        assert not np.array_equal(lv[0][l]["weights"], lv[1][l]["weights"]), l
        if l:
            assert not np.array_equal(lv[0][l]["t"], lv[1][l]["t"]), l


@pytest.mark.parametrize("stop", [1, 0])
def test_deterministic_and_callback(gpu, stop):
    import torch
    import nof
    from nof import synth

    n, samples = 8, (64, 64, 64)
    r = synth.blender_rays(n, seed=5)
    kw = dict(lindisp=1, distortion_loss_mult=0.01)
    post = lambda m: m.set_interlevel_loss(0.5)
    runs = [_run(gpu, TINY, n, samples, stop, rays=r, post=post, **kw) for _ in range(2)]
    for k in ("o_grad", "d_grad", "G"):
        assert np.array_equal(runs[0][k], runs[1][k]), k  # no float atomics: bitwise run to run
    for l in range(1, 3):
        a, b = runs[0]["cross"][l]["t_grad"], runs[1]["cross"][l]["t_grad"]
        assert (a is None) == bool(stop) and (a is None or (np.array_equal(a, b) and np.any(a)))
    assert np.any(runs[0]["o_grad"]) and np.any(runs[0]["d_grad"]) and np.all(np.isfinite(runs[0]["G"]))
    # the callback entry: bitwise the device entry
    b = _model(TINY, n, samples, stop_level_grad=stop, **kw)
    b.set_ray_grad(True)
    b.set_contraction(1)
    post(b)
    gc = nof.AcceleratedGradientCalculator(n, b.config)
    b.GetGradient(r["o"], r["d"], r["radius"], r["near"], r["far"], r["lossmult"],
                  lambda comp, level, msum, lm: gc.get_output_gradient(comp, r["pix"], lm, msum, level))
    torch.cuda.synchronize()
    og, dg = _ray_grads(b, n)
    assert np.array_equal(og, runs[0]["o_grad"]) and np.array_equal(dg, runs[0]["d_grad"])
    assert np.array_equal(_grads(b), runs[0]["G"])
    for l in range(1, 3):
        a = b.cross_numpy(l)["t_grad"]
        assert (a is None) == bool(stop) and (a is None or np.array_equal(a, runs[0]["cross"][l]["t_grad"]))
    gc.close(); b.close()


def test_inference_paths(gpu):
    """render_device is the training forward (randomized = 0); render_view is render_device on the materialised records"""
    import torch
    import nof
    from nof import synth
    from test_gpu_render_view import _host, _render_records, _same, _slice

    n, samples = 8, (64, 64)
    r = synth.blender_rays(n, seed=9)
    d = {k: _dev(v, gpu) for k, v in r.items()}
    m = _model(TINY, n, samples, randomized=0)
    comp = {}
    for mode in (1, 0):
        m.set_contraction(mode)
        if mode:
            _step(m, r, gpu)
            trained = [m.level_numpy(l)["comp_rgb"].copy() for l in range(2)]
        out = m.render_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], randomized=False)
        torch.cuda.synchronize()
        comp[mode] = [nof.to_numpy(*o["comp_rgb"]).copy() for o in out]
    for l in range(2):
        e = rel_l2(comp[1][l], trained[l])
        print(f"render_device vs the training forward, level {l}: rel L2 {e:.2e}")
        assert e <= TOL
        assert rel_l2(comp[0][l], comp[1][l]) > 100 * TOL
    m.close()
    # a whole view
    images = np.random.default_rng(17).random((V, H, W, 3), dtype=f32)
    scene = dict(poses=_poses(V, seed=1), width=W, height=H, focal=FOCAL, near=2.0, far=6.0, ndc=False,
                 images=torch.from_numpy(images).to(gpu), num_scales=1)
    ds = nof.RayDataset(scene=scene)
    rec = ds.materialize().cpu().numpy()
    lay = nof.multiscale_layout(W, H, FOCAL, 1, True, V)
    m = nof.AcceleratedMipNeRF(seed=5, max_rays=80, num_samples=(64, 64), net_depth=2, net_width=64,
                               net_depth_condition=1, net_width_condition=32)
    res = {}
    for mode in (0, 1):
        m.set_contraction(mode)
        rgb, dist, acc = _render_records(m, _slice(rec, lay, 1, 0), gpu)
        got_rgb, got_dist, got_acc = _host(ds.render_view(m, view=1, scale=0, score=False))
        for l in range(2):
            assert _same(got_rgb[l].reshape(-1, 3), rgb[l]), (mode, l)
        assert _same(got_dist.reshape(-1), dist) and _same(got_acc.reshape(-1), acc), mode
        res[mode] = got_rgb[-1]
    assert not np.array_equal(res[0], res[1])
    m.close(); ds.close()


# ---- refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 4])
def test_fused_objects_refuse_and_stay_usable(gpu, precision):
    import nof
    from nof import synth

    n = 4
    m = nof.AcceleratedMipNeRF(seed=1, max_rays=n, num_samples=(64, 64), precision=precision)  # the fused 8x256
    with pytest.raises(nof._lib.NofError) as e:
        m.set_contraction(1)
    assert e.value.status == 5 and "any-shape" in str(e.value)
    assert m.contraction() == 0
    m.set_contraction(0)  # accepted
    for bad in (2, -1):
        with pytest.raises(nof._lib.NofError) as e:
            m.set_contraction(bad)
        assert e.value.status == 1
    _step(m, synth.blender_rays(n, seed=3), gpu)
    assert np.all(np.isfinite(_grads(m))) and np.any(_grads(m))
    m.close()


def test_unknown_modes_and_the_getter(gpu):
    m = _model(TINY, 4, (64, 64))
    import nof

    assert m.contraction() == 0
    m.set_contraction(1)
    assert m.contraction() == 1
    for bad in (2, -1):
        with pytest.raises(nof._lib.NofError) as e:
            m.set_contraction(bad)
        assert e.value.status == 1
        assert m.contraction() == 1  # a refused call changes nothing
    m.set_contraction(0)
    assert m.contraction() == 0
    m.set_contraction(True)
    assert m.contraction() == 1
    m.close()


# ---- checked build, driver ---------------------------------------------------------------------------------------
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
for prec, stop in ((0, 1), (0, 0), (5, 1)):
    m = nof.AcceleratedMipNeRF(seed=5, max_rays=n, num_samples=(64, 128), precision=prec, stop_level_grad=stop,
                               net_depth=3, net_width=32, net_width_condition=16, skip_layer=2, max_deg_point=4, deg_view=2)
    m.set_ray_grad(True)
    m.set_contraction(1)
    m.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"], float(n))
    torch.cuda.synchronize()
    bits = nof.device_checks(clear=True)
    assert bits == 0, f"precision {prec}: failed checks {bits:#x}"
    og, dg = m.ray_grad()
    assert np.all(np.isfinite(nof.to_numpy(og, (n, 3)))) and np.all(np.isfinite(nof.to_numpy(dg, (n, 3))))
    G = nof.to_numpy(m.mlp.flat_grads()[0], (m.mlp.flat_grads()[1],))
    assert np.all(np.isfinite(G)) and np.any(G)
    m.close()
print("OK")
"""


def test_checked_build_runs_clean(gpu):
    lib = os.path.join(PKG, "lib", "libnof_check.so")
    assert os.path.exists(lib), "build it with: make -C nerf-or-nothing_amd check"
    out = subprocess.run([sys.executable, "-c", CHILD, PKG], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, NOF_LIB=lib))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_driver_trains_contracted(gpu, tmp_path):
    """python -m nof.train --contract --lindisp: test_driver_refines_poses's tiny network and scene with far = 200"""
    rng = np.random.default_rng(3)
    base = np.array([0.2, 0.5, 0.3], f32)
    images = (base + 0.05 * rng.random((V, H, W, 3), dtype=f32)).astype(f32)
    npz = tmp_path / "scene.npz"
    np.savez(npz, poses=_poses(V, seed=1), images=images, focal=FOCAL, near=2.0, far=200.0)
    common = [sys.executable, "-m", "nof.train", "--scene", str(npz), "--contract", "--lindisp", "--batch", "64"]
    cmd = common + ["--precision", "f16p", "--samples", "64", "64", "--net-depth", "3", "--net-width", "32",
                    "--net-width-condition", "16", "--steps", "30", "--print-every", "1", "--lr-init", "5e-3",
                    "--lr-delay-steps", "0", "--ckpt-dir", str(tmp_path)]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"Step \d+/1000000, Loss: (\S+)", out.stdout)]
    print("losses", losses[0], losses[-1])
    assert len(losses) == 30 and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    # the default precision (the fused 8x256) is refused before any step, with the library's message
    bad = subprocess.run(common + ["--steps", "1"], capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert bad.returncode != 0 and "any-shape" in bad.stderr and "Step" not in bad.stdout
