"""GPU parity of the ray and pose gradients (nof_mipnerf_set_ray_grad, nof_dataset_pose_grad) against the
fp64 autograd reference tests/raygrad_ref.py (pinned by finite differences in tests/test_raygrad_cpu.py).

Bounds.  Kernel entry point: rel L2 <= 1e-5 per output, the project's fp32 parity bound (what nof_kernel_encode_grad is
held to).  Whole step, F32: dL/do and dL/dd <= max(1e-5, 4 x e_param), e_param the same run's worst parameter-gradient
tensor error against the same reference (the parent's unchanged arithmetic on the same inputs, the floor
test_gpu_crosslevel.py uses); every ray counts.  F16_PRODUCTS (ReLU decisions adopted): max(2e-3, 4 x e_param).  The
pose reduction: an fp32 sum of at most n terms in any order is within (n - 1) 2^-24 sum |terms| of the exact sum.
DESIGN.md 6f has the measured figures.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_l2
from test_gpu_crosslevel import RAY_BASE, REF8, SEED, STEP, TINY, _dev, _gpu_index, _grads, _model, _net, _params, _step
from test_raygrad_cpu import RAY_SEED
from test_raygen import _poses

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-or-nothing_amd")
TOL = 1e-5
F16P_TOL = 2e-3


def _ray_grads(m, n):
    import nof

    o, d = m.ray_grad()
    return nof.to_numpy(o, (n, 3)), nof.to_numpy(d, (n, 3))


# ---- kernel entry point ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ray_shape", [0, 1])
@pytest.mark.parametrize("max_deg", [4, 16])  # P = 24: half of a sample's 8 threads idle; P = 96
@pytest.mark.parametrize("S", [64, 128])  # two and four 32-sample passes
def test_kernel_ray_grad_matches_autograd(gpu, S, max_deg, ray_shape):
    import torch
    import nof
    import crosslevel_ref as X
    import raygrad_ref as G
    from nof import synth

    n, P, dv_deg = 5, 6 * max_deg, 4
    rng = np.random.default_rng(1000 * S + 10 * max_deg + ray_shape)
    r = synth.blender_rays(n, seed=6)
    t = np.sort(2.0 + 4.0 * rng.random((n, S + 1)), axis=1).astype(np.float32)
    sigma = rng.gamma(1.0, 2.0, (n, S)).astype(np.float32)
    rgb = rng.random((n, S, 3), dtype=np.float32)
    gC = rng.standard_normal((n, 3)).astype(np.float32)
    genc = rng.standard_normal((n * S, P)).astype(np.float32)
    # degree f's features have a derivative 2^f times the feature: dEnc scaled by 2^-f lets every degree, the |d| term
    # and the view term weigh alike in dL/dd (unscaled, degree 15 alone would make up all of it)
    genc *= np.repeat(np.float32(2.0) ** -np.arange(max_deg, dtype=np.float32), 6)[None, :]
    gdir = rng.standard_normal((n, 27)).astype(np.float32)
    dv = {k: _dev(v, gpu) for k, v in dict(t=t, o=r["o"], d=r["d"], radius=r["radius"], sigma=sigma).items()}
    mean, cov = torch.zeros((n, S, 3), device=gpu), torch.zeros((n, S, 3), device=gpu)
    nof._lib.call("nof_kernel_cast_ex", n, S, dv["t"].data_ptr(), dv["o"].data_ptr(), dv["d"].data_ptr(),
                  dv["radius"].data_ptr(), mean.data_ptr(), cov.data_ptr(), None, ray_shape)
    ep96, ed = torch.zeros((n * S, 96), device=gpu), torch.zeros((n, 27), device=gpu)
    nof._lib.call("nof_kernel_encode", n, S, mean.data_ptr(), cov.data_ptr(), dv["d"].data_ptr(), ep96.data_ptr(),
                  ed.data_ptr(), None)
    enc = ep96[:, :P].contiguous()
    # the reference: IPE, the integrator (its dL/dsigma is the kernel's input, its dL/dd the |d| term) and the view PE
    T = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=g)
    results = {}
    for view in (True, False):
        o64, d64, s64 = T(r["o"], True), T(r["d"], True), T(sigma, True)
        m64, c64 = G.cast(T(t), o64, d64, r["radius"], bool(ray_shape))
        f = X.ipe(m64, c64, 0, max_deg)
        Cr, _ = G.render(s64, T(rgb), T(t), d64)
        Lr = (Cr * T(gC)).sum()
        dsig = torch.autograd.grad(Lr, s64, retain_graph=True)[0].numpy().astype(np.float32)
        total = Lr + (f * T(genc.reshape(n, S, P))).sum()
        if view:
            total = total + (G.dir_pe(d64, dv_deg) * T(gdir)).sum()
        total.backward()
        dg, ds, dd = _dev(genc, gpu), _dev(dsig, gpu), _dev(gdir, gpu)
        og, dgr = torch.full((n, 3), 7.0, device=gpu), torch.full((n, 3), 7.0, device=gpu)
        args = [n, S, dv["t"].data_ptr(), dv["o"].data_ptr(), dv["d"].data_ptr(), dv["radius"].data_ptr(), ray_shape, 0,
                max_deg, enc.data_ptr(), dg.data_ptr(), dv["sigma"].data_ptr(), ds.data_ptr(), dv_deg, ed.data_ptr(),
                dd.data_ptr() if view else None]
        nof._lib.call("nof_kernel_ray_grad", *args, 0, og.data_ptr(), dgr.data_ptr(), None)
        torch.cuda.synchronize()
        e_o, e_d = rel_l2(og.cpu().numpy(), o64.grad.numpy()), rel_l2(dgr.cpu().numpy(), d64.grad.numpy())
        print(f"ray_grad S={S} PE (0, {max_deg}) ray_shape {ray_shape} view {view}: do {e_o:.2e} dd {e_d:.2e}")
        assert e_o <= TOL and e_d <= TOL
        # accumulate: added to what is there (x + x is exact)
        o2, d2 = og.clone(), dgr.clone()
        nof._lib.call("nof_kernel_ray_grad", *args, 1, o2.data_ptr(), d2.data_ptr(), None)
        torch.cuda.synchronize()
        assert torch.equal(o2, 2 * og) and torch.equal(d2, 2 * dgr)
        results[view] = dgr.cpu().numpy()
    assert rel_l2(results[False], results[True]) > 100 * TOL  # the view term is there


# ---- whole step --------------------------------------------------------------------------------------------------
def _run(gpu, spec, n, samples, stop, precision=0, adopt=False, ray_grad=True, rays=None, **kw):
    from nof import synth

    r = synth.blender_rays(n, seed=RAY_SEED) if rays is None else rays
    m = _model(spec, n, samples, precision, stop_level_grad=stop, **kw)
    if ray_grad:
        m.set_ray_grad(True)
    _step(m, r, gpu)
    out = dict(G=_grads(m), params=_params(m), lv=[m.level_numpy(l) for l in range(len(samples))],
               masks={l: m.mlp.relu_masks(l) for l in range(len(samples))} if adopt else None, rays=r)
    if ray_grad:
        out["o_grad"], out["d_grad"] = _ray_grads(m, n)
    m.close()
    return out


def _reference(gpu, out, spec, samples, stop, pose=None, **kw):
    import raygrad_ref as G

    D, W, Dc, Wc, skip, lo, hi, dv = spec
    lv = out["lv"]
    return G.step(out["params"], out["rays"], net=_net(spec), samples=samples, min_deg=lo, max_deg=hi, deg_view=dv,
                  seed=SEED, step_idx=STEP, ray_base=RAY_BASE, cylinder=bool(kw.get("ray_shape", 0)),
                  idx=_gpu_index(lv, samples, gpu), t_value={l: lv[l]["t"] for l in range(1, len(samples))},
                  relu=out["masks"], detach=bool(stop), pose=pose)


def _e_param(G, ref, spec):
    import crosslevel_ref as X

    return max(rel_l2(G[o:o + s], ref["grads"][o:o + s]) for _, o, s in X.tensors(_net(spec)))


def _check_step(gpu, spec, n, samples, stop, precision=0, adopt=False, tol=TOL, **kw):
    out = _run(gpu, spec, n, samples, stop, precision, adopt, **kw)
    ref = _reference(gpu, out, spec, samples, stop, **kw)
    e_param = _e_param(out["G"], ref, spec)
    bound = max(tol, 4 * e_param)
    e_o, e_d = rel_l2(out["o_grad"], ref["o_grad"]), rel_l2(out["d_grad"], ref["d_grad"])
    print(f"{spec} {n} x {samples} stop {stop} precision {precision} {kw}: dL/do {e_o:.2e} dL/dd {e_d:.2e} "
          f"(bound {bound:.2e}, e_param {e_param:.2e})")
    assert e_o <= bound and e_d <= bound, (e_o, e_d, bound)


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
            m.set_ray_grad(True)
            m.set_ray_grad(False)
        _step(m, r, gpu)
        tally = {k for k, c in m.mlp.gen_dispatch().items() if c}
        assert tally == set(DISPATCH["configs0_4x128"]), sorted(tally ^ set(DISPATCH["configs0_4x128"]))
        got.append((_grads(m), dict(m.mlp.gen_dispatch())))
        m.close()
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]


@pytest.mark.parametrize("stop", [1, 0])
def test_option_on_leaves_the_parameter_gradient_bitwise(gpu, stop):
    off = _run(gpu, TINY, 3, (64, 64, 64), stop, ray_grad=False)
    on = _run(gpu, TINY, 3, (64, 64, 64), stop)
    assert np.array_equal(off["G"], on["G"])
    for l in range(3):
        for k in ("t", "weights", "comp_rgb"):
            assert np.array_equal(off["lv"][l][k], on["lv"][l][k]), (l, k)


@pytest.mark.parametrize("stop", [1, 0])
def test_deterministic_callback_and_accumulate(gpu, stop):
    import torch
    import nof
    from nof import synth

    n, samples = 8, (64, 64, 64)
    r = synth.blender_rays(n, seed=5)
    runs = [_run(gpu, TINY, n, samples, stop, rays=r) for _ in range(2)]
    for k in ("o_grad", "d_grad", "G"):
        assert np.array_equal(runs[0][k], runs[1][k]), k  # no float atomics: bitwise run to run
    assert np.any(runs[0]["o_grad"]) and np.any(runs[0]["d_grad"])
    # the callback path: bitwise the device path
    b = _model(TINY, n, samples, stop_level_grad=stop)
    b.set_ray_grad(True)
    gc = nof.AcceleratedGradientCalculator(n, b.config)
    b.GetGradient(r["o"], r["d"], r["radius"], r["near"], r["far"], r["lossmult"],
                  lambda comp, level, msum, lm: gc.get_output_gradient(comp, r["pix"], lm, msum, level))
    torch.cuda.synchronize()
    og, dg = _ray_grads(b, n)
    assert np.array_equal(og, runs[0]["o_grad"]) and np.array_equal(dg, runs[0]["d_grad"])
    gc.close(); b.close()
    # two accumulated micro-batches: the ray gradients belong to the call's own rays (the rays are independent)
    h = n // 2
    msum = float(np.sum(r["lossmult"], dtype=np.float32))
    m = _model(TINY, h, samples, stop_level_grad=stop)
    m.set_ray_grad(True)
    for i in range(2):
        p = {k: v[i * h:(i + 1) * h] for k, v in r.items()}
        m.set_rng(SEED, STEP, RAY_BASE + i * h)
        d = {k: _dev(v, gpu) for k, v in p.items()}
        m.get_gradient_device(h, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"], msum,
                              accumulate=i > 0, publish=i == 1)
        torch.cuda.synchronize()
        og, dg = _ray_grads(m, h)
        assert np.array_equal(og, runs[0]["o_grad"][i * h:(i + 1) * h]), i
        assert np.array_equal(dg, runs[0]["d_grad"][i * h:(i + 1) * h]), i
    m.close()


# ---- pose gradients ----------------------------------------------------------------------------------------------
V, W, H, SCALES, NP = 4, 40, 24, 2, 37
FOCAL = float(np.float32(0.5 * W / np.tan(0.5 * 0.6911112)))
DS_SEED, DS_STEP = 11, 6645  # this batch of 37 draws no ray of view 2, and rays of both scales (asserted below)


def _scene(gpu, ndc=False, poses=None):
    import torch

    images = np.random.default_rng(7).random((V, H, W, 3), dtype=np.float32)
    return dict(poses=_poses(V, seed=1, llff=ndc) if poses is None else poses, width=W, height=H, focal=FOCAL, near=2.0,
                far=6.0, ndc=ndc, images=torch.from_numpy(images).to(gpu), num_scales=SCALES)


def _view_cam(idx):
    """record index -> (view, pixel_dir's camera-space direction in fp32) by the multiscale layout"""
    first1 = V * W * H
    view, cam = np.zeros(len(idx), np.int64), np.zeros((len(idx), 3), np.float32)
    for r, i in enumerate(idx):
        s = int(i >= first1)
        w, h, f = W >> s, H >> s, np.float32(FOCAL) / np.float32(1 << s)
        local = int(i) - s * first1
        view[r], pix = divmod(local, w * h)
        y, x = divmod(pix, w)
        cam[r] = [(np.float32(x) - np.float32(w) * np.float32(0.5) + np.float32(0.5)) / f,
                  -(np.float32(y) - np.float32(h) * np.float32(0.5) + np.float32(0.5)) / f, -1.0]
    return view, cam


def _batch(ds, n, step=DS_STEP):
    import torch
    import nof

    b, msum = ds.next(n, DS_SEED, step, 0)
    torch.cuda.synchronize()
    rays = {k: nof.to_numpy(b[k][0], b[k][1]).copy() for k in ("o", "d", "radius", "near", "far", "lossmult", "pix")}
    return b, msum, rays, nof.to_numpy(b["record_index"][0], (n,), np.int32).copy()


def test_pose_grad_reduction(gpu):
    import torch
    import nof

    ds = nof.RayDataset(scene=_scene(gpu))
    b, msum, rays, idx = _batch(ds, NP)
    view, cam = _view_cam(idx)
    assert not np.any(view == 2) and all(np.any(view == v) for v in (0, 1, 3))
    assert np.any(idx >= V * W * H) and np.any(idx < V * W * H)
    # the step's own ray gradients
    m = nof.AcceleratedMipNeRF(seed=SEED, max_rays=NP, num_samples=(64, 64), num_levels=2,
                               **dict(net_depth=3, net_width=32, net_depth_condition=1, net_width_condition=16,
                                      skip_layer=2, min_deg_point=0, max_deg_point=4, deg_view=2))
    m.set_ray_grad(True)
    m.set_rng(SEED, STEP, RAY_BASE)
    p = {k: v[0] for k, v in b.items()}
    m.get_gradient_device(NP, p["o"], p["d"], p["radius"], p["near"], p["far"], p["lossmult"], p["pix"], msum)
    torch.cuda.synchronize()
    og_p, dg_p = m.ray_grad()
    og, dg = _ray_grads(m, NP)
    got = ds.pose_grad(og_p, dg_p, NP)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    # against an fp64 sum of the same fp32 terms
    terms = np.zeros((NP, V, 12), np.float32)
    for r in range(NP):
        terms[r, view[r], :9] = (dg[r][:, None] * cam[r][None, :]).reshape(9)  # fp32 products, as the kernel's
        terms[r, view[r], 9:] = og[r]
    want = terms.astype(np.float64).sum(0)
    slack = (NP - 1) * 2.0 ** -24 * np.abs(terms.astype(np.float64)).sum(0)
    assert np.all(np.abs(g - want) <= slack), np.max(np.abs(g - want) - slack)
    assert np.any(g[0]) and not np.any(g[2])  # the empty view: exactly 0
    # bitwise repeatable; accumulate adds, and leaves the empty view's row as it is
    again = ds.pose_grad(og_p, dg_p, NP)
    acc = torch.full((V, 12), 3.0, device=gpu)
    ds.pose_grad(og_p, dg_p, NP, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(again, got)
    assert torch.equal(acc, got + 3.0) and torch.all(acc[2] == 3.0)
    # end to end against the reference's pose gradient
    out = dict(G=_grads(m), params=_params(m), lv=[m.level_numpy(l) for l in range(2)], masks=None, rays=rays)
    ref = _reference(gpu, out, TINY, (64, 64), 1, pose=(ds.poses(), view, cam))
    bound = max(TOL, 4 * _e_param(out["G"], ref, TINY))
    e = rel_l2(g, ref["pose_grad"])
    print(f"pose gradient [V][12]: rel L2 {e:.2e} (bound {bound:.2e}); dL/do {rel_l2(og, ref['o_grad']):.2e} "
          f"dL/dd {rel_l2(dg, ref['d_grad']):.2e}")
    assert e <= bound
    m.close(); ds.close()


def test_set_poses_round_trip_and_use(gpu):
    import torch
    import nof

    P0 = _poses(V, seed=1)
    P1 = _poses(V, seed=2)
    ds = nof.RayDataset(scene=_scene(gpu))
    assert np.array_equal(ds.poses(), P0)
    before = ds.materialize()
    ds.set_poses(P1)
    assert np.array_equal(ds.poses(), P1)  # exact
    fresh = nof.RayDataset(scene=_scene(gpu, poses=P1))
    after, want = ds.materialize(), fresh.materialize()
    assert torch.equal(after, want) and not torch.equal(after, before)
    # the next batch and render_view use the new poses
    _, _, a, ia = _batch(ds, NP, step=3)
    _, _, w, iw = _batch(fresh, NP, step=3)
    assert np.array_equal(ia, iw) and all(np.array_equal(a[k], w[k]) for k in a)
    m = nof.AcceleratedMipNeRF(seed=SEED, max_rays=256, num_samples=(64, 64), net_depth=3, net_width=32,
                               net_width_condition=16, skip_layer=2, max_deg_point=4, deg_view=2)
    ra = ds.render_view(m, view=1, scale=1, score=False, outputs=("rgb",))
    rw = fresh.render_view(m, view=1, scale=1, score=False, outputs=("rgb",))
    torch.cuda.synchronize()
    assert torch.equal(ra["rgb"][1], rw["rgb"][1])
    m.close(); ds.close(); fresh.close()


# ---- refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 4])
def test_fused_objects_refuse_and_stay_usable(gpu, precision):
    import nof
    from nof import synth

    n = 4
    m = nof.AcceleratedMipNeRF(seed=1, max_rays=n, num_samples=(64, 64), precision=precision)  # the fused 8x256
    with pytest.raises(nof._lib.NofError) as e:
        m.set_ray_grad(True)
    assert e.value.status == 5 and "any-shape" in str(e.value)
    m.set_ray_grad(False)  # nothing to switch off: accepted
    with pytest.raises(nof._lib.NofError) as e:
        m.ray_grad()
    assert e.value.status == 1
    _step(m, synth.blender_rays(n, seed=3), gpu)
    assert np.all(np.isfinite(_grads(m))) and np.any(_grads(m))
    m.close()


def test_dataset_refusals_and_ray_grad_before_a_step(gpu):
    import torch
    import nof
    from nof import synth

    z = torch.zeros((NP, 3), device=gpu)
    out = torch.zeros((V, 12), device=gpu)
    ndc = nof.RayDataset(scene=_scene(gpu, ndc=True))
    ndc.next(NP, DS_SEED, 1, 0)
    with pytest.raises(nof._lib.NofError) as e:
        ndc.pose_grad(z, z, NP, out=out)
    assert e.value.status == 5 and "NDC" in str(e.value)
    ndc.next(NP, DS_SEED, 2, 0)  # still usable
    rec = nof.RayDataset(records=synth.pack_records(synth.blender_rays(64, seed=1)))
    rec.next(NP, DS_SEED, 1, 0)
    for call in (lambda: rec.pose_grad(z, z, NP, out=out), rec.poses, lambda: rec.set_poses(np.zeros((V, 12)))):
        with pytest.raises(nof._lib.NofError) as e:
            call()
        assert e.value.status == 5
    rec.next(NP, DS_SEED, 2, 0)
    ok = nof.RayDataset(scene=_scene(gpu))
    with pytest.raises(nof._lib.NofError) as e:  # no batch yet
        ok.pose_grad(z, z, NP, out=out)
    assert e.value.status == 1
    torch.cuda.synchronize()
    assert not torch.any(out)  # refused before any launch
    m = _model(TINY, 4, (64, 64))
    m.set_ray_grad(True)
    with pytest.raises(nof._lib.NofError) as e:
        m.ray_grad()
    assert e.value.status == 1
    m.close(); ndc.close(); rec.close(); ok.close()


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
    m.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"], float(n))
    torch.cuda.synchronize()
    bits = nof.device_checks(clear=True)
    assert bits == 0, f"precision {prec}: failed checks {bits:#x}"
    og, dg = m.ray_grad()
    assert np.all(np.isfinite(nof.to_numpy(og, (n, 3)))) and np.all(np.isfinite(nof.to_numpy(dg, (n, 3))))
    m.close()
print("OK")
"""


def test_checked_build_runs_clean(gpu):
    lib = os.path.join(PKG, "lib", "libnof_check.so")
    assert os.path.exists(lib), "build it with: make -C nerf-or-nothing_amd check"
    out = subprocess.run([sys.executable, "-c", CHILD, PKG], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, NOF_LIB=lib))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_driver_refines_poses(gpu, tmp_path):
    """python -m nof.train --refine-poses: tiny network, 64 rays x (64, 64), 30 steps on a scene of smooth images"""
    rng = np.random.default_rng(3)
    base = np.array([0.2, 0.5, 0.3], np.float32)
    images = (base + 0.05 * rng.random((V, H, W, 3), dtype=np.float32)).astype(np.float32)
    poses = _poses(V, seed=1)
    npz = tmp_path / "scene.npz"
    np.savez(npz, poses=poses, images=images, focal=FOCAL, near=2.0, far=6.0)
    cmd = [sys.executable, "-m", "nof.train", "--scene", str(npz), "--refine-poses", "1e-3", "--precision", "f16p",
           "--batch", "64", "--samples", "64", "64", "--net-depth", "3", "--net-width", "32", "--net-width-condition", "16",
           "--steps", "30", "--print-every", "1", "--lr-init", "5e-3", "--lr-delay-steps", "0", "--ckpt-dir", str(tmp_path)]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"Step \d+/1000000, Loss: (\S+)", out.stdout)]
    print("losses", losses[0], losses[-1])
    assert len(losses) == 30 and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    refined = np.load(tmp_path / "poses_refined.npy")
    assert refined.shape == (V, 12) and refined.dtype == np.float32 and not np.array_equal(refined, poses)
    for v in range(V):
        Rm = refined[v, :9].reshape(3, 3).astype(np.float64)
        assert np.max(np.abs(Rm @ Rm.T - np.eye(3))) <= 1e-5, v
    # a fused precision is refused before training, with the library's message
    bad = subprocess.run([sys.executable, "-m", "nof.train", "--scene", str(npz), "--refine-poses", "1e-3", "--steps", "1",
                          "--batch", "64"], capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert bad.returncode != 0 and "any-shape" in bad.stderr and "Step" not in bad.stdout
