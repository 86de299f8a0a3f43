"""GPU parity of the distortion loss (nof_config.distortion_loss_mult) against the fp64 reference
tests/distortion_ref.py (pinned by the O(S^2) definition and finite differences in tests/test_distortion_cpu.py).

Bounds: rel L2 <= 1e-5 (the project's fp32 contract: the integrator and the term are fp32 in every precision mode);
F16_PRODUCTS whole step with the ReLU decisions adopted: 2e-3, the mode's contract.  Wherever a gradient is compared
with the term on, it must also differ from the reference WITHOUT the term by more than 100 x its bound: a kernel that
dropped the term would fail.
"""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
F16P_TOL = 2e-3

# The multipliers and the ray seed below were chosen from the fp64 reference alone (distortion_ref on the CPU, Glorot
# parameters of seed 0x51 and its own bin indices), before any GPU gradient was looked at with them, so that the term
# is large against the bounds.  Kernel entry: with KERNEL_MULT = 1 the reference's dsigma differs from its
# dist_mult = 0 value by 0.096 .. 0.31 (rel L2 over S = 64 .. 512 and both lindisp).  Whole step (tiny 3x32 network,
# synth.blender_rays seed 7, the seed of tests/test_gpu_crosslevel.py): with STEP_MULT = 1 the reference's smallest
# per-tensor difference from the multiplier-0 reference over the trunk and the density head (W0 each time) is 0.78 at
# 5 rays x (64, 128) with stop_level_grad = 1, 0.79 with 0 (level 1's dL/dt: 1.65, level 0's dL/dw: 0.84), and 0.71 at
# 5 rays x (64, 64, 64) (seeds 23 / 2: 0.57 .. 0.63): above 100 x 2e-3, what the F16_PRODUCTS case needs, and far
# above 100 x 1e-5.  Each test asserts the difference again on its own reference.
KERNEL_MULT = 1.0
STEP_MULT = 1.0
RAY_SEED = 7
NEAR, FAR = 2.0, 6.0


def _dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---- kernel entry points -------------------------------------------------------------------------------------
def _kernel_inputs(S):
    """n = 5: one full block of four waves plus a partial one.  Inputs as test_render_grad_ex_matches_autograd
    (strictly increasing random t inside [near, far], gamma sigma); ray 0: sigma = 0; ray 1: lossmult = 0;
    ray 2: far = near; ray 3: a single dense sample; ray 4 (the partial block): an ordinary diffuse ray."""
    from nof import synth

    n = 5
    rng = np.random.default_rng(1000 + S)
    r = synth.blender_rays(n, seed=4)
    sigma = rng.gamma(1.0, 2.0, (n, S)).astype(np.float32)
    sigma[0] = 0.0
    sigma[3] = 0.0
    sigma[3, S // 3] = 400.0
    rgb = rng.random((n, S, 3), dtype=np.float32)
    t = np.sort(NEAR + (FAR - NEAR) * rng.random((n, S + 1)), axis=1).astype(np.float32)
    assert np.all(np.diff(t, axis=1) > 0) and t.min() > NEAR and t.max() < FAR
    lm = np.ones(n, np.float32)
    lm[1] = 0.0
    near = np.full(n, NEAR, np.float32)
    far = np.full(n, FAR, np.float32)
    far[2] = near[2]
    pix = rng.random((n, 3), dtype=np.float32)
    q = rng.standard_normal((n, S)).astype(np.float32)
    return dict(n=n, S=S, sigma=sigma, rgb=rgb, t=t, d=r["d"], lm=lm, near=near, far=far, pix=pix, q=q)


def _kernel_ref(inp, mult, lindisp, q):
    """X.render + distortion in fp64: sum mu |C - pix|^2 / sum mu (+ sum w q) + the term; dL/dsigma, dL/drgb, dL/dt"""
    import torch
    import crosslevel_ref as X
    import distortion_ref as D

    sg = torch.tensor(inp["sigma"].astype(np.float64), requires_grad=True)
    cg = torch.tensor(inp["rgb"].astype(np.float64), requires_grad=True)
    tg = torch.tensor(inp["t"].astype(np.float64), requires_grad=True)
    C, w = X.render(sg, cg, tg, inp["d"], True)
    lm = torch.from_numpy(inp["lm"]).double()
    msum = float(np.sum(inp["lm"], dtype=np.float32))
    loss = (lm[:, None] * (C - torch.from_numpy(inp["pix"]).double()) ** 2).sum() / msum
    if q:
        loss = loss + (w * torch.from_numpy(inp["q"]).double()).sum()
    dist, rays = D.term(w, tg, inp["near"], inp["far"], inp["lm"], mult, lindisp)
    (loss + dist).backward()
    return dict(dsigma=sg.grad.numpy(), drgb=cg.grad.numpy(), dt=tg.grad.numpy(), dist_rays=rays.detach().numpy())


def _kernel_run(gpu, inp, mult, lindisp, q, entry="nof_kernel_render_grad_dist"):
    """the entry point on the inputs; returns dsigma, drgb, dt (cross form), dist_rays as numpy"""
    import torch
    import nof

    n, S = inp["n"], inp["S"]
    dv = {k: _dev(inp[k], gpu) for k in ("sigma", "rgb", "t", "d", "lm", "near", "far", "pix", "q")}
    Cc, w = torch.zeros((n, 3), device=gpu), torch.zeros((n, S), device=gpu)
    nof._lib.call("nof_kernel_render", n, S, dv["sigma"].data_ptr(), dv["rgb"].data_ptr(), dv["t"].data_ptr(),
                  dv["d"].data_ptr(), 1, Cc.data_ptr(), w.data_ptr(), None)
    Z = lambda *s: torch.full(s, 7.0, device=gpu)
    ds, dc, dt, dr = Z(n, S), Z(n, S, 3), Z(n, S + 1), Z(n)
    msum = float(np.sum(inp["lm"], dtype=np.float32))
    args = [n, S, dv["sigma"].data_ptr(), dv["rgb"].data_ptr(), dv["t"].data_ptr(), dv["d"].data_ptr(), 1, Cc.data_ptr(),
            None, dv["pix"].data_ptr(), dv["lm"].data_ptr(), msum, 1.0, ds.data_ptr(), dc.data_ptr(),
            dv["q"].data_ptr() if q else None, dt.data_ptr() if q else None]
    if entry == "nof_kernel_render_grad_dist":
        args += [dv["near"].data_ptr(), dv["far"].data_ptr(), lindisp, mult, dr.data_ptr()]
    nof._lib.call(entry, *args, None)
    torch.cuda.synchronize()
    return dict(dsigma=ds.cpu().numpy(), drgb=dc.cpu().numpy(), dt=dt.cpu().numpy(), dist_rays=dr.cpu().numpy())


@pytest.mark.parametrize("lindisp", [0, 1])
@pytest.mark.parametrize("S", [64, 128, 256, 512])
def test_kernel_matches_autograd(gpu, S, lindisp):
    """k_render_bwd<PER, true> (dev_w_grad = dev_t_grad = NULL), every PER"""
    inp = _kernel_inputs(S)
    got = _kernel_run(gpu, inp, KERNEL_MULT, lindisp, q=False)
    ref = _kernel_ref(inp, KERNEL_MULT, lindisp, q=False)
    ref0 = _kernel_ref(inp, 0.0, lindisp, q=False)
    errs = {k: rel_l2(got[k], ref[k]) for k in ("dsigma", "drgb", "dist_rays")}
    away = rel_l2(got["dsigma"], ref0["dsigma"])
    print(f"render_grad_dist S={S} lindisp={lindisp}: {errs}; dsigma vs the reference without the term {away:.3g}; "
          f"dist_rays {got['dist_rays']}")
    assert all(np.all(np.isfinite(got[k])) for k in ("dsigma", "drgb", "dist_rays"))
    assert got["dist_rays"][0] == 0.0  # sigma = 0: exactly nothing
    assert got["dist_rays"][1] == 0.0 and got["dist_rays"][2] == 0.0  # lossmult = 0; far = near
    assert got["dist_rays"][3] > 0.0 and got["dist_rays"][4] > 0.0
    # far = near: no term, so the photometric adjoint alone
    assert rel_l2(got["dsigma"][2], ref0["dsigma"][2]) <= TOL
    for k, e in errs.items():
        assert e <= TOL, f"{k}: rel L2 {e:.3g}"
    assert rel_l2(ref["dsigma"], ref0["dsigma"]) > 100 * TOL  # (the choice of KERNEL_MULT, from the reference)
    assert away > 100 * TOL


@pytest.mark.parametrize("lindisp", [0, 1])
@pytest.mark.parametrize("S", [64, 128, 256, 512])
def test_kernel_cross_form_matches_autograd(gpu, S, lindisp):
    """k_render_bwd_x<PER, true>: a random q and a t_grad buffer"""
    inp = _kernel_inputs(S)
    got = _kernel_run(gpu, inp, KERNEL_MULT, lindisp, q=True)
    ref = _kernel_ref(inp, KERNEL_MULT, lindisp, q=True)
    ref0 = _kernel_ref(inp, 0.0, lindisp, q=True)
    errs = {k: rel_l2(got[k], ref[k]) for k in ("dsigma", "drgb", "dt", "dist_rays")}
    away = {k: rel_l2(got[k], ref0[k]) for k in ("dsigma", "dt")}
    print(f"render_grad_dist (cross) S={S} lindisp={lindisp}: {errs}; vs the reference without the term {away}")
    assert all(np.all(np.isfinite(got[k])) for k in ("dsigma", "drgb", "dt", "dist_rays"))
    assert not np.any(got["dt"][0]) and not np.any(ref["dt"][0])  # sigma = 0: t does not matter
    assert got["dist_rays"][0] == 0.0 and got["dist_rays"][2] == 0.0
    for k, e in errs.items():
        assert e <= TOL, f"{k}: rel L2 {e:.3g}"
    assert away["dsigma"] > 100 * TOL and away["dt"] > 100 * TOL


@pytest.mark.parametrize("S", [64, 128, 256, 512])
def test_kernel_mult_zero_is_render_grad_ex_bitwise(gpu, S):
    inp = _kernel_inputs(S)
    for q in (False, True):
        a = _kernel_run(gpu, inp, 0.0, 1, q=q)
        b = _kernel_run(gpu, inp, 0.0, 0, q=q, entry="nof_kernel_render_grad_ex")
        keys = ("dsigma", "drgb") + (("dt",) if q else ())
        for k in keys:
            assert a[k].tobytes() == b[k].tobytes(), (q, k)
        assert not np.any(a["dist_rays"])


# ---- whole steps -------------------------------------------------------------------------------------------------
def _rays(n):
    from nof import synth

    return synth.blender_rays(n, seed=RAY_SEED)


@pytest.mark.parametrize("precision", [0, 1, 2, 3, 4, 5])
def test_every_precision_mode(gpu, precision):
    """The reference 8x256 network, stop_level_grad = 1: the last level's adjoint against fp64 autograd of that
    level's own t, density, rgb, pixels and loss multipliers (photometric + distortion)."""
    import distortion_ref as D
    import test_gpu_crosslevel as XL

    n, samples, mult = 32, (64, 128), STEP_MULT
    r = _rays(n)
    r["lossmult"] = r["lossmult"].copy()
    r["lossmult"][3] = 0.0
    r["lossmult"][5] = 2.0
    runs = []
    for lam in (mult, mult, 0.0):
        m = XL._model(XL.REF8, n, samples, precision, distortion_loss_mult=lam)
        XL._step(m, r, gpu)
        runs.append(dict(lv=[m.level_numpy(l) for l in range(2)], G=XL._grads(m), loss=m.loss(),
                         dist=m.distortion_loss(), status=m.numeric_status()))
        m.close()
    a, b, z = runs
    assert a["status"] == 0 and z["status"] == 0
    # two runs: the same bits (no float atomics, fixed summation orders)
    assert a["G"].tobytes() == b["G"].tobytes() and a["dist"] == b["dist"]
    for l in range(2):
        for k in ("density_grad", "rgb_grad"):
            assert a["lv"][l][k].tobytes() == b["lv"][l][k].tobytes()
    # the forward, the photometric loss and the coarse level's adjoint are those of a model without the term
    assert a["loss"] == z["loss"] and z["dist"] == 0.0
    for k in ("t", "weights", "comp_rgb", "density", "rgb"):
        assert a["lv"][1][k].tobytes() == z["lv"][1][k].tobytes(), k
    assert a["lv"][0]["density_grad"].tobytes() == z["lv"][0]["density_grad"].tobytes()
    assert a["lv"][0]["rgb_grad"].tobytes() == z["lv"][0]["rgb_grad"].tobytes()
    lv = a["lv"][1]
    kw = dict(sigma=lv["density"], rgb=lv["rgb"], t=lv["t"], d=r["d"], pix=r["pix"], lossmult=r["lossmult"],
              near=r["near"], far=r["far"])
    ref = D.level_grads(mult=mult, **kw)
    ref0 = D.level_grads(mult=0.0, **kw)
    e_s, e_c = rel_l2(lv["density_grad"], ref["dsigma"]), rel_l2(lv["rgb_grad"], ref["drgb"])
    e_d = abs(a["dist"] - ref["dist"]) / abs(ref["dist"])
    away = rel_l2(lv["density_grad"], ref0["dsigma"])
    print(f"precision {precision}: density_grad {e_s:.2e} rgb_grad {e_c:.2e} distortion_loss {e_d:.2e} "
          f"({a['dist']:.6g}; photometric {a['loss']:.6g}); density_grad vs the reference without the term {away:.3g}")
    assert e_s <= TOL and e_c <= TOL and e_d <= TOL
    assert away > 100 * TOL
    assert rel_l2(z["lv"][1]["density_grad"], ref0["dsigma"]) <= TOL


def _whole_step(gpu, n, samples, precision, stop, adopt, tol, mult=STEP_MULT):
    import crosslevel_ref as X
    import distortion_ref as D
    import test_gpu_crosslevel as XL

    r = _rays(n)
    m = XL._model(XL.TINY, n, samples, precision, stop_level_grad=stop, distortion_loss_mult=mult)
    XL._step(m, r, gpu)
    L = len(samples)
    lv = [m.level_numpy(l) for l in range(L)]
    G, params = XL._grads(m), XL._params(m)
    masks = {l: m.mlp.relu_masks(l) for l in range(L)}
    cross = [m.cross_numpy(l) for l in range(L)]
    loss, dist = m.loss(), m.distortion_loss()
    assert m.numeric_status() == 0
    m.close()
    idx = XL._gpu_index(lv, samples, gpu)  # the GPU's bin indices and t-values, as _run_pair adopts them
    D_, W, Dc, Wc, skip, lo, hi, dv = XL.TINY
    net = XL._net(XL.TINY)
    rk = dict(net=net, samples=samples, min_deg=lo, max_deg=hi, deg_view=dv, seed=XL.SEED, step_idx=XL.STEP,
              ray_base=XL.RAY_BASE, idx=idx, t_value={l: lv[l]["t"] for l in range(1, L)},
              relu=masks if adopt else None, detach=bool(stop))
    ref = D.step(params, r, mult, **rk)
    ref0 = D.step(params, r, 0.0, **rk)
    lines, bad = [], []
    for i, (name, o, s) in enumerate(X.tensors(net)):
        sl = slice(o, o + s)
        e, away, chosen = rel_l2(G[sl], ref["grads"][sl]), rel_l2(G[sl], ref0["grads"][sl]), \
            rel_l2(ref["grads"][sl], ref0["grads"][sl])
        lines.append(f"{name}: {e:.2e} (bound {tol:.0e}); vs no term {away:.3g} (the reference's own {chosen:.3g})")
        if not e <= tol:
            bad.append(f"{name}: rel L2 {e:.3g} > {tol:.3g}")
        if i % net.L < net.D and not away > 100 * tol:  # every trunk tensor carries the term
            bad.append(f"{name}: differs from the reference without the term by only {away:.3g}")
    print(f"{n} x {samples} precision {precision} stop_level_grad {stop}:\n  " + "\n  ".join(lines))
    assert abs(loss - ref["loss"]) <= max(tol, 1e-5) * abs(ref["loss"])
    assert abs(dist - ref["dist"]) <= max(tol, 1e-5) * abs(ref["dist"])
    assert not bad, "\n".join(bad)
    return cross, ref, ref0


def test_step_f32_stop_level_grad_1(gpu):
    cross, _, _ = _whole_step(gpu, 5, (64, 128), 0, 1, False, TOL)
    assert all(c == {"w_grad": None, "t_grad": None} for c in cross)


def test_step_f32_stop_level_grad_0(gpu):
    """the term's dL/dt joins the integrator's in level 1's t gradient and reaches level 0's weights through the
    resampler adjoint"""
    cross, ref, ref0 = _whole_step(gpu, 5, (64, 128), 0, 0, False, TOL)
    e_t, e_w = rel_l2(cross[1]["t_grad"], ref["t_grad"][1]), rel_l2(cross[0]["w_grad"], ref["w_grad"][0])
    a_t, a_w = rel_l2(cross[1]["t_grad"], ref0["t_grad"][1]), rel_l2(cross[0]["w_grad"], ref0["w_grad"][0])
    print(f"level 1 dL/dt {e_t:.2e}, level 0 dL/dw {e_w:.2e}; vs no term {a_t:.3g}, {a_w:.3g}")
    assert e_t <= TOL and e_w <= TOL
    assert a_t > 100 * TOL and a_w > 100 * TOL


def test_step_f16_products_stop_level_grad_0(gpu):
    _whole_step(gpu, 5, (64, 128), 5, 0, True, F16P_TOL)


def test_step_three_levels(gpu):
    """(64, 64, 64), stop_level_grad = 0: only the last level carries the term (the reference puts it there alone and
    every tensor agrees), and it reaches level 0 through two resamplers"""
    cross, ref, ref0 = _whole_step(gpu, 5, (64, 64, 64), 0, 0, False, TOL)
    for l, key in ((2, "t_grad"), (1, "w_grad"), (1, "t_grad"), (0, "w_grad")):
        e, away = rel_l2(cross[l][key], ref[key][l]), rel_l2(cross[l][key], ref0[key][l])
        print(f"level {l} {key}: {e:.2e}; vs no term {away:.3g}")
        assert away > 100 * TOL, (l, key)


# ---- unchanged behaviour -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,spec,kw", [(4, "REF8", {}), (0, "TINY", {"stop_level_grad": 0})])
def test_multiplier_zero_is_the_default_bitwise(gpu, precision, spec, kw):
    import test_gpu_crosslevel as XL

    n, samples = 16, (64, 128)
    r = _rays(n)
    got = []
    for extra in ({}, {"distortion_loss_mult": 0.0}):
        m = XL._model(getattr(XL, spec), n, samples, precision, **kw, **extra)
        XL._step(m, r, gpu)
        got.append((XL._grads(m), m.loss(), m.distortion_loss()))
        m.close()
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1] == got[1][1]
    assert got[0][2] == 0.0 and got[1][2] == 0.0


def _mean_distortion(lv, near, far):
    """the unmultiplied mean L_r of a level, in numpy fp64 (the O(S) closed form on sorted t)"""
    w, t = lv["weights"].astype(np.float64), lv["t"].astype(np.float64)
    s = (t - near[:, None]) / (far - near)[:, None]
    m, dl = (s[:, :-1] + s[:, 1:]) / 2, s[:, 1:] - s[:, :-1]
    A = np.cumsum(w, 1) - w
    P = np.cumsum(w * m, 1) - w * m
    B = w.sum(1, keepdims=True) - A - w
    Q = (w * m).sum(1, keepdims=True) - P - w * m
    return float(np.mean((w * (m * (A - B) - (P - Q))).sum(1) + (w * w * dl).sum(1) / 3))


def test_training_smoke(gpu):
    """300 Adam steps of the tiny network on 64 synthetic rays x (64, 64), with the term (lambda_d = 0.1) and without:
    the regularised run ends with the lower mean L_r (what the term is for), both photometric losses finite."""
    import torch
    import nof
    import test_gpu_crosslevel as XL

    n, samples = 64, (64, 64)
    r = _rays(n)
    d = {k: _dev(v, gpu) for k, v in r.items()}
    msum = float(np.sum(r["lossmult"], dtype=np.float32))
    out = {}
    for lam in (0.1, 0.0):
        m = XL._model(XL.TINY, n, samples, distortion_loss_mult=lam)
        opt = nof.AcceleratedAdamOptimizer(m.GetLayerSizes(), m.config)
        for it in range(300):
            m.set_rng(XL.SEED, it, 0)
            g = m.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"], msum)
            opt.step(m.mlp.allParams, g, 5e-3)
        m.set_rng(XL.SEED, 300, 0)  # one evaluation step on the same samples for both runs
        m.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"], msum)
        torch.cuda.synchronize()
        out[lam] = (m.loss(), _mean_distortion(m.level_numpy(1), r["near"].astype(np.float64), r["far"].astype(np.float64)),
                    m.distortion_loss())
        opt.close(); m.close()
    print(f"after 300 steps: with the term loss {out[0.1][0]:.5f} mean L_r {out[0.1][1]:.5f} (term {out[0.1][2]:.5f}); "
          f"without loss {out[0.0][0]:.5f} mean L_r {out[0.0][1]:.5f}")
    assert np.isfinite(out[0.1][0]) and np.isfinite(out[0.0][0])
    assert abs(out[0.1][2] - 0.1 * out[0.1][1]) <= 1e-4 * abs(out[0.1][2])  # lossmult = 1: the term is lambda_d mean L_r
    assert out[0.1][1] < out[0.0][1]
