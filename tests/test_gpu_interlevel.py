"""GPU parity of the interlevel (proposal) loss (nof_mipnerf_set_interlevel_loss) against the fp64
reference tests/interlevel_ref.py (pinned by its closed forms and finite differences in tests/test_interlevel_cpu.py).

Bounds: rel L2 <= 1e-5 (the project's fp32 contract: k_interlevel and the integrator adjoint are fp32 on stored values
in every precision mode); F16_PRODUCTS whole step with the ReLU decisions adopted: 2e-3, the mode's contract.  Wherever
a gradient is compared with the term on, it must also differ from the reference WITHOUT the term by more than 100 x its
bound: a step that dropped the term would fail.

The references evaluate the term at the weights the library stored (interlevel_ref.level_grads / step, w_value=: the
value of the stored fp32 w, the derivative of the fp64 w, crosslevel_ref._snap as for the resampler's cdf).  The
term's g_i = -2 (w_i - bound_i) / (w_i + eps) is O(1) at any weight magnitude, and the integrator's fp32
alpha = 1 - exp(-sigma delta) is off by up to 6e-8 absolute, percents of a thin region's weight: against a reference
that recomputes w^ from the stored density in fp64, level 0's density gradient of test_every_precision_mode measured
4.7e-2; against the one that takes the derivative where the library evaluates it, 6.5e-7.

The term is zero at a Glorot initialisation: the levels share one MLP, the densities are smooth, and a coarse weight
histogram of a smooth density is an envelope of the fine one already (that is what the loss asks for).  So the
whole-step cases install parameters under which it is not, `_install`: the Glorot draw times `scale`, the density
head's weights times `head` on top, its bias raised by `bias` (a rougher density).  The recipes and the multipliers
below were chosen from the fp64 reference alone (interlevel_ref.step on the CPU with torch_ref.glorot(net, 0x51) and
its own bin indices).  At multiplier 1 the reference's gradient differs from its multiplier-0 gradient, per tensor
over the trunk, by at least: 8x256, 32 rays x (64, 128), scale 2: 0.44 (22 % of the fine intervals with an active
hinge); tiny: 5 rays x (64, 128), density head x 32: 0.0238 (term 1.2e-4; x 16: 0.0081); 3 rays x (64, 64, 64),
density head x 8, bias + 2: 0.0123 (levels 0 and 1: 7.2e-5 and 5.9e-5).  The difference is linear in the multiplier,
so TINY_MULT = 100 puts the tiny cases above 100 x 2e-3, what the F16_PRODUCTS case needs.  Each test asserts the
difference again on its own reference.  (Rougher recipes were dropped for what they do to the PHOTOMETRIC gradient,
term or no term: the whole draw x 3 puts F16_PRODUCTS' at 5e-3, view branch included; the density head x 32 puts the
view branch of the F32 (64, 64, 64) step at 1.2e-5.)
"""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
F16P_TOL = 2e-3
REF8_MULT, REF8_RECIPE = 1.0, (2.0, 1.0, 0.0)  # (scale, head, bias)
TINY_MULT = 100.0
TINY_RECIPE = {(64, 128): (1.0, 32.0, 0.0), (64, 64, 64): (1.0, 8.0, 2.0)}
RAY_SEED = 7
KERNEL_CASES = [(64, 64), (64, 128), (128, 64), (64, 512), (512, 64), (512, 512)]
_KREF = {}


def _dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---- the kernel entry point ----------------------------------------------------------------------------------------
def _kernel_case(Sc, Sf):
    """the shared generator's case and its fp64 reference at mult = 1, computed once (read only)"""
    import interlevel_ref as IL

    if (Sc, Sf) not in _KREF:
        inp = IL.make_inputs(Sc, Sf)
        _KREF[(Sc, Sf)] = (inp, IL.kernel_ref(inp, 1.0))
    return _KREF[(Sc, Sf)]


def _kernel_run(gpu, inp, mult, accumulate=False, q0=None):
    import torch
    import nof

    n, Sc, Sf = inp["n"], inp["Sc"], inp["Sf"]
    dv = {k: _dev(inp[k], gpu) for k in ("tp", "wp", "t", "w", "lm")}
    q = torch.full((n, Sc), 7.0, device=gpu) if q0 is None else _dev(q0, gpu)
    rays = torch.full((n,), 7.0, device=gpu)
    nof.kernel_interlevel(n, Sc, dv["tp"], dv["wp"], Sf, dv["t"], dv["w"], dv["lm"],
                          float(np.sum(inp["lm"], dtype=np.float32)), mult, q, rays, accumulate=accumulate)
    torch.cuda.synchronize()
    return q.cpu().numpy(), rays.cpu().numpy()


@pytest.mark.parametrize("Sc,Sf", KERNEL_CASES)
def test_kernel_matches_reference(gpu, Sc, Sf):
    inp, ref = _kernel_case(Sc, Sf)
    assert 0.10 <= float(np.mean(ref["margin"] > 0)) <= 0.90  # (the reference alone: active hinges)
    q, rays = _kernel_run(gpu, inp, 1.0)
    e_q, e_r = rel_l2(q, ref["w_grad"]), rel_l2(rays, ref["rays"])
    print(f"k_interlevel ({Sc}, {Sf}): dL/dw^ {e_q:.2e}, per-ray term {e_r:.2e}; terms {rays}")
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(rays))
    assert e_q <= TOL and e_r <= TOL
    assert not np.any(q[3]) and rays[3] == 0.0  # w = 0: exactly nothing
    assert not np.any(q[4]) and rays[4] == 0.0  # lossmult = 0
    assert rays[2] > 0.0 and np.any(q[2])       # the one-surface ray
    # two runs: the same bits
    q2, rays2 = _kernel_run(gpu, inp, 1.0)
    assert q.tobytes() == q2.tobytes() and rays.tobytes() == rays2.tobytes()
    # accumulate = 1 onto a random q: q + the overwrite result, one fp32 addition per element
    q0 = np.random.default_rng(Sc + Sf).standard_normal(q.shape).astype(np.float32)
    qa, raysa = _kernel_run(gpu, inp, 1.0, accumulate=True, q0=q0)
    assert qa.tobytes() == (q0 + q).astype(np.float32).tobytes() and raysa.tobytes() == rays.tobytes()
    # mult = 0: zeros
    qz, raysz = _kernel_run(gpu, inp, 0.0)
    assert not np.any(qz) and not np.any(raysz)


def test_kernel_more_than_one_block_and_no_rays_buffer(gpu):
    """n = 70 rays (the shared case tiled), dev_rays = NULL: every ray's row is its own ray's"""
    import torch
    import nof

    inp, _ = _kernel_case(64, 128)
    reps = 12
    big = {k: np.concatenate([inp[k]] * reps)[:70] for k in ("tp", "wp", "t", "w", "lm")}
    big.update(n=70, Sc=64, Sf=128)
    q, _ = _kernel_run(gpu, big, 1.0)
    dv = {k: _dev(big[k], gpu) for k in ("tp", "wp", "t", "w", "lm")}
    q2 = torch.full((70, 64), 7.0, device=gpu)
    msum = float(np.sum(big["lm"], dtype=np.float32))
    nof.kernel_interlevel(70, 64, dv["tp"], dv["wp"], 128, dv["t"], dv["w"], dv["lm"], msum, 1.0, q2, None)
    torch.cuda.synchronize()
    assert q.tobytes() == q2.cpu().numpy().tobytes()
    for r in range(6, 70):
        assert q[r].tobytes() == q[r % 6].tobytes(), r


# ---- whole steps ---------------------------------------------------------------------------------------------------
def _rays(n):
    from nof import synth

    return synth.blender_rays(n, seed=RAY_SEED)


def _install(m, spec, recipe):
    """the model's Glorot draw times scale, the density head's weights times head, its bias + bias; returns the
    parameters (numpy fp32)"""
    import torch
    import nof
    import crosslevel_ref as X
    import test_gpu_crosslevel as XL

    scale, head, bias = recipe
    net = XL._net(spec)
    P = (XL._params(m) * np.float32(scale)).astype(np.float32)
    at = {name: slice(o, o + s) for name, o, s in X.tensors(net)}
    P[at[f"W{net.D}"]] *= np.float32(head)
    P[at[f"b{net.D}"]] += np.float32(bias)
    ptr, cnt = m.mlp.flat_params()
    nof.device_tensor(ptr, (cnt,)).copy_(torch.from_numpy(P))
    torch.cuda.synchronize()
    return P


@pytest.mark.parametrize("precision", [0, 1, 2, 3, 4, 5])
def test_every_precision_mode(gpu, precision):
    """The reference 8x256 network, stop_level_grad = 1: level 0's adjoint against fp64 autograd of that level's own
    stored t, density, rgb (photometric x coarse_loss_mult + the term with the GPU's level-1 t, w as the target)."""
    import interlevel_ref as IL
    import test_gpu_crosslevel as XL

    n, samples, mult = 32, (64, 128), REF8_MULT
    r = _rays(n)
    r["lossmult"] = r["lossmult"].copy()
    r["lossmult"][3] = 0.0
    r["lossmult"][5] = 2.0
    runs = []
    for lam in (mult, None):
        m = XL._model(XL.REF8, n, samples, precision)
        _install(m, XL.REF8, REF8_RECIPE)
        if lam is not None:
            m.set_interlevel_loss(lam)
        XL._step(m, r, gpu)
        runs.append(dict(lv=[m.level_numpy(l) for l in range(2)], G=XL._grads(m), loss=m.loss(),
                         prop=m.interlevel_loss(), status=m.numeric_status(), cross=m.cross_numpy(0),
                         lam0=m.config.coarse_loss_mult))
        m.close()
    a, z = runs
    assert a["status"] == 0 and z["status"] == 0
    # the forward, the photometric loss and the last level's adjoint are those of a model with the option off
    assert a["loss"] == z["loss"] and z["prop"] == 0.0
    for l in range(2):
        for k in ("t", "weights", "comp_rgb", "density", "rgb"):
            assert a["lv"][l][k].tobytes() == z["lv"][l][k].tobytes(), (l, k)
    assert a["lv"][1]["density_grad"].tobytes() == z["lv"][1]["density_grad"].tobytes()
    assert a["lv"][1]["rgb_grad"].tobytes() == z["lv"][1]["rgb_grad"].tobytes()
    assert z["cross"] == {"w_grad": None, "t_grad": None}
    assert a["cross"]["t_grad"] is None and a["cross"]["w_grad"] is not None
    lv = a["lv"][0]
    kw = dict(sigma=lv["density"], rgb=lv["rgb"], t=lv["t"], d=r["d"], pix=r["pix"], lossmult=r["lossmult"],
              t_tgt=a["lv"][1]["t"], w_tgt=a["lv"][1]["weights"], lam=a["lam0"], w_value=lv["weights"])
    ref = IL.level_grads(mult=mult, **kw)
    ref0 = IL.level_grads(mult=0.0, **kw)
    e_s, e_c = rel_l2(lv["density_grad"], ref["dsigma"]), rel_l2(lv["rgb_grad"], ref["drgb"])
    e_p = abs(a["prop"] - ref["prop"]) / abs(ref["prop"])
    away, chosen = rel_l2(lv["density_grad"], ref0["dsigma"]), rel_l2(ref["dsigma"], ref0["dsigma"])
    print(f"precision {precision}: level 0 density_grad {e_s:.2e} rgb_grad {e_c:.2e} interlevel_loss {e_p:.2e} "
          f"({a['prop']:.6g}; photometric {a['loss']:.6g}); density_grad vs the reference without the term {away:.3g} "
          f"(the reference's own {chosen:.3g})")
    assert e_s <= TOL and e_c <= TOL and e_p <= TOL
    assert chosen > 100 * TOL and away > 100 * TOL
    assert rel_l2(z["lv"][0]["density_grad"], ref0["dsigma"]) <= TOL


def _whole_step(gpu, n, samples, precision, stop, adopt, tol, mult=TINY_MULT, dist_mult=0.0, recipe=None):
    import crosslevel_ref as X
    import interlevel_ref as IL
    import test_gpu_crosslevel as XL

    r = _rays(n)
    kw = {"distortion_loss_mult": dist_mult} if dist_mult else {}
    m = XL._model(XL.TINY, n, samples, precision, stop_level_grad=stop, **kw)
    params = _install(m, XL.TINY, recipe or TINY_RECIPE[samples])
    m.set_interlevel_loss(mult)
    XL._step(m, r, gpu)
    L = len(samples)
    lv = [m.level_numpy(l) for l in range(L)]
    G = XL._grads(m)
    masks = {l: m.mlp.relu_masks(l) for l in range(L)}
    cross = [m.cross_numpy(l) for l in range(L)]
    loss, prop, dist = m.loss(), m.interlevel_loss(), m.distortion_loss()
    assert m.numeric_status() == 0
    m.close()
    idx = XL._gpu_index(lv, samples, gpu)  # the GPU's bin indices and t-values, as test_gpu_crosslevel adopts them
    D_, W, Dc, Wc, skip, lo, hi, dv = XL.TINY
    net = XL._net(XL.TINY)
    rk = dict(net=net, samples=samples, min_deg=lo, max_deg=hi, deg_view=dv, seed=XL.SEED, step_idx=XL.STEP,
              ray_base=XL.RAY_BASE, idx=idx, t_value={l: lv[l]["t"] for l in range(1, L)},
              relu=masks if adopt else None, detach=bool(stop), dist_mult=dist_mult,
              w_value={l: lv[l]["weights"] for l in range(L)})
    ref = IL.step(params, r, mult, **rk)
    ref0 = IL.step(params, r, 0.0, **rk)
    lines, bad = [], []
    for i, (name, o, s) in enumerate(X.tensors(net)):
        sl = slice(o, o + s)
        e, away, chosen = rel_l2(G[sl], ref["grads"][sl]), rel_l2(G[sl], ref0["grads"][sl]), \
            rel_l2(ref["grads"][sl], ref0["grads"][sl])
        lines.append(f"{name}: {e:.2e} (bound {tol:.0e}); vs no term {away:.3g} (the reference's own {chosen:.3g})")
        if not e <= tol:
            bad.append(f"{name}: rel L2 {e:.3g} > {tol:.3g}")
        if i % net.L < net.D and not (away > 100 * tol and chosen > 100 * tol):  # every trunk tensor carries the term
            bad.append(f"{name}: differs from the reference without the term by only {away:.3g}")
    print(f"{n} x {samples} precision {precision} stop_level_grad {stop}: interlevel {prop:.6g} (reference "
          f"{ref['prop']:.6g}, per level {ref['prop_levels']})\n  " + "\n  ".join(lines))
    assert all(p > 0 for p in ref["prop_levels"])  # every coarser level carries a term
    assert abs(loss - ref["loss"]) <= max(tol, 1e-5) * abs(ref["loss"])
    assert abs(prop - ref["prop"]) <= max(tol, 1e-5) * abs(ref["prop"])
    if dist_mult:
        assert ref["dist"] > 0 and abs(dist - ref["dist"]) <= max(tol, 1e-5) * abs(ref["dist"])
    assert not bad, "\n".join(bad)
    return cross, ref, ref0, lv


def test_step_f32_stop_level_grad_1(gpu):
    """q^0 is the term's own dL/dw^0 (nof_mipnerf_cross_view returns it with the option on; no t gradient)"""
    cross, ref, _, _ = _whole_step(gpu, 5, (64, 128), 0, 1, False, TOL)
    assert cross[1] == {"w_grad": None, "t_grad": None} and cross[0]["t_grad"] is None
    e = rel_l2(cross[0]["w_grad"], ref["w_grad_prop"][0])
    print(f"level 0 q: {e:.2e}")
    assert e <= TOL


def test_step_f32_stop_level_grad_0(gpu):
    """The term is added to the q^0 the resampler adjoint wrote.  q's bound is test_gpu_crosslevel's (the cdf's format
    term).  The rays of this case are opaque, unlike that test's: behind a surface the stored fp32 weights are exactly
    0 or an ulp apart, and at a tie in the blur-pool's max the reference splits the gradient equally (torch.maximum,
    crosslevel_ref's docstring) where the resampler adjoint gives it to one side: there q differs by half its value
    (measured 5.6e-4 of the whole tensor) although w, T and with them every parameter gradient's share are 0.  So q is
    compared on the samples whose weight differs from both neighbours' by more than 1e-4 of the larger, and the
    term's own part, q with the term minus q of the same step without it, on every sample."""
    import test_gpu_crosslevel as XL

    samples, n = (64, 128), 5
    cross, ref, ref0, lv = _whole_step(gpu, n, samples, 0, 0, False, TOL)
    xtol = 2 * 2.0 ** -24 * (1 + samples[0] * 0.01) / 0.01
    q, rq = cross[0]["w_grad"], ref["w_grad"][0]
    w = lv[0]["weights"].astype(np.float64)
    wp = np.concatenate([w[:, 1:2], w, w[:, -2:-1]], 1)  # (the end samples have one neighbour)
    gap = lambda a, b: np.abs(a - b) > 1e-4 * np.maximum(np.abs(a), np.abs(b))
    free = gap(wp[:, 1:-1], wp[:, :-2]) & gap(wp[:, 1:-1], wp[:, 2:])
    e, e_all, away = rel_l2(q[free], rq[free]), rel_l2(q, rq), rel_l2(q, ref0["w_grad"][0])
    print(f"level 0 q: {e:.2e} on the {100 * free.mean():.0f} % of the samples without a tie (bound {xtol:.2e}), "
          f"{e_all:.2e} on all; vs no term {away:.3g}")
    assert free.mean() >= 0.25
    assert e <= xtol and away > 100 * xtol
    assert cross[1]["w_grad"] is None and cross[1]["t_grad"] is not None
    # the same step without the term: the resampler's share alone, bit for bit what the term was added to
    m = XL._model(XL.TINY, n, samples, 0, stop_level_grad=0)
    _install(m, XL.TINY, TINY_RECIPE[samples])
    XL._step(m, _rays(n), gpu)
    q0 = m.cross_numpy(0)["w_grad"]
    m.close()
    e_term = rel_l2(q.astype(np.float64) - q0, ref["w_grad_prop"][0])
    print(f"level 0 q minus the step's q without the term, against the reference's term: {e_term:.2e}")
    assert e_term <= TOL


@pytest.mark.parametrize("stop", [1, 0])
def test_step_three_levels(gpu, stop):
    """(64, 64, 64): levels 0 and 1 both carry a term against level 2 (_whole_step asserts both are > 0)"""
    cross, ref, _, _ = _whole_step(gpu, 3, (64, 64, 64), 0, stop, False, TOL)
    if stop:
        for l in (0, 1):
            assert rel_l2(cross[l]["w_grad"], ref["w_grad_prop"][l]) <= TOL, l


def test_step_f16_products_stop_level_grad_0(gpu):
    """The density head x 16 here, not x 32: at x 32 this mode's photometric gradient alone (multiplier 0) is
    3.4e-3 off on the trunk, outside its 2e-3 contract whatever the term does; at x 16 it is 1.4e-3, and the
    reference's term still moves every trunk tensor by 0.0081 per unit of the multiplier (0.81 at 100)."""
    _whole_step(gpu, 5, (64, 128), 5, 0, True, F16P_TOL, recipe=(1.0, 16.0, 0.0))


def test_step_with_the_distortion_loss(gpu):
    """both regularisers in one F32 step (stop_level_grad = 0: the distortion term's dL/dt reaches level 0 as well)"""
    _whole_step(gpu, 5, (64, 128), 0, 0, False, TOL, dist_mult=1.0)


# ---- unchanged behaviour, the interface ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,spec,kw", [(4, "REF8", {}), (0, "TINY", {"stop_level_grad": 0})])
def test_never_set_is_set_to_zero_bitwise(gpu, precision, spec, kw):
    import test_gpu_crosslevel as XL

    n, samples = 16, (64, 128)
    r = _rays(n)
    got = []
    for setter in (False, True):
        m = XL._model(getattr(XL, spec), n, samples, precision, **kw)
        if setter:
            m.set_interlevel_loss(0.0)
        XL._step(m, r, gpu)
        got.append((XL._grads(m), m.loss(), m.interlevel_loss()))
        m.close()
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1] == got[1][1]
    assert got[0][2] == 0.0 and got[1][2] == 0.0


def test_setter_refusals_and_single_level(gpu):
    import nof
    import test_gpu_crosslevel as XL

    n = 4
    r = _rays(n)
    got = []
    for lam in (None, 1.0):
        m = XL._model(XL.TINY, n, (64,))
        if lam is not None:
            for bad in (-1.0, float("nan"), float("inf")):
                with pytest.raises(nof.NofError) as e:
                    m.set_interlevel_loss(bad)
                assert e.value.status == 1 and "interlevel_loss_mult" in str(e.value)
            m.set_interlevel_loss(lam)  # num_levels == 1: a no-op
        XL._step(m, r, gpu)
        got.append((XL._grads(m), m.interlevel_loss()))
        m.close()
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[1][1] == 0.0
    m = XL._model(XL.TINY, n, (64, 64))
    m.set_interlevel_loss(1.0)
    with pytest.raises(nof.NofError):  # before a step
        m.interlevel_loss()
    m.close()


def _mean_interlevel(lv0, lv1):
    """the unmultiplied mean L_r^0 in numpy fp64 (interlevel_ref's closed form of the bound, direct sums)"""
    import interlevel_ref as IL

    out = []
    for r in range(lv0["t"].shape[0]):
        a = [x[r].astype(np.float64) for x in (lv0["weights"], lv0["t"], lv1["weights"], lv1["t"])]
        out.append(IL._g(*a)[1].sum())
    return float(np.mean(out))


def test_training_smoke(gpu):
    """300 Adam steps of the tiny network on 64 synthetic rays x (64, 64), with the term (lambda_p = 1) and without:
    the run with it ends with the strictly lower mean L_r^0 (what the term is for), both photometric losses finite."""
    import torch
    import nof
    import test_gpu_crosslevel as XL

    n, samples = 64, (64, 64)
    r = _rays(n)
    d = {k: _dev(v, gpu) for k, v in r.items()}
    msum = float(np.sum(r["lossmult"], dtype=np.float32))
    out = {}
    for lam in (1.0, 0.0):
        m = XL._model(XL.TINY, n, samples)
        m.set_interlevel_loss(lam)
        opt = nof.AcceleratedAdamOptimizer(m.GetLayerSizes(), m.config)
        for it in range(300):
            m.set_rng(XL.SEED, it, 0)
            g = m.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"], msum)
            opt.step(m.mlp.allParams, g, 5e-3)
        m.set_rng(XL.SEED, 300, 0)  # one evaluation step on the same samples for both runs
        m.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"], msum)
        torch.cuda.synchronize()
        out[lam] = (m.loss(), _mean_interlevel(m.level_numpy(0), m.level_numpy(1)), m.interlevel_loss())
        opt.close(); m.close()
    print(f"after 300 steps: with the term loss {out[1.0][0]:.5f} mean L_r^0 {out[1.0][1]:.6g} (term {out[1.0][2]:.6g}); "
          f"without loss {out[0.0][0]:.5f} mean L_r^0 {out[0.0][1]:.6g}")
    assert np.isfinite(out[1.0][0]) and np.isfinite(out[0.0][0])
    assert abs(out[1.0][2] - out[1.0][1]) <= 1e-4 * abs(out[1.0][1]) + 1e-12  # lossmult = 1: the term is the mean L_r^0
    assert out[1.0][1] < out[0.0][1]
