"""CPU checks of the per-view appearance embeddings (nof_mipnerf_create_ex): the fp64 reference the GPU
tests compare against (tests/appearance_ref.py) is pinned by central finite differences, the parameter layout of the
widened view layer is torch_ref's, the rays the GPU tests use make the embedding matter, and the new entry points
exist and refuse bad arguments without a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import appearance_ref as A
import torch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (D, W, Dc, Wc, skip, min_deg, max_deg, deg_view): test_gpu_crosslevel's tiny network
TINY = (3, 32, 1, 16, 2, 0, 4, 2)
TINY_PE = dict(min_deg=0, max_deg=4, deg_view=2)
# The rays, view ids and table of the GPU tests' whole-step cases (tests/test_gpu_appearance.py imports these).  Chosen
# here from the reference alone (test_inputs_make_the_embedding_matter), before any GPU gradient was looked at:
# synth.blender_rays seed 7 is the seed test_gpu_crosslevel.py uses.
RAY_SEED = 7
GPU_TOL = 1e-5  # the GPU tests' F32 floor
CASES = [(5, (64, 128), 4), (3, (64, 64, 64), 7)]
# the case the GPU tests run with ray gradients and the contraction on: the three-level one.  Contracted, the two-level
# case's density-bias sum cancels to 1 / 26 of its terms in the fp64 reference already at E = 0 (1 / 30 with the
# table): a single number that no fp32 sum holds to 1e-5, whatever the code.  The three-level case stays at 1.13.
CONTRACTED_CASE = CASES[1]
KAPPA_MAX = 8.0  # (the two-level case, uncontracted, is at 6.2: the worst conditioning a whole-step case may have)
VIEWS = 3


def _rays(n, seed):
    from nof import synth

    return synth.blender_rays(n, seed=seed)


def view_ids(n):
    """view of ray r of the whole-step cases: every view of VIEWS drawn, with repeats"""
    return (np.arange(n) * 2 % VIEWS).astype(np.int32)


def table(dim, seed=0):
    """E = 0.5 N(0, 1), fp32.  The seed is chosen from the reference alone (test_table_keeps_the_density_bias_sum
    _conditioned): the density head's bias gradient is ONE number, the sum of dL/dz_sigma over every sample, and the
    colours, hence E, move its terms.  With seed 4 the fp64 reference's own terms cancel 3.6 x more (sum |terms| /
    |sum| = 22.8 against 6.3 at E = 0, two-level case), so any fp32 sum of them is 3.6 x less accurate than the G = 0
    run that sets the GPU tests' floor 4 x e_off: a property of the inputs, not of the code.  Seed 0 keeps the ratio
    at E = 0's (6.2)."""
    return (0.5 * np.random.default_rng(seed).standard_normal((VIEWS, dim))).astype(np.float32)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("detach", [True, False])
@pytest.mark.parametrize("n,samples,dim", CASES)
def test_autograd_matches_central_finite_differences(n, samples, dim, detach):
    """The directional derivative of the pure-fp64 step (snap=False) in E, and in the view layer's weight, along random
    unit directions, bin indices held at the base point's.  Bound 1e-6 relative, h = 1e-6: test_raygrad_cpu's."""
    net = A.net(TINY, dim)
    P0 = R.glorot(net, 11).astype(np.float64)
    E0 = table(dim).astype(np.float64)
    rays, view = _rays(n, 5), view_ids(n)
    kw = dict(net=net, samples=samples, seed=3, step_idx=1, ray_base=7, snap=False, detach=detach, **TINY_PE)
    base = A.step(P0, E0, view, rays, **kw)
    idx = {l: base["idx"][l] for l in range(1, len(samples))}
    # (E and the view layer reach the colours only: w, hence every level's t, does not move with them, so the
    # detached step needs no held t-values for its difference quotient)
    rng = np.random.default_rng(1)
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    h = 1e-6

    def f(P, E):
        return A.step(T(P), T(E), view, rays, idx=idx, backward=False, **kw)["loss"].item()

    # dE
    vE = rng.standard_normal(E0.shape)
    vE /= np.linalg.norm(vE)
    fd = (f(P0, E0 + h * vE) - f(P0, E0 - h * vE)) / (2 * h)
    ad = float((base["e_grad"] * vE).sum())
    rel_e = abs(fd - ad) / abs(fd)
    # the view layer's weight (layer D + 1), every column: h_{D-1}, view PE and the embedding
    lo = sum(net.outs[l] * net.ins[l] for l in range(net.D + 1))
    sz = net.outs[net.D + 1] * net.ins[net.D + 1]
    vW = np.zeros_like(P0)
    vW[lo:lo + sz] = rng.standard_normal(sz)
    vW /= np.linalg.norm(vW)
    fd = (f(P0 + h * vW, E0) - f(P0 - h * vW, E0)) / (2 * h)
    ad = float((base["grads"] * vW).sum())
    rel_w = abs(fd - ad) / abs(fd)
    print(f"{n} x {samples} G={dim} detach={detach}: dE rel {rel_e:.2e}, dW_view rel {rel_w:.2e}")
    assert rel_e <= 1e-6 and rel_w <= 1e-6


def test_zero_dim_reference_is_raygrad_refs():
    """without an embedding (G = 0, E [V, 0]) the step is tests/raygrad_ref.py's: same loss, parameter and ray gradients"""
    import raygrad_ref as G

    net = A.net(TINY, 0)
    P0 = R.glorot(net, 9)
    rays = _rays(4, 2)
    kw = dict(net=net, samples=(64, 64), seed=5, step_idx=2, ray_base=3, **TINY_PE)
    for detach in (False, True):
        a = A.step(P0, np.zeros((VIEWS, 0)), view_ids(4), rays, detach=detach, **kw)
        b = G.step(P0, rays, detach=detach, **kw)
        assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(b["loss"])
        assert _rel(a["grads"], b["grads"]) <= 1e-9 and _rel(a["d_grad"], b["d_grad"]) <= 1e-9


def test_out_of_range_view_reads_zeros_and_reaches_no_row():
    net = A.net(TINY, 4)
    P0 = R.glorot(net, 9)
    rays = _rays(4, 2)
    kw = dict(net=net, samples=(64, 64), seed=5, step_idx=2, ray_base=3, **TINY_PE)
    E = table(4)
    a = A.step(P0, E, np.array([-1, VIEWS, -1, VIEWS]), rays, **kw)
    b = A.step(P0, np.zeros_like(E), np.array([0, 1, 2, 0]), rays, **kw)
    assert np.all(a["e_grad"] == 0) and a["loss"] == b["loss"]
    assert np.array_equal(a["grads"], b["grads"])


@pytest.mark.parametrize("dim", [1, 4, 7, 32])
def test_layout_of_the_widened_view_layer(dim):
    """the arena of Net(dir_in = Vd + G): only layer D + 1 is wider, by Wc G; Glorot's bound uses the widened fan-in"""
    D, W, Dc, Wc, skip, lo, hi, dv = TINY
    Vd = 3 * (2 * dv + 1)
    n0, n1 = A.net(TINY, 0), A.net(TINY, dim)
    assert n1.ins[D + 1] == W + Vd + dim and n1.outs == n0.outs
    assert [a - b for a, b in zip(n1.ins, n0.ins)] == [dim if l == D + 1 else 0 for l in range(n1.L)]
    P0, P1 = R.glorot(n0, 0x51), R.glorot(n1, 0x51)
    assert P1.size == P0.size + Wc * dim
    off = sum(n1.outs[l] * n1.ins[l] for l in range(D + 1))
    assert np.array_equal(P1[:off], P0[:off])  # the layers before it: the same Philox draws, the same bounds
    w = P1[off:off + Wc * (W + Vd + dim)]
    bound = np.float32(np.sqrt(np.float32(6.0) / np.float32(W + Vd + dim + Wc)))
    assert np.all(np.abs(w) <= bound) and np.abs(w).max() > 0.9 * bound
    assert np.all(P1[-sum(n1.outs):] == 0)


@pytest.mark.parametrize("n,samples,dim", CASES)
def test_inputs_make_the_embedding_matter(n, samples, dim):
    """With the GPU tests' rays, ids and table: the reference's dE is more than 100 x the GPU bound of the view layer's
    weight gradient (the tensor its operand feeds), and the parameter gradient with the table differs from the one
    with E = 0 by more than 100 x the bound: a step that dropped the gather or the table's gradient could not pass."""
    net = A.net(TINY, dim)
    P0 = R.glorot(net, 0x51)
    rays, view, E = _rays(n, RAY_SEED), view_ids(n), table(dim)
    kw = dict(net=net, samples=samples, seed=0x51, step_idx=3, ray_base=20, **TINY_PE)
    a = A.step(P0, E, view, rays, **kw)
    z = A.step(P0, np.zeros_like(E), view, rays, **kw)
    lo = sum(net.outs[l] * net.ins[l] for l in range(net.D + 1))
    gw = a["grads"][lo:lo + net.outs[net.D + 1] * net.ins[net.D + 1]]
    r_e = float(np.linalg.norm(a["e_grad"]) / np.linalg.norm(gw))
    r_p = _rel(z["grads"], a["grads"])
    print(f"{n} x {samples} G={dim}: |dE| / |dW_view| {r_e:.2e}, grads(E) vs grads(0) {r_p:.2e}")
    assert r_e > 100 * GPU_TOL and r_p > 100 * GPU_TOL
    assert all(np.any(view == v) for v in range(VIEWS))


@pytest.mark.parametrize("stop", [1, 0])
@pytest.mark.parametrize("n,samples,dim,contraction", [c + (False,) for c in CASES] + [CONTRACTED_CASE + (True,)])
def test_table_keeps_the_density_bias_sum_conditioned(n, samples, dim, contraction, stop):
    """The GPU tests' floor is 4 x the error of the G = 0 step on the same rays.  That floor is meaningful for a
    single-number tensor only if its sum is as well conditioned with the table as without: the cancellation ratio
    sum |dL/dz_sigma| / |sum dL/dz_sigma| of the reference with table(dim) stays within 1.25 x the ratio at E = 0,
    and under KAPPA_MAX."""
    import crosslevel_ref as X

    net = A.net(TINY, dim)
    P0 = R.glorot(net, 0x51)
    rays, view = _rays(n, RAY_SEED), view_ids(n)
    kw = dict(net=net, samples=samples, seed=0x51, step_idx=3, ray_base=20, detach=bool(stop),
              contraction=contraction, **TINY_PE)
    forward0 = X.forward

    def kappa(E):
        caps = []

        def forward(*a, **k):
            zs, zc = forward0(*a, **k)
            zs.retain_grad()
            caps.append(zs)
            return zs, zc

        X.forward = forward
        try:
            A.step(P0, E, view, rays, **kw)
        finally:
            X.forward = forward0
        g = np.concatenate([z.grad.numpy().ravel() for z in caps])
        return float(np.abs(g).sum() / abs(g.sum()))

    k0, k1 = kappa(np.zeros((VIEWS, dim))), kappa(table(dim))
    print(f"{n} x {samples} G={dim} stop {stop} contraction {contraction}: sum |terms| / |sum| {k0:.2f} at E = 0, "
          f"{k1:.2f} with the table")
    assert k1 <= 1.25 * k0 and k1 <= KAPPA_MAX


# ---- the interface, without a device ---------------------------------------------------------------------------------
NEW = ["nof_mipnerf_create_ex", "nof_mipnerf_appearance", "nof_mipnerf_set_ray_views",
       "nof_mipnerf_set_render_appearance", "nof_dataset_batch_views", "nof_kernel_appearance_gather",
       "nof_kernel_appearance_grad"]
INVALID, UNSUPPORTED = 1, 5


def test_symbols_exported_and_bound():
    import nof

    lib = nof.lib()
    with open(os.path.join(ROOT, "include", "nof.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in nof._lib.SIGNATURES, name
        assert name + "(" in header, name
    assert "typedef struct nof_model_ext" in header
    for m in ("appearance", "set_ray_views", "set_render_appearance"):
        assert hasattr(nof.AcceleratedMipNeRF, m), m
    assert hasattr(nof.RayDataset, "batch_views")
    assert [f[0] for f in nof._lib.nof_model_ext._fields_] == ["size", "appearance_views", "appearance_dim"]
    assert C.sizeof(nof._lib.nof_model_ext) == 12


def test_null_handles_refused_without_a_device_call():
    import nof

    lib = nof.lib()
    p = C.c_void_p()
    v, g = C.c_int32(7), C.c_int32(7)
    buf = (C.c_float * 64)()
    b = C.cast(buf, C.c_void_p)
    assert lib.nof_mipnerf_appearance(None, C.byref(p), C.byref(p), C.byref(v), C.byref(g)) == INVALID
    assert v.value == 7 and g.value == 7
    assert lib.nof_mipnerf_set_ray_views(None, b) == INVALID
    assert lib.nof_mipnerf_set_render_appearance(None, 0) == INVALID
    assert lib.nof_dataset_batch_views(None, 4, b, None) == INVALID
    assert b"invalid argument" in lib.nof_last_error()
    assert lib.nof_mipnerf_create_ex(None, None, None) == INVALID
    # the kernel entry points: bad shapes and null pointers are refused before a launch
    gather = lambda n=0, dim=4, views=3, t=b, out=b: lib.nof_kernel_appearance_gather(n, 15, dim, views, b, t, None, -1,
                                                                                      out, None)
    assert gather(n=-1) == INVALID and gather(dim=0) == INVALID and gather(dim=257) == INVALID
    assert gather(views=0) == INVALID and gather(t=None) == INVALID and gather(out=None) == INVALID
    grad = lambda n=0, dim=4, views=3, ids=b, acc=0: lib.nof_kernel_appearance_grad(n, dim, views, ids, b, b, acc, None)
    assert grad(n=-1) == INVALID and grad(dim=0) == INVALID and grad(dim=257) == INVALID and grad(views=0) == INVALID
    assert grad(ids=None) == INVALID and grad(acc=2) == INVALID


def _create_ex(cfg, views, dim, size=None):
    import nof

    ext = nof._lib.nof_model_ext(C.sizeof(nof._lib.nof_model_ext) if size is None else size, views, dim)
    h = C.c_void_p()
    st = nof.lib().nof_mipnerf_create_ex(C.byref(cfg), C.byref(ext), C.byref(h))
    assert st != 0 and not h.value
    return st, nof.lib().nof_last_error().decode()


def test_create_ex_refusals_come_before_any_device_call():
    """(this machine may have no device: a call that reached one would return NOF_ERR_HIP, not these)"""
    import nof

    tiny = dict(net_depth=3, net_width=32, net_depth_condition=1, net_width_condition=16, skip_layer=2,
                min_deg_point=0, max_deg_point=4, deg_view=2, num_samples=(64, 64), max_rays=8)
    cfg = nof.default_config(**tiny)
    assert _create_ex(cfg, 3, -1)[0] == INVALID
    assert _create_ex(cfg, 3, 257)[0] == INVALID
    assert _create_ex(cfg, 0, 4)[0] == INVALID
    assert _create_ex(cfg, -2, 4)[0] == INVALID
    assert _create_ex(cfg, 1 << 23, 256)[0] == INVALID  # views * dim = 2^31
    assert _create_ex(cfg, 3, 4, size=8)[0] == INVALID
    assert _create_ex(cfg, 3, 4, size=0)[0] == INVALID
    # the fused 8x256 object: precision modes 0..4 with the reference shape and stop_level_grad = 1
    for prec in range(5):
        st, msg = _create_ex(nof.default_config(precision=prec, max_rays=8), 3, 4)
        assert st == UNSUPPORTED and "any-shape" in msg, (prec, st, msg)
    # a bad config is still the config's refusal
    assert _create_ex(nof.default_config(max_rays=0), 3, 4)[0] == INVALID


def test_ext_null_and_dim_zero_are_accepted():
    """ext = NULL and dim = 0 pass every argument check: the call goes on to the device (NOF_OK with one, NOF_ERR_HIP /
    NOF_ERR_OOM without), exactly as nof_mipnerf_create does; dim = 0 ignores the views"""
    import nof

    lib = nof.lib()
    cfg = nof.default_config(net_depth=2, net_width=16, net_depth_condition=1, net_width_condition=16, skip_layer=2,
                             min_deg_point=0, max_deg_point=2, deg_view=1, num_samples=(64,), max_rays=4)

    def status(fn):
        h = C.c_void_p()
        st = fn(h)
        if st == 0:
            assert lib.nof_mipnerf_destroy(h) == 0
        return st

    base = status(lambda h: lib.nof_mipnerf_create(C.byref(cfg), C.byref(h)))
    assert base not in (INVALID, UNSUPPORTED)
    assert status(lambda h: lib.nof_mipnerf_create_ex(C.byref(cfg), None, C.byref(h))) == base
    for views in (0, -5, 3):
        ext = nof._lib.nof_model_ext(12, views, 0)
        assert status(lambda h: lib.nof_mipnerf_create_ex(C.byref(cfg), C.byref(ext), C.byref(h))) == base


def test_config_struct_is_unchanged():
    import nof

    assert nof.lib().nof_config_size() == C.sizeof(nof._lib.nof_config)
    assert nof._lib.nof_config._fields_[-1][0] == "stop_level_grad"
    assert not hasattr(nof.default_config(), "appearance_dim")


def test_python_driver_flags():
    from nof import train

    a = train.parse_args(["--scene", "s.npz", "--appearance-dim", "4"])
    assert a.appearance_dim == 4 and a.appearance_lr == 1e-3
    a = train.parse_args(["--scene", "s.npz", "--appearance-dim", "32", "--appearance-lr", "5e-3", "--refine-poses",
                          "1e-3", "--contract", "--distortion-loss-mult", "0.01", "--interlevel-loss-mult", "1",
                          "--precision", "f16p"])
    assert a.appearance_dim == 32 and a.appearance_lr == 5e-3 and a.contract and a.refine_poses == 1e-3
    assert train.parse_args(["--synthetic", "64"]).appearance_dim == 0
    for bad in (["--appearance-dim", "-1"], ["--appearance-dim", "257"], ["--appearance-dim", "4", "--appearance-lr", "0"]):
        with pytest.raises(SystemExit):
            train.parse_args(["--scene", "s.npz"] + bad)


def test_python_driver_help_names_the_flags(capsys):
    from nof import train

    with pytest.raises(SystemExit):
        train.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--appearance-dim" in text and "--appearance-lr" in text and "appearance.npy" in text
    assert "neutral (zero) vector" in text
