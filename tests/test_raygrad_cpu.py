"""CPU checks of the ray gradients (nof_mipnerf_set_ray_grad): the fp64 reference the GPU tests compare
against (tests/raygrad_ref.py) is pinned by central finite differences, the rays the GPU tests use exercise every term
of the derivative, and the new entry points exist and refuse null handles without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import raygrad_ref as G
import torch_ref as R

# tiny 3x32 network, skip 2, PE (0, 4), deg_view 2 (test_crosslevel_cpu's)
TINY = dict(D=3, W=32, Dc=1, Wc=16, skip=2, pos_in=24, dir_in=15)
TINY_PE = dict(min_deg=0, max_deg=4, deg_view=2)
# the rays of the GPU tests' whole-step cases (tests/test_gpu_raygrad.py imports these): synth.blender_rays(n, RAY_SEED).
# Chosen here from the reference alone (test_inputs_exercise_every_term), before any GPU gradient was looked at.
RAY_SEED = 7
GPU_TOL = 1e-5  # the GPU tests' F32 bound
CASES = [(5, (64, 128)), (3, (64, 64, 64))]


def _rays(n, seed):
    from nof import synth

    return synth.blender_rays(n, seed=seed)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("detach", [True, False])
@pytest.mark.parametrize("n,samples", CASES)
def test_autograd_matches_central_finite_differences(n, samples, detach):
    """The directional derivative of the pure-fp64 step (snap=False) in (o, d) along a random unit direction, bin
    indices held at the base point's; the detached (stop_level_grad = 1) and the cross-level reference.  Bound 1e-6
    relative: what test_crosslevel_cpu asks of its reference for the same cases (h = 1e-6)."""
    net = R.Net(**TINY)
    P0 = R.glorot(net, 11).astype(np.float64)
    rays = _rays(n, 5)
    kw = dict(net=net, samples=samples, seed=3, step_idx=1, ray_base=7, snap=False, detach=detach, **TINY_PE)
    base = G.step(P0, rays, **kw)
    idx = {l: base["idx"][l] for l in range(1, len(samples))}
    if detach:  # stop_level_grad = 1 holds every level's t: the difference quotient must hold them too
        kw["t_value"] = {l: base["t"][l] for l in range(1, len(samples))}
    rng = np.random.default_rng(1)
    vo, vd = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    nrm = np.sqrt((vo ** 2).sum() + (vd ** 2).sum())
    vo, vd = vo / nrm, vd / nrm
    o0, d0 = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    T = lambda a: torch.tensor(a, dtype=torch.float64)

    def f(h):
        return G.step(T(P0), rays, idx=idx, backward=False, od=(T(o0 + h * vo), T(d0 + h * vd)), **kw)["loss"].item()

    h = 1e-6
    fd = (f(h) - f(-h)) / (2 * h)
    ad = float((base["o_grad"] * vo).sum() + (base["d_grad"] * vd).sum())
    rel = abs(fd - ad) / abs(fd)
    print(f"{n} x {samples} detach={detach}: autograd {ad:.12e} fd {fd:.12e} rel {rel:.2e}")
    assert rel <= 1e-6


def test_parameter_gradient_is_crosslevel_refs():
    """the same step as tests/crosslevel_ref.py: its loss and its parameter gradient (two fp64 evaluations in a
    different operation order, torch's sin / cos / sqrt instead of numpy's: 1e-9, four decades under any bound either
    reference is used for)"""
    import crosslevel_ref as X

    net = R.Net(**TINY)
    P0 = R.glorot(net, 9)
    rays = _rays(4, 2)
    kw = dict(net=net, samples=(64, 64), seed=5, step_idx=2, ray_base=3, **TINY_PE)
    for detach in (False, True):
        a, b = G.step(P0, rays, detach=detach, **kw), X.step(P0, rays, detach=detach, **kw)
        assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(b["loss"])
        assert _rel(a["grads"], b["grads"]) <= 1e-9


@pytest.mark.parametrize("n,samples", CASES)
def test_inputs_exercise_every_term(n, samples):
    """With the GPU tests' rays, holding one part of the forward constant in the ray moves the reference's dL/dd (and,
    for the IPE, dL/do) by more than 100 x the GPU tests' bound: a kernel that dropped the term could not pass."""
    net = R.Net(**TINY)
    P0 = R.glorot(net, 0x51)
    rays = _rays(n, RAY_SEED)
    kw = dict(net=net, samples=samples, seed=0x51, step_idx=3, ray_base=20, **TINY_PE)
    full = G.step(P0, rays, **kw)
    for hold in ("ipe", "render", "view"):
        ab = G.step(P0, rays, hold=(hold,), **kw)
        e_d = _rel(ab["d_grad"], full["d_grad"])
        e_o = _rel(ab["o_grad"], full["o_grad"])
        print(f"{n} x {samples} hold {hold}: dL/dd moves {e_d:.2e}, dL/do {e_o:.2e}")
        assert e_d > 100 * GPU_TOL
        if hold == "ipe":
            assert e_o > 100 * GPU_TOL


def test_pose_gradient_is_the_chain_rule():
    """dL/dposes through d = R cam, o = t equals the per-view sums of the ray gradients"""
    net = R.Net(**TINY)
    P0 = R.glorot(net, 3)
    n, V = 6, 3
    rays = _rays(n, 4)
    rng = np.random.default_rng(0)
    view = np.array([0, 2, 2, 0, 2, 0])  # view 1 draws no ray
    cam = np.concatenate([rng.standard_normal((n, 2)) * 0.3, -np.ones((n, 1))], 1).astype(np.float32)
    poses = rng.standard_normal((V, 12)).astype(np.float32)
    kw = dict(net=net, samples=(64, 64), seed=5, step_idx=2, ray_base=3, **TINY_PE)
    a = G.step(P0, rays, pose=(poses, view, cam), **kw)
    want = np.zeros((V, 12))
    for r in range(n):
        want[view[r], :9] += np.outer(a["d_grad"][r], cam[r].astype(np.float64)).reshape(9)
        want[view[r], 9:] += a["o_grad"][r]
    assert np.allclose(a["pose_grad"], want, rtol=1e-12, atol=1e-15)
    assert not np.any(a["pose_grad"][1])
    b = G.step(P0, rays, **kw)  # the rays as leaves: the same ray gradients
    assert np.array_equal(a["o_grad"], b["o_grad"]) and np.array_equal(a["d_grad"], b["d_grad"])


NEW = ["nof_mipnerf_set_ray_grad", "nof_mipnerf_ray_grad", "nof_kernel_ray_grad", "nof_dataset_pose_grad",
       "nof_dataset_get_poses", "nof_dataset_set_poses"]


def test_symbols_and_null_handles():
    import nof

    lib = nof.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in nof._lib.SIGNATURES, name
    assert hasattr(nof.AcceleratedMipNeRF, "set_ray_grad") and hasattr(nof.AcceleratedMipNeRF, "ray_grad")
    for m in ("pose_grad", "poses", "set_poses"):
        assert hasattr(nof.RayDataset, m), m
    a, b = C.c_void_p(), C.c_void_p()
    buf = (C.c_float * 12)()
    assert lib.nof_mipnerf_set_ray_grad(None, 1) == 1  # NOF_ERR_INVALID_ARG
    assert lib.nof_mipnerf_ray_grad(None, C.byref(a), C.byref(b)) == 1
    assert lib.nof_dataset_pose_grad(None, 1, buf, buf, buf, 0, None) == 1
    assert lib.nof_dataset_get_poses(None, buf) == 1
    assert lib.nof_dataset_set_poses(None, buf) == 1
    assert lib.nof_kernel_ray_grad(1, 64, *([None] * 4), 0, 0, 4, *([None] * 4), 2, None, None, 0, None, None, None) == 1


def test_config_struct_unchanged():
    """the option is a setter, not a field: nof_config ends where it did"""
    import nof

    assert nof.lib().nof_config_size() == C.sizeof(nof._lib.nof_config)
    assert nof._lib.nof_config._fields_[-1][0] == "stop_level_grad"
