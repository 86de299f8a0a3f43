"""CPU checks of the cross-level gradient (nof_config.stop_level_grad = 0): the fp64 reference the GPU tests
compare against (tests/crosslevel_ref.py) is pinned by central finite differences and by the existing detached
reference, and the option's configuration rules hold without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import crosslevel_ref as X
import torch_ref as R

# tiny 3x32 network, skip 2, PE (0, 4), deg_view 2
TINY = dict(D=3, W=32, Dc=1, Wc=16, skip=2, pos_in=24, dir_in=15)
TINY_PE = dict(min_deg=0, max_deg=4, deg_view=2)


def _rays(n, seed):
    from nof import synth

    return synth.blender_rays(n, seed=seed)


@pytest.mark.parametrize("n,samples", [(5, (64, 128)), (3, (64, 64, 64))])
def test_autograd_matches_central_finite_differences(n, samples):
    """The directional derivative of the pure-fp64 step (snap=False: fp32 snapping is noise to a difference
    quotient) along a random unit direction, bin indices held at the base point's.  Bound 1e-6 relative (measured
    1e-9 and 6e-9; the bound leaves room for the truncation at h = 1e-6)."""
    net = R.Net(**TINY)
    P0 = R.glorot(net, 11).astype(np.float64)
    rays = _rays(n, 5)
    kw = dict(net=net, samples=samples, seed=3, step_idx=1, ray_base=7, snap=False, **TINY_PE)
    base = X.step(P0, rays, **kw)
    idx = {l: base["idx"][l] for l in range(1, len(samples))}
    v = np.random.default_rng(1).standard_normal(P0.size)
    v /= np.linalg.norm(v)
    h = 1e-6
    f = lambda p: X.step(torch.tensor(p, dtype=torch.float64), rays, idx=idx, backward=False, **kw)["loss"].item()
    fd = (f(P0 + h * v) - f(P0 - h * v)) / (2 * h)
    ad = float(base["grads"] @ v)
    rel = abs(fd - ad) / abs(fd)
    # the cross-level term is part of what is checked: the detached gradient misses the same quotient
    det = float(X.step(P0, rays, detach=True, **kw)["grads"] @ v)
    print(f"{n} x {samples}: autograd {ad:.12e} fd {fd:.12e} rel {rel:.2e}; detached off by {abs(det - fd) / abs(fd):.2e}")
    assert rel <= 1e-6
    assert abs(det - fd) / abs(fd) > 100 * 1e-6


def test_detached_step_is_the_existing_reference():
    """With every level detached the new reference IS torch_ref.step (PE (0, 16), deg_view 4: its fixed degrees)."""
    net = R.Net(D=3, W=32, Dc=1, Wc=16, skip=2)
    P0 = R.glorot(net, 9)
    rays = _rays(4, 2)
    a = X.step(P0, rays, net=net, samples=(64, 64), seed=5, step_idx=2, ray_base=3, detach=True)
    b = R.step(P0, rays, samples=(64, 64), seed=5, step_idx=2, ray_base=3, net=net)
    for l in range(2):
        assert np.array_equal(a["t"][l].astype(np.float32), b["t"][l])
    assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(b["loss"])
    err = np.linalg.norm(a["grads"] - b["grads"]) / np.linalg.norm(b["grads"])
    assert err <= 1e-12, err
    full = X.step(P0, rays, net=net, samples=(64, 64), seed=5, step_idx=2, ray_base=3)
    assert np.linalg.norm(full["grads"] - b["grads"]) / np.linalg.norm(b["grads"]) > 1e-4  # the option does something


def test_config_default_and_struct_size():
    import nof

    c = nof.default_config()
    assert c.stop_level_grad == 1  # MipNerfModel.StopLevelGrad = true (MipNerfModel.cs:13)
    assert nof.lib().nof_config_size() == C.sizeof(nof._lib.nof_config)
    assert nof._lib.nof_config._fields_[-1][0] == "stop_level_grad"  # the struct grows at its end


@pytest.mark.parametrize("fields,status", [
    ({"stop_level_grad": 0, "precision": 1}, 5),  # the fused 8x256 modes give no input gradient
    ({"stop_level_grad": 0, "precision": 2}, 5),
    ({"stop_level_grad": 0, "precision": 3}, 5),
    ({"stop_level_grad": 0, "precision": 4}, 5),
    ({"stop_level_grad": 2}, 1),
    ({"stop_level_grad": -1}, 1),
])
def test_config_refused_before_any_device_call(fields, status):
    import nof

    cfg = nof.default_config(**fields)
    h = C.c_void_p()
    assert nof.lib().nof_mipnerf_create(C.byref(cfg), C.byref(h)) == status
    msg = nof.lib().nof_last_error().decode()
    assert "stop_level_grad" in msg
    if status == 5:
        assert "input" in msg  # says why: the fused kernels produce no gradient of the encoded input
