"""CPU checks of the distortion loss (nof_config.distortion_loss_mult): the fp64 reference the GPU tests
compare against (tests/distortion_ref.py) is pinned by the O(S^2) definition and by central finite differences, and
the option's configuration rules, entry points and driver flags hold without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import distortion_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ray_set(n, S, seed, lindisp):
    """diffuse, one-surface and two-surface weights on sorted t inside [near, far]; one ray with far = near"""
    rng = np.random.default_rng(seed)
    near = (1.5 + rng.random(n)).astype(np.float32)
    far = (near + 2.0 + 3.0 * rng.random(n)).astype(np.float32)
    t = np.sort(near[:, None] + (far - near)[:, None] * rng.random((n, S + 1)), axis=1)
    w = rng.random((n, S)) ** 3
    w[1] = 1e-6
    w[1, S // 3] = 0.9  # one surface
    w[2] = 1e-6
    w[2, S // 4] = 0.5  # two surfaces
    w[2, (3 * S) // 4] = 0.4
    w /= np.maximum(1.0, w.sum(1, keepdims=True) * 1.05)
    far[n - 1] = near[n - 1]  # a degenerate ray: no term, no gradient
    return w, t, near, far


@pytest.mark.parametrize("lindisp", [0, 1])
def test_closed_form_is_the_pairwise_definition(lindisp):
    w, t, near, far = _ray_set(6, 96, 3, lindisp)
    a = D.distortion(torch.from_numpy(w), torch.from_numpy(t), near, far, lindisp).numpy()
    b = D.pairwise(torch.from_numpy(w), torch.from_numpy(t), near, far, lindisp).numpy()
    assert np.all(a[:-1] > 0) and a[-1] == 0 and b[-1] == 0
    assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) <= 1e-12
    # and the O(S) form the kernel evaluates (exclusive prefix sums on sorted t), in fp64
    s, ok = D.normalised(torch.from_numpy(t), near, far, lindisp)
    s = s.numpy()
    m, dl = (s[:, :-1] + s[:, 1:]) / 2, s[:, 1:] - s[:, :-1]
    A = np.cumsum(w, 1) - w
    P = np.cumsum(w * m, 1) - w * m
    B = w.sum(1, keepdims=True) - A - w
    Q = (w * m).sum(1, keepdims=True) - P - w * m
    Dm = m * (A - B) - (P - Q)
    c = np.where(ok.numpy(), (w * Dm).sum(1) + (w * w * dl).sum(1) / 3, 0.0)
    assert np.max(np.abs(c - b) / np.maximum(np.abs(b), 1e-300)) <= 1e-12


@pytest.mark.parametrize("lindisp", [0, 1])
def test_autograd_matches_central_finite_differences(lindisp):
    """directional derivatives in w and in t (t kept sorted: the step 1e-7 is far below the smallest gap)"""
    w, t, near, far = _ray_set(5, 64, 11, lindisp)
    ww = torch.tensor(w, requires_grad=True)
    tt = torch.tensor(t, requires_grad=True)
    D.distortion(ww, tt, near, far, lindisp).sum().backward()
    assert not np.any(ww.grad.numpy()[-1]) and not np.any(tt.grad.numpy()[-1])  # the degenerate ray
    rng = np.random.default_rng(2)
    f = lambda a, b: float(D.distortion(torch.from_numpy(a), torch.from_numpy(b), near, far, lindisp).sum())
    for name, grad, h in (("w", ww.grad.numpy(), 1e-6), ("t", tt.grad.numpy(), 1e-7)):
        v = rng.standard_normal(grad.shape)
        v /= np.linalg.norm(v)
        assert np.min(np.diff(t, axis=1)) > 100 * 1e-7
        if name == "w":
            fd = (f(w + h * v, t) - f(w - h * v, t)) / (2 * h)
        else:
            fd = (f(w, t + h * v) - f(w, t - h * v)) / (2 * h)
        ad = float((grad * v).sum())
        rel = abs(fd - ad) / abs(fd)
        print(f"lindisp {lindisp} d/d{name}: autograd {ad:.12e} fd {fd:.12e} rel {rel:.2e}")
        assert rel <= 1e-6


def test_closed_form_gradients_are_autograd():
    """dL/dw_i = 2 D_i + (2/3) w_i delta_i, dL/dm_i = 2 w_i (A_i - B_i), dL/ddelta_i = w_i^2 / 3 and the dL/ds_k
    assembly of DESIGN.md 6g, against autograd of the ordered pair sum"""
    w, t, near, far = _ray_set(4, 64, 5, 0)
    w, t, near, far = w[:3], t[:3], near[:3], far[:3]
    ww = torch.tensor(w, requires_grad=True)
    tt = torch.tensor(t, requires_grad=True)
    D.distortion(ww, tt, near, far, 0).sum().backward()
    inv = 1.0 / (far.astype(np.float64) - near)[:, None]
    s = (t - near[:, None]) * inv
    m, dl = (s[:, :-1] + s[:, 1:]) / 2, s[:, 1:] - s[:, :-1]
    A = np.cumsum(w, 1) - w
    B = w.sum(1, keepdims=True) - A - w
    P = np.cumsum(w * m, 1) - w * m
    Q = (w * m).sum(1, keepdims=True) - P - w * m
    Dm = m * (A - B) - (P - Q)
    dw = 2 * Dm + (2.0 / 3.0) * w * dl
    dm, dd = 2 * w * (A - B), w * w / 3
    z = np.zeros((3, 1))
    ds = 0.5 * (np.concatenate([z, dm], 1) + np.concatenate([dm, z], 1)) + np.concatenate([z, dd], 1) - np.concatenate([dd, z], 1)
    assert np.allclose(dw, ww.grad.numpy(), rtol=1e-10, atol=1e-14)
    assert np.allclose(ds * inv, tt.grad.numpy(), rtol=1e-10, atol=1e-14)


def test_config_default_and_struct_size():
    import nof

    c = nof.default_config()
    assert c.distortion_loss_mult == 0.0
    assert nof.lib().nof_config_size() == C.sizeof(nof._lib.nof_config)
    # the struct grows at its end: the field follows stop_level_grad (in the ctypes binding a property over the
    # struct's former tail padding, nof/_lib.py) and lies inside the struct
    off = nof._lib.nof_config.stop_level_grad.offset + 4
    assert nof._lib._DIST_MULT_OFFSET == off and off + 4 <= C.sizeof(nof._lib.nof_config)
    cfg = nof.default_config(distortion_loss_mult=0.01)
    assert cfg.distortion_loss_mult == np.float32(0.01)
    assert C.c_float.from_buffer(cfg, off).value == np.float32(0.01) and cfg.stop_level_grad == 1
    lib_default = nof._lib.nof_config()
    C.memset(C.byref(lib_default), 0xFF, C.sizeof(lib_default))
    nof.lib().nof_config_default(C.byref(lib_default))  # the library itself writes the field: 0
    assert lib_default.distortion_loss_mult == 0.0


@pytest.mark.parametrize("value", [-1.0, float("nan"), float("inf"), -0.001])
@pytest.mark.parametrize("precision", [0, 4])
def test_bad_multiplier_refused_before_any_device_call(value, precision):
    import nof

    cfg = nof.default_config(distortion_loss_mult=value, precision=precision)
    h = C.c_void_p()
    assert nof.lib().nof_mipnerf_create(C.byref(cfg), C.byref(h)) == 1  # NOF_ERR_INVALID_ARG
    assert "distortion_loss_mult" in nof.lib().nof_last_error().decode()


def test_symbols_and_null_handles():
    import nof

    lib = nof.lib()
    for name in ("nof_mipnerf_distortion_loss", "nof_kernel_render_grad_dist"):
        assert hasattr(lib, name), name
        assert name in nof._lib.SIGNATURES, name
    assert hasattr(nof.AcceleratedMipNeRF, "distortion_loss")
    out = C.c_float()
    assert lib.nof_mipnerf_distortion_loss(None, C.byref(out)) == 1  # NOF_ERR_INVALID_ARG
    # the kernel entry refuses null arrays, a negative multiplier and a multiplier without loss multipliers
    nul = [None] * 4
    assert lib.nof_kernel_render_grad_dist(1, 64, *nul, 1, None, None, None, None, 1.0, 1.0, None, None, None, None,
                                           None, None, 0, 0.0, None, None) == 1
    one = (C.c_float * 256)()
    p = C.cast(one, C.c_void_p)
    args = lambda lm, mult: (0, 64, p, p, p, p, 1, p, p, None, lm, 1.0, 1.0, p, p, None, None, p, p, 0, mult, None, None)
    assert lib.nof_kernel_render_grad_dist(*args(None, -1.0)) == 1
    assert lib.nof_kernel_render_grad_dist(*args(None, 0.5)) == 1
    assert lib.nof_kernel_render_grad_dist(*args(p, 0.5)) == 0  # n = 0: nothing is launched


def test_python_driver_flag():
    from nof import train

    a = train.parse_args(["--synthetic", "64", "--distortion-loss-mult", "0.01"])
    assert a.distortion_loss_mult == 0.01
    assert train.parse_args(["--synthetic", "64"]).distortion_loss_mult == 0.0
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            train.parse_args(["--synthetic", "64", "--distortion-loss-mult", bad])


def test_native_driver_flag(tmp_path):
    exe = os.path.join(ROOT, "nerf-or-nothing_amd", "bin", "nof_train")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nerf-or-nothing_amd"), "bin/nof_train"])
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--distortion-loss-mult X" in out.stdout
    # the flag takes a value (none: usage, status 2); with one the arguments parse and the run goes on to the
    # missing record file (status 1, the library's message), and a negative value is the library's refusal
    out = subprocess.run([exe, "--records", "x.bin", "--distortion-loss-mult"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage:" in out.stderr
    out = subprocess.run([exe, "--records", str(tmp_path / "missing.bin"), "--steps", "1", "--distortion-loss-mult", "0.01"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "unknown argument" not in out.stderr and "failed (status" in out.stderr
