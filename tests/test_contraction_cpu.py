"""CPU checks of the scene contraction (nof_mipnerf_set_contraction): the fp32 restatement of the kernel's
operation order (tests/contraction_ref.py contract32, what the GPU tests require bit for bit) against fp64, the fp64
reference against the definition (J by autograd, continuity at |m| = 1, finite differences, the radius-2 ball), and the
C ABI, the binding and both drivers' flags without a device.

The bound of contract32 against fp64, |got - ref| <= 1e-5 |ref| element-wise: every output is a sum of non-negative
terms over fewer than 20 correctly rounded operations, so the error is at most about 1.2e-6; 1e-5 is the project's fp32
bound.  The naive expansion of v' is shown to break it at u = (1, 0, 0), n = 1e3, v = (1, 1e-6, 1e-6)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import contraction_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
TOL = 1e-5
NORMS = [f32(0.5), np.nextafter(f32(1), f32(0)), f32(1), np.nextafter(f32(1), f32(2)), f32(1.5), f32(10), f32(1e3),
         f32(1e4)]
_CASES = {}


def _dirs():
    rng = np.random.default_rng(11)
    g = rng.standard_normal((5, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    return np.concatenate([axes, g, [[1, 1, 1] / np.sqrt(3.0), [0.6, 0.8, 0.0]]])


def _covs():
    rng = np.random.default_rng(12)
    fixed = [[1, 1, 1], [1, 1e-6, 1e-6], [1e-6, 1, 1e-6], [1e-6, 1e-6, 1], [1, 1e-3, 1e-6], [1e-6, 1, 1], [3e-4, 3e-4, 3e-4]]
    return np.concatenate([fixed, 10.0 ** rng.uniform(-6, 0, (4, 3))])


def _cases():
    """every (|m|, direction, cov) once, with contract32's and the fp64 reference's results (shared, read only)"""
    if not _CASES:
        U, V = _dirs(), _covs()
        m = np.stack([f32(n) * u.astype(f32) for n in NORMS for u in U for _ in V]).astype(f32)
        v = np.stack([c for _ in NORMS for _ in U for c in V]).astype(f32)
        pinned = (np.array([[1e3, 0, 0]], f32), np.array([[1, 1e-6, 1e-6]], f32))
        m, v = np.concatenate([pinned[0], m]), np.concatenate([pinned[1], v])  # row 0: the case the naive form fails
        got = CR.contract32(m, v)
        ref = CR.contract(torch.from_numpy(m.astype(np.float64)), torch.from_numpy(v.astype(np.float64)))
        _CASES.update(m=m, v=v, got=got, ref=tuple(x.numpy() for x in ref))
    return _CASES


def test_contract32_matches_fp64_elementwise():
    c = _cases()
    assert c["v"].max() / c["v"].min() >= 1e6
    n = np.linalg.norm(c["m"].astype(np.float64), axis=1)
    assert np.any(n <= 1) and np.any(n > 1) and n.max() >= 9e3
    worst = 0.0
    for got, ref, name in zip(c["got"], c["ref"], ("mean", "cov")):
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - ref)
        ok = err <= TOL * np.abs(ref)
        rel = float(np.max(err / np.maximum(np.abs(ref), 1e-300)))
        worst = max(worst, rel)
        print(f"contract32 vs fp64, {name}: worst element-wise relative error {rel:.3e}")
        assert np.all(ok), (name, c["m"][~ok.all(1)][:3], c["v"][~ok.all(1)][:3], got[~ok.all(1)][:3], ref[~ok.all(1)][:3])
    # the stated error budget holds with room: fewer than 20 roundings of non-negative terms
    assert worst <= 20 * 2.0 ** -24


def test_naive_expansion_breaks_the_bound():
    c = _cases()
    m, v = c["m"][:1], c["v"][:1]
    assert np.array_equal(m, [[f32(1e3), 0, 0]]) and np.array_equal(v, np.array([[1, 1e-6, 1e-6]], f32))
    ref = c["ref"][1][0]
    naive = CR.naive32(m, v)[0].astype(np.float64)
    rel = abs(naive[0] - ref[0]) / ref[0]  # the radial axis: a^2 + 2 a c + c^2 = b^2 cancels by n^2
    print(f"naive expansion at n = 1e3, radial axis: relative error {rel:.3e}")
    assert rel > TOL
    assert abs(float(c["got"][1][0][0]) - ref[0]) <= TOL * ref[0]


def test_identity_inside_is_bitwise_and_nan_passes_through():
    m = np.array([[0.3, -0.4, 0.5], [1, 0, 0], [0, -1, 0], [np.nan, 0.1, 0.2], [0.1, np.nan, 5.0], [-0.0, 0.0, 1e-30]], f32)
    v = np.array([[1e-3, 2e-3, 3e-3], [1, 2, 3], [1e-6, 1, 1e-3], [1, 2, 3], [4, 5, 6], [np.nan, 1e-40, 0]], f32)
    gm, gv = CR.contract32(m, v)
    assert np.array_equal(gm.view(np.uint32), m.view(np.uint32)) and np.array_equal(gv.view(np.uint32), v.view(np.uint32))


def _mean_jacobian(m):
    return torch.autograd.functional.jacobian(lambda x: CR.contract(x, torch.ones(3, dtype=torch.float64))[0], m)


def test_cov_is_the_diagonal_of_J_cov_Jt():
    """element-wise, relative 1e-12.  |m| up to 100: autograd's own J holds the radial entry a + c = b only to
    2 n eps64 of a (it forms the cancelling sum), 4e-14 there and past 1e-12 from n = 2e3 on"""
    rng = np.random.default_rng(13)
    for n in (0.5, 1.5, 10.0, 100.0):
        for u in _dirs()[3:]:
            m = torch.tensor(n * u, dtype=torch.float64)
            v = torch.tensor(10.0 ** rng.uniform(-6, 0, 3), dtype=torch.float64)
            J = _mean_jacobian(m)
            want = torch.diagonal(J @ torch.diag(v) @ J.T)
            got = CR.contract(m, v)[1]
            assert torch.all(torch.abs(got - want) <= 1e-12 * torch.abs(want)), (n, u, got, want)


def test_value_and_jacobian_agree_across_the_unit_sphere():
    eps = 1e-6
    for u in _dirs()[6:]:
        v = torch.tensor([1e-2, 3e-4, 5e-3], dtype=torch.float64)
        lo, hi = torch.tensor((1 - eps) * u, dtype=torch.float64), torch.tensor((1 + eps) * u, dtype=torch.float64)
        (m0, v0), (m1, v1) = CR.contract(lo, v), CR.contract(hi, v)
        assert torch.equal(m0, lo) and torch.equal(v0, v)  # inside: the identity
        assert not torch.equal(m1, hi)
        assert torch.allclose(m0, m1, rtol=0, atol=4 * eps) and torch.allclose(v0, v1, rtol=8 * eps, atol=0)
        J0, J1 = _mean_jacobian(lo), _mean_jacobian(hi)
        assert torch.equal(J0, torch.eye(3, dtype=torch.float64))
        assert torch.allclose(J0, J1, rtol=0, atol=8 * eps)  # J = I at n = 1: the mean map is C^1


def test_reference_adjoint_matches_finite_differences():
    """central differences with h = 1e-4 max(|x|, 1e-2): the truncation h^2 |L'''| / 6 (1e-8 relative, L cubic-ish in
    m at these points) and the rounding eps64 |L| / h (1e-10 of a gradient of order 1e-2 and more) stay under the
    bound 1e-7"""
    rng = np.random.default_rng(14)
    worst = 0.0
    for n in (0.7, 1.3, 4.0, 50.0):
        for u in _dirs()[6:]:
            m0, v0 = n * u, 10.0 ** rng.uniform(-4, -1, 3)
            gm, gv = rng.standard_normal(3), rng.standard_normal(3)

            def L(x):
                a, b = CR.contract(x[:3], x[3:], snap=False)
                return (a * torch.from_numpy(gm)).sum() + (b * torch.from_numpy(gv)).sum()

            x = torch.tensor(np.concatenate([m0, v0]), dtype=torch.float64, requires_grad=True)
            L(x).backward()
            fd = np.zeros(6)
            for k in range(6):
                h = 1e-4 * max(abs(float(x.detach()[k])), 1e-2)
                e = torch.zeros(6, dtype=torch.float64)
                e[k] = h
                with torch.no_grad():
                    fd[k] = float(L(x + e) - L(x - e)) / (2 * h)
            err = np.linalg.norm(x.grad.numpy() - fd) / np.linalg.norm(fd)
            worst = max(worst, err)
            assert err <= 1e-7, (n, u, x.grad.numpy(), fd)
    print(f"reference adjoint vs central differences: worst rel L2 {worst:.2e}")


def test_contracted_means_stay_inside_radius_two():
    """|m'| = 2 - 1 / n < 2.  In fp32 the margin 1 / n has to exceed the rounding of (2 - 1 / n) u, about 3e-7: checked
    up to |m| = 1e5, a hundred times the far planes the option is meant for"""
    c = _cases()
    for mean in (c["got"][0], c["ref"][0]):
        assert np.all(np.linalg.norm(mean.astype(np.float64), axis=1) < 2.0)
    rng = np.random.default_rng(15)
    u = rng.standard_normal((4096, 3))
    far = (u / np.linalg.norm(u, axis=1, keepdims=True) * 10.0 ** rng.uniform(0, 5, (4096, 1))).astype(f32)
    gm, gv = CR.contract32(far, np.ones_like(far))
    r = np.linalg.norm(gm.astype(np.float64), axis=1)
    assert np.all(r < 2.0) and np.all(np.isfinite(gm)) and np.all(gv >= 0) and r.max() > 1.9999


# ---- the interface, without a device ---------------------------------------------------------------------------------
NEW = ["nof_mipnerf_set_contraction", "nof_mipnerf_get_contraction", "nof_kernel_cast_contract",
       "nof_kernel_encode_grad_ex", "nof_kernel_ray_grad_ex"]


def test_symbols_exported_and_bound():
    import nof

    lib = nof.lib()
    with open(os.path.join(ROOT, "include", "nof.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in nof._lib.SIGNATURES, name
        assert name + "(" in header, name
    assert "NOF_CONTRACT_NONE = 0" in header and "NOF_CONTRACT_SPHERE = 1" in header
    assert hasattr(nof.AcceleratedMipNeRF, "set_contraction") and hasattr(nof.AcceleratedMipNeRF, "contraction")
    # the extended entry points: the entry point's own argument list plus one trailing int32
    S = nof._lib.SIGNATURES
    assert S["nof_kernel_cast_contract"] == S["nof_kernel_cast_ex"] + [C.c_int32]
    assert S["nof_kernel_encode_grad_ex"] == S["nof_kernel_encode_grad"] + [C.c_int32]
    assert S["nof_kernel_ray_grad_ex"] == S["nof_kernel_ray_grad"] + [C.c_int32]


def test_null_handle_refused_without_a_device_call():
    import nof

    lib = nof.lib()
    mode = C.c_int32(7)
    for m in (0, 1, 2):
        assert lib.nof_mipnerf_set_contraction(None, m) == 1  # NOF_ERR_INVALID_ARG
    assert lib.nof_mipnerf_get_contraction(None, C.byref(mode)) == 1 and mode.value == 7
    assert b"invalid argument" in lib.nof_last_error()
    # the kernel entry points: n = 0 launches nothing; an unknown mode or a null pointer is refused before a launch
    buf = (C.c_float * 1024)()
    p = C.cast(buf, C.c_void_p)
    cast = lambda n=0, t=p, con=1: lib.nof_kernel_cast_contract(n, 64, t, p, p, p, p, p, None, 0, con)
    assert cast() == 0 and cast(con=0) == 0
    assert cast(con=2) == 1 and cast(con=-1) == 1 and cast(t=None) == 1 and cast(n=-1) == 1
    eg = lambda con: lib.nof_kernel_encode_grad_ex(0, 64, p, p, p, p, 0, 0, 4, p, p, p, None, con)
    rg = lambda con: lib.nof_kernel_ray_grad_ex(0, 64, p, p, p, p, 0, 0, 4, p, p, p, p, 2, p, p, 0, p, p, None, con)
    for f in (eg, rg):
        assert f(0) == 0 and f(1) == 0 and f(2) == 1 and f(-1) == 1


def test_config_struct_is_unchanged():
    import nof

    assert nof.lib().nof_config_size() == C.sizeof(nof._lib.nof_config)
    assert nof._lib.nof_config._fields_[-1][0] == "stop_level_grad"
    assert not hasattr(nof.default_config(), "contraction")


def test_python_driver_flag():
    from nof import train

    assert train.parse_args(["--synthetic", "64", "--contract"]).contract is True
    assert train.parse_args(["--synthetic", "64"]).contract is False
    a = train.parse_args(["--synthetic", "64", "--contract", "--lindisp", "--precision", "f16p"])
    assert a.contract and a.lindisp and a.precision == "f16p"


def test_python_driver_help_names_the_expectations(capsys):
    from nof import train

    with pytest.raises(SystemExit):
        train.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--contract" in text and "inside the unit ball" in text and "--lindisp with a large far plane" in text


def test_native_driver_flag(tmp_path):
    exe = os.path.join(ROOT, "nerf-or-nothing_amd", "bin", "nof_train")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nerf-or-nothing_amd"), "bin/nof_train"])
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    text = " ".join(out.stdout.split())
    assert out.returncode == 0 and "[--contract]" in text
    assert "inside the unit ball" in text and "--lindisp with a large far plane" in text
    # the flag parses and the run goes on to the missing record file (status 1, the library's message)
    out = subprocess.run([exe, "--records", str(tmp_path / "missing.bin"), "--steps", "1", "--contract", "--lindisp"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "unknown argument" not in out.stderr and "failed (status" in out.stderr
