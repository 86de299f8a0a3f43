"""CPU checks of the interlevel (proposal) loss (nof_mipnerf_set_interlevel_loss): the fp64 reference
the GPU tests compare against (tests/interlevel_ref.py) is pinned here by its two closed forms, finite differences
and the properties of the definition; an fp32 numpy emulation of the kernel's summation order bounds what fp32 can
reach; the C ABI, the binding and both drivers' flags are checked without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import interlevel_ref as IL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(64, 64), (128, 128), (64, 512), (512, 64), (512, 512)]
_INPUTS = {}


def _inputs(Sc, Sf):
    """one generated case and its fp64 reference at mult = 1, computed once and shared (read only)"""
    if (Sc, Sf) not in _INPUTS:
        inp = IL.make_inputs(Sc, Sf)
        _INPUTS[(Sc, Sf)] = (inp, IL.kernel_ref(inp, 1.0))
    return _INPUTS[(Sc, Sf)]


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("Sc,Sf", CASES)
def test_generator_has_active_hinges(Sc, Sf):
    """on the reference alone: 10 % .. 90 % of the target intervals carry an active hinge, the special rays are there"""
    inp, ref = _inputs(Sc, Sf)
    frac = float(np.mean(ref["margin"] > 0))
    print(f"({Sc}, {Sf}): {100 * frac:.1f} % of the target intervals have an active hinge")
    assert 0.10 <= frac <= 0.90
    for row in (inp["tp"], inp["t"]):
        assert np.all(np.diff(row, axis=1) >= 0) and row.min() >= IL.NEAR and row.max() <= IL.FAR
    assert np.isin(inp["t"][1], inp["tp"][1]).sum() >= min((Sf + 1) // 4, Sc + 1)  # ties
    assert not np.any(inp["w"][3]) and inp["lm"][4] == 0.0 and inp["lm"][5] == 2.0
    assert np.sum(inp["w"][2] == np.float32(0.9)) == 1 and np.sum(inp["w"][2] == np.float32(1e-6)) == Sf - 1
    assert ref["margin"][2].max() > 0.1  # the surface's hinge is active


@pytest.mark.parametrize("Sc,Sf", CASES)
def test_range_form_is_scatter_form_is_definition(Sc, Sf):
    inp, ref = _inputs(Sc, Sf)
    msum = float(np.sum(inp["lm"], dtype=np.float32))
    for r in range(inp["n"]):
        a = [x[r].astype(np.float64) for x in (inp["wp"], inp["tp"], inp["w"], inp["t"])]
        sc, rg = IL.grad_scatter(*a), IL.grad_range(*a)
        auto = ref["w_grad"][r] * msum / float(inp["lm"][r]) if inp["lm"][r] else None
        assert np.max(np.abs(sc - rg)) <= 1e-12 * max(1.0, np.max(np.abs(sc)))
        if auto is not None:
            assert np.max(np.abs(sc - auto)) <= 1e-12 * max(1.0, np.max(np.abs(sc)))
        else:
            assert not np.any(ref["w_grad"][r])  # lossmult = 0
        lo, hi = IL._g(*a)[2:]
        aj, bj = IL.ranges(a[1], a[3])
        assert np.all(aj <= bj) and np.all(lo <= hi)


def test_finite_differences():
    """The directional derivative in w^ against central differences, h = 1e-6, on rays whose hinge margins
    |w_i - bound_i| all exceed 100 h (the hinge is C^1, its second derivative jumps at 0).  The generated target
    weights closer than that to their bound are moved 2e-4 off it, on the side they are on."""
    h = 1e-6
    inp, ref = _inputs(64, 64)
    w = inp["w"].astype(np.float64)
    margin = ref["margin"]
    near = np.abs(margin) <= 2e-4
    near[3] = False  # (the w = 0 ray stays as it is)
    w = np.where(near, (w - margin) + np.where(margin > 0, 2e-4, -2e-4), w)
    w = np.maximum(w, 0.0)
    wp = torch.tensor(inp["wp"].astype(np.float64), requires_grad=True)
    tp, t = inp["tp"].astype(np.float64), inp["t"].astype(np.float64)
    with torch.no_grad():
        m = (torch.from_numpy(w) - IL.bound(wp, tp, t)).abs().numpy()
    rays = [r for r in range(inp["n"]) if m[r].min() > 100 * h]
    assert len(rays) >= 3, rays
    L = IL.loss_rays(wp, tp, w, t)
    rng = np.random.default_rng(5)
    v = torch.from_numpy(rng.standard_normal(tuple(wp.shape)))
    (g,) = torch.autograd.grad(L.sum(), wp)
    with torch.no_grad():
        fd = (IL.loss_rays(wp + h * v, tp, w, t) - IL.loss_rays(wp - h * v, tp, w, t)) / (2 * h)
        ad = (g * v).sum(1)
    for r in rays:
        print(f"ray {r}: autograd {float(ad[r]):.9g} central difference {float(fd[r]):.9g}")
        assert abs(float(fd[r]) - float(ad[r])) <= 1e-6 * max(1.0, abs(float(ad[r])))
    assert max(abs(float(ad[r])) for r in rays) > 1e-2  # (something to compare)


@pytest.mark.parametrize("Sc,Sf", [(64, 64), (512, 64), (64, 512)])
def test_envelope_and_empty_target(Sc, Sf):
    """a proposal that is an envelope costs nothing; a ray with w = 0 gives exactly 0 value and gradient"""
    inp, ref = _inputs(Sc, Sf)
    assert ref["L"][3] == 0.0 and ref["rays"][3] == 0.0 and not np.any(ref["w_grad"][3])
    # every target interval lies inside the union of the proposal intervals it touches only if the proposal row
    # spans the target row: give both rows the same end points, then bound_i >= the proposal mass under interval i
    tp, t = inp["tp"].astype(np.float64).copy(), inp["t"].astype(np.float64).copy()
    tp[:, 0] = t[:, 0] = IL.NEAR
    tp[:, -1] = t[:, -1] = IL.FAR
    # a piecewise-constant density and its two histograms: the proposal's doubled is an envelope
    rng = np.random.default_rng(3)
    dens = rng.gamma(0.5, 1.0, (inp["n"], 97))
    grid = np.linspace(IL.NEAR, IL.FAR, 98)
    cum = lambda x: np.stack([np.interp(x[r], grid, np.concatenate([[0.0], np.cumsum(dens[r] * np.diff(grid))]))
                              for r in range(inp["n"])])
    wp, w = np.diff(cum(tp), axis=1), np.diff(cum(t), axis=1)
    L1 = IL.loss_rays(torch.from_numpy(wp), tp, w, t).numpy()
    L2 = IL.loss_rays(torch.from_numpy(2 * wp), tp, w, t).numpy()
    assert np.all(L1 <= 1e-20) and np.all(L2 == 0.0)  # (the histogram of the same density is an envelope already)
    # and the generated rays: the weights doubled everywhere never cost more, and a large enough multiple costs nothing
    wpg = torch.from_numpy(inp["wp"].astype(np.float64))
    a = [inp["tp"].astype(np.float64), inp["w"].astype(np.float64), inp["t"].astype(np.float64)]
    assert np.all(IL.loss_rays(2 * wpg, *a).numpy() <= ref["L"])


def test_doubled_weights_cost_nothing():
    """w^ doubled everywhere: with w^ the target's own histogram on the same edges bound_i >= w_i, so L = 0 for both;
    with w^ = w / 2 the hinge is active, and doubling that removes it"""
    inp, _ = _inputs(64, 64)
    t = inp["t"].astype(np.float64)
    w = inp["w"].astype(np.float64)
    half = torch.from_numpy(w / 2)
    L_half = IL.loss_rays(half, t, w, t).numpy()
    L_full = IL.loss_rays(2 * half, t, w, t).numpy()
    assert np.all(L_half[[0, 1, 2, 4, 5]] > 0) and np.all(L_full == 0.0)


@pytest.mark.parametrize("Sc,Sf", CASES)
def test_fp32_emulation_of_the_kernel_order(Sc, Sf):
    """the kernel's summation order in fp32 (direct bound, prefix sums of g): rel L2 <= 1e-5 per tensor"""
    inp, ref = _inputs(Sc, Sf)
    msum = np.float32(np.sum(inp["lm"], dtype=np.float32))
    gw, gr = np.zeros_like(inp["wp"]), np.zeros(inp["n"], np.float32)
    for r in range(inp["n"]):
        c = np.float32(np.float32(1.0) * inp["lm"][r]) / msum
        gw[r], gr[r] = IL.emulate_f32(inp["wp"][r], inp["tp"][r], inp["w"][r], inp["t"][r], c)
    e_w, e_r = _rel(gw, ref["w_grad"]), _rel(gr, ref["rays"])
    print(f"({Sc}, {Sf}): fp32 emulation dL/dw^ {e_w:.2e}, per-ray term {e_r:.2e}")
    assert e_w <= 1e-5 and e_r <= 1e-5
    assert not np.any(gw[3]) and gr[3] == 0.0 and not np.any(gw[4]) and gr[4] == 0.0


# ---- the interface, without a device ---------------------------------------------------------------------------------
NEW = ["nof_mipnerf_set_interlevel_loss", "nof_mipnerf_interlevel_loss", "nof_kernel_interlevel"]


def test_symbols_exported_and_bound():
    import nof

    lib = nof.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in nof._lib.SIGNATURES, name
    assert hasattr(nof.AcceleratedMipNeRF, "set_interlevel_loss") and hasattr(nof.AcceleratedMipNeRF, "interlevel_loss")
    assert callable(nof.kernel_interlevel)
    with open(os.path.join(ROOT, "include", "nof.h")) as f:
        header = f.read()
    for name in NEW:
        assert name + "(" in header, name


def test_config_struct_is_unchanged():
    import nof

    assert nof.lib().nof_config_size() == C.sizeof(nof._lib.nof_config)
    assert nof._lib.nof_config._fields_[-1][0] == "stop_level_grad"
    assert not hasattr(nof.default_config(), "interlevel_loss_mult")


def test_bad_arguments_refused_without_a_device_call():
    import nof

    lib = nof.lib()
    out = C.c_float()
    assert lib.nof_mipnerf_set_interlevel_loss(None, 1.0) == 1  # NOF_ERR_INVALID_ARG
    assert lib.nof_mipnerf_interlevel_loss(None, C.byref(out)) == 1
    # (a bad multiplier with a real handle is named in nof_last_error: tests/test_gpu_interlevel.py)
    buf = (C.c_float * 1024)()
    p = C.cast(buf, C.c_void_p)
    order = ("n", "Sc", "tp", "wp", "Sf", "t", "w", "lm", "msum", "mult", "acc", "q", "rays", "stream")
    good = dict(n=0, Sc=64, tp=p, wp=p, Sf=64, t=p, w=p, lm=p, msum=1.0, mult=1.0, acc=0, q=p, rays=None, stream=None)

    def ok(**k):
        a = {**good, **k}
        return lib.nof_kernel_interlevel(*[a[x] for x in order])

    assert ok() == 0  # n = 0: nothing is launched
    for key in ("tp", "wp", "t", "w", "lm", "q"):
        assert ok(**{key: None}) == 1, key
    for S in (0, 32, 96, 1024, -64):
        assert ok(Sc=S) == 1 and ok(Sf=S) == 1, S
    for mult in (-1.0, float("nan"), float("inf")):
        assert ok(mult=mult) == 1
    assert ok(n=-1) == 1 and ok(msum=0.0) == 1 and ok(acc=2) == 1
    assert ok(n=1, q=None) == 1  # refused before the launch
    assert b"invalid argument" in lib.nof_last_error()


def test_python_driver_flag():
    from nof import train

    a = train.parse_args(["--synthetic", "64", "--interlevel-loss-mult", "0.5"])
    assert a.interlevel_loss_mult == 0.5
    assert train.parse_args(["--synthetic", "64"]).interlevel_loss_mult == 0.0
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            train.parse_args(["--synthetic", "64", "--interlevel-loss-mult", bad])


def test_native_driver_flag(tmp_path):
    exe = os.path.join(ROOT, "nerf-or-nothing_amd", "bin", "nof_train")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nerf-or-nothing_amd"), "bin/nof_train"])
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--interlevel-loss-mult X" in out.stdout
    out = subprocess.run([exe, "--records", "x.bin", "--interlevel-loss-mult"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage:" in out.stderr
    for bad in ("-1", "nan", "inf"):
        out = subprocess.run([exe, "--records", "x.bin", "--interlevel-loss-mult", bad], capture_output=True, text=True,
                             timeout=60)
        assert out.returncode == 2 and "--interlevel-loss-mult must be a finite number >= 0" in out.stderr, bad
    # a good value parses and the run goes on to the missing record file (status 1, the library's message)
    out = subprocess.run([exe, "--records", str(tmp_path / "missing.bin"), "--steps", "1", "--interlevel-loss-mult", "0.5"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "unknown argument" not in out.stderr and "failed (status" in out.stderr
