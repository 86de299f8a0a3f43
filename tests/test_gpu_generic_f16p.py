"""GPU tests of NOF_PRECISION_F16_PRODUCTS (mode 5): the any-shape path with one fp16 product per term
(gemm_h.hip, k_gemm_h on v_mfma_f32_16x16x32_f16), for every network.

Product level (nof_kernel_gemm_h against a numpy emulation, sum over k of f16(s X) f16(Y) / s in fp64): the bound is
the project's fp32 contract, relative L2 <= 1e-5 — only the fp32 accumulation separates the two (sequential fp32
accumulation of the same products on the CPU: 3e-7 at K = 300, 1.6e-6 at K = 8192) — and the result must be
MORE than 1e-4 from the unrounded fp64 product (the emulation itself is 2.9e-4 from it for these inputs), so an
fp32 kernel cannot pass.  Step level: the structure of test_gpu_generic._check at the perf-mode contract
(DESIGN section 3): t bit-exact, outputs / integrator adjoint within 2e-3 of the fp64 oracle with its own ReLU
decisions, every gradient tensor within 2e-3 with the GPU's decisions adopted, loss within 2e-3.

Measured on an MI355X: see MEASURED below (filled from the printed figures of a run).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import rel_l2
from test_gpu_generic import SPECS, _cfg, _ospec

pytestmark = pytest.mark.gpu
TOL_EMU = 1e-5      # GPU vs the emulation: fp32 accumulation only
FAR_EXACT = 1e-4    # GPU vs the unrounded product: at least this far (fp16 operand rounding, about 2.9e-4)
TOL = 2e-3          # the perf-mode contract
REFERENCE = (8, 256, 1, 128, 4, 0, 16, 4)

# Measured on an MI355X (printed by the tests): product level, GPU vs emulation / vs the unrounded product; step
# level, worst / median gradient tensor and the worst output.
MEASURED = """
product level (vs emulation, bound 1e-5 / vs the unrounded product, must exceed 1e-4):
  boundary 6.3e-8 / 2.86e-4, ragged 1.2e-7 / 2.91e-4, head 7.8e-8 / 3.01e-4, dh 5.2e-8 / 2.96e-4, per_ray 4.8e-8 / 2.99e-4,
  wgrad30 1.1e-7 / 2.91e-4 (rowsum 2.5e-8), wgrad136 1.1e-7 / 2.93e-4 (rowsum 2.5e-8),
  delta: scaled 4.8e-8 / 2.88e-4, with scale_amax null 0.175 from the product (must exceed 1e-2)
step level (gradient tensors worst / median, outputs and adjoint worst; bound 2e-3), 4 rays x (64, 64):
  wide_3x272_2x136 4.3e-4 / 3.3e-4, 1.3e-4;  unaligned_2x50_1x30 4.4e-4 / 3.2e-4, 2.1e-4;
  odd_5x96_3x40 7.5e-4 / 3.5e-4, 1.6e-4;  tiny_2x32_skip1 3.1e-4 / 1.9e-4, 2.6e-4;  configs0_4x128 4.2e-4 / 2.5e-4, 1.3e-4
  8 rays x (64, 128): wide 4.3e-4 / 3.3e-4, 1.4e-4;  odd 7.1e-4 / 4.0e-4, 2.4e-4
  reference 8x256, 2 rays x (64, 64): 6.6e-4 / 3.8e-4, 1.6e-4
mode 5 against mode 0 of the same model (odd_5x96_3x40, 16 rays x (64, 128)): gradient arena rel L2 1.7e-3
ten Adam steps on configs0_4x128: loss 0.359 -> 0.142
"""


# ---------------------------------------------------------------------------------------------------------------
# product level
# ---------------------------------------------------------------------------------------------------------------
def _f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def _scale(amax):
    """delta_scale (mlp_common.h): 2^(8 - floor(log2 amax)), 1 for amax = 0 or not finite"""
    if not (amax > 0 and np.isfinite(amax)):
        return 1.0
    _, e = np.frexp(np.float32(amax))
    return float(np.ldexp(1.0, int(np.clip(8 - (int(e) - 1), -100, 100))))


def _emulate(A, B, s=1.0, rounded=True):
    """sum_k f16(s A(i, k)) f16(B(j, k)) / s in fp64 (rounded = False: the plain fp64 product)"""
    if not rounded:
        return A.astype(np.float64) @ B.astype(np.float64).T
    a = _f16(np.float32(s) * A.astype(np.float32))
    return (a @ _f16(B).T) / s


@functools.lru_cache(maxsize=None)
def _case(name):
    """Seeded operands of a product case: standard-normal A, 0.1 x normal B (dense [rows][k] matrices) and what the
    kernel is told about them."""
    rng = np.random.default_rng({"boundary": 1, "ragged": 2, "head": 3, "dh": 4, "per_ray": 5, "wgrad30": 6,
                                 "wgrad136": 7, "delta": 8}[name])
    n = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    c = dict(name=name, K2=0, bias=None, relu=0, G=None, ksplit=1, rowsum=False, amax=None, idiv2=1)
    if name == "boundary":    # source boundary and tail inside a 32-step; widths off 8 halves
        c.update(M=192, N=50, K1=50, K2=24)
    elif name == "ragged":    # ragged row tile, 5 column tiles with the last 16 wide; bias + ReLU
        c.update(M=70, N=272, K1=272, K2=30, relu=1)
        c["bias"] = 0.1 * n(272)
    elif name == "head":      # a head: 3 live columns, C rows 4 floats apart
        c.update(M=200, N=3, K1=136)
        c["bias"] = 0.1 * n(3)
    elif name == "dh":        # the dh_{D-1} product: B read transposed, B2.sk == 0, G mask
        c.update(M=130, N=272, K1=40, K2=1)
        c["G"] = n(130, 272)
    elif name == "per_ray":   # A2 per ray through idiv = 64
        c.update(M=128, N=9, K1=20, K2=9, idiv2=64)
    elif name == "wgrad30":   # split-K weight gradient, A = dZ^T (si = 1), kchunk 256, rowsum; 64-column tiles
        c.update(M=272, N=30, K1=1024, ksplit=4, rowsum=True)
    elif name == "wgrad136":  # ... 128-column tiles
        c.update(M=272, N=136, K1=1024, ksplit=4, rowsum=True)
    elif name == "delta":     # A about 1e-7: vanishes in fp16 without the scale
        c.update(M=130, N=64, K1=40)
    K = c["K1"] + c["K2"]
    A = n(c["M"], K)
    if name == "per_ray":     # rows of a ray share the second source
        A[:, c["K1"]:] = np.repeat(A[::64, c["K1"]:], 64, axis=0)
    if name == "delta":
        A *= np.float32(1e-7)
        c["amax"] = float(np.abs(A).max())
    c["A"], c["B"] = A, (0.1 * n(c["N"], K)).astype(np.float32)
    return c


def _reference(c, s):
    """(emulated, exact) results of a case in fp64, epilogue applied; split-K: [ksplit][M][N] partials"""
    out = []
    for rounded in (True, False):
        if c["ksplit"] > 1:
            kc = c["K1"] // c["ksplit"]
            r = np.stack([_emulate(c["A"][:, z * kc:(z + 1) * kc], c["B"][:, z * kc:(z + 1) * kc], s, rounded)
                          for z in range(c["ksplit"])])
        else:
            r = _emulate(c["A"], c["B"], s, rounded)
        if c["bias"] is not None:
            r = r + c["bias"].astype(np.float64)
        if c["relu"]:
            r = np.maximum(r, 0.0)
        if c["G"] is not None:
            r = np.where(c["G"] > 0, r, 0.0)
        out.append(r)
    return out


def _launch(c, gpu, scaled=True):
    """Run the case through nof_kernel_gemm_h with the operand layouts gen_forward / gen_backward use."""
    import torch
    import nof

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    M, N, K1, K2, name = c["M"], c["N"], c["K1"], c["K2"], c["name"]
    A, B = c["A"], c["B"]
    keep, kw = [], {}
    if name in ("wgrad30", "wgrad136"):  # A(o, m) = dZ[m][o], B(j, m) = X[m][j]
        dz, x = dev(A.T), dev(B.T)
        keep += [dz, x]
        kw.update(A1=(dz, 1, M), B1=(x, 1, N))
    elif name == "dh":  # A = [cur | dz_density (4 floats apart)], B = [W_view^T | w_D (sk 0)]
        cur, dz = dev(A[:, :K1]), dev(np.pad(A[:, K1:], ((0, 0), (3, 0))))
        wv, wd = dev(np.pad(B[:, :K1].T, ((0, 0), (0, 9)))), dev(B[:, K1])  # W_view [Wc][W + Vd]
        keep += [cur, dz, wv, wd]
        kw.update(A1=(cur, K1, 1), A2=(dz[:, 3:], 4, 1), B1=(wv, 1, N + 9), B2=(wd, 1, 0))
    else:
        a1, w = dev(A[:, :K1]), dev(B)
        keep += [a1, w]
        kw.update(A1=(a1, K1, 1), B1=(w, K1 + K2, 1))
        if K2:
            a2 = dev(A[::c["idiv2"], K1:])
            keep.append(a2)
            kw.update(A2=(a2, K2, 1, c["idiv2"]), B2=(w[:, K1:], K1 + K2, 1))
    ci = 4 if name == "head" else N
    out = torch.full((c["ksplit"], M, ci), float("nan"), device=gpu)
    kw.update(C=out, ci=ci, cj=1, slab_stride=M * ci)
    rs = None
    if c["rowsum"]:
        rs = torch.full((c["ksplit"], M), float("nan"), device=gpu)
        kw["rowsum"] = rs
    for k in ("bias", "G"):
        if c[k] is not None:
            t = dev(c[k])
            keep.append(t)
            kw[k] = t
    if c["G"] is not None:
        kw.update(gi=N, gj=1)
    if c["amax"] is not None and scaled:
        am = torch.from_numpy(np.array([c["amax"]], np.float32).view(np.int32)).to(gpu)
        keep.append(am)
        kw.update(scale_amax=am)
    if c["amax"] is not None:
        kw["scale_src"] = 1
    kchunk = K1 // c["ksplit"] if c["ksplit"] > 1 else (K1 + K2 + 31) // 32 * 32
    nof.kernel_gemm_h(M=M, N=N, K1=K1, K2=K2, relu=c["relu"], kchunk=kchunk, ksplit=c["ksplit"], **kw)
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:, :, :N]
    if name == "head":
        assert np.all(np.isnan(out.cpu().numpy()[:, :, 3])), "the kernel wrote past its 3 live columns"
    return (got if c["ksplit"] > 1 else got[0]), (rs.cpu().numpy() if rs is not None else None)


@pytest.mark.parametrize("name", ["boundary", "ragged", "head", "dh", "per_ray", "wgrad30", "wgrad136"])
def test_gemm_h_product(gpu, name):
    """One product per place the kernel can go wrong (the table in _case), against the emulation within 1e-5 and
    away from the unrounded product by more than 1e-4; the row sums (split-K cases) likewise against
    sum_k f16(A(i, k))."""
    c = _case(name)
    got, rs = _launch(c, gpu)
    emu, exact = _reference(c, 1.0)
    e_emu, e_exact = rel_l2(got, emu), rel_l2(got, exact)
    print(f"gemm_h {name}: vs emulation {e_emu:.2e}, vs the unrounded product {e_exact:.2e}")
    assert np.all(np.isfinite(got))
    assert e_emu <= TOL_EMU and e_exact > FAR_EXACT
    if rs is not None:
        kc = c["K1"] // c["ksplit"]
        want = np.stack([_f16(c["A"][:, z * kc:(z + 1) * kc]).sum(axis=1) for z in range(c["ksplit"])])
        e_rs = rel_l2(rs, want)
        print(f"gemm_h {name}: rowsum vs emulation {e_rs:.2e}")
        assert e_rs <= TOL_EMU


def test_gemm_h_delta_scale(gpu):
    """An A operand of about 1e-7 (fp16's smallest subnormal is 6e-8): with the amax word set the product meets
    the 1e-5 bound against the scaled emulation, and with scale_amax null it is wrong by more than 1e-2 (the CPU
    emulation of the unscaled product: 0.17) — the scale is applied, inside the product."""
    c = _case("delta")
    s = _scale(c["amax"])
    assert 256.0 <= s * c["amax"] < 512.0
    emu, exact = _reference(c, s)
    got, _ = _launch(c, gpu, scaled=True)
    raw, _ = _launch(c, gpu, scaled=False)
    e_emu, e_exact, e_raw = rel_l2(got, emu), rel_l2(got, exact), rel_l2(raw, exact)
    print(f"gemm_h delta: scaled vs emulation {e_emu:.2e}, vs the unrounded product {e_exact:.2e}; unscaled {e_raw:.2e}")
    assert e_emu <= TOL_EMU and e_exact > FAR_EXACT
    assert e_raw > 1e-2


# ---------------------------------------------------------------------------------------------------------------
# step level
# ---------------------------------------------------------------------------------------------------------------
_U = ("k_gemm_h<64,false,false>.unsplit", "k_gemm_h<64,true,false>.unsplit", "k_gemm_h<64,false,true>.unsplit",
      "k_gemm_h<64,true,true>.unsplit")
_S64, _S128 = "k_gemm_h<64,false,false>.splitk", "k_gemm_h<128,false,false>.splitk"
# Which k_gemm_h variants a spec's step launches, exactly.  Every network runs the four unsplit ones (layer 0; the
# view layer's two sources; the masked dX products; the dh_{D-1} product with two sources and a mask); with at
# least 4 rays x 64 samples every weight gradient is split, on 128-column tiles where its input block is wider
# than 64 and on 64-column tiles else.
DISPATCH_H = {
    "wide_3x272_2x136": (*_U, _S64, _S128),        # columns 272, 136 | 30 (the IPE), 9
    "unaligned_2x50_1x30": (*_U, _S64),            # columns 50, 30, 24
    "odd_5x96_3x40": (*_U, _S64, _S128),           # columns 96 | 40, 48
    "tiny_2x32_skip1": (*_U, _S64),                # columns 32, 16, 24
    "configs0_4x128": (*_U, _S128),                # columns 128, 96
    "reference_8x256": (*_U, _S128),               # columns 256, 128, 96
}
UNREACHED_H = {}  # every name is reached


def _spec(name):
    return REFERENCE if name == "reference_8x256" else SPECS[name]


def _run(model, r, dev, msum=None):
    import torch

    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in r.items()}
    n = r["o"].shape[0]
    if msum is None:
        msum = float(np.sum(r["lossmult"], dtype=np.float32))
    return model.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"],
                                     msum)


def _assert_dispatch(model, name, levels):
    """The fp16 tally's non-zero set is exactly DISPATCH_H[name]; in the shared tally no k_gemm_ws ran, the k_gemm
    launches are the view PE's weight gradient alone (one per level), and the shared kernels are counted."""
    got = {k for k, c in model.mlp.gen_dispatch_h(clear=True).items() if c}
    print(f"dispatch_h {name!r}: {sorted(got)!r}")
    assert not any(model.mlp.gen_dispatch_h().values()), "gen_dispatch_h(clear=True) left counts behind"
    want = set(DISPATCH_H[name])
    assert got == want, f"{name}: launched but not tabulated {sorted(got - want)}, tabulated but not launched " \
                        f"{sorted(want - got)}"
    old = model.mlp.gen_dispatch(clear=True)
    assert not any(c for k, c in old.items() if k.startswith("k_gemm_ws<")), old
    assert sum(c for k, c in old.items() if k.startswith("k_gemm<")) == levels, old
    assert old["k_ray_sum"] == levels and old["k_slab_sums"] >= levels
    assert old["k_encode_g"] + old["k_encode_g4"] == levels


def _check(gpu, oracle, name, n, samples, params=None):
    """params: None for the model's own Glorot draw, or a callable (oracle, spec, Glorot arena) -> arena that is
    installed before the step (tests/param_sets.py)."""
    import torch
    import nof
    from nof import synth
    from param_sets import install, same_bits

    spec = _spec(name)
    seed, step, ray_base = 0x77, 2, 40
    model = nof.AcceleratedMipNeRF(seed=seed, max_rays=n, num_samples=samples, num_levels=len(samples), precision=5,
                                   **_cfg(spec))
    model.set_rng(seed, step, ray_base)
    sp = _ospec(oracle, spec)
    sizes = oracle.layer_sizes(sp)
    assert model.GetLayerSizes() == list(sizes)
    pptr, P = model.mlp.flat_params()
    installed = None if params is None else install(model, params(oracle, sp, nof.to_numpy(pptr, (P,))))
    r = synth.blender_rays(n, seed=23)
    grads = _run(model, r, gpu)
    torch.cuda.synchronize()
    assert len(grads) == len(sizes)
    assert model.numeric_status() == 0
    lv = [model.level_numpy(l) for l in range(len(samples))]
    params = nof.to_numpy(pptr, (P,))
    assert installed is None or same_bits(params, installed), "the step changed the installed parameters"
    G = nof.to_numpy(model.mlp.flat_grads()[0], (P,))

    t0 = oracle.sample_stratified(r["near"], r["far"], samples[0], True, seed, step, 0, ray_base)
    assert np.array_equal(lv[0]["t"], t0)
    tov = {}
    for l in range(1, len(samples)):  # later levels: bit-exact given the GPU's weights
        tl, _ = oracle.sample_pdf(lv[l - 1]["t"], lv[l - 1]["weights"], samples[l], 0.01, True, seed, step, l, ray_base)
        assert np.array_equal(lv[l]["t"], tl)
        tov[l] = lv[l]["t"]
    masks = {l: model.mlp.relu_masks(l).reshape(n, samples[l], -1) for l in range(len(samples))}
    kw = dict(samples=samples, seed=seed, step_idx=step, ray_base=ray_base, t_override=tov, nthreads=16)
    ref = oracle.step(sp, params, r, relu_mask=masks, want=("grads",), **kw)
    free = oracle.step(sp, params, r, want=("sigma", "rgb", "w", "C", "dsigma", "drgb"), **kw)
    oerrs = []
    for l in range(len(samples)):
        for key, fk in (("density", "sigma"), ("rgb", "rgb"), ("weights", "w"), ("comp_rgb", "C"),
                        ("density_grad", "dsigma"), ("rgb_grad", "drgb")):
            oerrs.append(rel_l2(lv[l][key], free[fk][l]))
            assert oerrs[-1] < TOL, f"{key} level {l}: rel L2 {oerrs[-1]:.3g}"
    errs = [rel_l2(a, b) for a, b in zip(np.split(G, np.cumsum(sizes)[:-1]),
                                         np.split(ref["grads"], np.cumsum(sizes)[:-1]))]
    print(f"f16p {name} {spec} {n} x {samples}: gradient rel L2 worst {max(errs):.2e} (tensor {int(np.argmax(errs))}) "
          f"median {np.median(errs):.2e}; outputs worst {max(oerrs):.2e}")
    for i, e in enumerate(errs):
        assert e < TOL, f"gradient tensor {i} (size {sizes[i]}): rel L2 {e:.3g}"
    assert abs(model.loss() - free["loss"]) <= TOL * abs(free["loss"])
    _assert_dispatch(model, name, len(samples))
    model.close()


@pytest.mark.parametrize("name", ["wide_3x272_2x136", "unaligned_2x50_1x30", "odd_5x96_3x40", "tiny_2x32_skip1",
                                  "configs0_4x128"])
def test_f16p_step_parity(gpu, oracle, name):
    _check(gpu, oracle, name, 4, (64, 64))


@pytest.mark.parametrize("name", ["wide_3x272_2x136", "odd_5x96_3x40"])
def test_f16p_step_parity_split_k(gpu, oracle, name):
    """8 rays x (64, 128): k = 512 and 1024 samples, longer split-K chunks."""
    _check(gpu, oracle, name, 8, (64, 128))


def test_f16p_step_parity_reference_net(gpu, oracle):
    """The reference's 8x256 network runs on the any-shape path in mode 5 (generic_ by the mode)."""
    _check(gpu, oracle, "reference_8x256", 2, (64, 64))


def test_dispatch_h_table_reaches_every_variant():
    import nof

    names = nof.gen_dispatch_h_names()
    reached = set().union(*DISPATCH_H.values())
    assert reached <= set(names), sorted(reached - set(names))
    assert set(names) - reached == set(UNREACHED_H), sorted(set(names) - reached)


def _arena(gpu, name, precision, n, samples, msum=None, seed=4):
    import torch
    import nof
    from nof import synth

    r = synth.blender_rays(n, seed=3)
    m = nof.AcceleratedMipNeRF(seed=seed, max_rays=n, num_samples=samples, precision=precision, **_cfg(_spec(name)))
    m.set_rng(9, 1, 0)
    _run(m, r, gpu, msum)
    torch.cuda.synchronize()
    gp, P = m.mlp.flat_grads()
    g = nof.to_numpy(gp, (P,)).copy()
    tally = m.mlp.gen_dispatch_h()
    m.close()
    return g, tally


def test_f16p_is_not_fp32_and_deterministic(gpu):
    """Two mode-5 runs give identical bits; the mode-5 gradient is more than 1e-5 from the same model's mode-0
    gradient (the fp16 kernel ran, not the fp32 one), whose own run leaves the fp16 tally at zero."""
    a, ta = _arena(gpu, "odd_5x96_3x40", 5, 16, (64, 128))
    b, _ = _arena(gpu, "odd_5x96_3x40", 5, 16, (64, 128))
    f, tf = _arena(gpu, "odd_5x96_3x40", 0, 16, (64, 128))
    assert np.array_equal(a, b)
    assert np.all(np.isfinite(a)) and any(ta.values()) and not any(tf.values())
    d = rel_l2(a, f)
    print(f"f16p vs f32 gradient arena: rel L2 {d:.2e}")
    assert d > 1e-5


def test_f16p_power_of_two_loss_scale_is_exact(gpu):
    """loss_mult_sum times 2^12: every output gradient and delta is exactly 2^-12 times smaller, the level's amax
    with them, so s grows by 2^12, the fp16 images are the same bits and the gradient arena times 2^12 equals the
    first run's bitwise.  Without the scale the head deltas (about 1e-9 and below) would vanish in fp16."""
    from nof import synth

    n, samples = 16, (64, 128)
    msum = float(np.sum(synth.blender_rays(n, seed=3)["lossmult"], dtype=np.float32))
    a, _ = _arena(gpu, "odd_5x96_3x40", 5, n, samples, msum)
    b, _ = _arena(gpu, "odd_5x96_3x40", 5, n, samples, msum * 4096.0)
    assert np.any(a != 0)
    assert np.array_equal(a, b * np.float32(4096.0))


def test_f16p_render_equals_training_forward(gpu):
    """render_device equals the training step's forward bitwise on the same Philox state (both run gen_forward
    on k_gemm_h)."""
    import torch
    import nof
    from nof import synth

    n, samples = 24, (64, 128)
    r = synth.blender_rays(n, seed=31)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in r.items()}
    m = nof.AcceleratedMipNeRF(seed=2, max_rays=n, num_samples=samples, precision=5, **_cfg(SPECS["unaligned_2x50_1x30"]))
    m.set_rng(0xABC, 4, 100)
    lv = m.render_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], randomized=True)
    torch.cuda.synchronize()
    out = [nof.to_numpy(*L["comp_rgb"]) for L in lv]
    m.set_rng(0xABC, 4, 100)
    _run(m, r, gpu)
    torch.cuda.synchronize()
    for l in range(2):
        assert np.array_equal(m.level_numpy(l)["comp_rgb"], out[l]), f"level {l}"
    m.close()


def test_f16p_adam_training_lowers_loss(gpu):
    """Ten Adam steps on configs[0]'s 4x128 network in mode 5 lower the loss."""
    import torch
    import nof
    from nof import synth

    n = 256
    r = synth.blender_rays(n, seed=8)
    m = nof.AcceleratedMipNeRF(seed=1, max_rays=n, num_samples=(64, 64), precision=5, **_cfg(SPECS["configs0_4x128"]))
    adam = nof.AcceleratedAdamOptimizer(m.GetLayerSizes(), m.config)
    losses = []
    for s in range(10):
        m.set_rng(5, s, 0)
        g = _run(m, r, gpu)
        losses.append(m.loss())
        adam.step(m.mlp.allParams, g, 5e-3)
    torch.cuda.synchronize()
    print(f"f16p losses {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert np.all(np.isfinite(losses)) and m.numeric_status() == 0
    assert losses[-1] < losses[0], losses
    adam.close()
    m.close()


def test_f16p_mode_boundary(gpu):
    """Modes 1-4 with a non-reference shape still return NOF_ERR_UNSUPPORTED; mode 5 is accepted for a
    non-reference shape and for the reference net (which then runs on the any-shape path: debug_view says so)."""
    import nof

    small = _cfg(SPECS["tiny_2x32_skip1"])
    for p in (1, 2, 3, 4):
        cfg = nof.default_config(max_rays=4, num_samples=(64, 64), precision=p, **small)
        h = C.c_void_p()
        assert nof.lib().nof_mipnerf_create(C.byref(cfg), C.byref(h)) == 5, p
    for net in (small, {}):
        m = nof.AcceleratedMipNeRF(seed=1, max_rays=4, num_samples=(64, 64), precision=5, **net)
        assert m.config.precision == 5 and m.mlp.debug_view(0)["generic"] == 1
        m.close()


def test_f16p_native_and_python_drivers(gpu, tmp_path):
    """--precision f16p through both training drivers on a non-reference network (bin/nof_train on the C ABI
    alone, `python -m nof.train`): both run, and the native driver's parameter dump is the finite 4x128 arena."""
    import os
    import subprocess
    import sys

    from nof import synth

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "nerf-or-nothing_amd", "bin", "nof_train")
    path = str(tmp_path / "rays.bin")
    synth.pack_records(synth.blender_rays(2048, seed=4)).tofile(path)
    dump = str(tmp_path / "params.bin")
    net = ["--net-depth", "4", "--net-width", "128", "--precision", "f16p", "--batch", "256", "--steps", "3",
           "--print-every", "1", "--records", path]
    p = subprocess.run([exe, *net, "--samples", "64,64", "--seed", "77", "--dump-params", dump], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    P = np.fromfile(dump, np.float32)
    D, W, pos, dirs = 4, 128, 96, 27
    assert P.size == pos * W + (D - 1) * W * W + W + 128 * (W + dirs) + 3 * 128 + (D * W + 1 + 128 + 3)
    assert np.all(np.isfinite(P))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "nerf-or-nothing_amd"))
    q = subprocess.run([sys.executable, "-m", "nof.train", *net, "--samples", "64", "64"], capture_output=True,
                       text=True, timeout=300, env=env)
    assert q.returncode == 0, q.stderr[-2000:]
    assert "rays/s" in q.stdout
