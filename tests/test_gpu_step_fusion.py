"""The fused 8x256 step's launch fusions against the unfused launches, bit for bit.

AcceleratedMipNeRF.set_step_fusion switches each fusion off inside one build; a fusion may change how the work is
launched, never a result, so every comparison here is np.array_equal.

Shapes.  The fused path accepts 64 / 128 / 256 / 512 samples per level (32 is refused at construction), so a level
has 2 n S / 64 blocks of 32 samples, always an even count, and a k_mlp_bwd16 workgroup (4 blocks) is either full or
has its second wave quartet clamped onto the level's last block.  The shapes are the smallest with every such edge:
  1 ray  x (64, 64):   2 + 2 blocks: each level one half-clamped workgroup, the level boundary after workgroup 0
  3 rays x (64, 128):  6 + 12 blocks: level 0's second workgroup half clamped right before the level boundary
  3 rays x (64, 64):   6 + 6 blocks: a half-clamped workgroup on both sides of the boundary
  5 rays x (128, 128): 20 + 20 blocks: full workgroups only, equal levels
  4 rays x (64, 128):  8 + 16 blocks: full workgroups only, unequal levels
and 3 rays x (64, 128) in a model created for 8 rays (the buffers' capacity is not the call's size).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = [0, 2, 3]  # NOF_PRECISION_F32, _F16X2, _F32_F16SPLIT: the modes of k_mlp_fwd16 / k_mlp_bwd16
SHAPES = [(1, (64, 64), 1), (3, (64, 128), 3), (3, (64, 64), 3), (5, (128, 128), 5), (4, (64, 128), 4),
          (3, (64, 128), 8)]  # (rays, samples, max_rays)
LEVEL_KEYS = ("t", "weights", "comp_rgb", "density", "rgb", "density_grad", "rgb_grad")


def _rays(n, seed=21):
    from nof import synth

    return synth.blender_rays(n, seed=seed)


def _step(model, r, dev, fusion):
    """one get_gradient_device step at the given fusion flags -> {name: array}"""
    import torch
    import nof

    n = r["o"].shape[0]
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in r.items()}
    model.set_step_fusion(fusion)
    model.set_rng(0xF00D, 4, 100)
    model.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"],
                              float(np.sum(r["lossmult"], dtype=np.float32)))
    torch.cuda.synchronize()
    gptr, P = model.mlp.flat_grads()
    out = {"flat_grads": nof.to_numpy(gptr, (P,)).copy(), "loss": np.float32(model.loss())}
    for l in range(2):
        for k, v in model.level_numpy(l).items():
            assert k in LEVEL_KEYS
            out[f"{k}{l}"] = v.copy()
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"
    assert np.all(np.isfinite(a["flat_grads"])) and np.any(a["flat_grads"] != 0.0)


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("n,samples,max_rays", SHAPES)
def test_pair_launch_equals_two_launches(gpu, n, samples, max_rays, precision):
    """One k_mlp_bwd16 launch for both levels == one launch per level."""
    import nof

    r = _rays(n)
    model = nof.AcceleratedMipNeRF(seed=31, max_rays=max_rays, num_samples=samples, precision=precision)
    on = _step(model, r, gpu, nof.STEP_FUSION_ALL)
    off = _step(model, r, gpu, nof.STEP_FUSION_ALL & ~nof.STEP_FUSION_BWD_PAIR)
    again = _step(model, r, gpu, nof.STEP_FUSION_ALL)
    model.close()
    _assert_same(on, off, "pair launch vs per-level launches")
    _assert_same(on, again, "pair launch after per-level launches")


def _render(model, r, dev):
    import torch
    import nof

    n = r["o"].shape[0]
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in r.items()}
    out = model.render_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"])
    torch.cuda.synchronize()
    return {f"render_{k}{l}": nof.to_numpy(*lv[k]).copy() for l, lv in enumerate(out) for k in lv}


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("n,samples,max_rays", SHAPES)
def test_view_tables_equal_in_kernel_view_work(gpu, n, samples, max_rays, precision):
    """The pack launch's per-ray view-PE rows and view biases, read by k_mlp_fwd16 == every wave computing them;
    render_device (which always computes them in the kernel) is the same at both settings."""
    import nof

    r = _rays(n)
    model = nof.AcceleratedMipNeRF(seed=31, max_rays=max_rays, num_samples=samples, precision=precision)
    on = _step(model, r, gpu, nof.STEP_FUSION_ALL)
    on.update(_render(model, r, gpu))
    off = _step(model, r, gpu, nof.STEP_FUSION_ALL & ~nof.STEP_FUSION_VIEW_TABLES)
    off.update(_render(model, r, gpu))
    none = _step(model, r, gpu, 0)
    none.update(_render(model, r, gpu))
    model.close()
    _assert_same(on, off, "view tables vs in-kernel view work")
    _assert_same(on, none, "every fusion vs none")


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("kind", ["zero_component", "non_unit"])
def test_view_tables_odd_directions(gpu, kind, precision):
    """Directions with a zero component (sin 0, cos 0 and a -0.0 among the PE values) and far from unit length
    (arguments of the PE up to 2^3 |d|): the tables hold the kernel's own values."""
    import nof

    n = 3
    r = {k: v.copy() for k, v in _rays(n).items()}
    if kind == "zero_component":
        r["d"][0, 1] = 0.0
        r["d"][1, 0] = -0.0
        r["d"][2, 2] = 0.0
    else:
        r["d"] *= np.array([[3.5], [0.125], [17.0]], np.float32)
    model = nof.AcceleratedMipNeRF(seed=31, max_rays=n, num_samples=(64, 128), precision=precision)
    on = _step(model, r, gpu, nof.STEP_FUSION_ALL)
    off = _step(model, r, gpu, 0)
    model.close()
    _assert_same(on, off, f"{kind}: view tables vs in-kernel view work")


@pytest.mark.parametrize("precision", MODES)
def test_api_paths_unchanged(gpu, precision):
    """The API paths at 3 rays x (64, 128), every fusion on against every fusion off: the callback entry
    (GetGradient), AcceleratedMLP.get_gradient level by level (always a single-level backward launch) and
    AcceleratedMLP.get_output on encoded inputs."""
    import torch
    import nof

    n, samples = 3, (64, 128)
    r = _rays(n)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in r.items()}
    res = []
    for fusion in (nof.STEP_FUSION_ALL, 0):
        model = nof.AcceleratedMipNeRF(seed=31, max_rays=n, num_samples=samples, precision=precision)
        model.set_step_fusion(fusion)
        model.set_rng(0xF00D, 4, 100)
        gc = nof.AcceleratedGradientCalculator(n, model.config)
        model.GetGradient(r["o"], r["d"], r["radius"], r["near"], r["far"], r["lossmult"],
                          lambda comp, level, msum, lm: gc.get_output_gradient(comp, r["pix"], lm, msum, level))
        torch.cuda.synchronize()
        gptr, P = model.mlp.flat_grads()
        out = {"cb_grads": nof.to_numpy(gptr, (P,)).copy()}
        views = [model.level_view(l) for l in range(2)]
        for l in range(2):
            for k, (p, shp) in views[l].items():
                out[f"cb_{k}{l}"] = nof.to_numpy(p, shp).copy()
        for l in range(2):  # per-level calls on the step's own output gradients
            model.mlp.get_gradient(views[l]["rgb_grad"][0], views[l]["density_grad"][0], l)
        torch.cuda.synchronize()
        out["level_grads"] = nof.to_numpy(gptr, (P,)).copy()
        # encoded inputs: level 0's samples through the stand-alone cast and encode kernels
        S = samples[0]
        t = torch.from_numpy(out["cb_t0"]).to(gpu)
        mean = torch.zeros((n, S, 3), device=gpu)
        cov = torch.zeros((n, S, 3), device=gpu)
        nof._lib.call("nof_kernel_cast", n, S, t.data_ptr(), dev["o"].data_ptr(), dev["d"].data_ptr(),
                      dev["radius"].data_ptr(), mean.data_ptr(), cov.data_ptr(), None)
        ep = torch.zeros((n * S, 96), device=gpu)
        ed = torch.zeros((n, 27), device=gpu)
        nof._lib.call("nof_kernel_encode", n, S, mean.data_ptr(), cov.data_ptr(), dev["d"].data_ptr(), ep.data_ptr(),
                      ed.data_ptr(), None)
        dptr, rptr = model.mlp.get_output(ep, ed, 0, n, S)
        torch.cuda.synchronize()
        out["enc_density"] = nof.to_numpy(dptr, (n, S)).copy()
        out["enc_rgb"] = nof.to_numpy(rptr, (n, S, 3)).copy()
        assert np.array_equal(out["enc_density"], out["cb_density0"])  # the encoded path == the fused prologue
        gc.close()
        model.close()
        res.append(out)
    assert res[0].keys() == res[1].keys()
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k], equal_nan=True), f"{k} differs"
    assert np.any(res[0]["cb_grads"] != 0.0) and np.any(res[0]["level_grads"] != 0.0)


@pytest.mark.parametrize("precision", MODES)
def test_fused_step_deterministic(gpu, precision):
    """5 rays x (128, 128) twice with every fusion on, in two models: all arrays equal."""
    import nof

    r = _rays(5)
    outs = []
    for _ in range(2):
        model = nof.AcceleratedMipNeRF(seed=31, max_rays=5, num_samples=(128, 128), precision=precision)
        outs.append(_step(model, r, gpu, nof.STEP_FUSION_ALL))
        model.close()
    _assert_same(outs[0], outs[1], "two runs")


def test_unknown_fusion_bits_refused(gpu):
    import nof

    model = nof.AcceleratedMipNeRF(seed=1, max_rays=1, num_samples=(64, 64))
    with pytest.raises(nof.NofError):
        model.set_step_fusion(1 << 30)
    model.close()
