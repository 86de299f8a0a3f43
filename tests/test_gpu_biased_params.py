"""GPU step parity with non-zero biases on every MLP forward path.

Every other comparison with the fp64 oracle runs on the parameters a fresh model draws, whose biases are all 0
(glorot_init).  The bias gradients do not depend on the bias values, so wherever a forward kernel READS
a bias — the LDS copy of the packed image's tail and fwd_epilogue's `bias + 4*h` (mlp_fwd.hip), the C operand of
each tile's first MFMA and the step's view_bias table (mlp_fwd16.hip / mlp16.h), cinit_load and the kDirb operands
(mlp_f16.hip / mlp_h32.h), the any-shape path's tile epilogue (gemm_tile.h, under k_gemm, k_gemm_ws and k_gemm_h),
the three pack kernels' bias tails — a wrong index gives the right answer at 0.  Here the existing step checkers run
unchanged (same rays, shapes, bounds, ReLU adoption and dispatch tables) on param_sets.biased: the model's Glorot
weights with every bias uniform in (-0.25, 0.25).  tests/test_param_sets_cpu.py shows that a bias tensor read one
or four places off moves a forward output by at least 1e-2, against bounds of at most 2e-3.

Measured on an MI355X: see MEASURED below (filled from the printed figures of a run).
"""
import numpy as np
import pytest

import test_gpu_generic as GEN
import test_gpu_generic_f16p as F16P
import test_gpu_step as STEP
from param_sets import biased_for, install

pytestmark = pytest.mark.gpu

MEASURED = """
every case passes: no bias read was found wrong.  Gradient tensors, rel L2 worst / median (the checkers' prints):
fused 8x256, 6 rays x (64, 128), bounds 1e-5 / 1e-5 / 2e-3 / 1e-5 / 2e-3:
  mode 0 6.9e-7 / 3.5e-7, mode 1 7.3e-7 / 4.0e-7, mode 2 1.2e-4 / 2.8e-5, mode 3 1.0e-6 / 5.7e-7, mode 4 6.3e-4 / 3.8e-4
any-shape fp32, bound 1e-5:
  configs0_4x128 4.8e-7 / 3.5e-7, odd_5x96_3x40 7.4e-7 / 3.5e-7 (8 x (64, 128));
  wide_3x272_2x136 3.5e-7 / 2.6e-7, unaligned_2x50_1x30 3.3e-7 / 2.5e-7 (4 x (64, 64))
fp16 products, bound 2e-3 (and the worst output or adjoint):
  wide_3x272_2x136 4.3e-4 / 3.0e-4, 1.4e-4;  reference 8x256, 2 rays x (64, 64): 6.5e-4 / 3.7e-4, 3.4e-4
encoded API: density and rgb bitwise equal
"""


@pytest.mark.parametrize("precision", STEP.PRECISIONS)
def test_biased_step_parity_fused(gpu, oracle, precision):
    """The fused 8x256 kernels, every precision mode, held to test_gpu_step.TOLS."""
    STEP._check_step(gpu, oracle, "blender", 6, (64, 128), precision, params=biased_for)


@pytest.mark.parametrize("name,n,samples", [("configs0_4x128", 8, (64, 128)), ("odd_5x96_3x40", 8, (64, 128)),
                                            ("wide_3x272_2x136", 4, (64, 64)), ("unaligned_2x50_1x30", 4, (64, 64))])
def test_biased_step_parity_generic(gpu, oracle, name, n, samples):
    """The any-shape fp32 path at the shapes of these specs' existing cases (so their DISPATCH entries hold):
    k_gemm_ws's static and runtime shapes, k_gemm above 128 columns, and the scalar stores of widths 50 / 30."""
    GEN._check(gpu, oracle, name, "blender", n, samples, params=biased_for)


@pytest.mark.parametrize("name,n,samples", [("wide_3x272_2x136", 4, (64, 64)), ("reference_8x256", 2, (64, 64))])
def test_biased_step_parity_f16p(gpu, oracle, name, n, samples):
    """fp16 products (mode 5, k_gemm_h): test_f16p_step_parity's first spec and the reference network."""
    F16P._check(gpu, oracle, name, n, samples, params=biased_for)


def test_biased_encoded_get_output_equals_fused(gpu, oracle):
    """test_gpu_step.test_encoded_get_output_equals_fused with biased parameters: get_output on the cast and encode
    kernels (the forward's own view-bias prologue) == the fused forward (the step's view_bias table), bitwise."""
    import torch
    import nof
    from nof import synth

    n, S = 8, 128
    r = synth.blender_rays(n, seed=9)
    model = nof.AcceleratedMipNeRF(seed=3, max_rays=n)
    pptr, P = model.mlp.flat_params()
    installed = install(model, biased_for(oracle, oracle.Spec(), nof.to_numpy(pptr, (P,))))
    STEP._run_gpu(model, r, gpu)
    torch.cuda.synchronize()
    v0 = model.level_numpy(0)
    dev = STEP._device_rays(r, gpu)
    t = torch.from_numpy(v0["t"]).to(gpu)
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
    assert np.array_equal(nof.to_numpy(pptr, (P,)).view(np.uint32), installed.view(np.uint32))
    assert np.array_equal(nof.to_numpy(dptr, (n, S)), v0["density"])
    assert np.array_equal(nof.to_numpy(rptr, (n, S, 3)), v0["rgb"])
    model.close()
