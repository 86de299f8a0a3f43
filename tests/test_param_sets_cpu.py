"""The biased parameter set (tests/param_sets.py) can see a wrong bias index: on the fp64 oracle alone, shifting
any one bias tensor by one place, or by four, moves a forward output by at least 1e-2 — five times the loosest
forward bound of any precision mode (2e-3).  This is a condition on the inputs of tests/test_gpu_biased_params.py,
not a measurement of any kernel: a forward kernel that reads a bias one element, one 4-float lane group or one
table row off computes what the oracle computes for the shifted tensor, so it is that far out of bound.

Measured (smallest change over the bias tensors and both shifts; level-1 sigma, rgb ranges of the unshifted set):
  reference 8x256     1.44e-2 (b0, roll 1)   sigma [0.265, 0.369]  rgb [0.320, 0.709]
  configs0_4x128      5.36e-2 (b2, roll 1)   sigma [0.254, 0.412]  rgb [0.277, 0.661]
  odd_5x96_3x40       3.36e-2 (b6, roll 4)   sigma [0.247, 0.959]  rgb [0.368, 0.701]
  wide_3x272_2x136    4.51e-2 (b5, roll 1)   sigma [0.131, 0.346]  rgb [0.244, 0.579]
  unaligned_2x50_1x30 4.98e-2 (b3, roll 1)   sigma [0.165, 0.606]  rgb [0.309, 0.748]
so nothing saturates: softplus and the sigmoid are both on their steep parts.
"""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from param_sets import AMP, bias_slices, biased
from test_gpu_generic import SPECS, _ospec

MIN_CHANGE = 1e-2   # 5 x the loosest forward bound (2e-3: modes 2, 4 and 5)
NETS = ["reference_8x256", "configs0_4x128", "odd_5x96_3x40", "wide_3x272_2x136", "unaligned_2x50_1x30"]
N, SAMPLES, SEED, STEP, RAY_BASE = 4, (64, 64), 0x77, 2, 40


def _sp(oracle, name):
    return oracle.Spec() if name == "reference_8x256" else _ospec(oracle, SPECS[name])


@functools.lru_cache(maxsize=None)
def _rays():
    from nof import synth

    return synth.blender_rays(N, seed=23)


def _forward(oracle, sp, P):
    out = oracle.step(sp, P, _rays(), samples=SAMPLES, seed=SEED, step_idx=STEP, ray_base=RAY_BASE, nthreads=16,
                      want=("sigma", "rgb"))
    return out["sigma"], out["rgb"]


def test_biased_touches_the_biases_only(oracle):
    for name in NETS:
        sp = _sp(oracle, name)
        sizes = oracle.layer_sizes(sp)
        P0 = oracle.glorot_init(sp, SEED)
        sls = bias_slices(sizes)
        assert sls[-1].stop == P0.size and [s.stop - s.start for s in sls] == [int(x) for x in sizes[len(sls):]]
        assert not np.any(np.concatenate([P0[s] for s in sls])), "the Glorot draw's biases are 0 (SURVEY D6)"
        P = biased(P0, sizes)
        assert P.dtype == np.float32 and P is not P0
        assert np.array_equal(P[:sls[0].start], P0[:sls[0].start])  # the weights, bitwise
        b = P[sls[0].start:]
        assert np.all(np.abs(b) <= AMP) and np.all(b != 0) and np.abs(b).mean() > AMP / 4
        # one generator, arena order
        want = np.random.default_rng(1).uniform(-AMP, AMP, sls[0].stop - sls[0].start).astype(np.float32)
        assert np.array_equal(P[sls[0]], want)
        assert np.array_equal(biased(P0, sizes), P) and not np.array_equal(biased(P0, sizes, seed=2), P)


@pytest.mark.parametrize("name", NETS)
def test_bias_shift_moves_the_forward(oracle, name):
    sp = _sp(oracle, name)
    sizes = oracle.layer_sizes(sp)
    P = biased(oracle.glorot_init(sp, SEED), sizes)
    sigma, rgb = _forward(oracle, sp, P)
    for l in range(len(SAMPLES)):  # nothing saturates: softplus and sigmoid both away from their flat ends
        assert np.all(np.isfinite(sigma[l])) and np.all(np.isfinite(rgb[l]))
        assert 0.05 < sigma[l].min() and sigma[l].max() < 2.0, (sigma[l].min(), sigma[l].max())
        assert 0.1 < rgb[l].min() and rgb[l].max() < 0.9, (rgb[l].min(), rgb[l].max())
    print(f"{name}: level-1 sigma in [{sigma[1].min():.3f}, {sigma[1].max():.3f}], rgb in "
          f"[{rgb[1].min():.3f}, {rgb[1].max():.3f}]")
    worst = (np.inf, None)
    for i, sl in enumerate(bias_slices(sizes)):
        size = sl.stop - sl.start
        for shift in (1, 4):
            Q = P.copy()
            Q[sl] = np.roll(P[sl], shift) if size > 1 else 0.0
            assert not np.array_equal(Q, P)
            s2, c2 = _forward(oracle, sp, Q)
            change = max(max(rel_l2(s2[l], sigma[l]), rel_l2(c2[l], rgb[l])) for l in range(len(SAMPLES)))
            worst = min(worst, (change, f"b{i} roll {shift}"))
            assert change >= MIN_CHANGE, f"{name} b{i} (size {size}) shifted by {shift}: the forward moves {change:.3g}"
            if size == 1:
                break
    print(f"{name}: smallest forward change of a shifted bias tensor {worst[0]:.3g} ({worst[1]})")
