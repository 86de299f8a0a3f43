"""The fp32 weight-gradient kernel's ring of 16-sample stages at the smallest shapes where it can go wrong.

`k_wgrad` (wgrad.hip) streams every operand block as two 16-sample stages through a four-slot LDS ring:
the DMA runs three stages ahead behind counted waits, fragments are read across the stage barrier, and
the ring is drained between the items of a workgroup.  A level takes 64, 128, 256 or 512 samples per ray
(nof_mipnerf_create), i.e. at least two 32-sample blocks per ray, and the host cuts the (problem, block)
sequence of a step into one piece per workgroup of the 256 at cumulative-cost marks; the cases are the
smallest supported shapes with the item shapes wanted:

  * one ray x 64+64 samples: two blocks per problem and level, some 50 blocks for 256 workgroups, so
    the marks are closer than one block of any wide problem and its items are single blocks = two
    stages: the prologue (three stages staged, one of them a clamped duplicate), the steady state and
    the drain coincide;
  * twelve rays x 64+128 samples: 24 and 48 blocks per problem, the levels differ in block count, and a
    workgroup's share is about 2.4 blocks of a 256 x 256 problem: its items are 2 or 3 blocks (an odd
    count leaves the two-block loop through its tail, so items end on both slot parities) and the
    narrow problems' items are longer;
  * three rays x 64+128 samples with grad_buckets set: the bucket-aligned cut gives every workgroup a
    piece of every bucket, many short items each, so the ring is reused across items again and again.

Each case holds all 22 gradient tensors to the fp32 bound of the step parity tests (1e-5 relative L2
per tensor against the fp64 oracle, which adopts the GPU's ReLU decisions as there), and two runs of
the same step to bitwise-equal gradients.
"""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5  # fp32 per-tensor bound (test_gpu_step.TOLS[0])

CASES = [(1, (64, 64), 0), (12, (64, 128), 0), (3, (64, 128), 1)]


def _step(gpu, n, samples, grad_buckets, r, seed, step, ray_base):
    import torch
    import nof

    model = nof.AcceleratedMipNeRF(seed=seed, max_rays=n, num_samples=samples, precision=0,
                                   grad_buckets=grad_buckets)
    model.set_rng(seed, step, ray_base)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in r.items()}
    msum = float(np.sum(r["lossmult"], dtype=np.float32))
    model.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"], d["pix"], msum)
    torch.cuda.synchronize()
    return model


@pytest.mark.parametrize("n,samples,grad_buckets", CASES)
def test_stage_ring_gradients(gpu, oracle, n, samples, grad_buckets):
    import nof
    from nof import synth

    seed, step, ray_base = 0x1234, 3, 500
    r = synth.blender_rays(n, seed=11)
    G = []
    for _ in range(2):
        model = _step(gpu, n, samples, grad_buckets, r, seed, step, ray_base)
        gptr, P = model.mlp.flat_grads()
        G.append(nof.to_numpy(gptr, (P,)).copy())
        if len(G) < 2:
            model.close()
    assert np.array_equal(G[0], G[1]), "two runs of the same step differ"

    t1 = model.level_numpy(1)["t"]
    params = nof.to_numpy(model.mlp.flat_params()[0], (P,))
    masks = {l: model.mlp.relu_masks(l).reshape(n, samples[l], -1) for l in range(2)}
    ref = oracle.step(oracle.Spec(), params, r, samples=samples, seed=seed, step_idx=step, ray_base=ray_base,
                      t_override={1: t1}, relu_mask=masks, nthreads=16, want=("grads",))
    model.close()
    sizes = oracle.layer_sizes(oracle.Spec())
    assert len(sizes) == 22 and sum(sizes) == P
    off, errs = 0, []
    for s in sizes:
        errs.append(rel_l2(G[0][off:off + s], ref["grads"][off:off + s]))
        off += s
    print(f"{n} x {samples} buckets {grad_buckets}: gradient rel L2 max {max(errs):.2e} median {np.median(errs):.2e}")
    for i, e in enumerate(errs):
        assert e < TOL, f"gradient tensor {i}: rel L2 {e:.3g}"
