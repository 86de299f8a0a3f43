"""Parameter sets away from the fresh Glorot draw, for the tests that compare a step with the fp64 oracle.

A fresh model's biases are all 0 (glorot_init), and at 0 a forward kernel that reads a bias through a
wrong index, lane group or table offset still gives the right answer.  biased() fills every bias tensor with
values of moderate size; tests/test_param_sets_cpu.py shows on the oracle alone that shifting any one of them by
one or four places then moves the forward outputs by at least 1e-2, five times the loosest forward bound.
"""
import numpy as np

AMP = 0.25  # fixed by test_param_sets_cpu.py's condition; not a knob for making a GPU test pass


def bias_slices(sizes):
    """The bias tensors' slices of the arena [W0..W(L-1), b0..b(L-1)] (oracle.layer_sizes' order)."""
    sizes = [int(s) for s in sizes]
    L = len(sizes) // 2
    assert len(sizes) == 2 * L
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [slice(int(off[i]), int(off[i + 1])) for i in range(L, 2 * L)]


def biased(P, sizes, amp=AMP, seed=1):
    """A copy of the Glorot arena P whose bias tensors are uniform(-amp, amp), drawn in arena order from one
    default_rng(seed); the weights stay untouched."""
    P = np.array(P, dtype=np.float32, copy=True)
    assert P.ndim == 1 and P.size == int(np.sum(sizes))
    rng = np.random.default_rng(seed)
    for sl in bias_slices(sizes):
        P[sl] = rng.uniform(-amp, amp, sl.stop - sl.start).astype(np.float32)
    return P


def biased_for(oracle, spec, P):
    """biased() in the form the step checkers' `params` argument takes: (oracle, oracle.Spec, Glorot arena)."""
    return biased(P, oracle.layer_sizes(spec))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def install(model, P):
    """Overwrite the model's parameter arena with P.  Before the step: the weight image is packed at the start
    of every step (AcceleratedMLP::pack_weights)."""
    import torch
    import nof

    P = np.ascontiguousarray(P, dtype=np.float32)
    ptr, cnt = model.mlp.flat_params()
    assert P.shape == (cnt,)
    nof.device_tensor(ptr, (cnt,)).copy_(torch.from_numpy(P))
    torch.cuda.synchronize()
    return P
