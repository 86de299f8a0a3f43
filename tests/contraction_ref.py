"""References of the scene contraction (nof_mipnerf_set_contraction; csrc/kernels/contract.h).

TEST INFRASTRUCTURE, not a test.
  contract32  fp32 numpy, the kernel's operation order restated: what k_cast_contract must store, bit for bit
  naive32     fp32 numpy, the expansion a^2 v_i + 2 a c q_i v_i + c^2 q_i sum_k q_k v_k that cancels (shown to break
              the bound in tests/test_contraction_cpu.py, so a test cannot pass on it)
  contract    fp64 torch, differentiable; snap=True: the values are contract32's of the fp32 inputs, the derivative
              fp64's (crosslevel_ref._snap), so derivatives are taken at the points the GPU works at
  step        the whole-step fp64 autograd reference: raygrad_ref.step with that module's cast wrapped (cast, then
              contract) for the duration of the call; also returns dL/dt of every level above 0 that has one
"""
from __future__ import annotations

import numpy as np
import torch

import crosslevel_ref as X
import raygrad_ref as G

f32 = np.float32


def contract32(m, v):
    """m, v [..., 3] fp32 -> (m', v') fp32, every operation rounded to fp32 in contract.h's order"""
    m, v = np.asarray(m, f32), np.asarray(v, f32)
    m0, m1, m2 = m[..., 0], m[..., 1], m[..., 2]
    with np.errstate(all="ignore"):
        n2 = (m0 * m0 + m1 * m1) + m2 * m2
        out = n2 > f32(1)  # False for NaN: the pass-through
        n = np.sqrt(np.where(out, n2, f32(4)))  # (inside the ball: any value, the result is discarded)
        inv = f32(1) / n
        b = inv * inv
        a = (f32(2) * n - f32(1)) * b
        c = f32(-2) * (n - f32(1)) * b
        u = [m0 * inv, m1 * inv, m2 * inv]
        q = [x * x for x in u]
        ms = f32(2) - inv
        cc = c * c
        mo, vo = [], []
        for i in range(3):
            i1, i2 = (i + 1) % 3, (i + 2) % 3
            D = a * (q[i1] + q[i2]) + b * q[i]
            mo.append(ms * u[i])
            vo.append((D * D) * v[..., i] + (cc * q[i]) * (q[i1] * v[..., i1] + q[i2] * v[..., i2]))
    mo, vo = np.stack(mo, -1).astype(f32), np.stack(vo, -1).astype(f32)
    return np.where(out[..., None], mo, m), np.where(out[..., None], vo, v)


def naive32(m, v):
    """the cancelling expansion of v' in fp32 (outside the ball only)"""
    m, v = np.asarray(m, f32), np.asarray(v, f32)
    n = np.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
    inv = f32(1) / n
    b = inv * inv
    a = (f32(2) * n - f32(1)) * b
    c = b - a
    u = m * inv[..., None]
    q = u * u
    s = (q[..., 0] * v[..., 0] + q[..., 1] * v[..., 1]) + q[..., 2] * v[..., 2]
    return ((a * a)[..., None] * v + (f32(2) * a * c)[..., None] * q * v + (c * c)[..., None] * q * s[..., None]).astype(f32)


def contract(m, v, snap=False):
    """m, v [..., 3] torch fp64 -> (m', v'), differentiable; the branch is the fp32 forward's with snap, fp64's without"""
    n2 = (m * m).sum(-1, keepdim=True)
    if snap:
        m32 = m.detach().numpy().astype(f32)
        out = torch.from_numpy(((m32[..., 0] * m32[..., 0] + m32[..., 1] * m32[..., 1]) + m32[..., 2] * m32[..., 2]
                                > f32(1))[..., None])
    else:
        out = n2 > 1
    n = torch.sqrt(torch.where(out, n2, torch.full_like(n2, 4.0)))
    u = m / n
    a, b, c = (2 * n - 1) / (n * n), 1 / (n * n), -2 * (n - 1) / (n * n)
    q = u * u
    q1, q2 = torch.roll(q, -1, -1), torch.roll(q, -2, -1)
    v1, v2 = torch.roll(v, -1, -1), torch.roll(v, -2, -1)
    D = a * (q1 + q2) + b * q  # J_ii (non-negative terms, as the kernel's: fp64 would lose 2 n eps too)
    mc = (2 - 1 / n) * u
    vc = D * D * v + c * c * q * (q1 * v1 + q2 * v2)
    mo, vo = torch.where(out, mc, m), torch.where(out, vc, v)
    if snap:
        m32c, v32c = contract32(m.detach().numpy().astype(f32), v.detach().numpy().astype(f32))
        mo, vo = X._snap(mo, m32c), X._snap(vo, v32c)
    return mo, vo


def step(*args, contraction=True, **kw):
    """raygrad_ref.step with the contraction after every cast.  Adds "t_grad": per level dL/dt^l (None for level 0 and
    for detached levels)."""
    cast0 = G.cast
    ts = []

    def cast(t, o, d, radius, cylinder=False, snap_=True):
        if torch.is_tensor(t) and t.requires_grad and not t.is_leaf:
            t.retain_grad()
        ts.append(t)
        mean, cov = cast0(t, o, d, radius, cylinder, snap_)
        return contract(mean, cov, snap=snap_) if contraction else (mean, cov)

    G.cast = cast
    try:
        res = G.step(*args, **kw)
    finally:
        G.cast = cast0
    if kw.get("backward", True):
        res["t_grad"] = [None if (l == 0 or not torch.is_tensor(t) or t.grad is None) else t.grad.numpy().copy()
                         for l, t in enumerate(ts)]
    return res
