"""fp64 torch-autograd reference of the per-view appearance embeddings (nof_mipnerf_create_ex): the
mip-NeRF step of tests/raygrad_ref.py with the view layer's per-ray input [viewPE(d) | E[view]], E [V, G] a leaf.

TEST INFRASTRUCTURE, not a test.  Reuses crosslevel_ref's resample, ipe and forward, raygrad_ref's cast, render and
dir_pe (differentiable in o and d) and contraction_ref's contract, with the same fp32 snapping: snap=True (the
default) takes every geometric value from the fp32 forward, so derivatives are taken at the points the GPU works at;
snap=False is pure fp64, for finite differences.  A view id outside [0, V) reads the zero vector and reaches no row
of E, as the library's gather does.
"""
from __future__ import annotations

import numpy as np
import torch

import contraction_ref as K
import crosslevel_ref as X
import raygrad_ref as G
import torch_ref as R

f32 = np.float32


def net(spec, dim):
    """torch_ref.Net of (D, W, Dc, Wc, skip, min_deg, max_deg, deg_view) with the view layer widened by dim"""
    D, W, Dc, Wc, skip, lo, hi, dv = spec
    return R.Net(D=D, W=W, Dc=Dc, Wc=Wc, skip=skip, pos_in=6 * (hi - lo), dir_in=3 * (2 * dv + 1) + dim)


def embed(E, view):
    """rows E[view] [n, G]; zeros for an id outside [0, V)"""
    v = np.asarray(view, np.int64)
    ok = (v >= 0) & (v < E.shape[0])
    rows = E[torch.from_numpy(np.where(ok, v, 0))]
    return rows * torch.from_numpy(ok.astype(np.float64))[:, None]


def step(P, E, view, rays, net, samples, min_deg=0, max_deg=16, deg_view=4, seed=0, step_idx=0, ray_base=0, padding=0.01,
         coarse_mult=0.1, white=True, cylinder=False, density_bias=-1.0, rgb_padding=0.001, detach=False, idx=None,
         t_value=None, relu=None, snap=True, backward=True, contraction=False, lindisp=False):
    """One step.  P: numpy parameters or a torch fp64 leaf; E: numpy [V, G] or a torch fp64 leaf; view: [n] ints.
    detach: every level's t a constant (stop_level_grad = 1).  idx / t_value / relu: {level: array} of the bin indices,
    the fp32 t values and the ReLU decisions to adopt.  backward=False returns the loss tensor under "loss".  Returns
    loss, grads (parameters), e_grad [V, G], o_grad / d_grad [n, 3], t / idx per level and t_grad per level (dL/dt^l;
    None for level 0 and for detached levels)."""
    n = rays["o"].shape[0]
    gids = np.arange(ray_base, ray_base + n)
    leaf = lambda a: a if torch.is_tensor(a) else torch.tensor(np.asarray(a, np.float64), dtype=torch.float64,
                                                               requires_grad=True)
    P, E = leaf(P), leaf(E)
    o, d = leaf(rays["o"]), leaf(rays["d"])
    rad = rays["radius"]
    dirv = torch.cat([G.dir_pe(d, deg_view), embed(E, view)], -1)
    msum = float(np.sum(rays["lossmult"], dtype=np.float32))
    pix = torch.from_numpy(rays["pix"]).double()
    lm = torch.from_numpy(rays["lossmult"]).double()
    NL = len(samples)
    res = {"t": [], "idx": [], "C": []}
    ts, ws = [], []
    loss = 0
    for lv, S in enumerate(samples):
        if lv == 0:
            t = torch.from_numpy(R.stratified(rays["near"], rays["far"], S,
                                              R.uniforms(seed, step_idx, 0, 1, gids, S + 1), lindisp)
                                 .astype(np.float64))
            ix = None
        else:
            t, ix = X.resample(ts[-1], ws[-1], S, padding, R.uniforms(seed, step_idx, lv, 2, gids, S + 1),
                               idx=(idx or {}).get(lv), snap=snap, t_value=(t_value or {}).get(lv))
            if detach:
                t = t.detach()
            elif t.requires_grad:
                t.retain_grad()
        ts.append(t)
        mean, cov = G.cast(t, o, d, rad, cylinder, snap)
        if contraction:
            mean, cov = K.contract(mean, cov, snap=snap)
        enc = X.ipe(mean, cov, min_deg, max_deg, snap)
        m = None if relu is None else torch.from_numpy(np.asarray(relu[lv], np.float64)).reshape(n, S, -1)
        zs, zc = X.forward(net, P, enc, dirv[:, None, :].expand(n, S, dirv.shape[-1]), m)
        pad = f32(rgb_padding)
        sigma = torch.nn.functional.softplus(zs + float(f32(density_bias)), beta=1, threshold=20)
        rgb = torch.sigmoid(zc) * float(f32(1) + f32(2) * pad) - float(pad)
        C, w = G.render(sigma, rgb, t, d, white, snap)
        ws.append(w)
        lam = float(f32(coarse_mult)) if lv < NL - 1 else 1.0
        loss = loss + lam * (lm[:, None] * (C - pix) ** 2).sum() / msum
        res["t"].append(t.detach().numpy()); res["idx"].append(ix); res["C"].append(C.detach().numpy())
    if not backward:
        res["loss"] = loss
        return res
    loss.backward()
    res["loss"] = float(loss.detach())
    zero = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy().copy()
    res["grads"], res["e_grad"] = zero(P), zero(E)
    res["o_grad"], res["d_grad"] = zero(o), zero(d)
    res["t_grad"] = [None if (l == 0 or not t.requires_grad or t.grad is None) else t.grad.numpy().copy()
                     for l, t in enumerate(ts)]
    return res
