"""fp64 torch-autograd reference of the mip-NeRF step with cross-level gradients (stop_level_grad = 0).

TEST INFRASTRUCTURE, not a test.  Reuses tests/torch_ref.py (Net, uniforms, stratified, dir_pe, glorot and the
fp32 numpy geometry) and adds differentiable resample / cast / IPE / render:

    t^l = resample(t^{l-1}, w^{l-1}; u),  differentiable in w^{l-1} AND t^{l-1} (the bin edges),

with the bin index an argument (held), the other discrete decisions (tt clamped, den > 0, min(1, run)
saturated, the pad branch, the blur-pool's max picks) taken by torch's own clamp / where / minimum / maximum at the
forward values (a tie in a max splits the gradient equally, as torch.maximum does).  Level 0's t and every
Philox uniform are constants.

snap=True (the default): every geometric value (t, the resampler's cdf, mean / cov, the phase y + pi / 2, delta) is
the fp32 one torch_ref computes (x = x64 + (x32 - x64).detach()),
so with detach=True the step IS torch_ref.step, and derivatives are taken at the points the GPU works at.
snap=False: pure fp64, for finite differences (fp32 snapping is noise to a difference quotient).
"""
from __future__ import annotations

import numpy as np
import torch

import torch_ref as R

f32 = np.float32


def _snap(x64, x32):
    """value of x32 (numpy fp32), derivative of x64"""
    return x64 + (torch.from_numpy(np.asarray(x32, np.float64)) - x64).detach()


def resample(t, w, S_out, padding, u_raw, idx=None, snap=True, t_value=None):
    """ResampleAlongRay, differentiable in t [n, B + 1] and w [n, B] (torch fp64).  u_raw: Philox uniforms
    [n, S_out + 1] (fp32).  idx [n, S_out + 1]: the bin of every sample (None: this function's own).  t_value
    (snap only): the fp32 values the result takes (None: torch_ref.resample's).  Returns (t_out, idx)."""
    n, B = w.shape
    wpad = torch.cat([w[:, :1], w, w[:, -1:]], 1)
    wmax = torch.maximum(wpad[:, :-1], wpad[:, 1:])
    wb = 0.5 * (wmax[:, :-1] + wmax[:, 1:]) + float(f32(padding))
    wsum = wb.sum(1)
    pad = torch.clamp(float(f32(1e-5)) - wsum, min=0.0)
    wb = wb + (pad / B)[:, None]
    wsum = wsum + pad
    pdf = wb / wsum[:, None]
    run = torch.cumsum(pdf[:, :-1], 1)
    cdf = torch.cat([torch.zeros(n, 1, dtype=torch.float64), torch.minimum(torch.ones_like(run), run),
                     torch.ones(n, 1, dtype=torch.float64)], 1)
    if snap:
        # the forward's sequential fp32 cdf (torch_ref.resample's lines): tt = (u - c0) / (c1 - c0) cancels, so an
        # fp64 cdf 1e-7 away moves tt by 1e-4 of a bin; the derivative is taken where the forward evaluates it
        w32 = w.detach().numpy().astype(f32)
        p32 = np.concatenate([w32[:, :1], w32, w32[:, -1:]], 1)
        m32 = np.maximum(p32[:, :-1], p32[:, 1:])
        b32 = (f32(0.5) * (m32[:, :-1] + m32[:, 1:]) + f32(padding)).astype(f32)
        s32 = b32.astype(np.float64).sum(1).astype(f32)
        pd32 = np.maximum(f32(0), f32(1e-5) - s32)
        b32 = np.where(pd32[:, None] > 0, b32 + (pd32 / f32(B))[:, None], b32).astype(f32)
        s32 = np.where(pd32 > 0, s32 + pd32, s32).astype(f32)
        r32 = np.cumsum((b32 / s32[:, None]).astype(f32)[:, :-1], axis=1, dtype=f32)
        cdf = _snap(cdf, np.concatenate([np.zeros((n, 1), f32), np.minimum(f32(1), r32), np.ones((n, 1), f32)], 1))
    ns = S_out + 1
    s1 = f32(1) / f32(ns)
    i = np.arange(ns, dtype=f32)[None, :]
    u32 = np.minimum(i * s1 + u_raw * (s1 - f32(1e-7)), f32(1) - f32(1e-7)).astype(f32)
    u = torch.from_numpy(u32.astype(np.float64))
    if idx is None:
        c = cdf.detach().numpy()
        idx = np.stack([np.searchsorted(c[r], u32[r].astype(np.float64), side="right") - 1 for r in range(n)])
        idx = np.clip(idx, 0, B - 1)
    j = torch.from_numpy(np.asarray(idx, np.int64))
    b0, b1 = torch.gather(t, 1, j), torch.gather(t, 1, j + 1)
    c0, c1 = torch.gather(cdf, 1, j), torch.gather(cdf, 1, j + 1)
    den = c1 - c0
    safe = torch.where(den > 0, den, torch.ones_like(den))
    tt = torch.where(den > 0, (u - c0) / safe, torch.zeros_like(den))
    tt = torch.clamp(tt, 0.0, 1.0)
    out = b0 + tt * (b1 - b0)
    if snap:
        if t_value is None:
            t_value, _ = R.resample(t.detach().numpy().astype(f32), w.detach().numpy().astype(f32), S_out, padding,
                                    u_raw)
        out = _snap(out, t_value)
    return out, np.asarray(idx, np.int32)


def cast(t, o, d, radius, cylinder=False, snap=True):
    """CastRay, differentiable in t (torch fp64 [n, S + 1]); o, d, radius numpy fp32"""
    t0, t1 = t[:, :-1], t[:, 1:]
    rad = torch.from_numpy(radius.astype(np.float64))[:, None]
    if cylinder:
        tmean = (t0 + t1) / 2
        rvar = (rad * rad / 4).expand_as(tmean)
        tvar = (t1 - t0) * (t1 - t0) / 12
    else:
        mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
        mu2, hw2 = mu * mu, hw * hw
        den = 3 * mu2 + hw2
        tmean = mu + (2 * mu * hw2) / den
        tvar = hw2 / 3 - (4.0 / 15.0) * (hw2 * hw2 * (12 * mu2 - hw2)) / (den * den)
        rvar = rad * rad * (mu2 / 4 + (5.0 / 12.0) * hw2 - (4.0 / 15.0) * (hw2 * hw2) / den)
    dms = np.maximum(f32(1e-10), (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    dd = d * d
    nul = f32(1) - dd / dms[:, None]
    D = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    mean = D(d)[:, None, :] * tmean[..., None] + D(o)[:, None, :]
    cov = tvar[..., None] * D(dd)[:, None, :] + rvar[..., None] * D(nul)[:, None, :]
    if snap:
        m32, c32 = R.cast(t.detach().numpy().astype(f32), o, d, radius, cylinder)
        mean, cov = _snap(mean, m32), _snap(cov, c32)
    return mean, cov


def ipe(mean, cov, min_deg, max_deg, snap=True):
    """IntegratedPositionalEncoding in the encoder's feature order, differentiable in mean and cov"""
    half_pi = f32(3.14159274) * f32(0.5)
    feats = []
    for f in range(min_deg, max_deg):
        s = float(1 << f)
        y, yv = mean * s, cov * s * s
        damp = torch.exp(-0.5 * yv)
        yc = y + float(half_pi)
        if snap:  # the forward's fl32(y + pi / 2)
            yc = _snap(yc, y.detach().numpy().astype(f32) + half_pi)
        feats += [damp * torch.sin(y), damp * torch.sin(yc)]
    return torch.cat(feats, -1)


def render(sigma, rgb, t, d, white=True, snap=True):
    """VolumetricRendering, differentiable in sigma, rgb and t"""
    dl = torch.from_numpy(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(f32)).double()
    delta = t[:, 1:] - t[:, :-1]
    if snap:
        t32 = t.detach().numpy().astype(f32)
        delta = _snap(delta, t32[:, 1:] - t32[:, :-1])
    alpha = 1 - torch.exp(-sigma * delta * dl[:, None])
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha[:, :-1]], 1), 1)
    w = alpha * trans
    C = (w[..., None] * rgb).sum(1)
    if white:
        C = C + (1 - w.sum(1))[:, None]
    return C, w


def forward(net, P, enc, dirv, relu=None):
    """Net.forward with the ReLU decisions optionally given: relu [..., D W + Dc Wc] (0 / 1), the layout of
    AcceleratedMLP.relu_masks"""
    Ws, bs = net.views(P)
    off = 0

    def act(z, width):
        nonlocal off
        if relu is None:
            return torch.relu(z)
        m = relu[..., off:off + width]
        off += width
        return z * m

    h = enc
    for l in range(net.D):
        x = torch.cat([h, enc], -1) if (l % net.skip == 0 and l > 0) else h
        h = act(x @ Ws[l].T + bs[l], net.W)
    zs = (h @ Ws[net.D].T + bs[net.D])[..., 0]
    x = torch.cat([h, dirv], -1)
    for i in range(net.Dc):
        l = net.D + 1 + i
        x = act(x @ Ws[l].T + bs[l], net.Wc)
    zc = x @ Ws[-1].T + bs[-1]
    return zs, zc


def step(P, rays, net, samples, min_deg=0, max_deg=16, deg_view=4, seed=0, step_idx=0, ray_base=0, padding=0.01,
         coarse_mult=0.1, white=True, cylinder=False, density_bias=-1.0, rgb_padding=0.001, detach=False, idx=None,
         t_value=None, relu=None, snap=True, backward=True):
    """One step.  P: numpy parameters, or a torch fp64 leaf (then backward=False returns the loss tensor for the
    caller's own differentiation).  detach: every level's t a constant (stop_level_grad = 1).  idx / t_value / relu:
    {level: array} of the bin indices, the fp32 t values and the ReLU decisions to adopt (the GPU's).  Returns
    t, w, C, idx per level, loss, grads, and w_grad / t_grad per level (dL/dw^l through the next level's
    resampler only, dL/dt^l; None where a level has none)."""
    n = rays["o"].shape[0]
    gids = np.arange(ray_base, ray_base + n)
    if not torch.is_tensor(P):
        P = torch.tensor(np.asarray(P, np.float64), dtype=torch.float64, requires_grad=True)
    o, d, rad = rays["o"], rays["d"], rays["radius"]
    dirv = torch.from_numpy(R.dir_pe(d, deg_view))
    msum = float(np.sum(rays["lossmult"], dtype=np.float32))
    pix = torch.from_numpy(rays["pix"]).double()
    lm = torch.from_numpy(rays["lossmult"]).double()
    NL = len(samples)
    res = {"t": [], "w": [], "C": [], "idx": []}
    ts, wtaps = [], []
    loss = 0
    for lv, S in enumerate(samples):
        if lv == 0:
            t = torch.from_numpy(R.stratified(rays["near"], rays["far"], S, R.uniforms(seed, step_idx, 0, 1, gids, S + 1))
                                 .astype(np.float64))
            ix = None
        else:
            wtap = res["w"][-1] + 0  # a node of its own: its gradient is the resampler's share of dL/dw alone
            if wtap.requires_grad:
                wtap.retain_grad()
            wtaps.append(wtap)
            t, ix = resample(ts[-1], wtap, S, padding, R.uniforms(seed, step_idx, lv, 2, gids, S + 1),
                             idx=(idx or {}).get(lv), snap=snap, t_value=(t_value or {}).get(lv))
            if detach:
                t = t.detach()
            elif t.requires_grad:
                t.retain_grad()
        ts.append(t)
        mean, cov = cast(t, o, d, rad, cylinder, snap)
        enc = ipe(mean, cov, min_deg, max_deg, snap)
        m = None if relu is None else torch.from_numpy(np.asarray(relu[lv], np.float64)).reshape(n, S, -1)
        zs, zc = forward(net, P, enc, dirv[:, None, :].expand(n, S, dirv.shape[-1]), m)
        pad = f32(rgb_padding)
        sigma = torch.nn.functional.softplus(zs + float(f32(density_bias)), beta=1, threshold=20)
        rgb = torch.sigmoid(zc) * float(f32(1) + f32(2) * pad) - float(pad)
        C, w = render(sigma, rgb, t, d, white, snap)
        lam = float(f32(coarse_mult)) if lv < NL - 1 else 1.0
        loss = loss + lam * (lm[:, None] * (C - pix) ** 2).sum() / msum
        res["t"].append(t); res["w"].append(w); res["C"].append(C); res["idx"].append(ix)
    if not backward:
        res["loss"] = loss
        return res
    loss.backward()
    g = lambda x: None if (x is None or x.grad is None) else x.grad.numpy().copy()
    res["grads"] = P.grad.numpy().copy()
    res["loss"] = float(loss.detach())
    res["w_grad"] = [g(wtaps[l]) if (l < NL - 1 and not detach) else None for l in range(NL)]
    res["t_grad"] = [g(ts[l]) if (l > 0 and ts[l].requires_grad) else None for l in range(NL)]
    res["t"] = [t.detach().numpy() for t in res["t"]]
    res["w"] = [w.detach().numpy() for w in res["w"]]
    res["C"] = [C.detach().numpy() for C in res["C"]]
    return res


def tensors(net):
    """(name, start, size) of the arena's tensors [W0..W_{L-1}, b0..b_{L-1}]"""
    out, o = [], 0
    for l in range(net.L):
        s = net.outs[l] * net.ins[l]
        out.append((f"W{l}", o, s)); o += s
    for l in range(net.L):
        out.append((f"b{l}", o, net.outs[l])); o += net.outs[l]
    return out
