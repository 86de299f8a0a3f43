"""fp64 torch-autograd reference of the ray gradients (nof_mipnerf_set_ray_grad): the mip-NeRF step of
tests/crosslevel_ref.py with the ray origins and directions as leaves.

TEST INFRASTRUCTURE, not a test.  Reuses crosslevel_ref's resample, ipe and forward; its own cast, render and dir_pe
are differentiable in o and d.  Constants of the derivative, as in the library: radius, near, far, level 0's t,
every Philox uniform (and, detach=True, every level's t).  snap=True (the default): every geometric value is the fp32
forward's (x = x64 + (x32 - x64).detach()), so derivatives are taken at the points the GPU works at; snap=False: pure
fp64, for finite differences.

hold: parts of the forward whose dependence on the ray is cut, for the tests that show each term matters:
"ipe" (cast + IPE constant in o and d), "render" (the integrator's |d| constant), "view" (the view PE constant).

pose: (poses [V, 12], view [n], cam [n, 3]) makes the rays from a pose table leaf, d = R cam, o = t (raygen.h with
ndc = 0, the radius held), and the step also returns dL/dposes.
"""
from __future__ import annotations

import numpy as np
import torch

import crosslevel_ref as X
import torch_ref as R

f32 = np.float32
_snap = X._snap


def cast(t, o, d, radius, cylinder=False, snap=True):
    """CastRay, differentiable in t [n, S + 1], o and d [n, 3] (torch fp64); radius numpy fp32"""
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
    dd = d * d
    dms = torch.clamp(dd.sum(1), min=1e-10)
    nul = 1 - dd / dms[:, None]
    mean = d[:, None, :] * tmean[..., None] + o[:, None, :]
    cov = tvar[..., None] * dd[:, None, :] + rvar[..., None] * nul[:, None, :]
    if snap:
        m32, c32 = R.cast(t.detach().numpy().astype(f32), o.detach().numpy().astype(f32),
                          d.detach().numpy().astype(f32), radius, cylinder)
        mean, cov = _snap(mean, m32), _snap(cov, c32)
    return mean, cov


def render(sigma, rgb, t, d, white=True, snap=True):
    """VolumetricRendering, differentiable in sigma, rgb, t and d (alpha = 1 - exp(-sigma delta |d|))"""
    dl = torch.sqrt((d * d).sum(1))
    delta = t[:, 1:] - t[:, :-1]
    if snap:
        d32 = d.detach().numpy().astype(f32)
        dl = _snap(dl, np.sqrt((d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2]).astype(f32))
        t32 = t.detach().numpy().astype(f32)
        delta = _snap(delta, t32[:, 1:] - t32[:, :-1])
    alpha = 1 - torch.exp(-sigma * delta * dl[:, None])
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha[:, :-1]], 1), 1)
    w = alpha * trans
    C = (w[..., None] * rgb).sum(1)
    if white:
        C = C + (1 - w.sum(1))[:, None]
    return C, w


def dir_pe(d, deg):
    """the view encoding of the unnormalised direction (torch_ref.dir_pe), differentiable in d"""
    out = [d]
    for f in range(deg):
        xb = d * float(1 << f)
        out += [torch.sin(xb), torch.cos(xb)]
    return torch.cat(out, -1)


def rays_from_poses(poses, view, cam):
    """raygen.h ray_at with ndc = 0: d = R cam, o = t; poses torch [V, 12], view [n] ints, cam [n, 3] fp32"""
    Pv = poses[torch.from_numpy(np.asarray(view, np.int64))]
    c = torch.from_numpy(np.asarray(cam, np.float64))
    d = (Pv[:, :9].reshape(-1, 3, 3) * c[:, None, :]).sum(-1)
    return Pv[:, 9:], d


def step(P, rays, net, samples, min_deg=0, max_deg=16, deg_view=4, seed=0, step_idx=0, ray_base=0, padding=0.01,
         coarse_mult=0.1, white=True, cylinder=False, density_bias=-1.0, rgb_padding=0.001, detach=False, idx=None,
         t_value=None, relu=None, snap=True, backward=True, od=None, hold=(), pose=None):
    """One step (crosslevel_ref.step's arguments).  od: (o, d) torch fp64 leaves to use instead of the rays' (for finite
    differences, with backward=False).  Returns loss, grads (parameters), o_grad, d_grad [n, 3], pose_grad [V, 12]
    (with pose), and t / idx per level."""
    n = rays["o"].shape[0]
    gids = np.arange(ray_base, ray_base + n)
    if not torch.is_tensor(P):
        P = torch.tensor(np.asarray(P, np.float64), dtype=torch.float64, requires_grad=True)
    leaf = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)
    poses = None
    if od is not None:
        o, d = od
    elif pose is not None:
        poses = leaf(pose[0])
        o64, d64 = rays_from_poses(poses, pose[1], pose[2])
        o, d = _snap(o64, rays["o"]), _snap(d64, rays["d"])  # the gather's fp32 rays
        o.retain_grad(); d.retain_grad()
    else:
        o, d = leaf(rays["o"]), leaf(rays["d"])
    rad = rays["radius"]
    cut = lambda x, name: x.detach() if name in hold else x
    dirv = dir_pe(cut(d, "view"), deg_view)
    msum = float(np.sum(rays["lossmult"], dtype=np.float32))
    pix = torch.from_numpy(rays["pix"]).double()
    lm = torch.from_numpy(rays["lossmult"]).double()
    NL = len(samples)
    res = {"t": [], "idx": []}
    ts, ws = [], []
    loss = 0
    for lv, S in enumerate(samples):
        if lv == 0:
            t = torch.from_numpy(R.stratified(rays["near"], rays["far"], S, R.uniforms(seed, step_idx, 0, 1, gids, S + 1))
                                 .astype(np.float64))
            ix = None
        else:
            t, ix = X.resample(ts[-1], ws[-1], S, padding, R.uniforms(seed, step_idx, lv, 2, gids, S + 1),
                               idx=(idx or {}).get(lv), snap=snap, t_value=(t_value or {}).get(lv))
            if detach:
                t = t.detach()
                if not snap and (t_value or {}).get(lv) is not None:
                    # a finite difference sees what detach hides from autograd (t^l moves with d through w^{l-1}):
                    # the held t-values are given
                    t = torch.from_numpy(np.asarray(t_value[lv], np.float64))
        ts.append(t)
        mean, cov = cast(t, cut(o, "ipe"), cut(d, "ipe"), rad, cylinder, snap)
        enc = X.ipe(mean, cov, min_deg, max_deg, snap)
        m = None if relu is None else torch.from_numpy(np.asarray(relu[lv], np.float64)).reshape(n, S, -1)
        zs, zc = X.forward(net, P, enc, dirv[:, None, :].expand(n, S, dirv.shape[-1]), m)
        pad = f32(rgb_padding)
        sigma = torch.nn.functional.softplus(zs + float(f32(density_bias)), beta=1, threshold=20)
        rgb = torch.sigmoid(zc) * float(f32(1) + f32(2) * pad) - float(pad)
        C, w = render(sigma, rgb, t, cut(d, "render"), white, snap)
        ws.append(w)
        lam = float(f32(coarse_mult)) if lv < NL - 1 else 1.0
        loss = loss + lam * (lm[:, None] * (C - pix) ** 2).sum() / msum
        res["t"].append(t.detach().numpy()); res["idx"].append(ix)
    if not backward:
        res["loss"] = loss
        return res
    loss.backward()
    res["loss"] = float(loss.detach())
    res["grads"] = P.grad.numpy().copy()
    zero = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy().copy()
    res["o_grad"], res["d_grad"] = zero(o), zero(d)
    if poses is not None:
        res["pose_grad"] = poses.grad.numpy().copy()
    return res
