"""fp64 torch reference of the distortion loss on the last level (nof_config.distortion_loss_mult).

TEST INFRASTRUCTURE, not a test.  Per ray, with s the normalised distance of t, m_k = (s_k + s_{k+1}) / 2 and
delta_k = s_{k+1} - s_k:

    L_r = sum_i sum_j w_i w_j |m_i - m_j| + (1 / 3) sum_i w_i^2 delta_i

`distortion` writes the first term as 2 sum_{i<j} w_i w_j (m_j - m_i): the same value on nondecreasing t, and at
tied midpoints the derivative convention of the O(S) closed form the kernel evaluates (|x| has no derivative at 0;
the ordered form's is that of the sorted order).  `pairwise` is the |m_i - m_j| double sum itself.  `step` adds the
term to crosslevel_ref.step's loss and differentiates; tests/torch_ref.py and tests/crosslevel_ref.py are imported
and left as they are.
"""
from __future__ import annotations

import numpy as np
import torch

import crosslevel_ref as X

f32 = np.float32


def _T(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64))


def normalised(t, near, far, lindisp=0):
    """s(t) [n, S + 1] and the rays' validity [n] (bool): far - near a positive finite number and, lindisp = 1, near > 0
    and 1 / near - 1 / far a positive finite number.  An invalid ray's s is 0 (it contributes nothing)."""
    near, far = _T(near).double(), _T(far).double()
    span = far - near
    ok = torch.isfinite(span) & (span > 0)
    if lindisp:
        okn = ok & (near > 0)
        nn = torch.where(okn, near, torch.ones_like(near))
        ff = torch.where(okn, far, 2 * torch.ones_like(far))
        dsp = 1 / nn - 1 / ff
        ok = okn & torch.isfinite(dsp) & (dsp > 0)
        dsp = torch.where(ok, dsp, torch.ones_like(dsp))
        tt = torch.where(ok[:, None], t, torch.ones_like(t))
        s = (1 / nn[:, None] - 1 / tt) / dsp[:, None]
    else:
        sp = torch.where(ok, span, torch.ones_like(span))
        nn = torch.where(ok, near, torch.zeros_like(near))
        s = (t - nn[:, None]) / sp[:, None]
    return torch.where(ok[:, None], s, torch.zeros_like(s)), ok


def _m_delta(t, near, far, lindisp):
    s, ok = normalised(t, near, far, lindisp)
    return (s[:, :-1] + s[:, 1:]) / 2, s[:, 1:] - s[:, :-1], ok


def distortion(w, t, near, far, lindisp=0):
    """L_r [n] (torch fp64, differentiable in w [n, S] and t [n, S + 1]); 0 for an invalid ray"""
    m, delta, ok = _m_delta(t, near, far, lindisp)
    S = w.shape[1]
    upper = torch.triu(torch.ones(S, S, dtype=torch.float64), diagonal=1)  # i < j
    pair = (w[:, :, None] * w[:, None, :] * (m[:, None, :] - m[:, :, None]) * upper).sum((1, 2))
    L = 2 * pair + (w * w * delta).sum(1) / 3
    return torch.where(ok, L, torch.zeros_like(L))


def pairwise(w, t, near, far, lindisp=0):
    """the definition: sum_i sum_j w_i w_j |m_i - m_j| + (1 / 3) sum_i w_i^2 delta_i"""
    m, delta, ok = _m_delta(t, near, far, lindisp)
    L = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2)) + (w * w * delta).sum(1) / 3
    return torch.where(ok, L, torch.zeros_like(L))


def term(w, t, near, far, lossmult, mult, lindisp=0):
    """(lambda_d sum_r mu_r L_r / sum mu, the per-ray c_r L_r): the term of the objective; mult and the loss
    multipliers' sum as the fp32 numbers the library is given"""
    lm = _T(np.asarray(lossmult, f32)).double()
    msum = float(np.sum(np.asarray(lossmult, f32), dtype=f32))
    rays = float(f32(mult)) * lm * distortion(w, t, near, far, lindisp) / msum
    return rays.sum(), rays


def level_grads(sigma, rgb, t, d, pix, lossmult, near, far, mult, lam=1.0, lindisp=0, white=True):
    """One level on its own (numpy fp32 inputs): dL/dsigma, dL/drgb of lam sum mu |C - pix|^2 / sum mu + the distortion
    term, and the term's per-ray values."""
    sg = torch.tensor(np.asarray(sigma, np.float64), requires_grad=True)
    cg = torch.tensor(np.asarray(rgb, np.float64), requires_grad=True)
    tt = torch.tensor(np.asarray(t, np.float64))
    C, w = X.render(sg, cg, tt, d, white)
    lm = _T(np.asarray(lossmult, f32)).double()
    msum = float(np.sum(np.asarray(lossmult, f32), dtype=f32))
    photo = lam * (lm[:, None] * (C - _T(np.asarray(pix, f32)).double()) ** 2).sum() / msum
    dist, rays = term(w, tt, near, far, lossmult, mult, lindisp)
    (photo + dist).backward()
    return dict(dsigma=sg.grad.numpy(), drgb=cg.grad.numpy(), dist_rays=rays.detach().numpy(), dist=float(dist.detach()),
                photo=float(photo.detach()), w=w.detach().numpy())


def step(P, rays, mult, lindisp=0, detach=False, **kw):
    """crosslevel_ref.step's objective + the distortion term on the last level's w and t.  Returns t, w per level,
    loss (photometric), dist, grads, and w_grad / t_grad per level as crosslevel_ref.step does (w_grad[l]: dL/dw^l
    through level l + 1's resampler alone)."""
    P = torch.tensor(np.asarray(P, np.float64), dtype=torch.float64, requires_grad=True)
    res = X.step(P, rays, detach=detach, backward=False, **kw)
    NL = len(res["t"])
    dist, per_ray = term(res["w"][-1], res["t"][-1], rays["near"], rays["far"], rays["lossmult"], mult, lindisp)
    total = res["loss"] + dist
    G = lambda y, x, go=None: torch.autograd.grad(y, x, grad_outputs=go, retain_graph=True)[0]
    out = dict(loss=float(res["loss"].detach()), dist=float(dist.detach()), dist_rays=per_ray.detach().numpy(),
               grads=G(total, P).numpy().copy())
    tg = [None] * NL
    wg = [None] * NL
    if not detach:
        for l in range(1, NL):
            tg[l] = G(total, res["t"][l])
        for l in range(NL - 1):  # (dt^{l+1} / dw^l)^T dL/dt^{l+1}: t^{l+1} sees w^l through the resampler only
            wg[l] = G(res["t"][l + 1], res["w"][l], tg[l + 1])
    out["t_grad"] = [None if x is None else x.numpy().copy() for x in tg]
    out["w_grad"] = [None if x is None else x.numpy().copy() for x in wg]
    out["t"] = [t.detach().numpy() for t in res["t"]]
    out["w"] = [w.detach().numpy() for w in res["w"]]
    out["idx"] = res["idx"]
    return out
