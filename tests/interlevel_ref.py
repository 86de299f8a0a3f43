"""fp64 torch reference of the interlevel (proposal) loss (nof_mipnerf_set_interlevel_loss).

TEST INFRASTRUCTURE, not a test.  Per ray, with the proposal (t^ [S_c + 1], w^ [S_c]) and the target (t [S_f + 1],
w [S_f], a constant):

    c(v) = #{j in 0..S_c : t^_j <= v},  lo(v) = max(c(v) - 1, 0),  hi(v) = min(c(v), S_c)
    bound_i = sum of w^_j over j in [lo(t_i), hi(t_{i+1}))
    L_r = sum_i max(0, w_i - bound_i)^2 / (w_i + eps),  eps = 2^-23

`loss_rays` is that definition literally: an [S_c + 1] x [S_f + 1] comparison table, cumsum, take; autograd gives
dL/dw^.  `grad_scatter` / `grad_range` are the two closed forms of that gradient in numpy fp64, `emulate_f32` the
kernel's fp32 summation order in numpy, `make_inputs` the generator the CPU and the GPU tests share.  `step` adds the
term to distortion_ref.step / crosslevel_ref.step's objective with the target detached; tests/torch_ref.py,
tests/crosslevel_ref.py and tests/distortion_ref.py are imported and left as they are.
"""
from __future__ import annotations

import numpy as np
import torch

import crosslevel_ref as X
import distortion_ref as D

f32 = np.float32
EPS = 2.0 ** -23
NEAR, FAR = 2.0, 6.0


def _T(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64))


def lo_hi(tp, t):
    """lo(t_k), hi(t_k) for every target edge k: int64 [n, S_f + 1] each (comparisons on the values as given)"""
    tp, t = _T(tp).detach(), _T(t).detach()
    Sc = tp.shape[1] - 1
    c = (tp[:, :, None] <= t[:, None, :]).sum(1)  # the [S_c + 1] x [S_f + 1] table, summed over j
    return torch.clamp(c - 1, min=0), torch.clamp(c, max=Sc)


def bound(wp, tp, t):
    """bound_i [n, S_f] (differentiable in wp)"""
    lo, hi = lo_hi(tp, t)
    cw = torch.cat([torch.zeros_like(wp[:, :1]), torch.cumsum(wp, 1)], 1)
    return torch.gather(cw, 1, hi[:, 1:]) - torch.gather(cw, 1, lo[:, :-1])


def loss_rays(wp, tp, w, t):
    """L_r [n] (torch fp64, differentiable in wp); w, t: the target, used as constants"""
    w = _T(w).detach()
    m = torch.clamp(w - bound(wp, tp, t), min=0.0)
    return (m * m / (w + EPS)).sum(1)


def term(wp, tp, w, t, lossmult, mult):
    """(lambda_p sum_r mu_r L_r / sum mu, the per-ray c_r L_r); mult and sum mu as the fp32 numbers the library gets"""
    lm = _T(np.asarray(lossmult, f32)).double()
    msum = float(np.sum(np.asarray(lossmult, f32), dtype=f32))
    rays = float(f32(mult)) * lm * loss_rays(wp, tp, w, t) / msum
    return rays.sum(), rays


def kernel_ref(inp, mult):
    """the kernel entry's outputs in fp64: dL/dw^ [n, S_c], the per-ray term [n], the unmultiplied L_r [n], and the
    hinge margins w_i - bound_i [n, S_f]"""
    wp = torch.tensor(inp["wp"].astype(np.float64), requires_grad=True)
    tot, rays = term(wp, inp["tp"], inp["w"], inp["t"], inp["lm"], mult)
    tot.backward()
    with torch.no_grad():
        margin = _T(inp["w"]) - bound(wp, inp["tp"], inp["t"])
        L = loss_rays(wp, inp["tp"], inp["w"], inp["t"])
    return dict(w_grad=wp.grad.numpy(), rays=rays.detach().numpy(), L=L.numpy(), margin=margin.numpy())


# ---- the two closed forms of dL_r/dw^ (numpy fp64, one ray) and the kernel's fp32 order -----------------------
def _g(wp, tp, w, t, dtype=np.float64):
    """g_i = -2 max(0, w_i - bound_i) / (w_i + eps) with bound_i summed directly over its own range, ascending j;
    also the hinge terms and (lo(t_i), hi(t_{i+1}))"""
    Sc, Sf = len(wp), len(w)
    c = np.searchsorted(tp, t, side="right")  # #{j : t^_j <= t_k}
    lo, hi = np.maximum(c - 1, 0)[:-1], np.minimum(c, Sc)[1:]
    g, terms = np.zeros(Sf, dtype), np.zeros(Sf, dtype)
    eps = dtype(EPS)
    for i in range(Sf):
        b = dtype(0)
        for j in range(lo[i], hi[i]):
            b = dtype(b + wp[j])
        m = max(dtype(0), dtype(w[i] - b))
        den = dtype(w[i] + eps)
        g[i] = dtype(dtype(-2) * m) / den
        terms[i] = dtype(m * m) / den
    return g, terms, lo, hi


def grad_scatter(wp, tp, w, t):
    """add g_i to every j in [lo(t_i), hi(t_{i+1}))"""
    g, _, lo, hi = _g(wp, tp, w, t)
    out = np.zeros(len(wp))
    for i in range(len(w)):
        out[lo[i]:hi[i]] += g[i]
    return out


def ranges(tp, t):
    """a_j = #{k in 1..S_f : t_k < t^_j}, b_j = #{i in 0..S_f-1 : t_i < t^_{j+1}}"""
    a = np.searchsorted(t[1:], tp[:-1], side="left")
    b = np.searchsorted(t[:-1], tp[1:], side="left")
    return a, b


def grad_range(wp, tp, w, t):
    """sum of g_i over i in [a_j, b_j)"""
    g, _, _, _ = _g(wp, tp, w, t)
    a, b = ranges(tp, t)
    return np.array([g[a[j]:b[j]].sum() for j in range(len(wp))])


def emulate_f32(wp, tp, w, t, c):
    """k_interlevel's arithmetic in numpy fp32, one ray: the direct bound; h = -g summed per lane (S_f / 64
    consecutive intervals, ascending), a Hillis-Steele inclusive scan over the 64 lanes, G[i + 1] = base + running
    sum; dL/dw^_j = c (G[a_j] - G[b_j]); the per-ray term c times a butterfly sum of the lanes' hinge sums"""
    wp, tp, w, t, c = (np.asarray(x, f32) for x in (wp, tp, w, t, c))
    Sf = len(w)
    PF = Sf // 64
    g, terms, _, _ = _g(wp, tp, w, t, f32)
    h = (-g).astype(f32).reshape(64, PF)
    lane = np.zeros(64, f32)
    ls = np.zeros(64, f32)
    tl = terms.reshape(64, PF)
    for p in range(PF):
        lane = (lane + h[:, p]).astype(f32)
        ls = (ls + tl[:, p]).astype(f32)
    inc = lane.copy()
    o = 1
    while o < 64:
        y = np.concatenate([np.zeros(o, f32), inc[:-o]])
        inc = np.where(np.arange(64) >= o, (inc + y).astype(f32), inc)
        o <<= 1
    base = np.concatenate([np.zeros(1, f32), inc[:-1]])
    G = np.zeros(Sf + 1, f32)
    for p in range(PF):
        base = (base + h[:, p]).astype(f32)
        G[1 + p + PF * np.arange(64)] = base
    o = 32
    while o >= 1:
        ls = (ls + ls[np.arange(64) ^ o]).astype(f32)
        o >>= 1
    a, b = ranges(tp, t)
    return (c * (G[a] - G[b]).astype(f32)).astype(f32), f32(c * ls[0])


# ---- the shared input generator ----------------------------------------------------------------------------------
def make_inputs(Sc, Sf, n=6, seed=0, active=0.7):
    """n >= 6 rays, numpy fp32: sorted random edges in [NEAR, FAR] on both rows and heavy-tailed weights; the proposal
    weights of every ray are scaled so that about 1 - `active` of the ray's target intervals have an active hinge
    (the scale is the `active` quantile of w_i / bound_i, taken from this reference alone).  Ray 1: the target row
    takes a quarter of its edges verbatim from the proposal row (ties).  Ray 2: one surface (weights 1e-6, 0.9 in one
    target interval, 0.6 in the proposal interval under its midpoint).  Ray 3: w = 0.  lossmult: ray 4 has 0, ray 5
    has 2."""
    assert n >= 6
    rng = np.random.default_rng(7000 + 13 * Sc + Sf + seed)
    edges = lambda S: np.sort(NEAR + (FAR - NEAR) * rng.random((n, S + 1)), axis=1).astype(f32)
    tp, t = edges(Sc), edges(Sf)
    q = min((Sf + 1) // 4, Sc + 1)
    t[1, rng.choice(Sf + 1, q, replace=False)] = tp[1, rng.choice(Sc + 1, q, replace=False)]
    t[1] = np.sort(t[1])
    weights = lambda S: (lambda x: (0.9 * x / x.sum(1, keepdims=True)))(rng.gamma(0.5, 1.0, (n, S)) + 1e-4).astype(f32)
    wp, w = weights(Sc), weights(Sf)
    w[3] = 0.0
    with torch.no_grad():
        b0 = bound(_T(wp), tp, t).numpy()
    for r in range(n):
        if r in (2, 3):
            continue
        wp[r] = (wp[r].astype(np.float64) * np.quantile(w[r] / np.maximum(b0[r], 1e-30), active)).astype(f32)
    w[2] = 1e-6
    wp[2] = 1e-6
    k = Sf // 3
    w[2, k] = 0.9
    mid = 0.5 * (float(t[2, k]) + float(t[2, k + 1]))
    j = int(np.clip(np.searchsorted(tp[2], mid, side="right") - 1, 0, Sc - 1))
    wp[2, j] = 0.6
    lm = np.ones(n, f32)
    lm[4] = 0.0
    lm[5] = 2.0
    return dict(n=n, Sc=Sc, Sf=Sf, tp=tp, wp=wp, t=t, w=w, lm=lm)


# ---- one level and whole steps -----------------------------------------------------------------------------------
def level_grads(sigma, rgb, t, d, pix, lossmult, t_tgt, w_tgt, mult, lam, white=True, w_value=None):
    """A coarser level on its own (numpy fp32 inputs): dL/dsigma, dL/drgb of lam sum mu |C - pix|^2 / sum mu + the
    interlevel term against the target (t_tgt, w_tgt), and the term's per-ray values.  w_value: the level's stored fp32
    weights; the term is then evaluated at them (value of w_value, derivative of the fp64 w: crosslevel_ref._snap).
    g_i = -2 (w_i - bound_i) / (w_i + eps) is O(1) at any weight magnitude, and the integrator's fp32
    alpha = 1 - exp(-sigma delta) carries an absolute error of 6e-8, a relative one of percents at the weights of thin
    regions: the derivative is taken where the library evaluates it, as for the resampler's cdf."""
    sg = torch.tensor(np.asarray(sigma, np.float64), requires_grad=True)
    cg = torch.tensor(np.asarray(rgb, np.float64), requires_grad=True)
    tt = torch.tensor(np.asarray(t, np.float64))
    C, w = X.render(sg, cg, tt, d, white)
    lm = _T(np.asarray(lossmult, f32)).double()
    msum = float(np.sum(np.asarray(lossmult, f32), dtype=f32))
    photo = float(f32(lam)) * (lm[:, None] * (C - _T(np.asarray(pix, f32)).double()) ** 2).sum() / msum
    wq = w if w_value is None else X._snap(w, w_value)
    prop, rays = term(wq, tt, np.asarray(w_tgt, np.float64), np.asarray(t_tgt, np.float64), lossmult, mult)
    (photo + prop).backward()
    return dict(dsigma=sg.grad.numpy(), drgb=cg.grad.numpy(), prop_rays=rays.detach().numpy(),
                prop=float(prop.detach()), photo=float(photo.detach()))


def step(P, rays, mult, dist_mult=0.0, lindisp=0, detach=False, w_value=None, **kw):
    """crosslevel_ref.step's objective (+ distortion_ref's term when dist_mult > 0) + the interlevel term of every level
    l < L - 1 against the last level's detached (t, w).  Returns what distortion_ref.step returns, and prop (the
    term), prop_levels (per level) and w_grad_prop[l] = the term's own dL/dw^l; w_grad[l] (not detach) is the
    resampler's share plus that, what the library's q^l holds.  w_value: {level: stored fp32 weights}, the values
    the term is evaluated at (level_grads says why); the photometric and distortion terms are as they were."""
    P = torch.tensor(np.asarray(P, np.float64), dtype=torch.float64, requires_grad=True)
    res = X.step(P, rays, detach=detach, backward=False, **kw)
    NL = len(res["t"])
    W = lambda l: res["w"][l] if w_value is None else X._snap(res["w"][l], w_value[l])
    tt, wt = res["t"][-1].detach(), W(NL - 1).detach()
    zero = torch.zeros((), dtype=torch.float64)
    props = [term(W(l), res["t"][l], wt, tt, rays["lossmult"], mult)[0] for l in range(NL - 1)]
    prop = sum(props, zero)
    dist = zero
    if dist_mult:
        dist, _ = D.term(res["w"][-1], res["t"][-1], rays["near"], rays["far"], rays["lossmult"], dist_mult, lindisp)
    total = res["loss"] + prop + dist
    G = lambda y, x, go=None: torch.autograd.grad(y, x, grad_outputs=go, retain_graph=True, allow_unused=True)[0]
    out = dict(loss=float(res["loss"].detach()), prop=float(prop.detach()), dist=float(dist.detach()),
               prop_levels=[float(p.detach()) for p in props], grads=G(total, P).numpy().copy())
    tg, wg = [None] * NL, [None] * NL
    wgp = [G(props[l], res["w"][l]).numpy().copy() if mult else np.zeros(tuple(res["w"][l].shape)) for l in range(NL - 1)]
    if not detach:
        for l in range(1, NL):
            tg[l] = G(total, res["t"][l])
        for l in range(NL - 1):
            wg[l] = G(res["t"][l + 1], res["w"][l], tg[l + 1]).numpy() + wgp[l]
    out["t_grad"] = [None if x is None else x.numpy().copy() for x in tg]
    out["w_grad"] = wg
    out["w_grad_prop"] = wgp + [None]
    out["t"] = [t.detach().numpy() for t in res["t"]]
    out["w"] = [w.detach().numpy() for w in res["w"]]
    return out
