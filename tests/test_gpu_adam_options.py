"""Adam's options on the GPU: weight decay, clip by value, clip by global norm and the step statistics
(include/nof.h nof_adam_set_options; Config.GradMaxNorm / GradMaxVal / WeightDecayMult, TrainState.cs:58-59,70;
StatsUtil.cs:13,16-18), driven through AcceleratedAdamOptimizer over torch device tensors: no model.

Sizes: the smallest at which the wave64 / block reductions and the grid-stride loops can go wrong (one lane,
one wave -+ 1, one block + 1, 2048 blocks x 256 threads + 1, the reference arena), and a list of separately
allocated tensors with an empty one.  The inputs keep the regime unambiguous: the norm the clip compares is
checked in fp64 to sit a factor 2 or more away from grad_max_norm before anything relies on it.

What is asserted: grad_abs_max bit for bit; the norms, weight_l2 and clip_scale within 1e-5 relative of fp64
(the fp32 contract); the parameters, m and v bit for bit against oracle.adam_step fed the gradient
clipped in numpy float32 with the library's reported clip_scale, over two steps.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAT_SIZES = [1, 63, 64, 65, 256, 257, 524288, 524289, 546948]
NONFLAT = [5, 0, 300, 1]
LAYOUTS = [(n,) for n in FLAT_SIZES] + [tuple(NONFLAT)]
GMN = 1.0  # grad_max_norm where the norm clip is on
# (name, norm clip on, value clip on, decay on, |g| / grad_max_norm)
CASES = [("val", False, True, False, 10.0), ("norm_active", True, False, False, 10.0),
         ("norm_inactive", True, False, False, 0.1), ("all_active", True, True, True, 10.0),
         ("all_inactive", True, True, True, 0.1)]
LRS = (1e-3, 7e-4)
F32 = np.float32


def _ids(v):
    return v[0] if isinstance(v[0], str) else "x".join(map(str, v))


@functools.lru_cache(maxsize=None)
def _inputs(total, ratio, seed=0):
    """p and two steps' gradients, |g| = ratio * GMN (to fp32 rounding)."""
    rng = np.random.default_rng(1000 * seed + total)
    p = (0.5 * rng.standard_normal(total)).astype(F32)
    gs = []
    for _ in LRS:
        z = rng.standard_normal(total)
        z[np.abs(z) < 1e-3] = 1e-3  # n = 1: a lone element is never ~0
        gs.append((z * (ratio * GMN / np.linalg.norm(z))).astype(F32))
    for a in (p, *gs):
        a.setflags(write=False)
    return p, gs


def _options(case, p, g):
    """grad_max_norm, grad_max_val (the median |g|), weight_decay_mult (|wdc p| ~ 0.3 |g|) of a case."""
    _, norm, val, decay, _ = case
    P = p.size
    gmv = float(F32(np.median(np.abs(g)))) if val else 0.0
    wd = float(F32(0.3 * np.linalg.norm(g.astype(np.float64)) / np.linalg.norm(p.astype(np.float64)) * P / 2)) \
        if decay else 0.0
    return (GMN if norm else 0.0), gmv, wd


def _expect(p, g, gmn, gmv, wd):
    """The issue's steps 1-5: g1, g2 in numpy float32 (one rounded operation per line), the statistics in fp64."""
    P = p.size
    if wd:
        wdc = F32(F32(2.0) * F32(wd)) / F32(P)
        assert wdc.dtype == F32
        t = wdc * p
        g1 = g + t
    else:
        g1 = g
    g2 = np.minimum(np.maximum(g1, F32(-gmv)), F32(gmv)) if gmv else g1
    assert g1.dtype == F32 and g2.dtype == F32
    g1d, g2d, pd = (a.astype(np.float64) for a in (g1, g2, p))
    n2 = float(np.sqrt(np.sum(g2d * g2d)))
    scale = min(1.0, gmn / (1e-7 + n2)) if gmn else 1.0
    return dict(g2=g2, n2=n2, grad_abs_max=F32(np.max(np.abs(g1))), grad_norm=float(np.sqrt(np.sum(g1d * g1d))),
                weight_l2=float(np.sum(pd * pd) / P), clip_scale=scale, grad_norm_clipped=scale * n2)


class _Run:
    """An optimizer over device tensors: one arena for a flat layout, else one allocation per tensor."""

    def __init__(self, dev, sizes, p, **opts):
        import torch

        import nof

        self.sizes, self.dev = list(sizes), dev
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        if len(sizes) == 1:
            self.pt, self.gt = [torch.empty(sizes[0], device=dev)], [torch.empty(sizes[0], device=dev)]
        else:  # every tensor its own allocation, padded apart so that no two are views of one arena
            self.pt = [torch.empty(s, device=dev) for s in sizes]
            self._pad = [torch.empty(777, device=dev) for _ in sizes]
            self.gt = [torch.empty(s, device=dev) for s in sizes]
            assert any(a.data_ptr() != self.pt[0].data_ptr() + 4 * int(o)
                       for a, o, s in zip(self.pt, self.off, sizes) if s), "the layout came out flat"
        self._put(self.pt, p)
        self.opt = nof.AcceleratedAdamOptimizer(self.sizes, **opts)

    def _put(self, tensors, a):
        import torch

        for t, o, s in zip(tensors, self.off, self.sizes):
            if s:
                t.copy_(torch.from_numpy(np.array(a[o:o + s])))

    def _get(self, tensors):
        return np.concatenate([t.cpu().numpy() for t in tensors]).astype(F32, copy=False)

    def step(self, g, lr):
        import torch

        self._put(self.gt, g)
        torch.cuda.synchronize()
        self.opt.step([t.data_ptr() for t in self.pt], [t.data_ptr() for t in self.gt], lr)
        torch.cuda.synchronize()

    def params(self):
        return self._get(self.pt)

    def moments(self):
        import nof

        m, v, n = self.opt.moments()
        assert n == int(self.off[-1])
        return nof.to_numpy(m, (n,)), nof.to_numpy(v, (n,))


def _rel(a, b):
    return abs(float(a) - b) / abs(b) if b else abs(float(a))


@pytest.mark.parametrize("case", CASES, ids=_ids)
@pytest.mark.parametrize("sizes", LAYOUTS, ids=_ids)
def test_options_match_numpy_and_oracle(gpu, oracle, sizes, case):
    total = sum(sizes)
    p0, gs = _inputs(total, case[4])
    gmn, gmv, wd = _options(case, p0, gs[0])
    run = _Run(gpu, sizes, p0, grad_max_norm=gmn, grad_max_val=gmv, weight_decay_mult=wd)
    assert run.opt.get_options() == dict(grad_max_norm=float(F32(gmn)), grad_max_val=float(F32(gmv)),
                                         weight_decay_mult=float(F32(wd)), stats=False)
    p = np.array(p0)
    m, v = np.zeros(total, F32), np.zeros(total, F32)
    for it, (g, lr) in enumerate(zip(gs, LRS), start=1):
        e = _expect(p, g, gmn, gmv, wd)
        if gmn:  # the regime is unambiguous in fp64 before anything relies on it
            r = e["n2"] / gmn
            assert (r >= 2.0) if "inactive" not in case[0] else (r <= 0.5), r
        run.step(g, lr)
        st = run.opt.stats()
        print(f"{sizes} {case[0]} step {it}: {st}  fp64 " +
              str({k: e[k] for k in ("grad_norm", "grad_norm_clipped", "weight_l2", "clip_scale")}))
        assert st["iteration"] == it
        assert F32(st["grad_abs_max"]) == e["grad_abs_max"]
        for k in ("grad_norm", "grad_norm_clipped", "weight_l2", "clip_scale"):
            assert _rel(st[k], e[k]) <= 1e-5, (k, st[k], e[k])
        if not gmn or "inactive" in case[0]:
            assert st["clip_scale"] == 1.0
        else:
            assert st["clip_scale"] < 0.5
        g3 = e["g2"] * F32(st["clip_scale"])
        assert g3.dtype == F32
        oracle.adam_step(p, np.ascontiguousarray(g3), m, v, lr, it)
        gm, gv = run.moments()
        assert np.array_equal(run.params(), p), f"parameters, step {it}"
        assert np.array_equal(gm, m) and np.array_equal(gv, v), f"moments, step {it}"


@pytest.mark.parametrize("sizes", [(546948,), tuple(NONFLAT)], ids=_ids)
def test_two_runs_are_bit_identical(gpu, sizes):
    total = sum(sizes)
    p0, gs = _inputs(total, 10.0)
    gmn, gmv, wd = _options(CASES[3], p0, gs[0])
    out = []
    for _ in range(2):
        run = _Run(gpu, sizes, p0, grad_max_norm=gmn, grad_max_val=gmv, weight_decay_mult=wd)
        stats = []
        for g, lr in zip(gs, LRS):
            run.step(g, lr)
            stats.append(tuple(np.array(list(run.opt.stats().values()), np.float64).tobytes()))
        out.append((stats, run.params().tobytes(), [a.tobytes() for a in run.moments()]))
    assert out[0] == out[1]


@pytest.mark.parametrize("sizes", [(65,), (524289,), tuple(NONFLAT)], ids=_ids)
def test_flat_and_separate_tensors_agree(gpu, sizes):
    """One virtual arena: the same elements as one flat tensor or cut into separate ones give the same bits."""
    total = sum(sizes)
    p0, gs = _inputs(total, 10.0)
    gmn, gmv, wd = _options(CASES[3], p0, gs[0])
    cut = sizes if len(sizes) > 1 else (total // 3, total - total // 3)
    res = []
    for layout in ((total,), cut):
        run = _Run(gpu, layout, p0, grad_max_norm=gmn, grad_max_val=gmv, weight_decay_mult=wd)
        run.step(gs[0], LRS[0])
        res.append((run.opt.stats(), run.params().tobytes()))
    assert res[0] == res[1]


@pytest.mark.parametrize("sizes", [(257,), (546948,), tuple(NONFLAT)], ids=_ids)
def test_zero_gradient(gpu, sizes):
    total = sum(sizes)
    p0, _ = _inputs(total, 10.0)
    run = _Run(gpu, sizes, p0, grad_max_norm=GMN, grad_max_val=0.25)
    run.step(np.zeros(total, F32), LRS[0])
    st = run.opt.stats()
    assert st["clip_scale"] == 1.0 and st["grad_norm"] == 0.0 and st["grad_abs_max"] == 0.0
    assert st["grad_norm_clipped"] == 0.0
    assert np.array_equal(run.params(), p0)


@pytest.mark.parametrize("mode", ["off", "reset", "stats"])
@pytest.mark.parametrize("sizes", [(65,), (546948,), tuple(NONFLAT)], ids=_ids)
def test_options_off_is_the_plain_step(gpu, sizes, mode):
    """Every option 0 (never set, or set and taken back): the bits of nof_kernel_adam.  stats=True alone gathers
    the record and leaves the update the plain one."""
    import torch

    import nof
    from nof._lib import call

    total = sum(sizes)
    p0, gs = _inputs(total, 10.0)
    run = _Run(gpu, sizes, p0, stats=(mode == "stats"))
    if mode == "reset":
        run.opt.set_options(1.0, 0.5, 3.0, True)
        run.opt.set_options()
    tp, tm, tv = torch.from_numpy(np.array(p0)).to(gpu), torch.zeros(total, device=gpu), torch.zeros(total, device=gpu)
    for it, (g, lr) in enumerate(zip(gs, LRS), start=1):
        run.step(g, lr)
        tg = torch.from_numpy(np.array(g)).to(gpu)
        call("nof_kernel_adam", total, tp.data_ptr(), tg.data_ptr(), tm.data_ptr(), tv.data_ptr(), lr, it, None)
        torch.cuda.synchronize()
        assert np.array_equal(run.params(), tp.cpu().numpy()), f"step {it}"
        gm, gv = run.moments()
        assert np.array_equal(gm, tm.cpu().numpy()) and np.array_equal(gv, tv.cpu().numpy())
        if mode == "stats":
            st = run.opt.stats()
            assert st["clip_scale"] == 1.0 and st["iteration"] == it
            assert F32(st["grad_abs_max"]) == np.max(np.abs(g))
            assert _rel(st["grad_norm"], float(np.linalg.norm(g.astype(np.float64)))) <= 1e-5
            assert st["grad_norm_clipped"] == st["grad_norm"]
    if mode != "stats":
        with pytest.raises(nof.NofError):
            run.opt.stats()


def test_bad_options_and_early_stats_refused(gpu):
    import nof

    opt = nof.AcceleratedAdamOptimizer([4, 4], grad_max_norm=2.0, stats=True)
    with pytest.raises(nof.NofError) as e:  # no step has gathered anything yet
        opt.stats()
    assert e.value.status == 1 and "statistics" in str(e.value)
    for bad in (-1.0, float("nan"), -0.5):
        for k in ("grad_max_norm", "grad_max_val", "weight_decay_mult"):
            with pytest.raises(nof.NofError) as e:
                opt.set_options(**{k: bad})
            assert e.value.status == 1
            with pytest.raises(nof.NofError):
                nof.AcceleratedAdamOptimizer([4], **{k: bad})
    assert opt.get_options() == dict(grad_max_norm=2.0, grad_max_val=0.0, weight_decay_mult=0.0, stats=True)


def test_too_many_separate_tensors_refused(gpu):
    """Separately allocated tensors ride the launch's arguments, 64 at the most; a flat arena has no limit."""
    import torch

    import nof

    n = 65
    ps = [torch.zeros(1, device=gpu) for _ in range(n)]
    gs = [torch.zeros(1, device=gpu) for _ in range(n)]
    opt = nof.AcceleratedAdamOptimizer([1] * n, grad_max_norm=1.0)
    with pytest.raises(nof.NofError):
        opt.step([t.data_ptr() for t in ps], [t.data_ptr() for t in gs], 1e-3)
    arena, grena = torch.zeros(n, device=gpu), torch.ones(n, device=gpu)
    opt.step([arena.data_ptr() + 4 * i for i in range(n)], [grena.data_ptr() + 4 * i for i in range(n)], 1e-3)
    assert abs(opt.stats()["grad_norm"] - np.sqrt(n)) <= 1e-5 * np.sqrt(n)
