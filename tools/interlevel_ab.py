"""What nof_mipnerf_set_interlevel_loss costs, in ONE process, in the style of tools/raygrad_ab.py:
hipEvents around back-to-back get_gradient_device + Adam steps after a warm-up, the median of several windows,
lambda_p = 0 and > 0 alternating --reps times; then k_interlevel alone (nof_kernel_interlevel).

    python tools/interlevel_ab.py          # config 2 (8x256, 1024 x 128+128) in f16; configs[0] (4x128, 4096 x 64+64)
                                           # in f32 at stop_level_grad 1 and 0; the kernel at 1024 x (128, 128) and
                                           # 4096 x (64, 64)

bench.py runs none of this code: it never calls the setter.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-or-nothing_amd"))

# (label, rays, samples, model keywords)
STEPS = [
    ("f16 8x256 (config 2)", 1024, (128, 128), dict(precision=4)),
    ("f32 4x128 (configs[0]) stop_level_grad 1", 4096, (64, 64), dict(precision=0, net_depth=4, net_width=128)),
    ("f32 4x128 (configs[0]) stop_level_grad 0", 4096, (64, 64),
     dict(precision=0, net_depth=4, net_width=128, stop_level_grad=0)),
]
KERNEL = [(1024, 128, 128), (4096, 64, 64)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mult", type=float, default=1.0)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--steps", type=int, default=5, help="steps per window")
    p.add_argument("--warmup", type=int, default=3)
    a = p.parse_args()
    import torch
    import nof
    from nof import synth

    dev = torch.device("cuda", 0)
    for label, n, samples, kw in STEPS:
        r = {k: torch.from_numpy(v).to(dev) for k, v in synth.blender_rays(n, seed=1).items()}
        models = {}
        for on in (0, 1):
            m = nof.AcceleratedMipNeRF(max_rays=n, num_samples=samples, seed=3, **kw)
            m.set_interlevel_loss(a.mult if on else 0.0)
            models[on] = (m, nof.AcceleratedAdamOptimizer(m.GetLayerSizes(), m.config), [0])

        def step(on):
            m, adam, k = models[on]
            m.set_rng(3, k[0], 0)
            g = m.get_gradient_device(n, r["o"], r["d"], r["radius"], r["near"], r["far"], r["lossmult"], r["pix"],
                                      float(n))
            adam.step(m.mlp.allParams, g, nof.learning_rate_decay(k[0] + 1))
            k[0] += 1

        ms = {0: [], 1: []}
        for on in (0, 1):
            for _ in range(a.warmup):
                step(on)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for on in (0, 1):
                win = []
                for _ in range(a.windows):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        step(on)
                    e1.record()
                    e1.synchronize()
                    win.append(e0.elapsed_time(e1) / a.steps)
                ms[on].append(float(np.median(win)))
        parts = [f"lambda_p {a.mult if s else 0:g}: {np.median(ms[s]):.3f} ms/step ({min(ms[s]):.3f} .. {max(ms[s]):.3f}), "
                 f"loss {models[s][0].loss():.5f}" for s in (0, 1)]
        print(f"{label}, {n} rays x {'+'.join(map(str, samples))}: " + "; ".join(parts) +
              f"; term {models[1][0].interlevel_loss():.3g}; on / off = {np.median(ms[1]) / np.median(ms[0]):.3f}",
              flush=True)
        for m, adam, _ in models.values():
            adam.close()
            m.close()

    # the kernel alone: sorted random edges, random weights (about every fifth hinge active)
    for n, Sc, Sf in KERNEL:
        tp = torch.sort(2.0 + 4.0 * torch.rand((n, Sc + 1), device=dev), dim=1).values.contiguous()
        t = torch.sort(2.0 + 4.0 * torch.rand((n, Sf + 1), device=dev), dim=1).values.contiguous()
        wp = torch.rand((n, Sc), device=dev) / Sc
        w = 2.5 * torch.rand((n, Sf), device=dev) / Sf
        lm = torch.ones((n,), device=dev)
        q, rays = torch.zeros((n, Sc), device=dev), torch.zeros((n,), device=dev)

        def launch():
            nof.kernel_interlevel(n, Sc, tp, wp, Sf, t, w, lm, float(n), 1.0, q, rays)

        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                launch()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) / 20 * 1e3)
        nbytes = 4 * n * (3 * Sc + 2 * Sf + 4)
        print(f"k_interlevel {n} rays x ({Sc}, {Sf}): {np.median(us):.1f} us ({min(us):.1f} .. {max(us):.1f}), "
              f"{nbytes / 1e6:.2f} MB moved, term {float(rays.sum()):.3g}", flush=True)


if __name__ == "__main__":
    main()
