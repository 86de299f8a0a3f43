"""What per-view appearance embeddings cost, in ONE process, in the style of tools/contraction_ab.py:
hipEvents around back-to-back get_gradient_device + Adam steps after a warm-up, the median of several windows, a model
without the option (G = 0) and one with it (G = --dim, V = --views, its table stepped by a second Adam) alternating
--reps times; then the two new kernels alone at the step's shape (nof_kernel_appearance_gather / _grad).

    python tools/appearance_ab.py --modes f32 f16p     # configs[0]: 4x128, 4096 rays x 64 + 64; G = 32, V = 100

bench.py runs none of this code: its flagship is the fused 8x256 step, which has no appearance embeddings.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-or-nothing_amd"))

MODES = {"f32": 0, "f16p": 5}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--modes", nargs="+", default=["f32", "f16p"], choices=list(MODES))
    p.add_argument("--rays", type=int, default=4096)
    p.add_argument("--samples", type=int, nargs="+", default=[64, 64])
    p.add_argument("--depth", type=int, default=4)
    p.add_argument("--width", type=int, default=128)
    p.add_argument("--dim", type=int, default=32)
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--steps", type=int, default=5, help="steps per window")
    p.add_argument("--warmup", type=int, default=3)
    a = p.parse_args()
    import torch
    import nof
    from nof import synth

    dev = torch.device("cuda", 0)
    n, G, V = a.rays, a.dim, a.views
    r = {k: torch.from_numpy(v).to(dev) for k, v in synth.blender_rays(n, seed=1).items()}
    ids = torch.from_numpy(np.random.default_rng(0).integers(0, V, n).astype(np.int32)).to(dev)
    for mode in a.modes:
        steps = {}
        keep = []
        for on in (0, 1):
            m = nof.AcceleratedMipNeRF(max_rays=n, num_samples=a.samples, seed=3, precision=MODES[mode],
                                       net_depth=a.depth, net_width=a.width, appearance_views=V if on else 0,
                                       appearance_dim=G if on else 0)
            adam = nof.AcceleratedAdamOptimizer(m.GetLayerSizes(), m.config)
            app = None
            if on:
                tp, gp, _, _ = m.appearance()
                app = (nof.AcceleratedAdamOptimizer([V * G], m.config), [tp], [gp])
            k = [0]

            def step(m=m, adam=adam, app=app, k=k):
                m.set_rng(3, k[0], 0)
                if app:
                    m.set_ray_views(ids)
                g = m.get_gradient_device(n, r["o"], r["d"], r["radius"], r["near"], r["far"], r["lossmult"], r["pix"],
                                          float(n))
                adam.step(m.mlp.allParams, g, nof.learning_rate_decay(k[0] + 1))
                if app:
                    app[0].step(app[1], app[2], 1e-3)
                k[0] += 1

            for _ in range(a.warmup):
                step()
            steps[on] = step
            keep.append((m, adam, app))
        torch.cuda.synchronize()
        ms = {0: [], 1: []}
        for _ in range(a.reps):
            for on in (0, 1):
                win = []
                for _ in range(a.windows):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        steps[on]()
                    e1.record()
                    e1.synchronize()
                    win.append(e0.elapsed_time(e1) / a.steps)
                ms[on].append(float(np.median(win)))
        shape = f"{mode} {a.depth}x{a.width} {n} rays x {'+'.join(map(str, a.samples))}"
        print(f"{shape}: " + "; ".join(f"G = {G if s else 0}: {np.median(ms[s]):.3f} ms/step ({min(ms[s]):.3f} .. "
                                       f"{max(ms[s]):.3f})" for s in (0, 1))
              + f"; on / off = {np.median(ms[1]) / np.median(ms[0]):.4f}, on - off = "
              f"{(np.median(ms[1]) - np.median(ms[0])) * 1e3:.1f} us over {len(a.samples)} levels", flush=True)
        for m, adam, app in keep:
            if app:
                app[0].close()
            adam.close()
            m.close()

    # the two kernels alone, one level of the shape above (Vd = 27: deg_view 4)
    Vd = 27
    ed = torch.randn((n, Vd), device=dev)
    E = torch.randn((V, G), device=dev)
    out = torch.zeros((n, Vd + G), device=dev)
    dapp = torch.randn((n, G), device=dev)
    dE = torch.zeros((V, G), device=dev)
    launches = {
        "k_appearance_gather": (lambda: nof._lib.call("nof_kernel_appearance_gather", n, Vd, G, V, ed.data_ptr(),
                                                      E.data_ptr(), ids.data_ptr(), -1, out.data_ptr(), None),
                                n * (2 * Vd + 2 * G + 1) * 4),
        "k_appearance_grad": (lambda: nof._lib.call("nof_kernel_appearance_grad", n, G, V, ids.data_ptr(),
                                                    dapp.data_ptr(), dE.data_ptr(), 0, None),
                              n * G * 4 + V * ((G + 7) // 8) * n * 4 + V * G * 4),
    }
    for name, (launch, nbytes) in launches.items():
        meds = []
        for _ in range(a.reps):
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
            meds.append(float(np.median(us)))
        print(f"{name} {n} rays, G = {G}, V = {V}: {np.median(meds):.1f} us ({min(meds):.1f} .. {max(meds):.1f}) back "
              f"to back, {nbytes / 1e6:.2f} MB read + written (the gradient's id scans included)", flush=True)


if __name__ == "__main__":
    main()
