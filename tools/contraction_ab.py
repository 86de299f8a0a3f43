"""What nof_mipnerf_set_contraction costs, in ONE process, in the style of tools/raygrad_ab.py: hipEvents
around back-to-back get_gradient_device + Adam steps after a warm-up, the median of several windows, the option off and
on alternating --reps times on one model (the setter allocates nothing and holds from the next call); then the same
alternation with the library's mlp_fwd timer on (id 2: it brackets cast + encode and the layer GEMMs of every level);
then k_cast next to k_cast_contract alone at one level's shape (nof_kernel_cast_contract).

    python tools/contraction_ab.py          # configs[0]: 4x128, 4096 rays x 64 + 64, f32

bench.py runs none of this code: its flagship is the fused 8x256 step, which has no contraction.
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
    p.add_argument("--modes", nargs="+", default=["f32"], choices=list(MODES))
    p.add_argument("--rays", type=int, default=4096)
    p.add_argument("--samples", type=int, nargs="+", default=[64, 64])
    p.add_argument("--depth", type=int, default=4)
    p.add_argument("--width", type=int, default=128)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--steps", type=int, default=5, help="steps per window")
    p.add_argument("--warmup", type=int, default=3)
    a = p.parse_args()
    import torch
    import nof
    from nof import synth

    dev = torch.device("cuda", 0)
    n = a.rays
    r = {k: torch.from_numpy(v).to(dev) for k, v in synth.blender_rays(n, seed=1).items()}
    for mode in a.modes:
        m = nof.AcceleratedMipNeRF(max_rays=n, num_samples=a.samples, seed=3, precision=MODES[mode], net_depth=a.depth,
                                   net_width=a.width)
        adam = nof.AcceleratedAdamOptimizer(m.GetLayerSizes(), m.config)
        k = [0]

        def step():
            m.set_rng(3, k[0], 0)
            g = m.get_gradient_device(n, r["o"], r["d"], r["radius"], r["near"], r["far"], r["lossmult"], r["pix"], float(n))
            adam.step(m.mlp.allParams, g, nof.learning_rate_decay(k[0] + 1))
            k[0] += 1

        for on in (0, 1):
            m.set_contraction(on)
            for _ in range(a.warmup):
                step()
        torch.cuda.synchronize()
        ms = {0: [], 1: []}
        for _ in range(a.reps):
            for on in (0, 1):
                m.set_contraction(on)
                win = []
                for _ in range(a.windows):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        step()
                    e1.record()
                    e1.synchronize()
                    win.append(e0.elapsed_time(e1) / a.steps)
                ms[on].append(float(np.median(win)))
        shape = f"{mode} {a.depth}x{a.width} {n} rays x {'+'.join(map(str, a.samples))}"
        print(f"{shape}: " + "; ".join(f"contraction {'on' if s else 'off'}: {np.median(ms[s]):.3f} ms/step "
                                       f"({min(ms[s]):.3f} .. {max(ms[s]):.3f})" for s in (0, 1))
              + f"; on / off = {np.median(ms[1]) / np.median(ms[0]):.4f}", flush=True)
        # the mlp_fwd timer alone (its events cost time of their own: a pass of its own)
        m.enable_timing(True, timers=["mlp_fwd"])
        fw = {0: [], 1: []}
        for _ in range(a.reps):
            for on in (0, 1):
                m.set_contraction(on)
                m.read_timing()  # (clears)
                for _ in range(a.windows * a.steps):
                    step()
                torch.cuda.synchronize()
                t, _ = m.read_timing()["mlp_fwd"]
                fw[on].append(t / (a.windows * a.steps))
        m.enable_timing(False)
        print(f"{shape}: mlp_fwd timer per step, " + "; ".join(
            f"contraction {'on' if s else 'off'}: {np.median(fw[s]) * 1e3:.1f} us ({min(fw[s]) * 1e3:.1f} .. "
            f"{max(fw[s]) * 1e3:.1f})" for s in (0, 1)) + f"; on - off = {(np.median(fw[1]) - np.median(fw[0])) * 1e3:.1f} us",
              flush=True)
        adam.close()
        m.close()

    # the two cast kernels alone, one level of the shape above
    S = a.samples[-1]
    t = torch.sort(2.0 + 4.0 * torch.rand((n, S + 1), device=dev), dim=1).values.contiguous()
    mean, cov = torch.zeros((n, S, 3), device=dev), torch.zeros((n, S, 3), device=dev)
    med = {}
    for on in (0, 1, 0, 1):
        launch = lambda: nof._lib.call("nof_kernel_cast_contract", n, S, t.data_ptr(), r["o"].data_ptr(), r["d"].data_ptr(),
                                       r["radius"].data_ptr(), mean.data_ptr(), cov.data_ptr(), None, 0, on)
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
        med.setdefault(on, []).append(float(np.median(us)))
        nbytes = n * S * 24 + n * (S + 1) * 4 + n * 28
        print(f"{'k_cast_contract' if on else 'k_cast'} {n} rays x {S}: {np.median(us):.1f} us ({min(us):.1f} .. "
              f"{max(us):.1f}) back to back, {nbytes / 1e6:.1f} MB", flush=True)
    print(f"k_cast_contract / k_cast = {np.median(med[1]) / np.median(med[0]):.3f}", flush=True)


if __name__ == "__main__":
    main()
