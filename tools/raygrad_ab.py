"""What nof_mipnerf_set_ray_grad costs, in ONE process, in the style of tools/crosslevel_ab.py:
hipEvents around back-to-back get_gradient_device + Adam steps after a warm-up, the median of several windows, the
option off and on alternating --reps times; then k_ray_grad alone (nof_kernel_ray_grad) next to k_encode_grad alone
(nof_kernel_encode_grad) at the same shape: the two stream the same 2 M P 4 bytes of enc and dEnc.

    python tools/raygrad_ab.py          # configs[0]: 4x128, 4096 rays x 64 + 64, f32 and f16p

bench.py runs none of this code: its flagship is the fused 8x256 step, which has no ray gradients.
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
    p.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
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
        models = {}
        for on in (0, 1):
            m = nof.AcceleratedMipNeRF(max_rays=n, num_samples=a.samples, seed=3, precision=MODES[mode],
                                       net_depth=a.depth, net_width=a.width)
            m.set_ray_grad(bool(on))
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
        parts = [f"ray_grad {'on' if s else 'off'}: {np.median(ms[s]):.3f} ms/step ({min(ms[s]):.3f} .. {max(ms[s]):.3f}), "
                 f"loss {models[s][0].loss():.5f}" for s in (0, 1)]
        print(f"{mode} {a.depth}x{a.width} {n} rays x {'+'.join(map(str, a.samples))}: " + "; ".join(parts) +
              f"; on / off = {np.median(ms[1]) / np.median(ms[0]):.3f}", flush=True)
        for m, adam, _ in models.values():
            adam.close()
            m.close()

    # the two adjoint kernels alone: PE (0, 16), one level of the shape above
    S, P = a.samples[-1], 96
    M = n * S
    t = torch.sort(2.0 + 4.0 * torch.rand((n, S + 1), device=dev), dim=1).values.contiguous()
    enc = torch.rand((M, P), device=dev) - 0.5
    denc = torch.rand((M, P), device=dev) - 0.5
    sig, dsig = torch.rand((M,), device=dev), torch.rand((M,), device=dev) - 0.5
    ed, dd = torch.rand((n, 27), device=dev) - 0.5, torch.rand((n, 27), device=dev) - 0.5
    tg = torch.zeros((n, S + 1), device=dev)
    og, dg = torch.zeros((n, 3), device=dev), torch.zeros((n, 3), device=dev)
    rays = (t.data_ptr(), r["o"].data_ptr(), r["d"].data_ptr(), r["radius"].data_ptr(), 0, 0, 16, enc.data_ptr(),
            denc.data_ptr())

    def encode_grad():
        nof._lib.call("nof_kernel_encode_grad", n, S, *rays, tg.data_ptr(), None)

    def ray_grad():
        nof._lib.call("nof_kernel_ray_grad", n, S, *rays, sig.data_ptr(), dsig.data_ptr(), 4, ed.data_ptr(),
                      dd.data_ptr(), 0, og.data_ptr(), dg.data_ptr(), None)

    med = {}
    for name, launch, extra in (("k_encode_grad", encode_grad, 2 * n * (S + 1) * 4 + n * 7 * 4),
                                ("k_ray_grad", ray_grad, n * (S + 1) * 4 + 2 * M * 4 + n * (7 + 2 * 27 + 6) * 4)):
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
        nbytes = 2 * M * P * 4 + extra
        med[name] = float(np.median(us))
        print(f"{name} {n} rays x {S}, P = {P}: {med[name]:.1f} us ({min(us):.1f} .. {max(us):.1f}), "
              f"{nbytes / 1e6:.1f} MB, {nbytes / med[name] / 1e6:.2f} TB/s", flush=True)
    print(f"k_ray_grad / k_encode_grad = {med['k_ray_grad'] / med['k_encode_grad']:.3f}", flush=True)


if __name__ == "__main__":
    main()
