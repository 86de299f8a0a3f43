"""A/B of the any-shape path's two precision modes, f32 (generic.hip / gemm_ws.hip) against f16p
(NOF_PRECISION_F16_PRODUCTS, gemm_h.hip), in ONE process: hipEvents around back-to-back get_gradient_device +
Adam steps after a warm-up, the median of several windows, the two models of a network alternating --reps times
in one session (the spread of the repetitions is the noise to hold a difference against).

    python tools/gen_f16p_ab.py                       # the three networks, 4096 rays x 64 + 64
    python tools/gen_f16p_ab.py --nets 8x512 --modes f16p --reps 1 --windows 1   # one model, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d bench_out/prof_f16p -- python tools/gen_f16p_ab.py --nets 8x512 \\
        --modes f16p --reps 1 --windows 1

Networks: 8x512 with a 1x256 view branch; the reference's 8x256 (f32: the fused kernels; f16p: the any-shape
path); BASELINE configs[0]'s 4x128.  Prints one line per network: ms per step of both modes (median over the
repetitions, min .. max) and the ratio.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-or-nothing_amd"))

NETS = {
    "8x512": dict(net_depth=8, net_width=512, net_depth_condition=1, net_width_condition=256),
    "8x256": dict(),
    "4x128": dict(net_depth=4, net_width=128),
}
MODES = {"f32": 0, "f16p": 5}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nets", nargs="+", default=list(NETS), choices=list(NETS))
    p.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    p.add_argument("--rays", type=int, default=4096)
    p.add_argument("--samples", type=int, nargs="+", default=[64, 64])
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
    for net in a.nets:
        models = {}
        for mode in a.modes:
            m = nof.AcceleratedMipNeRF(max_rays=n, num_samples=a.samples, seed=3, precision=MODES[mode], **NETS[net])
            models[mode] = (m, nof.AcceleratedAdamOptimizer(m.GetLayerSizes(), m.config), [0])

        def step(mode):
            m, adam, k = models[mode]
            m.set_rng(3, k[0], 0)
            g = m.get_gradient_device(n, r["o"], r["d"], r["radius"], r["near"], r["far"], r["lossmult"], r["pix"],
                                      float(n))
            adam.step(m.mlp.allParams, g, nof.learning_rate_decay(k[0] + 1))
            k[0] += 1

        ms = {mode: [] for mode in a.modes}
        for mode in a.modes:
            for _ in range(a.warmup):
                step(mode)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for mode in a.modes:
                win = []
                for _ in range(a.windows):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        step(mode)
                    e1.record()
                    e1.synchronize()
                    win.append(e0.elapsed_time(e1) / a.steps)
                ms[mode].append(float(np.median(win)))
        parts = []
        for mode in a.modes:
            m = models[mode][0]
            parts.append(f"{mode} {np.median(ms[mode]):.3f} ms/step ({min(ms[mode]):.3f} .. {max(ms[mode]):.3f}), "
                         f"loss {m.loss():.5f}, numeric {m.numeric_status()}")
        line = f"{net} {n} rays x {'+'.join(map(str, a.samples))}: " + "; ".join(parts)
        if len(a.modes) == 2:
            line += f"; f32 / f16p = {np.median(ms['f32']) / np.median(ms['f16p']):.2f}"
        print(line, flush=True)
        for m, adam, _ in models.values():
            adam.close()
            m.close()


if __name__ == "__main__":
    main()
