"""Bitwise A/B of two library builds: the same training steps, every output compared bit for bit.

    NOF_LIB=<lib A> python tools/ab_bits.py gpurun_out/a.npz
    NOF_LIB=<lib B> python tools/ab_bits.py gpurun_out/b.npz
    python tools/ab_bits.py --compare gpurun_out/a.npz gpurun_out/b.npz

Each run: for every precision mode, a config-2-shaped model (1024 rays x 128+128, and a 64+128 model for
the unequal-levels path) takes two training steps (get_gradient_device + Adam) on fixed synthetic batches;
the gradient arena, every level's per-ray outputs and adjoints, the loss and the parameters after Adam are
saved.  Then the any-shape path the same way: every network of GEN_SPECS (tests/test_gpu_generic.py's table)
in modes 0 and 5 at that file's sizes, 8 rays x 64+128 and, for the specs it runs with 128 rays or more, 128
rays x 64+64 (the view PE's weight gradient split as well), and one network with stop_level_grad = 0: between
them every k_gemm and k_gemm_h pick.  A refactoring that claims "same arithmetic" must compare equal here.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-or-nothing_amd"))


# tests/test_gpu_generic.py SPECS: (D, W, Dc, Wc, skip, min_deg, max_deg, deg_view)
GEN_SPECS = {
    "configs0_4x128": (4, 128, 1, 128, 4, 0, 16, 4),
    "odd_5x96_3x40": (5, 96, 3, 40, 2, 2, 10, 2),
    "tiny_2x32_skip1": (2, 32, 1, 16, 1, 0, 4, 1),
    "deep_10x64": (10, 64, 2, 32, 3, 0, 12, 0),
    "wide_3x272_2x136": (3, 272, 2, 136, 2, 0, 5, 1),
    "unaligned_2x50_1x30": (2, 50, 1, 30, 1, 0, 4, 1),
    "skip_overflow_5x128": (5, 128, 1, 128, 4, 0, 16, 2),
    "nt7_nt5": (3, 112, 2, 80, 2, 1, 5, 1),
    "nt8_runtime": (2, 120, 1, 72, 1, 0, 4, 0),
    "grid_2x30_1x14": (2, 30, 1, 14, 1, 0, 4, 1),
}
GEN_MANY_RAYS = ("configs0_4x128", "tiny_2x32_skip1", "grid_2x30_1x14")  # its DISPATCH entries with MANY_RAYS
GEN_CROSS = "odd_5x96_3x40"  # stop_level_grad = 0: three contributing layers (a two-source product and the part sum)


def cases():
    """(tag, rays, AcceleratedMipNeRF keywords) of every model"""
    for prec in (0, 1, 2, 3, 4):
        for samples in ((128, 128), (64, 128)):
            yield f"p{prec}_s{samples[0]}", 1024, dict(num_samples=samples, precision=prec)
    for name, (D, W, Dc, Wc, skip, lo, hi, dv) in GEN_SPECS.items():
        net = dict(net_depth=D, net_width=W, net_depth_condition=Dc, net_width_condition=Wc, skip_layer=skip,
                   min_deg_point=lo, max_deg_point=hi, deg_view=dv)
        for prec in (0, 5):
            yield f"gen_{name}_p{prec}", 8, dict(num_samples=(64, 128), precision=prec, **net)
            if name in GEN_MANY_RAYS:
                yield f"gen_{name}_p{prec}_r128", 128, dict(num_samples=(64, 64), precision=prec, **net)
            if name == GEN_CROSS:
                yield f"gen_{name}_p{prec}_cross", 8, dict(num_samples=(64, 128), precision=prec, stop_level_grad=0, **net)


def run(out):
    import torch

    import nof
    from nof import synth

    dev = torch.device("cuda", 0)
    res = {}
    for tag, n, kw in cases():
        model = nof.AcceleratedMipNeRF(seed=11, max_rays=n, **kw)
        P = model.mlp.flat_params()[1]
        opt = nof.AcceleratedAdamOptimizer(model.GetLayerSizes(), model.config)
        for step in range(2):
            r = synth.blender_rays(n, seed=100 + step)
            d = {k: torch.from_numpy(v).to(dev) for k, v in r.items()}
            model.set_rng(0x5EED0A0B, step, 0)
            grads = model.get_gradient_device(n, d["o"], d["d"], d["radius"], d["near"], d["far"], d["lossmult"],
                                              d["pix"], float(np.sum(r["lossmult"], dtype=np.float32)))
            torch.cuda.synchronize()
            G = nof.to_numpy(model.mlp.flat_grads()[0], (P,)).copy()
            res[f"{tag}_grads{step}"] = G
            res[f"{tag}_loss{step}"] = np.float32(model.loss())
            for l in range(2):
                lv = model.level_numpy(l)
                for k in ("t", "weights", "comp_rgb", "density_grad", "rgb_grad"):
                    res[f"{tag}_{k}{l}_{step}"] = lv[k].copy()
            opt.step(model.mlp.allParams, grads, nof.learning_rate_decay(step + 1))
            torch.cuda.synchronize()
        res[f"{tag}_params"] = nof.to_numpy(model.mlp.flat_params()[0], (P,)).copy()
        model.close()
    np.savez(out, **res)
    print(f"{out}: {len(res)} arrays")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = [k for k in A.files if k not in B.files or A[k].tobytes() != B[k].tobytes()]
    for k in bad[:20]:
        x, y = A[k].astype(np.float64), B[k].astype(np.float64)
        print(f"DIFF {k}: rel L2 {np.linalg.norm(x - y) / max(np.linalg.norm(x), 1e-300):.3g}")
    for block, gen in (("fused 8x256", False), ("any-shape", True)):
        keys = [k for k in A.files if k.startswith("gen_") == gen]
        print(f"{block}: {len(keys) - len([k for k in bad if k in keys])} / {len(keys)} arrays bitwise equal")
    return not bad


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    run(sys.argv[1])
