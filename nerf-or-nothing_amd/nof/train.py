"""Training driver: Program.Train / TrainStep (Program.cs:21-62) on the device
data path, with the checkpointing the reference declares (Config.SaveEvery, TrainState.cs:59) but
never implements.

    python -m nof.train --records train_data.bin --steps 1000 [--ckpt-dir ck --save-every 500 --resume]
    python -m nof.train --synthetic 100000 --steps 200          (Lego-shaped synthetic records)
    python -m nof.train --scene scene.npz --num-scales 4        (poses + images, rays made per batch)
    python -m nof.train --scene scene.npz --holdout 8 --eval-every 10000 [--eval-dir renders]
                                                                (every 8th view held out, rendered and scored)
    python -m nof.train --scene scene.npz --refine-poses 1e-3 --precision f16p
                                                                (the scene's poses refined jointly with the field)
    python -m nof.train --scene scene.npz --contract --lindisp --precision f16p
                                                                (an unbounded scene: space contracted into a ball)
    python -m nof.train --scene scene.npz --appearance-dim 32 --precision f16p
                                                                (a learned appearance vector per training image)

One step = dataset batch (device gather) -> AcceleratedMipNeRF.get_gradient_device (fused loss
gradient) -> [all-reduce of the gradient arena when torch.distributed is initialised] ->
AcceleratedAdamOptimizer.step(lr = LearningRateDecay(step)).  Every `print_every` steps the fine
level's loss is printed as Program.LossFn does (Program.cs:64).
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np

from . import api
from ._lib import PRECISION_NAMES, NofError, default_config


class Trainer:
    def __init__(self, dataset: api.RayDataset, batch_size: int = 1024, seed: int = 0x5EED0000, device: int = 0,
                 stream=None, print_every: int = 100, save_every: int = 0, ckpt_dir: str | None = None,
                 sync_check_every: int = 0, lr_init=5e-4, lr_final=5e-6, max_steps=1000000, lr_delay_steps=2500, lr_delay_mult=0.01,
                 grad_max_norm: float = 0.0, grad_max_val: float = 0.0, weight_decay_mult: float = 0.0,
                 stats: bool = False, refine_poses: float = 0.0, interlevel_loss_mult: float = 0.0,
                 contract: bool = False, appearance_dim: int = 0, appearance_lr: float = 1e-3, **config):
        import torch.distributed as dist

        self.dist = dist if dist.is_available() and dist.is_initialized() else None
        self.rank = self.dist.get_rank() if self.dist else 0
        self.world = self.dist.get_world_size() if self.dist else 1
        self.ds = dataset
        self.n = batch_size
        self.seed = seed
        self.stream = stream
        self.print_every, self.save_every, self.ckpt_dir = print_every, save_every, ckpt_dir
        self.sync_check_every = sync_check_every  # data parallel: parameter checksum across ranks
        self.lr = dict(lr_init=lr_init, lr_final=lr_final, max_steps=max_steps, lr_delay_steps=lr_delay_steps,
                       lr_delay_mult=lr_delay_mult)
        self.cfg = default_config(device=device, max_rays=batch_size, seed=seed, stream=stream, **config)
        # per-view appearance embeddings: one table row per view of the training dataset.  Refused
        # here, before training, with the library's message: by a dataset without views (a batch's views are asked
        # for once) and, at the model's creation, by a fused 8x256 precision
        self.appearance_dim, self.appearance_lr = int(appearance_dim), float(appearance_lr)
        app_views = 0
        if self.appearance_dim:
            dataset.next(batch_size, seed, 0, 0, stream, with_sum=False)
            self.view_ids = dataset.batch_views(batch_size, stream=stream)
            app_views = dataset.scene_info()["num_views"]
        self.model = api.AcceleratedMipNeRF(self.cfg, appearance_views=app_views, appearance_dim=self.appearance_dim)
        self.app_adam = None
        if self.appearance_dim:  # the table is the caller's to step: a second optimizer over its V * G floats
            self.app_table, self.app_grad, V, G = self.model.appearance()
            self.app_adam = api.AcceleratedAdamOptimizer([V * G], self.cfg)
        # Config.GradMaxNorm / GradMaxVal / WeightDecayMult (TrainState.cs:58-59,70): hyper-parameters, not
        # checkpoint state, so a resumed run passes them again
        self.adam = api.AcceleratedAdamOptimizer(self.model.GetLayerSizes(), self.cfg, grad_max_norm=grad_max_norm,
                                                 grad_max_val=grad_max_val, weight_decay_mult=weight_decay_mult,
                                                 stats=stats)
        self.with_stats = bool(stats or grad_max_norm or grad_max_val or weight_decay_mult)
        self.last_stats = None  # the optimizer's record of the last print step (with_stats)
        self.params = self.model.mlp.allParams
        self.step_idx = 0  # completed steps (Program.cs counts from 1)
        self.device = device
        self.last_loss = None
        self.last_distortion = None  # the distortion term of the last print step (distortion_loss_mult > 0)
        # the interlevel (proposal) loss: a setter, not a config field; every rank's model gets it
        self.interlevel_loss_mult = float(interlevel_loss_mult)
        self.last_interlevel = None  # its term of the last print step
        if self.interlevel_loss_mult:
            self.model.set_interlevel_loss(self.interlevel_loss_mult)
        # scene contraction: a setter as well; refused here, before training, by a fused 8x256 precision
        if contract:
            self.model.set_contraction(1)
        # data parallel: the gradient arena is all-reduced bucket by bucket on a communication
        # stream ordered after the library's stream (self.stream, which may be any stream), and the
        # library's stream waits for the last bucket before Adam (nof.dp.BucketedAllReduce)
        self._allreduce = None
        if self.dist is not None:
            from .dp import BucketedAllReduce

            self._allreduce = BucketedAllReduce(self.model, f"cuda:{device}")
        # camera refinement: refused here, before training, with the library's message, by a model
        # without ray gradients (a fused 8x256 precision) and by a dataset without pose gradients (NDC, records)
        self.refiner = None
        if refine_poses:
            self.model.set_ray_grad(True)
            self.refiner = PoseRefiner(dataset, batch_size, refine_poses, seed, device, stream)

    # --- checkpoints -----------------------------------------------------------------------------
    def save(self, path):
        api.save_checkpoint(path, self.model, self.adam)

    def resume(self, path):
        api.load_checkpoint(path, self.model, self.adam)
        self.step_idx = self.adam.iteration

    # --- one TrainStep (Program.cs:48-62) ---------------------------------------------------------
    def step(self):
        import torch

        step = self.step_idx + 1
        ray_base = self.rank * self.n  # global ray ids: shards draw what the whole batch would
        b, msum = self.ds.next(self.n, self.seed, step, ray_base, self.stream)
        if self.dist is not None:  # global loss-multiplier sum (D14 / SURVEY 8e)
            t = torch.tensor([msum], dtype=torch.float64, device=f"cuda:{self.device}")
            self.dist.all_reduce(t)
            msum = float(t.item())
        self.model.set_rng(self.seed, step, ray_base)
        p = {k: v[0] for k, v in b.items()}
        if self.app_adam is not None:  # this batch's view ids, for this step alone
            self.ds.batch_views(self.n, out=self.view_ids, stream=self.stream)
            self.model.set_ray_views(self.view_ids)
        grads = self.model.get_gradient_device(self.n, p["o"], p["d"], p["radius"], p["near"], p["far"],
                                               p["lossmult"], p["pix"], msum)
        self.adam.step(self.params, grads, api.learning_rate_decay(step, **self.lr))
        if self.app_adam is not None:
            if self.dist is not None:  # every rank's shard of the batch (the table is outside the gradient arena)
                V, G = self.model.appearance()[2:]
                api.call("nof_stream_sync", self.stream)
                self.dist.all_reduce(api.device_tensor(self.app_grad, (V, G),
                                                       device=torch.device("cuda", self.device)))
            self.app_adam.step([self.app_table], [self.app_grad], self.appearance_lr)
        if self.refiner is not None:  # this batch's pose gradient; the corrected poses make the next batch's rays
            self.refiner.step(self.model, self.n, self.dist)
        self.step_idx = step
        if self.print_every and step % self.print_every == 0:
            bad = self.model.numeric_status(clear=True)
            if self.dist is not None:  # every rank raises together (a lone raise would hang its peers)
                t = torch.tensor([bad], dtype=torch.int64, device=f"cuda:{self.device}")
                self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
                bad = int(t.item())
            if bad:  # e.g. fp16 activation overflow in the f16x2 perf mode: fail loudly, not silently
                raise FloatingPointError(f"step {step}: non-finite values in the training step on some rank "
                                         f"(flags {bad:#x}; 1 = forward outputs, 2 = output gradients)")
            self.last_loss = self.fine_loss(b)
            line = f"Step {step}/{self.lr['max_steps']}, Loss: {self.last_loss}"
            if self.cfg.distortion_loss_mult > 0:  # this rank's term, lambda_d sum mu L / sum mu (global sum mu)
                self.last_distortion = self.model.distortion_loss()
                line += f", Distortion: {self.last_distortion:.9g}"
            if self.interlevel_loss_mult > 0:  # this rank's term as well (over the global sum mu: the ranks' add up)
                self.last_interlevel = self.model.interlevel_loss()
                line += f", Interlevel: {self.last_interlevel:.9g}"
            if self.with_stats:  # StatsUtil.cs:13,16-18, of the all-reduced gradient (identical on every rank)
                self.last_stats = st = self.adam.stats()
                line += (f", grad_norm: {st['grad_norm']:.9g}, grad_abs_max: {st['grad_abs_max']:.9g}, "
                         f"grad_norm_clipped: {st['grad_norm_clipped']:.9g}, weight_l2: {st['weight_l2']:.9g}")
            if self.rank == 0:
                print(line, flush=True)
        if self.dist is not None and self.sync_check_every and step % self.sync_check_every == 0:
            self.check_sync()
        if self.save_every and self.ckpt_dir and step % self.save_every == 0 and self.rank == 0:
            os.makedirs(self.ckpt_dir, exist_ok=True)
            self.save(os.path.join(self.ckpt_dir, f"ckpt_{step:08d}.nof"))
            self.save_poses()
            self.save_appearance()

    def appearance(self) -> np.ndarray:
        """--appearance-dim: the appearance table [V, G] (host copy)"""
        api.call("nof_stream_sync", self.stream)
        t, _, V, G = self.model.appearance()
        return api.to_numpy(t, (V, G))

    def save_appearance(self):
        """--appearance-dim: the table as appearance.npy, wherever poses_refined.npy goes (a checkpoint does not hold
        it)"""
        if self.app_adam is None or self.rank != 0:
            return
        d = self.ckpt_dir or "."
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "appearance.npy"), self.appearance())

    def save_poses(self):
        """--refine-poses: the refined pose table [V, 12] as poses_refined.npy next to the checkpoints (a checkpoint
        does not hold poses)"""
        if self.refiner is None or self.rank != 0:
            return
        d = self.ckpt_dir or "."
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "poses_refined.npy"), self.refiner.poses())

    def check_sync(self):
        """SURVEY §8e's periodic assertion: every rank's parameters are bitwise identical (a rank that
        diverged — a missed all-reduce, a different Adam step — fails here instead of training on)."""
        import torch

        from .dp import params_in_sync

        api.call("nof_stream_sync", self.stream)  # Adam ran on self.stream
        pptr, P = self.model.mlp.flat_params()
        flat = api.device_tensor(pptr, (P,), device=torch.device("cuda", self.device))
        if not params_in_sync(flat):
            raise RuntimeError(f"step {self.step_idx}: parameters differ across the {self.world} ranks")

    def fine_loss(self, batch) -> float:
        """Program.LossFn (Program.cs:64): sum m |C_fine - p|^2 / sum m over this rank's batch."""
        api.call("nof_stream_sync", self.stream)  # the reads below are not ordered after self.stream
        L = self.cfg.num_levels
        C = self.model.level_numpy(L - 1)["comp_rgb"]
        pix = api.to_numpy(batch["pix"][0], (self.n, 3))
        m = api.to_numpy(batch["lossmult"][0], (self.n,))
        return float(np.sum(m * np.sum((C - pix) ** 2, axis=1)) / np.sum(m))

    def train(self, steps: int):
        for _ in range(steps):
            self.step()
        return self

    # --- the test split ---------------------------------------------------------------------------
    def evaluate(self, test_dataset: api.RayDataset, ssim: bool = True, eval_dir: str | None = None) -> list[dict]:
        """Every view of an image-backed test dataset at every scale, rendered and scored on the device
        (RayDataset.render_view).  Per scale: the mean over the views of the per-view PSNR of the last and of
        the coarse level (a mean of PSNRs, as mip-NeRF reports it) and of the SSIM (None without ssim), with
        the per-view figures.  eval_dir: each view's rgb (last level), distance and acc as float32 .npy
        files.  Leaves the training state (parameters, Adam, Philox state) as it is."""
        info = test_dataset.scene_info()
        if eval_dir:
            os.makedirs(eval_dir, exist_ok=True)
        last = self.cfg.num_levels - 1
        out = []
        for s in range(info["num_scales"]):
            views = []
            for v in range(info["num_views"]):
                names = None if eval_dir else ()
                r = test_dataset.render_view(self.model, view=v, scale=s, ssim=ssim, score=True, outputs=names)
                views.append(dict(psnr=r["psnr"][last], psnr_coarse=r["psnr"][0], ssim=r["ssim"]))
                if eval_dir:  # scored: the stream is synchronised
                    stem = os.path.join(eval_dir, f"step{self.step_idx:08d}_scale{s}_view{v:03d}_")
                    for name, t in (("rgb", r["rgb"][last]), ("distance", r["distance"]), ("acc", r["acc"])):
                        np.save(stem + name + ".npy", t.cpu().numpy())
            out.append(dict(scale=s, width=info["width"][s], height=info["height"][s], views=views,
                            psnr=float(np.mean([x["psnr"] for x in views])),
                            psnr_coarse=float(np.mean([x["psnr_coarse"] for x in views])),
                            ssim=float(np.mean([x["ssim"] for x in views])) if ssim else None))
        return out


class PoseRefiner:
    """Joint pose refinement: per view delta_v = (omega_v, tau_v) in R^6 (a small torch tensor, zero at the start),
    pose_v = (exp(hat omega_v) R0_v, t0_v + tau_v), so every rotation stays orthonormal by construction.  The
    library's pose gradient [V, 12] (RayDataset.pose_grad of AcceleratedMipNeRF.ray_grad) is pushed through that
    map by torch autograd with the surrogate (pose * grad.detach()).sum(), delta is stepped by torch.optim.Adam, and
    the new table goes back with RayDataset.set_poses before the next batch is drawn."""

    def __init__(self, dataset: api.RayDataset, n: int, lr: float, seed: int, device: int, stream=None):
        import torch

        self.ds, self.stream = dataset, stream
        self.dev = torch.device("cuda", device)
        # a batch and a zero gradient through the library once: an NDC scene or a record dataset is refused now
        dataset.next(n, seed, 0, 0, stream, with_sum=False)
        zero = torch.zeros((n, 3), dtype=torch.float32, device=self.dev)
        self.grad = dataset.pose_grad(zero, zero, n, stream=stream)
        P0 = torch.from_numpy(dataset.poses().astype(np.float64))
        self.R0, self.t0 = P0[:, :9].reshape(-1, 3, 3), P0[:, 9:]
        self.delta = torch.zeros((P0.shape[0], 6), dtype=torch.float64, requires_grad=True)
        self.opt = torch.optim.Adam([self.delta], lr=lr)

    def _poses(self):
        import torch

        w = self.delta[:, :3]
        z = torch.zeros_like(w[:, 0])
        hat = torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                           torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)
        R = torch.linalg.matrix_exp(hat) @ self.R0
        return torch.cat([R.reshape(-1, 9), self.t0 + self.delta[:, 3:]], 1)

    def poses(self) -> np.ndarray:
        import torch

        with torch.no_grad():
            return self._poses().numpy().astype(np.float32)

    def step(self, model: api.AcceleratedMipNeRF, n: int, dist=None):
        og, dg = model.ray_grad()
        self.ds.pose_grad(og, dg, n, out=self.grad, stream=self.stream)
        api.call("nof_stream_sync", self.stream)
        if dist is not None:  # every rank's shard of the batch
            dist.all_reduce(self.grad)
        g = self.grad.cpu().double()
        self.opt.zero_grad()
        (self._poses() * g).sum().backward()
        self.opt.step()
        self.ds.set_poses(self.poses())


def holdout_views(num_views: int, holdout: int, split: str = "train") -> list[int]:
    """Config.LlffHold (TrainState.cs:53): with holdout = N > 0 every N-th view (i % N == 0) is the test
    split and the rest the train split; N = 0: no test split, every view trains.  N = 1 would leave nothing
    to train on and is refused."""
    if split not in ("train", "test"):
        raise ValueError(f"split must be 'train' or 'test', not {split!r}")
    V, N = int(num_views), int(holdout)
    if V <= 0 or N < 0:
        raise ValueError("holdout_views needs num_views > 0 and holdout >= 0")
    if N == 1:
        raise ValueError("holdout 1 puts every view into the test split: nothing is left to train on")
    test = [i for i in range(V) if N > 0 and i % N == 0]
    return test if split == "test" else [i for i in range(V) if not (N > 0 and i % N == 0)]


def scene_dataset(path, num_scales=1, multiscale_loss=True, device=0, holdout=0, split="train") -> api.RayDataset:
    """The image-backed dataset of a scene file (.npz: poses [V,12], images [V,H,W,3], focal, near, far,
    optional ndc).  holdout = N > 0: only the views of `split` (holdout_views), chosen on the host."""
    import torch

    z = np.load(path)
    poses = np.asarray(z["poses"], dtype=np.float32)
    assert poses.size == z["images"].shape[0] * 12, "poses must be [V, 12] for images [V, H, W, 3]"
    keep = holdout_views(z["images"].shape[0], holdout, split)
    if not keep:
        raise ValueError(f"the {split} split of {path} is empty (holdout {holdout})")
    images = np.ascontiguousarray(z["images"][keep], dtype=np.float32)
    images = torch.from_numpy(images).to(torch.device("cuda", device))
    V, H, W, _ = images.shape
    return api.RayDataset(device=device, scene=dict(
        poses=poses.reshape(-1, 12)[keep], width=W, height=H, focal=float(z["focal"]), near=float(z["near"]),
        far=float(z["far"]), ndc=bool(z["ndc"]) if "ndc" in z else False, images=images, num_scales=num_scales,
        multiscale_loss=multiscale_loss))


def format_eval(step: int, results: list[dict]) -> list[str]:
    """one line per scale of Trainer.evaluate's results"""
    lines = []
    for r in results:
        ssim = "n/a" if r["ssim"] is None else f"{r['ssim']:.6f}"
        lines.append(f"Eval step {step}: scale {r['scale']} ({r['width']}x{r['height']}, {len(r['views'])} views) "
                     f"PSNR {r['psnr']:.4f} dB, coarse PSNR {r['psnr_coarse']:.4f} dB, SSIM {ssim}")
    return lines


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--records", help="BinDataset file of 64-byte records")
    src.add_argument("--synthetic", type=int, help="number of synthetic Lego-shaped records")
    src.add_argument("--scene", help=".npz of poses [V,12], images [V,H,W,3], focal, near, far and optional ndc: "
                                     "an image-backed dataset (rays generated in each batch's gather)")
    ap.add_argument("--num-scales", type=int, default=1, help="--scene: train on the images at 1..4 resolutions")
    ap.add_argument("--disable-multiscale-loss", action="store_true",
                    help="--scene: loss multiplier 1 at every scale instead of 4^scale")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--precision", choices=["f32", "split", "f16x2", "f16split", "f16", "f16p"], default="f32")
    ap.add_argument("--print-every", type=int, default=100)
    ap.add_argument("--save-every", type=int, default=0)
    ap.add_argument("--ckpt-dir")
    ap.add_argument("--resume", help="checkpoint to resume from")
    ap.add_argument("--sync-check-every", type=int, default=0,
                    help="under torch.distributed: assert bitwise-identical parameters across ranks every K steps")
    # the network (MLP.cs:64-86) and samples per level; other shapes than 8x256 run on the any-shape fp32
    # path (BASELINE configs[0]: --net-depth 4 --net-width 128 --samples 64 64)
    ap.add_argument("--net-depth", type=int)
    ap.add_argument("--net-width", type=int)
    ap.add_argument("--net-depth-condition", type=int)
    ap.add_argument("--net-width-condition", type=int)
    ap.add_argument("--samples", type=int, nargs="+")
    # MipNerfModel options (MipNerfModel.cs:14-15,20,22)
    ap.add_argument("--lindisp", action="store_true")
    ap.add_argument("--cylinder", action="store_true")
    ap.add_argument("--density-bias", type=float, default=-1.0)
    ap.add_argument("--rgb-padding", type=float, default=0.001)
    ap.add_argument("--no-stop-level-grad", action="store_true",
                    help="MipNerfModel.StopLevelGrad = false: backprop across levels (f32 / f16p, the any-shape path)")
    ap.add_argument("--distortion-loss-mult", type=float, default=0.0, metavar="X",
                    help="the distortion loss of mip-NeRF 360 on the last level's weights, times X (0 = off; every "
                         "precision; with --no-stop-level-grad it also trains the coarse pass); printed next to the loss")
    ap.add_argument("--interlevel-loss-mult", type=float, default=0.0, metavar="X",
                    help="the interlevel (proposal) loss of mip-NeRF 360, times X: every coarser level's weights are "
                         "pushed to be an upper envelope of the last level's (0 = off; every precision, with or "
                         "without --no-stop-level-grad); printed next to the loss")
    # Config.GradMaxNorm / GradMaxVal / WeightDecayMult (TrainState.cs:58-59,70; 0 = off) and the step statistics
    ap.add_argument("--grad-max-norm", type=float, default=0.0, help="clip the gradient's global norm")
    ap.add_argument("--grad-max-val", type=float, default=0.0, help="clip every gradient element to +-this")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="weight_decay_mult of the loss term sum p^2 / P")
    ap.add_argument("--stats", action="store_true", help="print the gradient statistics with the loss")
    # LearningRateDecay (Program.cs:27-33): the schedule's start and its warm-up (the defaults are the reference's)
    ap.add_argument("--lr-init", type=float, default=5e-4)
    ap.add_argument("--lr-delay-steps", type=int, default=2500, help="0: no warm-up")
    ap.add_argument("--refine-poses", type=float, default=0.0, metavar="LR",
                    help="--scene (not NDC): refine the poses jointly with the field, Adam with this learning rate on a "
                         "per-view (rotation vector, translation); writes poses_refined.npy into --ckpt-dir (default: "
                         "the working directory).  Needs the any-shape path: any other network than 8x256 in f32 or "
                         "f16p; for the reference network --precision f16p, or f32 with --no-stop-level-grad")
    ap.add_argument("--contract", action="store_true",
                    help="scene contraction for unbounded scenes (mip-NeRF 360): every sample's Gaussian is mapped into "
                         "the ball of radius 2 before it is encoded.  Cameras are expected inside the unit ball (scale the "
                         "poses accordingly); --lindisp with a large far plane goes with it.  Needs the any-shape path, as "
                         "--refine-poses does")
    ap.add_argument("--appearance-dim", type=int, default=0, metavar="G",
                    help="--scene: a learned appearance vector of G floats per training image (NeRF-W / mip-NeRF 360's "
                         "GLO vectors), fed to the view-dependent branch: absorbs per-image exposure and white balance; "
                         "writes appearance.npy into --ckpt-dir (default: the working directory); held-out views are "
                         "rendered with the neutral (zero) vector.  Needs the any-shape path, as --refine-poses does")
    ap.add_argument("--appearance-lr", type=float, default=1e-3, metavar="LR",
                    help="with --appearance-dim: the constant Adam learning rate of the appearance table")
    # the test split (Config.LlffHold / GcEvery, TrainState.cs:53,63): held-out views rendered and scored on the device
    ap.add_argument("--holdout", type=int, default=0, metavar="N",
                    help="--scene: hold out every N-th view (i %% N == 0) as the test split; evaluated at the end")
    ap.add_argument("--eval-every", type=int, default=0, metavar="K",
                    help="with --holdout: also evaluate the test split every K steps")
    ap.add_argument("--eval-dir", metavar="DIR",
                    help="with --holdout: write each rendered test view's rgb, distance and acc as .npy files")
    a = ap.parse_args(argv)
    if a.refine_poses < 0:
        ap.error("--refine-poses takes a learning rate > 0")
    if not (a.distortion_loss_mult >= 0 and a.distortion_loss_mult < float("inf")):
        ap.error("--distortion-loss-mult must be a finite number >= 0")
    if not (a.interlevel_loss_mult >= 0 and a.interlevel_loss_mult < float("inf")):
        ap.error("--interlevel-loss-mult must be a finite number >= 0")
    if a.appearance_dim < 0 or a.appearance_dim > 256:
        ap.error("--appearance-dim must be in [0, 256]")
    if not (a.appearance_lr > 0 and a.appearance_lr < float("inf")):
        ap.error("--appearance-lr takes a learning rate > 0")
    if a.refine_poses and not a.scene:
        ap.error("--refine-poses needs --scene: only a scene of poses and images has poses to refine")
    if a.holdout < 0 or a.holdout == 1:
        ap.error("--holdout must be 0 (off) or at least 2: every N-th view is held out, so 1 leaves nothing to train on")
    if a.eval_every < 0:
        ap.error("--eval-every must not be negative")
    if a.holdout and not a.scene:
        ap.error("--holdout needs --scene: only a scene of poses and images has views to hold out")
    if (a.eval_every or a.eval_dir) and not a.holdout:
        ap.error("--eval-every and --eval-dir need --holdout N: without held-out views there is nothing to evaluate")
    return a


def main(argv=None):
    from . import synth

    a = parse_args(argv)
    net = {k: getattr(a, k) for k in ("net_depth", "net_width", "net_depth_condition", "net_width_condition")
           if getattr(a, k) is not None}
    if a.samples:
        net["num_samples"] = tuple(a.samples)
    net.update(lindisp=int(a.lindisp), ray_shape=int(a.cylinder), density_bias=a.density_bias,
               rgb_padding=a.rgb_padding, stop_level_grad=0 if a.no_stop_level_grad else 1,
               distortion_loss_mult=a.distortion_loss_mult)
    if a.scene:
        ds = scene_dataset(a.scene, a.num_scales, not a.disable_multiscale_loss, a.device, holdout=a.holdout)
    elif a.records:
        ds = api.RayDataset(a.records, device=a.device)
    else:
        ds = api.RayDataset(records=synth.pack_records(synth.blender_rays(a.synthetic, seed=1)), device=a.device)
    try:
        tr = Trainer(ds, batch_size=a.batch, device=a.device, print_every=a.print_every, save_every=a.save_every,
                     ckpt_dir=a.ckpt_dir, sync_check_every=a.sync_check_every,
                     grad_max_norm=a.grad_max_norm, grad_max_val=a.grad_max_val, weight_decay_mult=a.weight_decay,
                     stats=a.stats, refine_poses=a.refine_poses, interlevel_loss_mult=a.interlevel_loss_mult,
                     contract=a.contract, appearance_dim=a.appearance_dim, appearance_lr=a.appearance_lr, lr_init=a.lr_init, lr_delay_steps=a.lr_delay_steps,
                     precision=PRECISION_NAMES[a.precision], **net)
    except NofError as e:
        if a.refine_poses and e.status == 5:  # NOF_ERR_UNSUPPORTED: the library says what --refine-poses needs
            raise SystemExit(f"--refine-poses: {e}")
        if a.contract and e.status == 5:
            raise SystemExit(f"--contract: {e}")
        if a.appearance_dim and e.status == 5:
            raise SystemExit(f"--appearance-dim: {e}")
        raise
    if a.resume:
        tr.resume(a.resume)
    test = None
    if a.holdout:
        test = scene_dataset(a.scene, a.num_scales, not a.disable_multiscale_loss, a.device, holdout=a.holdout,
                             split="test")

    def evaluate():
        for line in format_eval(tr.step_idx, tr.evaluate(test, eval_dir=a.eval_dir)):
            print(line, flush=True)

    t0 = time.perf_counter()
    if test is not None and a.eval_every:
        for _ in range(a.steps):
            tr.step()
            if tr.step_idx % a.eval_every == 0:
                evaluate()
        if tr.step_idx % a.eval_every != 0:
            evaluate()
    else:
        tr.train(a.steps)
        if test is not None:
            evaluate()
    import torch

    torch.cuda.synchronize()
    tr.save_poses()
    tr.save_appearance()
    dt = time.perf_counter() - t0
    print(f"{a.steps} steps in {dt:.3f} s: {a.steps * a.batch / dt:.1f} rays/s", flush=True)


if __name__ == "__main__":
    main()
