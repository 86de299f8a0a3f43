"""The image-backed multiscale dataset on the GPU (include/nof.h nof_dataset_from_images,
nof_dataset_materialize): 3 views of 40 x 24 at four scales, random images.  The last scale, 5 x 3, has odd
sizes: the last-column radius rule and the NDC neighbour swap at both borders are exercised there.

  * the materialised records are bit-identical to the oracle's rays of every scale over the numpy
    pyramid ((a + b) + (c + d)) * 0.25f, loss multiplier 4^s (or 1 with the multiscale loss disabled);
  * the fused gather-and-generate batch is bit-identical to the record gather of the materialised copy,
    whole and sharded, and with one scale to the existing generated dataset's;
  * a training step, a data-parallel step and both drivers end with the same bits from either form;
  * the checked build sees no failed bounds check."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_raygen import RG, _poses

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-or-nothing_amd")
EXE = os.path.join(PKG, "bin", "nof_train")
V, W, H, S = 3, 40, 24, 4
NEAR, FAR = 2.0, 6.0
FIRST, COUNT = [0, 2880, 3600, 3780], 3825
SEED = 11  # its 1000-ray batch at step 3 draws records of all four scales (asserted below)
FIELDS = ("o", "d", "viewdir", "radius", "near", "far", "lossmult", "pix")


def _focal(ndc):  # an fp32 value, so that focal / 2^s is the same number on both sides
    return float(np.float32(1.2 * W if ndc else 0.5 * W / np.tan(0.5 * 0.6911112)))


@pytest.fixture(scope="module")
def images():
    return np.random.default_rng(7).random((V, H, W, 3), dtype=np.float32)


@pytest.fixture(scope="module")
def pyramid(images):
    """numpy fp32 pyramid by the rule of the header: level s from level s - 1"""
    levels = [images]
    for _ in range(1, S):
        p = levels[-1]
        a, b, c, d = p[:, 0::2, 0::2], p[:, 0::2, 1::2], p[:, 1::2, 0::2], p[:, 1::2, 1::2]
        levels.append(((a + b) + (c + d)) * np.float32(0.25))
        assert levels[-1].dtype == np.float32
    return levels


def _scene(images, ndc, gpu, **kw):
    import torch

    return dict(poses=_poses(V, seed=1, llff=ndc), width=W, height=H, focal=_focal(ndc), near=NEAR, far=FAR, ndc=ndc,
                images=torch.from_numpy(images).to(gpu), **kw)


@pytest.fixture(scope="module")
def made(gpu, images):
    """per ndc: the image-backed dataset, its materialised records (host) and their record-backed copy"""
    import torch
    import nof

    out = {}
    for ndc in (False, True):
        ds = nof.RayDataset(scene=_scene(images, ndc, gpu, num_scales=S))
        rec = ds.materialize().cpu().numpy()
        out[ndc] = (ds, rec, nof.RayDataset(records=rec))
    torch.cuda.synchronize()
    return out


def _batch(ds, n, seed, step, ray_base):
    import torch
    import nof

    b, msum = ds.next(n, seed, step, ray_base)
    torch.cuda.synchronize()
    out = {k: nof.to_numpy(b[k][0], b[k][1]).copy() for k in FIELDS}
    out["record_index"] = nof.to_numpy(b["record_index"][0], (n,), np.int32).copy()
    return out, msum


def _same_batch(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in FIELDS + ("record_index",):
        x, y = a[k][rows_a], b[k][rows_b]
        assert x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)), k


@pytest.mark.parametrize("ndc", [False, True])
def test_materialised_records_bit_exact(gpu, images, pyramid, made, ndc):
    import nof

    ds, got, _ = made[ndc]
    assert len(ds) == COUNT and not ds.streaming and got.shape == (COUNT, 16)
    ref = []
    for s in range(S):
        r = RG.generate(_poses(V, seed=1, llff=ndc), W >> s, H >> s, _focal(ndc) / 2 ** s, NEAR, FAR, ndc=ndc,
                        images=pyramid[s])
        r[:, 12] = 4.0 ** s
        ref.append(r)
    ref = np.concatenate(ref)
    assert len(ref) == COUNT
    bad = np.argwhere(got.view(np.int32) != ref.view(np.int32))
    assert bad.size == 0, f"{len(bad)} mismatches, first {bad[:3]}: {got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
    # the multiscale loss disabled: multiplier 1 at every scale, everything else the same
    flat = nof.RayDataset(scene=_scene(images, ndc, gpu, num_scales=S, multiscale_loss=False)).materialize()
    flat = flat.cpu().numpy()
    assert np.all(flat[:, 12] == 1.0)
    ref[:, 12] = 1.0
    assert np.array_equal(flat.view(np.int32), ref.view(np.int32))


@pytest.mark.parametrize("ndc", [False, True])
def test_fused_gather_equals_record_gather(gpu, made, ndc):
    ds, _, copy = made[ndc]
    n = 1000  # not a multiple of the gather's block
    a, sa = _batch(ds, n, SEED, 3, 7)
    b, sb = _batch(copy, n, SEED, 3, 7)
    _same_batch(a, b)
    assert np.float32(sa).view(np.int32) == np.float32(sb).view(np.int32)
    scales = np.searchsorted(FIRST, a["record_index"], side="right") - 1
    assert sorted(set(scales.tolist())) == [0, 1, 2, 3], np.bincount(scales, minlength=S)
    assert sa != n  # the multipliers are live


def test_shards_draw_what_the_whole_batch_draws(gpu, made):
    ds = made[False][0]
    whole, _ = _batch(ds, 1000, SEED, 3, 0)
    lo, _ = _batch(ds, 500, SEED, 3, 0)
    hi, _ = _batch(ds, 500, SEED, 3, 500)
    _same_batch(lo, whole, rows_b=slice(0, 500))
    _same_batch(hi, whole, rows_b=slice(500, 1000))


@pytest.mark.parametrize("ndc", [False, True])
def test_one_scale_equals_the_generated_dataset(gpu, images, ndc):
    import nof

    sc = _scene(images, ndc, gpu)
    one = nof.RayDataset(scene=dict(sc, num_scales=1))
    gen = nof.RayDataset(generate=sc)
    assert len(one) == len(gen) == V * W * H
    for n, base in ((1000, 7), (64, 0)):
        a, sa = _batch(one, n, SEED, 2, base)
        b, sb = _batch(gen, n, SEED, 2, base)
        _same_batch(a, b)
        assert sa == sb == n


def _flat(m, which):
    import nof

    ptr, P = m.mlp.flat_grads() if which == "g" else m.mlp.flat_params()
    return nof.to_numpy(ptr, (P,)).copy()


def test_training_step_from_either_form(gpu, made):
    import torch
    import nof

    ds, _, copy = made[False]
    n, out = 64, []
    for d in (ds, copy):
        m = nof.AcceleratedMipNeRF(seed=5, max_rays=n, num_samples=(64, 64))
        b, msum = d.next(n, SEED, 3, 0)
        p = {k: v[0] for k, v in b.items()}
        m.set_rng(SEED, 3, 0)
        m.get_gradient_device(n, p["o"], p["d"], p["radius"], p["near"], p["far"], p["lossmult"], p["pix"], msum)
        torch.cuda.synchronize()
        out.append((_flat(m, "g"), m.loss(), msum))
        m.close()
    assert out[0][2] == out[1][2] != n
    assert np.any(out[0][0] != 0) and np.array_equal(out[0][0].view(np.int32), out[1][0].view(np.int32))
    assert out[0][1] == out[1][1]


def test_data_parallel_step_from_either_form(gpu, images, made):
    import torch
    import nof
    from nof import dp as ndp
    from nof.dp import NativeDP

    K, B = 2, 128
    rec = made[False][1]
    params = {}
    for form in ("images", "records"):
        dss = [nof.RayDataset(scene=_scene(images, False, gpu, num_scales=S)) if form == "images" else
               nof.RayDataset(records=rec) for _ in range(K)]
        ms = [nof.AcceleratedMipNeRF(seed=5, max_rays=B // K, num_samples=(64, 64)) for _ in range(K)]
        ad = [nof.AcceleratedAdamOptimizer(m.GetLayerSizes(), m.config) for m in ms]
        dps = NativeDP.init_loopback(K, 0)
        try:
            msum = ndp.train_step(dps, ms, ad, dss, B, 1, nof.learning_rate_decay(1), seed=SEED)
            torch.cuda.synchronize()
            params[form] = [_flat(m, "p") for m in ms]
            params[form + "_msum"] = msum
        finally:
            for d in dps:
                d.close()
            for m in ms:
                m.close()
    assert np.array_equal(params["images"][0], params["images"][1]), "replicas differ"
    assert np.array_equal(params["images"][0], params["records"][0])
    assert params["images_msum"] == params["records_msum"]


def test_drivers_train_the_same_from_either_form(gpu, images, made, tmp_path):
    import torch
    import nof
    from nof.train import Trainer

    seed, batch, steps = 0x5EED0000, 256, 3  # the drivers' default seed (python -m nof.train has no --seed)
    _, rec, _ = made[False]
    path = tmp_path / "multiscale.bin"
    rec.tofile(path)
    out = subprocess.run([EXE, "--records", str(path), "--batch", str(batch), "--seed", str(seed), "--print-every", "0",
                          "--steps", str(steps), "--dump-params", str(tmp_path / "p.bin")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]

    tr = Trainer(nof.RayDataset(scene=_scene(images, False, gpu, num_scales=S)), batch_size=batch, seed=seed,
                 print_every=1)
    losses = []
    for _ in range(steps):
        tr.step()
        losses.append(tr.last_loss)
    torch.cuda.synchronize()
    p_py = _flat(tr.model, "p")
    assert np.array_equal(np.fromfile(tmp_path / "p.bin", np.float32), p_py)

    npz = tmp_path / "scene.npz"
    np.savez(npz, poses=_poses(V, seed=1), images=images, focal=np.float32(_focal(False)), near=np.float32(NEAR),
             far=np.float32(FAR))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "nof.train", "--scene", str(npz), "--num-scales", str(S), "--batch",
                          str(batch), "--steps", str(steps), "--print-every", "1"],
                         capture_output=True, text=True, timeout=150, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [float(v) for v in re.findall(r"Step \d+/1000000, Loss: (\S+)", out.stdout)]
    assert got == losses


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import nof
assert nof._lib.LIB_PATH.endswith("libnof_check.so"), nof._lib.LIB_PATH
assert nof.device_checks(clear=True) == 0
rng = np.random.default_rng(7)
P = np.concatenate([np.tile(np.eye(3, dtype=np.float32).ravel(), (3, 1)), rng.normal(size=(3, 3)).astype(np.float32)], 1)
img = torch.from_numpy(rng.random((3, 24, 40, 3), dtype=np.float32)).cuda()
for ndc in (False, True):
    ds = nof.RayDataset(scene=dict(poses=P, width=40, height=24, focal=48.0, near=2.0, far=6.0, ndc=ndc, images=img,
                                   num_scales=4))
    b, msum = ds.next(1000, 11, 3, 7)
    rec = ds.materialize()
    torch.cuda.synchronize()
    assert msum != 1000 and rec.shape == (3825, 16)
    bits = nof.device_checks(clear=True)
    assert bits == 0, f"ndc {ndc}: failed checks {bits:#x}"
print("OK")
"""


def test_checked_build_runs_clean(gpu):
    lib = os.path.join(PKG, "lib", "libnof_check.so")
    assert os.path.exists(lib), "build it with: make -C nerf-or-nothing_amd check"
    out = subprocess.run([sys.executable, "-c", CHILD, PKG], capture_output=True, text=True, timeout=150,
                         env=dict(os.environ, NOF_LIB=lib))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
