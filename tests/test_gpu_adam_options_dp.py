"""Adam's options in the data-parallel step and in both training drivers.

  * a loopback group of K = 2 through nof_dp_train_step with the norm clip ACTIVE: every replica's parameters and
    statistics bitwise identical (the clip is computed on the all-reduced gradient, inside the library), and equal
    bit for bit to the step written out in Python: the two shard gradients added by torch (g0 + g1, the loopback
    order), clipped in numpy float32 with the reported clip_scale, oracle.adam_step; grouped and attached (bucketed);
  * bin/nof_train --grad-max-norm --weight-decay == nof.train.Trainer with the same keywords bit for bit, and the
    statistics the driver prints are the Trainer's last_stats.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_dp_loopback import EXE, SEED, _flat, _grad, _models, _records

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.mark.parametrize("attach", [False, True], ids=["grouped", "attached"])
def test_loopback_k2_norm_clip_matches_emulation(gpu, oracle, attach):
    import torch

    import nof
    from nof import dp as ndp
    from nof.dp import NativeDP

    B, K = 256, 2
    sh = B // K
    ds_py = nof.RayDataset(records=_records(3000, 9))
    ms_py, _ = _models(K, sh, grad_buckets=1)  # the emulation's gradients (bucket-aligned items, as attached)
    ms, ad = _models(K, sh, grad_buckets=1)
    dss = [nof.RayDataset(records=_records(3000, 9)) for _ in range(K)]
    dps = NativeDP.init_loopback(K, 0)
    if attach:
        for d, m in zip(dps, ms):
            d.attach(m)
    dev = torch.device("cuda", 0)
    try:
        p = _flat(ms[0], "p")
        P = p.size
        m1, v1 = np.zeros(P, F32), np.zeros(P, F32)
        gmn = None
        for step in (1, 2):
            lr = nof.learning_rate_decay(step)
            msum = F32(0.0)
            for r in range(K):
                msum = F32(msum + F32(ds_py.next(sh, SEED, step, r * sh)[1]))
            for r, m in enumerate(ms_py):
                _grad(m, ds_py, sh, step, r * sh, float(msum))
            torch.cuda.synchronize()
            g = [nof.device_tensor(m.mlp.flat_grads()[0], (P,), device=dev) for m in ms_py]
            G = (g[0] + g[1]).cpu().numpy()
            n2 = float(np.linalg.norm(G.astype(np.float64)))
            if gmn is None:  # a tenth of the first gradient's norm: the clip is active by a factor ~10
                gmn = float(F32(0.1 * n2))
                for o in ad:
                    o.set_options(grad_max_norm=gmn)
            assert n2 >= 2.0 * gmn, (n2, gmn)

            assert ndp.train_step(dps, ms, ad, dss, B, step, lr, seed=SEED) == float(msum)
            stats = [o.stats() for o in ad]
            assert stats[0] == stats[1], "the replicas' statistics differ"
            st = stats[0]
            assert st["iteration"] == step and st["clip_scale"] < 0.5
            assert F32(st["grad_abs_max"]) == np.max(np.abs(G))
            assert abs(st["grad_norm"] - n2) <= 1e-5 * n2
            scale = gmn / (1e-7 + n2)
            assert abs(st["clip_scale"] - scale) <= 1e-5 * scale
            assert abs(st["grad_norm_clipped"] - scale * n2) <= 1e-5 * scale * n2

            g3 = G * F32(st["clip_scale"])
            oracle.adam_step(p, np.ascontiguousarray(g3), m1, v1, lr, step)
            for r in range(K):
                assert np.array_equal(_flat(ms[r], "p"), p), f"replica {r} step {step}"
            for m in ms_py:  # the emulation's models follow
                nof.device_tensor(m.mlp.flat_params()[0], (P,), device=dev).copy_(torch.from_numpy(p))
            torch.cuda.synchronize()
    finally:
        for d in dps:
            if attach:
                d.attach(None)
            d.close()
        for m in ms + ms_py:
            m.close()


def test_native_driver_matches_python_trainer(gpu, tmp_path, capsys):
    import torch

    import nof
    from nof.train import Trainer

    path = tmp_path / "train.bin"
    _records(4000, 13).tofile(path)
    opts = dict(grad_max_norm=1e-3, weight_decay_mult=1.0)
    out = subprocess.run([str(x) for x in (EXE, "--records", path, "--batch", 256, "--seed", 77, "--print-every", 1,
                                           "--steps", 3, "--grad-max-norm", opts["grad_max_norm"], "--weight-decay",
                                           opts["weight_decay_mult"], "--dump-params", tmp_path / "p.bin")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    tr = Trainer(nof.RayDataset(path), batch_size=256, seed=77, print_every=1, **opts)
    tr.train(3)
    torch.cuda.synchronize()
    assert np.array_equal(np.fromfile(tmp_path / "p.bin", np.float32), _flat(tr.model, "p"))

    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Step 3/")]
    assert len(lines) == 1, out.stdout
    printed = {k: float(x) for k, x in re.findall(r"(grad_norm|grad_abs_max|grad_norm_clipped|weight_l2): (\S+?)(?:,|$)",
                                                  lines[0])}
    st = tr.last_stats
    assert st["iteration"] == 3 and st["clip_scale"] < 1.0, st  # the options did something
    assert set(printed) == {"grad_norm", "grad_abs_max", "grad_norm_clipped", "weight_l2"}, lines[0]
    for k, x in printed.items():
        assert abs(x - st[k]) <= 1e-6 * abs(st[k]), (k, x, st[k])
    # the Trainer prints the same record after the same prefix
    mine = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Step 3/")]
    assert len(mine) == 1 and ", Loss: " in mine[0] and mine[0].split(", grad_norm: ")[1] == \
        lines[0].split(", grad_norm: ")[1]


def test_native_driver_default_output_unchanged(gpu, tmp_path):
    """No option, no --stats: the print line is the loss alone; --stats adds the record after it."""
    path = tmp_path / "train.bin"
    _records(4000, 13).tofile(path)
    common = [EXE, "--records", path, "--batch", 256, "--seed", 77, "--print-every", 1, "--steps", 1]
    run = lambda *a: subprocess.run([str(x) for x in (*common, *a)], capture_output=True, text=True, timeout=120)
    plain, stats = run(), run("--stats")
    assert plain.returncode == 0 and stats.returncode == 0, plain.stderr[-1000:] + stats.stderr[-1000:]
    a, b = plain.stdout.splitlines()[0], stats.stdout.splitlines()[0]
    assert re.fullmatch(r"Step 1/1000000, Loss: \S+", a), a
    assert b.startswith(a + ", grad_norm: ") and "weight_l2: " in b, b
