"""bench.py --dump-outputs: a plain run writes what its last timed step computed (flat gradients, parameters
after Adam, each level's composited colours of the last micro-batch, loss) as float32 .npy files, and two
runs with the same arguments write the same bytes: the inputs are seeded and the step is deterministic
(fixed reduction orders; tools/ab_bits.py compares builds bitwise on the same footing).  96 rays in
micro-batches of 64: two get_gradient calls accumulated into one gradient, the last one 32 rays."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("params", "grads", "loss", "comp_rgb_level0", "comp_rgb_level1")


def _run(monkeypatch, capsys, out_dir):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--rays", "96",
                                      "--micro-batch", "64", "--dump-outputs", str(out_dir)])
    res = bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["value"] == res["value"]
    return res


def test_dump_outputs_plain_run(gpu, tmp_path, monkeypatch, capsys):
    res = _run(monkeypatch, capsys, tmp_path / "a")
    _run(monkeypatch, capsys, tmp_path / "b")
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["config"]["micro_batches_per_step"] == 2
    # a plain run carries the headline only: the live MLP timers, none of the --full legs
    assert set(res["kernels"]) == {"mlp_fwd", "mlp_bwd", "wgrad"}
    assert not {"alt_precision", "config5", "api_path_pcie", "roofline_integrator", "cpu_baseline"} & set(res)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in NAMES)
    arrays = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in NAMES}
    for n, x in arrays.items():
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert (tmp_path / "a" / (n + ".npy")).read_bytes() == (tmp_path / "b" / (n + ".npy")).read_bytes(), n
    assert arrays["params"].shape == arrays["grads"].shape and arrays["params"].size > 500000
    assert np.any(arrays["grads"] != 0) and arrays["loss"].shape == (1,) and arrays["loss"][0] > 0
    assert arrays["comp_rgb_level0"].shape == arrays["comp_rgb_level1"].shape == (32, 3)
    assert sum(x.nbytes for x in arrays.values()) < 64 << 20
