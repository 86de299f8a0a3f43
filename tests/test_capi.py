"""CPU checks of the drop-in boundary: libnof.so loads, exports every symbol include/nof.h declares,
host-only entry points behave, invalid configurations are rejected with a status (no abort)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "nof.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nof_[a-z0-9_]+)\s*\(", txt)) - {"nof_output_grad_fn"})


def test_library_exports_every_declared_symbol():
    import nof

    lib = nof.lib()
    names = declared_symbols()
    assert len(names) >= 45
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared but not exported: {missing}"
    # and the ctypes table covers them all
    assert set(names) <= set(nof._lib.SIGNATURES), set(names) - set(nof._lib.SIGNATURES)


def test_config_defaults_are_reference_constants():
    import nof

    c = nof.default_config()
    assert (c.max_rays, c.num_levels, c.num_samples[0], c.num_samples[1]) == (1024, 2, 128, 128)  # helpers.h:16-18
    assert (c.net_depth, c.net_width, c.net_depth_condition, c.net_width_condition, c.skip_layer) == (8, 256, 1, 128, 4)
    assert (c.min_deg_point, c.max_deg_point, c.deg_view) == (0, 16, 4)
    assert (c.randomized, c.white_bkgd) == (1, 1)
    assert c.resample_padding == np.float32(0.01) and c.coarse_loss_mult == np.float32(0.1)


def test_lr_decay_matches_oracle_bitwise(oracle):
    import nof

    for s in (0, 1, 17, 2500, 2501, 100000, 999999, 1000000, 2000000):
        assert nof.learning_rate_decay(s) == oracle.lr_decay(s)


@pytest.mark.parametrize("fields,status", [
    ({"num_samples": (100, 128)}, 5),          # GPU path needs 64/128/256/512 samples per level
    ({"net_width": 128, "precision": 4}, 5),   # other networks: the any-shape path, fp32 only
    ({"net_depth": 0}, 1),
    ({"net_depth": 14, "net_depth_condition": 1}, 1),  # D + Dc + 2 > 16 layers (checkpoint layout)
    ({"min_deg_point": 4, "max_deg_point": 4}, 1),
    ({"skip_layer": 0}, 1),
    ({"max_rays": 0}, 1),
])
def test_invalid_config_returns_status(fields, status):
    """Rejected before any device call (no GPU here)."""
    import nof

    cfg = nof.default_config(**fields)
    h = C.c_void_p()
    st = nof.lib().nof_mipnerf_create(C.byref(cfg), C.byref(h))
    assert st == status
    assert nof.lib().nof_last_error()
    with pytest.raises(nof.NofError):
        nof.AcceleratedMipNeRF(cfg)


def test_null_arguments_rejected():
    import nof

    assert nof.lib().nof_mipnerf_get_gradient_device(None, 1, *([None] * 7), 1.0, None) == 1
    assert nof.lib().nof_retrieve_output(0, 4, None) == 1
    assert nof.lib().nof_adam_step(None, None, None, 1e-3) == 1
    assert b"invalid argument" in nof.lib().nof_last_error()


def test_gen_dispatch_name_list():
    """The any-shape dispatch tally's name table through ctypes (host only): one distinct name per variant
    (the six k_gemm picks of launch_gemm, k_gemm_ws's six static and eight runtime shapes, both encoders,
    the slab and ray sums), a status past either end, null arguments refused."""
    import nof

    lib = nof.lib()
    names, name = [], C.c_char_p()
    while lib.nof_gen_dispatch_name(len(names), C.byref(name)) == 0:
        names.append(name.value.decode())
        assert len(names) <= 256
    assert names == nof.gen_dispatch_names()
    assert len(names) == len(set(names)) == 24
    assert sum(n.startswith("k_gemm<") for n in names) == 6
    assert sum(n.startswith("k_gemm_ws<") for n in names) == 14
    assert {f"k_gemm_ws<{nt}>" for nt in range(1, 9)} <= set(names)
    assert {"k_encode_g", "k_encode_g4", "k_slab_sums", "k_ray_sum"} <= set(names)
    assert lib.nof_gen_dispatch_name(len(names), C.byref(name)) == 1
    assert lib.nof_gen_dispatch_name(-1, C.byref(name)) == 1
    assert lib.nof_gen_dispatch_name(0, None) == 1
    n = C.c_int32()
    assert lib.nof_mlp_gen_dispatch(None, 0, None, 0, C.byref(n)) == 1
    assert hasattr(nof.AcceleratedMLP, "gen_dispatch")


def test_python_mirror_names():
    import nof

    for cls, meth in [("AcceleratedMipNeRF", "GetGradient"), ("AcceleratedMipNeRF", "GetLayerSizes"),
                      ("AcceleratedMLP", "get_output"), ("AcceleratedMLP", "get_gradient"),
                      ("AcceleratedAdamOptimizer", "step"), ("AcceleratedGradientCalculator", "get_output_gradient"),
                      ("OutputRetriever", "RetrieveOutput")]:
        assert hasattr(getattr(nof, cls), meth)


def test_grad_bucket_spans_partition_the_arena():
    """The gradient buckets of the overlapped all-reduce cover [W0..W10, b0..b10] exactly once:
    bucket 0 = W5..W10 (the layers whose weight gradients finish first), bucket 1 = the rest."""
    import nof

    sizes = [24576, 65536, 65536, 65536, 90112, 65536, 65536, 65536, 256, 36224, 384,
             256, 256, 256, 256, 256, 256, 256, 256, 1, 128, 3]  # MLPcpp:131-154
    b0, b1 = nof.grad_bucket_spans(sizes, 0), nof.grad_bucket_spans(sizes, 1)
    w5 = sum(sizes[:5])
    assert b0 == [(w5, sum(sizes[5:11]))]
    assert b1 == [(0, w5), (sum(sizes[:11]), sum(sizes[11:]))]
    spans = sorted(b0 + b1)
    pos = 0
    for off, cnt in spans:
        assert off == pos
        pos += cnt
    assert pos == sum(sizes) == 546948
    with pytest.raises(nof.NofError):
        nof.grad_bucket_spans(sizes, 2)


def test_device_checks_product_vs_checked_build():
    """The product library has no device checks (NOF_ERR_UNSUPPORTED, no GPU touched); the checked
    build (lib/libnof_check.so, `make check`) exports the same C ABI."""
    import nof

    with pytest.raises(nof.NofError) as e:
        nof.device_checks()
    assert e.value.status == 5  # NOF_ERR_UNSUPPORTED
    checked = os.path.join(ROOT, "nerf-or-nothing_amd", "lib", "libnof_check.so")
    assert os.path.exists(checked), "build it with: make -C nerf-or-nothing_amd check"
    lib = C.CDLL(checked)
    missing = [n for n in declared_symbols() if not hasattr(lib, n)]
    assert not missing, missing
