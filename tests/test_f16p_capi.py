"""CPU checks of NOF_PRECISION_F16_PRODUCTS's boundary (no device): the mode number past it is refused, the
fp16-product dispatch tally's name list through ctypes, the test entry's argument checks, the drivers' option."""
import ctypes as C

import pytest


def test_precision_past_f16_products_is_invalid():
    """Mode 5 is the last: 6 and above are NOF_ERR_INVALID_ARG for the reference net and any other (checked
    before any device call)."""
    import nof

    assert nof._lib.NOF_PRECISION_F16_PRODUCTS == 5 and nof._lib.PRECISION_NAMES["f16p"] == 5
    for fields in ({"precision": 6}, {"precision": 6, "net_width": 128}, {"precision": 7}, {"precision": -1}):
        cfg = nof.default_config(**fields)
        h = C.c_void_p()
        assert nof.lib().nof_mipnerf_create(C.byref(cfg), C.byref(h)) == 1, fields
        assert nof.lib().nof_last_error()


def test_gen_dispatch_h_name_list():
    """One distinct name per k_gemm_h instantiation and split / unsplit pick: the four unsplit <64, TWO, MASK>,
    the split-K <64> and <128> (split-K takes one k source and no mask).  A status past either end and with null
    arguments; the fp32 list is untouched."""
    import nof

    lib = nof.lib()
    names, name = [], C.c_char_p()
    while lib.nof_gen_dispatch_h_name(len(names), C.byref(name)) == 0:
        names.append(name.value.decode())
        assert len(names) <= 64
    assert names == nof.gen_dispatch_h_names()
    assert len(names) == len(set(names)) == 6
    assert all(n.startswith("k_gemm_h<") for n in names)
    assert sum(n.endswith(".unsplit") for n in names) == 4 and sum(n.endswith(".splitk") for n in names) == 2
    assert lib.nof_gen_dispatch_h_name(len(names), C.byref(name)) == 1
    assert lib.nof_gen_dispatch_h_name(-1, C.byref(name)) == 1
    assert lib.nof_gen_dispatch_h_name(0, None) == 1
    n = C.c_int32()
    assert lib.nof_mlp_gen_dispatch_h(None, 0, None, 0, C.byref(n)) == 1
    assert hasattr(nof.AcceleratedMLP, "gen_dispatch_h")
    assert not set(names) & set(nof.gen_dispatch_names()) and len(nof.gen_dispatch_names()) == 24


def test_kernel_gemm_h_refuses_bad_arguments():
    """nof_kernel_gemm_h's host-side checks (refused before any launch): null struct, no operands, a split that
    does not cover k, split-K with a second source."""
    import nof

    lib = nof.lib()
    assert lib.nof_kernel_gemm_h(None, None) == 1
    a = nof._lib.nof_gemm_args()
    assert lib.nof_kernel_gemm_h(C.byref(a), None) == 1  # all zero
    a.M, a.N, a.K1, a.kchunk, a.ksplit = 64, 64, 64, 32, 1
    a.A1.p = a.B1.p = a.C = 256  # never dereferenced: the k cover is refused first
    assert lib.nof_kernel_gemm_h(C.byref(a), None) == 1  # 1 x 32 < K
    a.kchunk, a.ksplit, a.K2 = 32, 3, 8
    a.A2.p = a.B2.p = 256
    assert lib.nof_kernel_gemm_h(C.byref(a), None) == 1  # split-K with two sources
    a.K2, a.ksplit, a.kchunk, a.scale_src = 0, 1, 64, 3
    assert lib.nof_kernel_gemm_h(C.byref(a), None) == 1  # scale_src outside 0..2


def test_train_driver_accepts_f16p():
    from nof import train

    a = train.parse_args(["--synthetic", "10", "--precision", "f16p"])
    assert a.precision == "f16p"
    with pytest.raises(SystemExit):
        train.parse_args(["--synthetic", "10", "--precision", "f16q"])
