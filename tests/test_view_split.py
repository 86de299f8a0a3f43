"""The test split without a GPU (include/nof.h nof_dataset_render_view): the hold-out selection
(Config.LlffHold, TrainState.cs:53), the driver's options, and the new entry points of libnof.so with
the ctypes signatures the binding declares."""
import ctypes as C

import pytest


def test_holdout_zero_trains_on_every_view():
    from nof.train import holdout_views

    assert holdout_views(7, 0, "train") == list(range(7))
    assert holdout_views(7, 0, "test") == []
    assert holdout_views(7, 0) == list(range(7))  # the default split is train


def test_holdout_every_eighth_view():
    from nof.train import holdout_views

    assert holdout_views(20, 8, "test") == [0, 8, 16]
    assert holdout_views(20, 8, "train") == [i for i in range(20) if i % 8]


@pytest.mark.parametrize("V,N", [(1, 0), (2, 2), (5, 2), (20, 8), (9, 3), (4, 7), (33, 8)])
def test_splits_partition_the_views(V, N):
    from nof.train import holdout_views

    train, test = holdout_views(V, N, "train"), holdout_views(V, N, "test")
    assert sorted(train + test) == list(range(V))
    assert not set(train) & set(test)
    assert train == sorted(train) and test == sorted(test)


def test_holdout_refusals():
    from nof.train import holdout_views

    with pytest.raises(ValueError, match="nothing is left to train on"):
        holdout_views(20, 1, "train")
    with pytest.raises(ValueError):
        holdout_views(20, 1, "test")
    with pytest.raises(ValueError):
        holdout_views(20, -2)
    with pytest.raises(ValueError):
        holdout_views(0, 2)
    with pytest.raises(ValueError, match="split"):
        holdout_views(20, 8, "val")


def test_train_options_parse():
    from nof.train import parse_args

    a = parse_args(["--scene", "s.npz", "--num-scales", "3", "--holdout", "2", "--eval-every", "2", "--steps", "4",
                    "--batch", "64", "--samples", "64", "64", "--eval-dir", "out"])
    assert (a.holdout, a.eval_every, a.eval_dir, a.scene, a.num_scales) == (2, 2, "out", "s.npz", 3)
    a = parse_args(["--scene", "s.npz", "--holdout", "8"])  # evaluated once, at the end
    assert (a.holdout, a.eval_every, a.eval_dir) == (8, 0, None)
    a = parse_args(["--synthetic", "1000"])  # without the options: as before
    assert (a.holdout, a.eval_every, a.eval_dir) == (0, 0, None)


@pytest.mark.parametrize("argv,needle", [
    (["--scene", "s.npz", "--eval-every", "2"], "need --holdout"),
    (["--scene", "s.npz", "--eval-dir", "out"], "need --holdout"),
    (["--scene", "s.npz", "--holdout", "1"], "nothing to train on"),
    (["--scene", "s.npz", "--holdout", "-3"], "--holdout"),
    (["--scene", "s.npz", "--holdout", "2", "--eval-every", "-1"], "--eval-every"),
    (["--synthetic", "1000", "--holdout", "2"], "--holdout needs --scene"),
])
def test_train_options_refused_with_a_message(capsys, argv, needle):
    from nof.train import parse_args

    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    assert needle in capsys.readouterr().err


def test_library_exports_the_view_entry_points():
    import nof
    from nof import _lib as L

    lib = nof.lib()
    I32P = C.POINTER(C.c_int32)
    want = {
        "nof_dataset_scene_info": [C.c_void_p, I32P, I32P, I32P, I32P, I32P],
        "nof_dataset_render_view": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint32,
                                    C.POINTER(L.nof_view_out), C.POINTER(L.nof_view_metrics)],
    }
    for name, args in want.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is C.c_int32, name
        assert L.SIGNATURES[name] == args
    assert L.NOF_VIEW_SSIM == 1
    # the structs as include/nof.h lays them out (NOF_MAX_LEVELS = 4, natural alignment)
    assert C.sizeof(L.nof_view_out) == 6 * C.sizeof(C.c_void_p)
    assert [f for f, _ in L.nof_view_metrics._fields_] == ["width", "height", "num_levels", "mse", "psnr", "ssim"]
    assert L.nof_view_metrics.mse.offset == 16 and L.nof_view_metrics.psnr.offset == 48
    assert L.nof_view_metrics.ssim.offset == 64 and C.sizeof(L.nof_view_metrics) == 72
    assert hasattr(nof.RayDataset, "render_view") and hasattr(nof.RayDataset, "scene_info")


def test_view_entry_points_refuse_null_arguments():
    """Host-only refusals (no device is touched): null ds, model or out."""
    import nof
    from nof import _lib as L

    lib = nof.lib()
    out = L.nof_view_out()
    n = C.c_int32()
    w = (C.c_int32 * 4)()
    assert lib.nof_dataset_render_view(None, None, 0, None, 0, 0, C.byref(out), None) == 1
    assert b"invalid argument" in lib.nof_last_error()
    assert lib.nof_dataset_scene_info(None, C.byref(n), C.byref(n), w, w, C.byref(n)) == 1
