"""Multiscale, image-backed scenes on the host (include/nof.h nof_multiscale_layout,
nof_dataset_from_images, nof_dataset_materialize): the three entry points are exported and bound, the
record layout of a 40 x 24 scene at four scales is the table the header states, every refused scene
comes back as NOF_ERR_INVALID_ARG with a message before any device call (there is no GPU here), and the
Python driver takes --scene as a third, mutually exclusive source."""
import ctypes as C

import numpy as np
import pytest

NEW = ("nof_multiscale_layout", "nof_dataset_from_images", "nof_dataset_materialize")


def test_new_symbols_exported_and_bound():
    import nof

    for name in NEW:
        assert hasattr(nof.lib(), name), name
        assert name in nof._lib.SIGNATURES, name
    assert hasattr(nof.RayDataset, "materialize")


@pytest.mark.parametrize("loss", [True, False])
def test_layout_of_the_40x24_scene(loss):
    import nof

    L = nof.multiscale_layout(40, 24, 30.0, num_scales=4, multiscale_loss=loss, num_views=3)
    assert L["width"] == [40, 20, 10, 5] and L["height"] == [24, 12, 6, 3]
    assert L["focal"] == [30.0, 15.0, 7.5, 3.75]
    assert L["lossmult"] == ([1.0, 4.0, 16.0, 64.0] if loss else [1.0] * 4)
    assert L["first"] == [0, 2880, 3600, 3780] and L["count"] == 3825


def test_layout_single_scale_is_the_plain_scene():
    import nof

    L = nof.multiscale_layout(37, 23, 12.5, num_views=2)
    assert L == dict(width=[37], height=[23], focal=[12.5], lossmult=[1.0], first=[0], count=2 * 37 * 23)


def _layout_status(W, H, focal, S, V):
    import nof

    w, h, first = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_int64 * 4)()
    f, lm, count = (C.c_float * 4)(), (C.c_float * 4)(), C.c_int64()
    st = nof.lib().nof_multiscale_layout(W, H, focal, S, 0, V, w, h, f, lm, first, C.byref(count))
    return st, nof.lib().nof_last_error()


def _from_images_status(W, H, focal, S, V, poses=True):
    import nof

    P = np.zeros((max(V, 1), 12), np.float32)
    h = C.c_void_p()
    st = nof.lib().nof_dataset_from_images(P.ctypes.data if poses else None, V, W, H, focal, 2.0, 6.0, 0, None, S, 0,
                                           0, C.byref(h))
    assert not h.value
    return st, nof.lib().nof_last_error()


REFUSED = [
    (42, 24, 30.0, 3, 3),        # W not divisible by 2^(S-1)
    (40, 22, 30.0, 3, 3),        # H not divisible by 2^(S-1)
    (8, 24, 30.0, 4, 3),         # w_3 = 1 < 2
    (40, 8, 30.0, 4, 3),         # h_3 = 1 < 2
    (40, 24, 30.0, 0, 3),        # S outside 1..4
    (40, 24, 30.0, 5, 3),
    (40000, 40000, 30.0, 1, 3),  # count = 4.8e9 > 0xFFFFFFFF
    (40, 24, 0.0, 4, 3),         # focal <= 0
    (40, 24, -1.0, 1, 3),
]


@pytest.mark.parametrize("W,H,focal,S,V", REFUSED)
def test_refused_scenes_return_invalid_arg(W, H, focal, S, V):
    for st, msg in (_layout_status(W, H, focal, S, V), _from_images_status(W, H, focal, S, V)):
        assert st == 1 and msg


def test_null_arguments_refused():
    import nof

    st, msg = _from_images_status(40, 24, 30.0, 4, 3, poses=False)
    assert st == 1 and b"poses" in msg
    assert nof.lib().nof_multiscale_layout(40, 24, 30.0, 4, 0, 3, None, None, None, None, None, None) == 1
    assert nof.lib().nof_dataset_materialize(None, None, None) == 1
    with pytest.raises(nof.NofError):
        nof.RayDataset(scene=dict(poses=np.zeros((3, 12)), width=42, height=24, focal=30.0, near=2.0, far=6.0,
                                  num_scales=3))


def test_python_driver_scene_is_an_exclusive_source(capsys):
    from nof import train

    with pytest.raises(SystemExit) as e:
        train.main(["--scene", "x.npz", "--records", "y.bin"])
    assert e.value.code == 2
    assert "not allowed with argument" in capsys.readouterr().err
