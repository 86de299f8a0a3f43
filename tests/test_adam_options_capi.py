"""Adam's options at the C boundary, host only: the new entry points refuse a null handle with a status (no
abort, no device touched) and the statistics record crosses the boundary with the layout include/nof.h
declares."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_handle_returns_invalid_arg():
    import nof
    from nof import _lib as L

    lib = nof.lib()
    st = L.nof_step_stats()
    f = [C.c_float() for _ in range(3)]
    s = C.c_int32()
    assert lib.nof_adam_set_options(None, 1.0, 1.0, 1.0, 1) == 1
    assert b"invalid argument" in lib.nof_last_error()
    assert lib.nof_adam_get_options(None, C.byref(f[0]), C.byref(f[1]), C.byref(f[2]), C.byref(s)) == 1
    assert lib.nof_adam_stats(None, C.byref(st)) == 1
    m, v, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    assert lib.nof_adam_moments(None, C.byref(m), C.byref(v), C.byref(n)) == 1


def test_step_stats_layout():
    from nof import _lib as L

    assert C.sizeof(L.nof_step_stats) == 24
    names = [k for k, _ in L.nof_step_stats._fields_]
    assert names == ["weight_l2", "grad_norm", "grad_abs_max", "grad_norm_clipped", "clip_scale", "iteration"]
    # the header declares the same fields in the same order
    txt = open(os.path.join(ROOT, "include", "nof.h")).read()
    body = re.search(r"typedef struct nof_step_stats \{(.*?)\} nof_step_stats;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"[a-z_0-9]+(?=\s*[,;])", body) == names


def test_python_mirror_has_the_options():
    import inspect

    import nof
    from nof.train import Trainer

    for name in ("set_options", "get_options", "stats", "moments"):
        assert hasattr(nof.AcceleratedAdamOptimizer, name)
    for cls in (nof.AcceleratedAdamOptimizer, Trainer):
        sig = inspect.signature(cls.__init__).parameters
        for k in ("grad_max_norm", "grad_max_val", "weight_decay_mult", "stats"):
            assert k in sig and sig[k].default in (0, 0.0, False), (cls.__name__, k)
