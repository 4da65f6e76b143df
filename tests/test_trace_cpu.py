"""CPU-side checks of the traced closed loop (mpopis_run_trials_traced): the header and the binding declare the struct and the
entry point, the library exports it, trace_plan_steps -- the definition of which MPC steps carry a plan -- on hand-made cases, and the argument
checks Engine.run_trials makes before it reaches the library.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("plan_every", "int32_t"), ("top", "int32_t"), ("states", "double"), ("rewards", "double"), ("iters", "int32_t"), ("within", "int32_t"),
          ("dist", "double"), ("beta", "double"), ("plan_controls", "double"), ("plan_traj", "double"), ("plan_cost", "double"),
          ("plan_idx0", "int32_t"), ("plan_weights", "double")]


def test_header_declares_the_struct_and_the_entry_point():
    from mpopis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpopis.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} mpopis_trace;", hdr)
    assert m, "no mpopis_trace"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    declared = []
    for typ, names in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        declared += [(n.strip().lstrip("*").strip(), typ) for n in names.split(",")]
    assert declared == FIELDS                                                   # names, types and order: the binding's struct mirrors them
    assert [(n, "int32_t" if t in (C.c_int32, C.POINTER(C.c_int32)) else "double") for n, t in _lib.Trace._fields_] == FIELDS
    assert [n for n, t in _lib.Trace._fields_ if t in (C.c_int32,)] == ["plan_every", "top"]
    assert C.sizeof(_lib.Trace) == 8 + 11 * C.sizeof(C.c_void_p)
    assert re.search(r"^int\s+mpopis_run_trials_traced\s*\(mpopis_handle \*h, int32_t num_steps, int32_t laps, double \*records, double \*actions,\s*"
                     r"const mpopis_trace \*trace", hdr, flags=re.M)
    assert "mpopis_run_trials_traced" in _lib.ABI_SYMBOLS
    assert re.search(r"^#define MPOPIS_ABI_VERSION 5$", hdr, flags=re.M)          # one more entry point, the same ABI version
    assert "Later gained ONE more entry point, mpopis_run_trials_traced" in hdr


def test_library_exports_the_symbol():
    from mpopis_amd import build, _lib
    build.build()
    L = _lib.lib()
    assert hasattr(L, "mpopis_run_trials_traced")
    assert L.mpopis_run_trials_traced(None, 1, 1, None, None, None) == _lib.ERR_ARG      # a NULL handle is an argument error
    tr = _lib.Trace()
    assert L.mpopis_run_trials_traced(None, 1, 1, None, None, C.byref(tr)) == _lib.ERR_ARG


@pytest.mark.parametrize("num_steps,plan_every,want", [
    (14, 1, list(range(15))),                  # every step: num_steps + 1 plans
    (14, 3, [0, 3, 6, 9, 12]),                 # nplans = 14 // 3 + 1
    (9, 3, [0, 3, 6, 9]),                      # the last step itself when plan_every divides num_steps
    (14, 14, [0, 14]),                         # plan_every = num_steps: the first and the last step
    (14, 15, [0]),                             # plan_every = num_steps + 1: only step 0
    (14, 1000, [0]),
    (0, 1, [0]),                               # a run of one MPC step
    (14, 0, []),                               # no plans
    (0, 0, []),
])
def test_trace_plan_steps(num_steps, plan_every, want):
    from mpopis_amd.engine import trace_plan_steps
    got = trace_plan_steps(num_steps, plan_every)
    assert list(got) == want and got.dtype == np.int64 and got.ndim == 1
    assert len(got) == (num_steps // plan_every + 1 if plan_every else 0)       # nplans of include/mpopis.h


def test_trace_plan_steps_refuses_negative_arguments():
    from mpopis_amd import _lib
    from mpopis_amd.engine import trace_plan_steps
    for a in ((5, -1), (-1, 1)):
        with pytest.raises(_lib.MPOPISError) as ei:
            trace_plan_steps(*a)
        assert ei.value.code == _lib.ERR_ARG


@pytest.mark.parametrize("trace,word", [
    (dict(plan_every=-1), "plan_every must be >= 0"),
    (dict(plan_every=1, top=-1), "top must be 0..10"),
    (dict(plan_every=1, top=11), "top must be 0..10"),
    (dict(plan_every=1, top=65), "top must be 0..10"),
    (dict(top=1), "top > 0 needs plan_every > 0"),
    (dict(plan_every=0, fields=["plan_traj"]), "needs plan_every > 0"),
    (dict(fields=["speed"]), "unknown trace field"),
    (dict(every=2), "unknown trace option"),
])
def test_run_trials_refuses_the_trace_before_the_library(trace, word):
    """Engine.run_trials checks plan_every, top and the field names itself: no handle is needed to be told so (K = 10 here)"""
    from mpopis_amd import _lib
    from mpopis_amd.engine import Engine
    eng = Engine.__new__(Engine)                                # no device on this machine: only the fields the checks read
    eng.K, eng.B, eng.as_, eng._h, eng.L = 10, 1, 2, None, None
    with pytest.raises(_lib.MPOPISError) as ei:
        eng.run_trials(num_steps=5, laps=1, trace=trace)
    assert ei.value.code == _lib.ERR_ARG and word in str(ei.value), str(ei.value)


def test_harness_functions_take_trace():
    import inspect
    from mpopis_amd import examples
    assert inspect.signature(examples.simulate_car_racing).parameters["trace"].default is None
    assert "trace" in examples._SIMPLE_KW and examples._SIMPLE_KW["trace"] is None
    assert inspect.signature(examples.Engine.run_trials).parameters["trace"].default is None
