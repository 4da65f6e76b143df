"""CPU-side checks of the plan read-out (mpopis_get_plan): the header and the binding declare it, plan_order -- the
definition of the order samples come back in -- on hand-made weight rows, and the argument check Engine.get_plan makes before it reaches the
library.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_entry_point():
    from mpopis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpopis.h")).read()
    assert re.search(r"^int\s+mpopis_get_plan\s*\(mpopis_handle \*h, int32_t top,", hdr, flags=re.M)
    m = re.search(r"^#define\s+MPOPIS_PLAN_MAX_TOP\s+(\d+)\s*$", hdr, flags=re.M)
    assert m and int(m.group(1)) == 64 == _lib.PLAN_MAX_TOP
    assert "mpopis_get_plan" in _lib.ABI_SYMBOLS
    assert re.search(r"^#define MPOPIS_ABI_VERSION 5$", hdr, flags=re.M)          # one more entry point, the same ABI version


def test_library_exports_the_symbol():
    from mpopis_amd import build, _lib
    build.build()
    assert hasattr(_lib.lib(), "mpopis_get_plan")
    assert _lib.lib().mpopis_get_plan(None, 0, None, None, None, None, None) == _lib.ERR_ARG      # a NULL handle is an argument error


def test_plan_order_all_weights_equal():
    from mpopis_amd.engine import plan_order
    w = np.full((2, 9), 1.0 / 9)
    assert np.array_equal(plan_order(w, 5), np.tile(np.arange(5), (2, 1)))
    assert plan_order(w, 5).dtype == np.int32


def test_plan_order_three_positive_weights_among_exact_zeros():
    from mpopis_amd.engine import plan_order
    w = np.zeros(64)
    w[40], w[7], w[22] = 0.2, 0.7, 0.1
    assert list(plan_order(w, 8)) == [7, 40, 22, 0, 1, 2, 3, 4]                 # the zeros follow in ascending index order


def test_plan_order_duplicated_maxima():
    from mpopis_amd.engine import plan_order
    w = np.array([[0.1, 0.3, 0.05, 0.3, 0.25], [0.5, 0.0, 0.5, 0.0, 0.0]])
    assert np.array_equal(plan_order(w, 3), [[1, 3, 4], [0, 2, 1]])


def test_plan_order_top_zero_and_top_K():
    from mpopis_amd.engine import plan_order
    w = np.array([0.25, 0.5, 0.0, 0.25])
    assert plan_order(w, 0).shape == (0,)
    assert list(plan_order(w, 4)) == [1, 0, 3, 2]
    assert plan_order(np.stack([w, w[::-1]]), 0).shape == (2, 0)
    # the reference's order: sortperm(w, rev=true) is a stable sort of the reversed comparison, i.e. descending weight, ties by ascending index
    assert list(plan_order(w, 4)) == sorted(range(4), key=lambda k: (-w[k], k))


@pytest.mark.parametrize("top", [-1, 65, 11])
def test_get_plan_refuses_top_before_the_library(top):
    """Engine.get_plan checks 0 <= top <= min(K, 64) itself: no handle is needed to be told so (K = 10 here)"""
    from mpopis_amd import _lib
    from mpopis_amd.engine import Engine
    eng = Engine.__new__(Engine)                                # no device on this machine: only the fields the check reads
    eng.K, eng.B, eng._h = 10, 1, None
    with pytest.raises(_lib.MPOPISError) as ei:
        eng.get_plan(top)
    assert ei.value.code == _lib.ERR_ARG and "top must be 0..10" in str(ei.value)
