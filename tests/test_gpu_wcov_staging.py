"""The staging of the pair-list covariance scatter with 64-column chunks (k_wcov_mfma_partial<64, SQ, false, false, NT>, cs <= 112): below the last row
tile a staged element is one multiply by the column's sqrt(w_k) -- 0 for a column outside the split's range -- and one LDS write; only the last tile's
elements are guarded (data row, the ones row, zero padding).  Driven through tools/kbench_mfma.hip like tests/test_gpu_mfma_harness.py, one process per
launch; cases, references (np.longdouble) and the bound 4 (m + 64) u T_ab come from tests/helpers/mfma_cases.py, the case list from
tests/helpers/wcov_staging_cases.py (tests/test_wcov_staging_cpu.py shows on the CPU what it reaches).  Every case asserts the form wcov_form reported."""
import os
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import mfma_cases as M
from tests.helpers import wcov_staging_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LD = M.LD
SPECS = W.specs()


@pytest.fixture(scope="module")
def harness():
    from mpopis_amd import build
    lib = build.build()                                               # the harness links the library's object files
    exe = os.path.join(ROOT, "tools", "kbench_mfma_bin")
    deps = [lib] + [os.path.join(ROOT, "tools", f) for f in ("kbench_mfma.hip", "kbench_dev.h", "kbench_io.h", "build_kbench.sh")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in deps):
        return exe                                                    # (tests/test_gpu_mfma_harness.py built it in this session)
    return HR.build("mfma")


def _run(exe, tmp_path, data):
    e = dict(os.environ)
    e.pop("MPOPIS_WCOV_ROWS", None)
    form, arrays = M.unpack_result(HR.run_case(exe, tmp_path, data, env=e))
    assert len(arrays) == 5                                           # S, mu_out, u_add, cmin, part
    return form, arrays


def _same(r1, r2):
    return r1[0] == r2[0] and len(r1[1]) == len(r2[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(r1[1], r2[1]))


def _body(a, shape, active, name, written=True):
    body, guard = M.split_guard(a, shape)
    assert np.all(M.is_poison(guard)), name + ": guard entries written"
    for b in range(shape[0]):
        if not active[b] or not written:
            assert np.all(M.is_poison(body[b])), "%s: slot %d written" % (name, b)
        else:
            assert not np.any(M.is_poison(body[b])) and not np.any(np.isnan(body[b])), "%s: slot %d keeps untouched entries or NaN" % (name, b)
    return body


def _ratio(got, ref, bound, what):
    err = np.abs(np.asarray(got).astype(LD) - ref)
    bound = np.asarray(bound, dtype=LD)
    zero = bound == 0
    assert np.all(err[zero] == 0), (what, "nonzero error where the bound is zero")
    r = float(np.max(np.where(zero, 0, err / np.where(zero, 1, bound))))
    print("RATIO %.4f  (%s)" % (r, what))
    assert r <= 1.0, (what, r, float(err.max()))


def _check(exe, tmp_path, c):
    """the form, the untouched entries, the partial workspace and the moments of one case against the longdouble reference"""
    r = _run(exe, tmp_path, c["data"])
    partial, sq, aug, from_cost = M.case_form(c)
    assert partial == M.WCOV_PAIR64 and r[0] == M.form_code(M.WCOV_PAIR64, sq, aug, from_cost), (r[0], partial, sq, aug, from_cost)
    B, cs, act, ks = c["B"], c["cs"], c["active"], c["ksplit"]
    S = _body(r[1][0], (B, cs, cs), act, "S")
    mu = _body(r[1][1], (B, cs), act, "mu_out", written=aug)
    u_all, u_guard = M.split_guard(r[1][2], (B, cs))
    assert np.all(M.is_poison(u_guard))
    nt = (cs + 15) // 16
    part = r[1][4].reshape(B, ks, nt * (nt + 1) // 2, 256)
    empty = M.empty_splits(cs, c["m"], ks)
    tag = W.case_id(dict(c, want_mu=None))
    for b in range(B):
        if not act[b]:
            assert np.all(np.isnan(part[b])), "partials of an inactive slot written"
            continue
        assert np.all(np.isfinite(part[b])), "a partial was left unwritten or is not finite"
        assert np.all(M.bits(part[b][empty]) == 0), "an empty split wrote something other than +0"
        assert np.array_equal(M.bits(S[b]), M.bits(S[b].T)), "S not bitwise symmetric"
        ref = M.wcov_reference(c, b)
        _ratio(S[b], ref["S"], ref["S_bound"], tag + " S slot %d" % b)
        if aug:
            _ratio(mu[b], ref["mu"], ref["mu_bound"], tag + " mu slot %d" % b)
            if c["u0"] is not None:
                assert np.array_equal(M.bits(u_all[b]), M.bits(c["u0"][b] + mu[b])), "u_add != u0 + mu_out"
    return r


@pytest.mark.parametrize("spec", SPECS, ids=[W.case_id(s) for s in SPECS])
def test_staging_against_the_reference(harness, tmp_path, spec):
    """every row count on both sides of the last tile's edges x column counts that leave splits empty, ending inside a chunk and on a chunk boundary x
    weights from w, from the costs (a +inf cost: weight exactly 0) and none x ones row on / off x gathered / contiguous columns, and the fourth-moment
    variant: S (and the mean from the ones row) within 4 (m + 64) u T of the longdouble reference, every partial written and finite, empty splits +0"""
    _check(harness, tmp_path, W.build(spec))


@pytest.mark.parametrize("variant,cs", [("idx", 100), ("idx_w", 97)])
def test_padding_of_a_range_contributes_nothing(harness, tmp_path, variant, cs):
    """m = 65 of 600 columns in two splits (64 + 1: the second split's chunk is one column and 63 of padding).  1e300 in every column outside the range, in
    the weights there, and idx[m:] pointing at them: the partials, S and the mean keep every bit"""
    for want in (False, True):
        c = W.build(dict(cs=cs, K=W.GATHER_K, ksplit=2, variant=variant, m=65, want_mu=want))
        clean = _check(harness, tmp_path, c)
        dirty = _run(harness, tmp_path, W.poisoned(c)["data"])
        assert _same(clean, dirty), [i for i, (a, b) in enumerate(zip(clean[1], dirty[1])) if a.tobytes() != b.tobytes()]


@pytest.mark.parametrize("spec", [dict(cs=100, K=257, ksplit=6, variant="cost"), dict(cs=97, K=65, ksplit=2, variant="w"),
                                  dict(cs=100, K=W.GATHER_K, ksplit=2, variant="ss", m=65)], ids=W.case_id)
def test_a_second_run_gives_the_same_bits(harness, tmp_path, spec):
    c = W.build(spec)
    assert _same(_run(harness, tmp_path, c["data"]), _run(harness, tmp_path, c["data"]))
