"""The two adaptation steps -- kernels_nes.hip (early break, signed scatter with its finish kernel, the triangular inverse, the batched GEMM in its plain,
transposed and symmetric forms with and without D and per-slot scales, the U update) and kernels_cma.hip (begin, paths, Sigma update) -- exercised directly,
below the policy level, through the C++ harness tools/kbench_adapt.hip: one process per launch, inputs written by the test, raw device outputs read back.
The shapes sit where the policy-level tests never go: cs a multiple of 16 and below 16, the step from 28 to 36 tile pairs, ragged and empty K splits, matrix
orders that are no multiple of 4, fewer than 64 columns per workgroup of the triangular inverse, the second pass of the paths kernel's four-at-a-time loop,
both sides of the h_sigma decision and of the early-break tolerance.  References are np.longdouble (tests/helpers/adapt_cases.py, where the error bounds are
derived; tests/test_adapt_cases_cpu.py shows on the CPU that inputs and references are what they claim), never the engine, and every stage is checked against
the bits the stage before it left on the device.  The harness poisons every output: inactive slots and guard entries must stay untouched and no active entry
may keep the poison.

Every check prints `RATIO <op> <worst error / bound>`; DESIGN.md ("kernel-level tests") records the worst per op."""
import os
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import adapt_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LD = A.LD


@pytest.fixture(scope="module")
def harness():
    return HR.build("adapt")


def _run(exe, tmp_path, data):
    return A.unpack_result(HR.run_case(exe, tmp_path, data))


def _body(a, shape, active, name):
    """guard untouched, inactive slots untouched, no poison left in an active slot"""
    body, guard = A.split_guard(a, shape)
    assert np.all(A.is_poison(guard)), name + ": guard entries written"
    for b in range(shape[0]):
        if not active[b]:
            assert np.all(A.is_poison(body[b])), "%s: slot %d written" % (name, b)
        else:
            assert not np.any(A.is_poison(body[b])), "%s: slot %d keeps %d untouched entries" % (name, b, int(np.sum(A.is_poison(body[b]))))
    return body


def _ratio(op, got, ref, bound, what):
    got = np.asarray(got)
    assert not np.any(np.isnan(got)), (what, "NaN")
    err = np.abs(got.astype(LD) - ref)
    bound = np.asarray(bound, dtype=LD)
    zero = bound == 0
    assert np.all(err[zero] == 0), (what, "nonzero error where the bound is zero")
    r = float(np.max(np.where(zero, 0, err / np.where(zero, 1, bound)))) if err.size else 0.0
    print("RATIO %s %.4f  (%s)" % (op, r, what))
    assert r <= 1.0, (what, r, float(err.max()))
    return r


def _mats(a, B, n, active, name):
    """[B] column-major n x n outputs as NumPy matrices"""
    body = _body(a, (B, n * n), active, name)
    return [A.cm(body[b], n) for b in range(B)]


def _bit_symmetric(Mx, what):
    assert np.array_equal(A.bits(Mx), A.bits(Mx.T)), what + " is not bit-symmetric"


# ================================================================ early break ==================================================================
def _check_break(harness, tmp_path, c):
    r = _run(harness, tmp_path, c["data"])
    act, ag = A.split_guard(r[0], (c["B"],))
    st, sg = A.split_guard(r[1], (c["B"],))
    assert np.all(A.is_poison(ag)) and np.all(A.is_poison(sg))
    ract, rst = A.break_ref(c["cost"], c["active"], c["status"])
    assert list(act) == list(ract), (list(act), list(ract), c["intent"])
    assert list(st) == list(rst), (list(st), list(rst))


@pytest.mark.parametrize("K", A.BREAK_KS)
def test_break_on_both_sides_of_the_tolerance(harness, tmp_path, K):
    """the deciding difference first, across the 256-thread stride and last; exactly 0.01 keeps the slot (strict <), the next double below stops it;
    an inactive slot keeps active and status"""
    _check_break(harness, tmp_path, A.break_case(K))


def test_break_nonfinite_costs_raise_the_action_error(harness, tmp_path):
    """+inf, NaN, -inf -> MPOPIS_ERR_ACTION and active 0; a higher-ranked status stays; an inactive slot keeps everything"""
    _check_break(harness, tmp_path, A.break_nonfinite_case())


# ================================================================ signed scatter ===============================================================
def _scatter_outputs(c, r):
    B, cs = c["B"], c["cs"]
    return _mats(r[0], B, cs, c["active"], "M"), _body(r[1], (B, cs), c["active"], "g"), _body(r[2], (B,), c["active"], "Csum")


@pytest.mark.parametrize("cs,K,ksplit,slot0", A.SCATTER_CASES)
def test_scatter_against_longdouble(harness, tmp_path, cs, K, ksplit, slot0):
    """M = sum c_k E_k E_k', g = sum c_k E_k, C = sum c_k with costs of both signs; no NaN of the poisoned partial workspace reaches an output (an
    empty split must have written zeros); M bit-symmetric; B = 3 with the middle slot inactive.  At (K, ksplit) = (100, 3) also: slot 2 alone (B = 1)
    gives the same bits"""
    c = A.scatter_case(cs, K, ksplit, slot0)
    r = _run(harness, tmp_path, c["data"])
    M, g, C = _scatter_outputs(c, r)
    for b in np.flatnonzero(c["active"]):
        (rM, rg, rC), (tM, tg, tC) = A.scatter_reference(c["E"][b], c["cost"][b])
        what = "cs %d K %d ksplit %d slot %d (%s)" % (cs, K, ksplit, b, c["kinds"][b])
        _ratio("SCATTER", M[b], rM, A.sum_bound(K, tM), what + " M")
        _ratio("SCATTER", g[b], rg, A.sum_bound(K, tg), what + " g")
        _ratio("SCATTER", C[b], rC, A.sum_bound(K, tC), what + " C")
        _bit_symmetric(M[b], what)
    if (K, ksplit) == (100, 3):
        c1 = A.scatter_case(cs, K, ksplit, slot0, single=True)
        M1, g1, C1 = _scatter_outputs(c1, _run(harness, tmp_path, c1["data"]))
        assert np.array_equal(A.bits(M1[0]), A.bits(M[2])) and np.array_equal(A.bits(g1[0]), A.bits(g[2])) and np.array_equal(A.bits(C1[0]), A.bits(C[2]))


# ================================================================ Sigma^-1 from the factor =====================================================
@pytest.mark.parametrize("n,kind,shared,use_active", A.POTRI_CASES)
def test_potri_inverse_and_symmetric_product(harness, tmp_path, n, kind, shared, use_active):
    """X = L^-1: componentwise residual of a backward-stable substitution, exactly zero above the diagonal; S = X'X (transposed operand, sym) against
    the device's X, bit-symmetric.  n = 301 and 400 run with 63 and 48 columns per workgroup"""
    c = A.potri_case(n, kind, shared, use_active)
    r = _run(harness, tmp_path, c["data"])
    X, S = _mats(r[0], c["B"], n, c["computed"], "X"), _mats(r[1], c["B"], n, c["computed"], "S")
    for b in np.flatnonzero(c["computed"]):
        what = "n %d %s slot %d" % (n, kind, b)
        L = c["L"][0 if shared else b]
        assert not np.any(np.triu(X[b], 1)), what + ": X is not zero above the diagonal"
        err, bound = A.trtri_residual(L, X[b])
        _ratio("POTRI", err, 0, bound, what + " L X - I")
        ref, terms = A.gemm_reference(X[b].T, X[b])
        _ratio("POTRI", S[b], ref, A.sum_bound(n, terms), what + " S")
        _bit_symmetric(S[b], what)


# ================================================================ the whole update ===============================================================
def _update_outputs(c, r):
    B, cs, act = c["B"], c["cs"], c["active"]
    names = ("T", "G", "g", "Csum", "Aout", "Sig", "U")
    out = {}
    for name, a in zip(names, r):
        if name == "U":                                                # in / out: an inactive slot keeps the case's values
            out[name], guard = A.split_guard(a, (B, cs))
            assert np.all(A.is_poison(guard)), "U: guard entries written"
            for b in np.flatnonzero(act == 0):
                assert np.array_equal(A.bits(out[name][b]), A.bits(c["U0"][b])), "U: slot %d written" % b
        elif name == "g":
            out[name] = _body(a, (B, cs), act, name)
        elif name == "Csum":
            out[name] = _body(a, (B,), act, name)
        else:
            out[name] = _mats(a, B, cs, act, name)
    return out


@pytest.mark.parametrize("cs,s_per_slot,a_per_slot,per_slot_scale", A.UPDATE_CASES)
def test_update_stage_by_stage(harness, tmp_path, cs, s_per_slot, a_per_slot, per_slot_scale):
    """launch_nes_update: the scatter's outputs are the bits launch_nes_scatter gives alone; T = S M against those bits, G = T S - C S against the
    device's T and C, A' = A + a_b A G against the device's G, Sigma' = A''A' against the device's A' (bit-symmetric), U - u_b S g against the device's
    g.  Shared and per-slot S and A, one scale or one per slot with another value in every slot.  Slot 2 alone (B = 1) gives the same bits"""
    c = A.update_case(cs, s_per_slot, a_per_slot, per_slot_scale)
    B, K = c["B"], c["K"]
    o = _update_outputs(c, _run(harness, tmp_path, c["data"]))
    Ms, gs, Cs = _scatter_outputs(c, _run(harness, tmp_path, c["scatter_data"]))
    for b in np.flatnonzero(c["active"]):
        what = "cs %d S %s A %s scales %s slot %d " % (cs, "own" if s_per_slot else "shared", "own" if a_per_slot else "shared", "own" if per_slot_scale else "one", b)
        S, Ain = c["S"][b if s_per_slot else 0], c["A"][b if a_per_slot else 0]
        assert np.array_equal(A.bits(o["g"][b]), A.bits(gs[b])) and np.array_equal(A.bits(o["Csum"][b]), A.bits(Cs[b])), what + "g, C differ from the scatter's"
        ref, terms = A.gemm_reference(S, Ms[b])
        _ratio("UPDATE", o["T"][b], ref, A.sum_bound(cs, terms), what + "T = S M")
        ref, terms = A.gemm_reference(o["T"][b], S, 1.0, D=S, beta=-o["Csum"][b])
        _ratio("UPDATE", o["G"][b], ref, A.sum_bound(cs, terms), what + "G = T S - C S")
        ref, terms = A.gemm_reference(Ain, o["G"][b], c["a_scale"][b], D=Ain, beta=1.0)
        _ratio("UPDATE", o["Aout"][b], ref, A.sum_bound(cs, terms), what + "A'")
        ref, terms = A.gemm_reference(o["Aout"][b].T, o["Aout"][b])
        _ratio("UPDATE", o["Sig"][b], ref, A.sum_bound(cs, terms), what + "Sigma'")
        _bit_symmetric(o["Sig"][b], what + "Sigma'")
        Sl, gl, u = S.astype(LD), o["g"][b].astype(LD), LD(c["u_scale"][b])
        ref = c["U0"][b].astype(LD) - u * (Sl @ gl)
        terms = np.abs(c["U0"][b].astype(LD)) + abs(u) * (np.abs(Sl) @ np.abs(gl))
        _ratio("UPDATE", o["U"][b], ref, A.sum_bound(cs, terms), what + "U")
    c1 = A.update_case(cs, s_per_slot, a_per_slot, per_slot_scale, single=True)
    o1 = _update_outputs(c1, _run(harness, tmp_path, c1["data"]))
    for name in o:
        assert np.array_equal(A.bits(o1[name][0]), A.bits(o[name][2])), name + ": slot 2 of B = 3 and the same slot alone differ"


# ================================================================ CMA ==========================================================================
@pytest.mark.parametrize("cs,per_slot", A.CMA_BEGIN_CASES)
def test_cma_begin_is_bit_exact(harness, tmp_path, cs, per_slot):
    c = A.cma_begin_case(cs, per_slot)
    B = c["B"]
    r = _run(harness, tmp_path, c["data"])
    scal, g0 = A.split_guard(r[0], (B, 8))
    vec, g1 = A.split_guard(r[1], (B, 3 * cs))
    sig2, g2 = A.split_guard(r[2], (B,))
    assert np.all(A.is_poison(g0)) and np.all(A.is_poison(g1)) and np.all(A.is_poison(g2))
    assert np.array_equal(A.bits(scal[:, 0]), A.bits(c["sigma0"])) and np.all(A.is_poison(scal[:, 1:]))
    assert not np.any(A.bits(vec))                                                          # +0.0 everywhere
    assert np.array_equal(A.bits(sig2), A.bits(c["sigma0"] * c["sigma0"]))


def _check_paths(harness, tmp_path, c):
    B, cs = c["B"], c["cs"]
    r = _run(harness, tmp_path, c["data"])
    Uo, g0 = A.split_guard(r[0], (B, cs))
    scal, g1 = A.split_guard(r[1], (B, 8))
    vec, g2 = A.split_guard(r[2], (B, 3 * cs))
    sig2 = _body(r[3], (B,), c["computed"], "sig2")
    assert np.all(A.is_poison(g0)) and np.all(A.is_poison(g1)) and np.all(A.is_poison(g2))
    for b in range(B):
        what = "cs %d K %d n %d %s slot %d " % (cs, c["K"], c["n_iter"], c["kind"], b)
        if not c["computed"][b]:
            assert np.array_equal(A.bits(Uo[b]), A.bits(c["U0"][b])) and np.array_equal(A.bits(scal[b]), A.bits(c["scal"][b])) and \
                   np.array_equal(A.bits(vec[b]), A.bits(c["vec"][b])), what + "inactive slot written"
            continue
        ps, pS, dw = vec[b, :cs], vec[b, cs:2 * cs], vec[b, 2 * cs:]
        ref = A.cma_paths_reference(c, b, ps_dev=ps)
        _ratio("CMA_PATHS", Uo[b], *ref["U"], what + "U")
        _ratio("CMA_PATHS", ps, *ref["ps"], what + "p_sigma")
        _ratio("CMA_PATHS", pS, *ref["pS"], what + "p_Sigma")
        assert np.array_equal(A.bits(dw), A.bits(c["vec"][b, 2 * cs:])), what + "dw written"
        _ratio("CMA_PATHS", scal[b, 3], *ref["nps"], what + "||p_sigma||")
        _ratio("CMA_PATHS", scal[b, 0], *ref["sigma"], what + "sigma")
        _ratio("CMA_PATHS", sig2[b], *ref["sig2"], what + "sigma^2")
        assert scal[b, 2] == ref["h"], what + "h_sigma %r, reference %d (margin %.3g)" % (scal[b, 2], ref["h"], ref["h_margin"])
        assert A.bits(scal[b, 4:5])[0] == A.bits(c["fro"][b:b + 1])[0] and np.array_equal(A.bits(scal[b, 5:]), A.bits(c["scal"][b, 5:]))
        if np.isnan(ref["ts"][0]):
            assert np.isnan(scal[b, 1]), what + "temp_sum %r where the IEEE result is NaN" % scal[b, 1]
        else:
            _ratio("CMA_PATHS", scal[b, 1], *ref["ts"], what + "temp_sum")
    return scal


@pytest.mark.parametrize("cs,K,m,n_iter,kind", A.CMA_PATHS_CASES)
def test_cma_paths(harness, tmp_path, cs, K, m, n_iter, kind):
    """U += sigma dw, p_sigma, ||p_sigma||, sigma, sigma^2, h_sigma, p_Sigma and temp_sum; K = 4097 enters the four-at-a-time loop a second time with one
    term; h_sigma on either side of its threshold at 1e-6 relative; a zero sample under a negative weight gives the NaN the IEEE formula gives"""
    c = A.cma_paths_case(cs, K, m, n_iter, kind)
    scal = _check_paths(harness, tmp_path, c)
    if kind in ("h_below", "h_above"):
        assert all(scal[b, 2] == (1.0 if kind == "h_below" else 0.0) for b in np.flatnonzero(c["computed"]))


def test_cma_paths_without_active(harness, tmp_path):
    _check_paths(harness, tmp_path, A.cma_paths_case(20, 192, 38, 3, "plain", use_active=False))


def _check_sigma(harness, tmp_path, c):
    B, cs = c["B"], c["cs"]
    r = _run(harness, tmp_path, c["data"])
    body, guard = A.split_guard(r[0], (B, cs * cs))
    assert np.all(A.is_poison(guard))
    for b in range(B):
        S = A.cm(body[b], cs)
        if not c["computed"][b]:
            assert np.array_equal(A.bits(S), A.bits(c["Sig"][b])), "inactive slot written"
            continue
        ref, bound = A.cma_sigma_reference(c["Sig"][b], c["scal"][b, 1], c["h"], c["vec"][b, cs:2 * cs], c["consts"])
        _ratio("CMA_SIGMA", S, ref, bound, "cs %d h %d slot %d" % (cs, c["h"], b))
        _bit_symmetric(S, "Sigma")


@pytest.mark.parametrize("cs,h", A.CMA_SIGMA_CASES)
def test_cma_sigma_update(harness, tmp_path, cs, h):
    """the rank-one update with and without the h_sigma correction; the upper triangle of the input drives both halves of a bit-symmetric result"""
    _check_sigma(harness, tmp_path, A.cma_sigma_case(cs, h))


def test_cma_sigma_update_without_active(harness, tmp_path):
    _check_sigma(harness, tmp_path, A.cma_sigma_case(17, 0, use_active=False))
