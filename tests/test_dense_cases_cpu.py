"""CPU side of the direct tests of the dense linear algebra (tests/test_gpu_dense_harness.py): the inputs, references and bounds of
tests/helpers/dense_cases.py are what they claim.  The file format round-trips; every A^-1/2 and sqrt(A) reference is certified (symmetric, positive
definite, Y A Y = I or S S = A to 1 / 100 of the case's tolerance); LAPACK factors every Cholesky input in float64 within the bound and rejects every
not-positive-definite one at the intended pivot; every shape of the case lists reaches the form, chunk count, round count, block count and columns per
cooperative workgroup its list names, computed from constants that are read back from the kernel sources -- a constant that moves fails here instead of
dropping an edge from the GPU file."""
import os
import re
import numpy as np
import pytest
from tests.helpers import dense_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = D.LD


def _src(name):
    with open(os.path.join(ROOT, "mpopis_amd", "csrc", name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"\b%s\s*=\s*([0-9.e+-]+)" % name, text)
    assert m, name
    return float(m.group(1))


# ---- constants ------------------------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_sources():
    lin, inv, eng, diag = _src("kernels_linalg.hip"), _src("kernels_invsqrt.hip"), _src("engine.h"), _src("linalg_diag.h")
    assert _const(diag, "kNB") == D.NB and _const(eng, "kPanelRows") == D.PANEL_ROWS
    assert _const(lin, "kRegMinPan") == D.REG_MIN_PAN and _const(lin, "kRegMaxPan") == D.REG_MAX_PAN and _const(lin, "kCoopMaxOwn") == D.COOP_MAX_OWN
    assert "kCoopPS = kNB + 1" in lin and D.COOP_PS == D.NB + 1
    body = lin[lin.index("PotrfForm potrf_form("):lin.index("void launch_potrf(")]
    assert body.count("150 * 1024") == 2 and D.LDS_LIMIT == 150 * 1024            # the LDS kernel's and the cluster's limit
    assert "env_G >= 0 ? env_G : %d;" % D.POTRF_G in body
    assert "(rows & 31) ? rows : rows + 16" in body and "B * G * share <= coop_max_workgroups()" in body
    assert _const(inv, "kLanTol") == D.LAN_TOL and _const(inv, "kTB") == D.TRI_B
    assert "kLanPrep = 4 + 2 * 64" in inv and D.LAN_PREP == 132
    assert "kLanRed = kLanWaves + 4 + 16" in inv and "kLanThreads = 1024" in inv and D.LAN_RED == 1024 // 64 + 20
    assert _const(inv, "kLanPivLds") == D.LAN_PIV_LDS
    grp = inv[inv.index("int invsqrt_coop_groups("):inv.index("void launch_lanczos_invsqrt(")]
    assert "env_G >= 0 ? env_G : %d;" % D.LAN_G in grp and "n < %d" % D.LAN_MIN_N in grp and "<= 150 * 1024 ? G : 1" in grp
    assert "(size_t)6 * n + 1 + kLanRed + 2 * kLanPivLds * 64 + (size_t)((n + G - 1) / G) * n" in grp and "(fixed + (size_t)4 * n)" in grp
    # the panel layout the test rebuilds is the one the kernel's comment states
    assert "[chunk = j / 16][p = (j & 3) 4 + ((j & 15) >> 2)][i < 128]" in lin
    # status codes and ranks
    hdr = open(os.path.join(ROOT, "include", "mpopis.h")).read()
    for name, v in (("MPOPIS_ERR_NOT_PD", D.ERR_NOT_PD), ("MPOPIS_ERR_NUMERIC", D.ERR_NUMERIC), ("MPOPIS_ERR_HIP", D.ERR_HIP), ("MPOPIS_ERR_ACTION", D.ERR_ACTION)):
        assert re.search(r"%s\s*=?\s*\(?(-\d+)" % name, hdr) and int(re.search(r"%s\s*=?\s*\(?(-\d+)" % name, hdr).group(1)) == v
    assert "c == MPOPIS_ERR_HIP ? 4 : c == MPOPIS_ERR_ACTION ? 3 : c == MPOPIS_ERR_NOT_PD ? 2 : c == MPOPIS_ERR_NUMERIC ? 1 : c < 0 ? 5 : 0" in eng
    assert D.status_after(D.OK, D.ERR_NOT_PD) == D.ERR_NOT_PD and D.status_after(D.ERR_NUMERIC, D.ERR_NOT_PD) == D.ERR_NOT_PD
    assert D.status_after(D.ERR_HIP, D.ERR_NOT_PD) == D.ERR_HIP and D.status_after(D.ERR_ACTION, D.ERR_NOT_PD) == D.ERR_ACTION
    assert D.status_after(D.ERR_NOT_PD, D.ERR_NUMERIC) == D.ERR_NOT_PD


# ---- files ----------------------------------------------------------------------------------------------------------------------------------------
def test_case_and_result_files_round_trip():
    cases = [D.potrf_case(17, "graded", shared=True, scaled=True), D.solve_case(2, "graded", False, True, True, True), D.gvec_case(2, True),
             D.trtri_case(17, "random", False, True, 2, True), D.invsqrt_case(3, ("cluster", "dec4"), in_vec=True, scaled=True), D.sym_sqrt_case(3, "dec4")]
    for c in cases:
        op, B, ipar, dpar, arrays = D.unpack_case(c["data"])
        assert B == c["B"] and ipar[0] == c["n"] and arrays[0][0] == D.I32 and arrays[0][1].size == B
        assert D.pack_case(op, B, ipar, dpar, [(t, a if a.size else None) for t, a in arrays]) == c["data"]
    op, B, ipar, dpar, arrays = D.unpack_case(cases[0]["data"])
    assert op == D.OP_POTRF and ipar == [17, 0, 1, 1, 1] and arrays[1][1].size == 289 and list(arrays[2][1]) == [0.25, 1.0, 9.0]
    assert np.array_equal(D.cm(arrays[1][1], 17), cases[0]["A"][0])
    op, B, ipar, dpar, arrays = D.unpack_case(cases[4]["data"])
    assert ipar == [3, 1, 1, 1, 9, 6] and arrays[3][1].size == 27
    bb = arrays[3][1].reshape(3, 9)
    assert np.all(D.is_poison(bb[:, :6])) and np.array_equal(bb[:, 6:], cases[4]["b"])
    body = np.arange(6.0).reshape(3, 2); body[1] = D.POISON_F64
    arr = np.concatenate([body.reshape(-1), np.full(D.GUARD, D.POISON_F64)])
    words = np.concatenate([np.zeros(6, dtype=np.uint64), np.full(D.GUARD, D.POISON_F64_BITS, dtype=np.uint64)])
    form, out = D.unpack_result(D.pack_result(D.POTRF_COOP | 6 << 8 | 8 << 16, [(D.F64, arr), (D.U64, words), (D.I32, np.full(D.GUARD + 1, D.POISON_I32))]))
    assert form == (D.POTRF_COOP, 6, 8)
    b, g = D.split_guard(out[0], (3, 2))
    assert np.all(D.is_poison(g)) and list(D.is_poison(b).all(axis=1)) == [False, True, False]
    w, g = D.split_guard(out[1], (6,))
    assert not np.any(w) and np.all(D.is_poison(g)) and np.all(D.is_poison(out[2]))


def test_single_slot_cases_carry_slot_two():
    for a, b in ((D.potrf_case(17, "graded", scaled=True), D.potrf_case(17, "graded", scaled=True, single=True)),
                 (D.potrf_case(17, "cma", shared=True, scaled=True), D.potrf_case(17, "cma", shared=True, scaled=True, single=True))):
        assert np.array_equal(a["A"][2], b["A"][0]) and a["scale"][2] == b["scale"][0] == 9.0 and list(a["active"]) == [1, 0, 1] and list(b["active"]) == [1]
    a, b = D.solve_case(5, "graded", False, True, True, True), D.solve_case(5, "graded", False, True, True, True, single=True)
    assert np.array_equal(a["L"][2], b["L"][0]) and np.array_equal(a["U"][2], b["U"][0]) and a["gamma"][2] == b["gamma"][0] == 0.0 and a["isc"][2] == b["isc"][0]
    a, b = D.trtri_case(17, "graded", False, True, 2, True), D.trtri_case(17, "graded", False, True, 2, True, single=True)
    assert np.array_equal(a["L"][2], b["L"][0]) and np.array_equal(a["A"][2], b["A"][0]) and a["scale"][2] == b["scale"][0]
    a, b = D.invsqrt_case(5, ("cluster", "dec4"), scaled=True), D.invsqrt_case(5, ("cluster", "dec4"), scaled=True, single=True)
    assert np.array_equal(a["A"][2], b["A"][0]) and np.array_equal(a["b"][2], b["b"][0]) and a["scale"][2] == b["scale"][0]


# ---- Cholesky: forms and edges -------------------------------------------------------------------------------------------------------------------
def test_potrf_shapes_reach_their_forms():
    for n in D.POTRF_LDS_NS:
        assert D.potrf_form(3, n) == (D.POTRF_LDS, 0)
    assert D.potrf_form(3, 128)[0] == D.POTRF_LDS and D.potrf_form(3, 129)[0] != D.POTRF_LDS
    assert {n: D.potrf_form(3, n) for n in D.POTRF_COOP_NS} == {129: (D.POTRF_COOP, 6), 144: (D.POTRF_COOP, 6), 145: (D.POTRF_COOP, 6), 240: (D.POTRF_COOP, 6),
                                                                305: (D.POTRF_COOP, 6), 320: (D.POTRF_COOP, 6), 400: (D.POTRF_GLOBAL, 0)}
    # n = 400: five owned panels of workgroup 0 + the strip need more than 150 KiB; a panel count that G = 6 does not divide: 9, 10, 15, 20
    assert [(n + 15) // 16 % 6 for n in (129, 144, 145, 240, 305, 320)] == [3, 3, 4, 3, 2, 2]
    for n in D.POTRF_REG_NS:
        assert D.potrf_form(3, n) == (D.POTRF_REG, 0) and D.potrf_form(3, n, reg=False) == (D.POTRF_COOP, 6)
    assert D.potrf_form(3, 240)[0] == D.POTRF_COOP and D.potrf_form(3, 241)[0] == D.POTRF_REG and D.potrf_form(3, 304)[0] == D.POTRF_REG
    assert sorted({(n + 15) // 16 for n in D.POTRF_REG_NS}) == [16, 17, 18, 19]
    for n in D.POTRF_GLOBAL_NS:
        assert D.potrf_form(3, n, coop=False, reg=False) == (D.POTRF_GLOBAL, 0)
        assert D.potrf_form(3, n, reg=False, G=0) == (D.POTRF_GLOBAL, 0)
        assert D.potrf_form(2, n, reg=False, max_wg=8) == (D.POTRF_GLOBAL, 0)                     # 2 x 6 workgroups > 8
        assert D.potrf_form(1, n, reg=False, max_wg=8)[0] == (D.POTRF_GLOBAL if n == 400 else D.POTRF_COOP)
    ids = [i for i, _ in D.potrf_cases()]
    assert len(ids) == len(set(ids))
    for name, kw in D.potrf_cases():
        c = D.potrf_case(**kw)
        assert D.expected_form(c)[0] == kw["expect"] == c["expect"], name
        assert name.split("-")[0] == D.FORM_NAMES[kw["expect"]] or name == "coop-400", name
        assert int(c["env"].get("MPOPIS_COOP_MAX_WG", D.MAX_WG)) <= D.MAX_WG
    for form, kw in D.FORM_CASES.items():
        assert D.FORM_NAMES[D.expected_form(D.potrf_case(**kw))[0]] == form
    # every option meets every form
    for form in range(4):
        cs = [D.potrf_case(**kw) for _, kw in D.potrf_cases() if kw["expect"] == form]
        assert {c["shared"] for c in cs} == {False, True} and {c["scaled"] for c in cs} == {False, True} and {c["kind"] for c in cs} == {"cma", "graded"}, form
        assert {c["use_active"] for c in cs} == {False, True}, form


def test_lds_shapes_reach_every_round_and_chunk_count():
    e = {n: D.lds_edges(n) for n in D.POTRF_LDS_NS}
    assert {v[2] for v in e.values()} == {1, 2, 3, 4}                                           # sub-block rounds of the last diagonal block
    assert [e[n][2] for n in (1, 3, 4, 5, 12, 13, 16, 17)] == [1, 1, 1, 2, 3, 4, 4, 1]
    assert {v[0]: v[1] for v in e.values()} == {16: 1, 32: 1, 48: 1, 64: 2, 80: 2, 112: 2, 128: 3}
    assert e[100] == (112, 2, 1) and e[113] == (128, 3, 1) and e[127] == (128, 3, 4) and e[65][0] == 80
    assert D.panel_doubles(128) == 8 * 16 * 128 and D.panel_doubles(1) == 16 * 128 and D.panel_doubles(129) == 0
    L = np.tril(np.arange(1.0, 401.0).reshape(20, 20))
    P = D.panel_of(L).reshape(2, 16, 128)
    assert P[0, 4, 1] == L[1, 1] and P[0, 1, 9] == L[9, 4] and P[1, 12, 19] == L[19, 19] and P[1, 0, 15] == 0.0 and P[1, 4, 16] == 0.0 and P[1, 4, 19] == L[19, 17] and P[0, 0, 20] == 0.0
    assert np.count_nonzero(P) == 210


def test_potrf_inputs_are_what_they_claim():
    for n, kind in ((1, "cma"), (17, "graded"), (100, "cma"), (145, "graded"), (300, "graded")):
        A = D.spd(n, kind, 42)
        assert np.array_equal(A, A.T)
        for s in D.SCALES:
            L = np.linalg.cholesky(s * A)
            err, bound = D.potrf_residual(A, s, L)
            assert np.all(err <= bound), (n, kind)
            assert np.max(err / bound) < 0.5                                                     # LAPACK sits well inside; a wrong entry is ~1e12 bounds away
            Lw = L.copy(); Lw[n - 1, 0] *= 1 + 1e-9
            e2, _ = D.potrf_residual(A, s, Lw)
            assert np.any(e2 > bound)
    d = np.diag(D.spd(300, "graded", 42))
    assert 1e7 < d.max() / d.min() < 1e9                                                         # graded over 8 decades
    c = D.potrf_case(17, upper=True)
    op, B, ipar, dpar, arrays = D.unpack_case(c["data"])
    Ain = D.cm(arrays[1][1][:289], 17)
    assert np.all(Ain[np.triu_indices(17, 1)] == 1e300) and np.array_equal(np.tril(Ain), np.tril(c["A"][0]))


@pytest.mark.parametrize("form", sorted(D.FORM_CASES))
@pytest.mark.parametrize("where", D.NOTPD)
def test_not_pd_inputs_fail_at_the_intended_pivot(form, where):
    n = D.FORM_CASES[form]["n"]
    c = D.potrf_case(notpd=where, scaled=True, **D.FORM_CASES[form])
    A = c["A"][0]
    p, (i, j) = D.notpd_position(n, where)
    npan = (n + 15) // 16
    assert {"first": p // 16 == 0, "interior": 0 < p // 16 < npan - 1, "last": p // 16 == npan - 1 and n % 16 != 0}.get(where, 0 < p // 16 < npan - 1)
    if where == "nan_off":
        assert i == p and j < p and j // 16 < p // 16 and np.isnan(A[i, j]) and np.isnan(A[j, i]) and np.sum(np.isnan(A)) == 2
    try:                                                                                        # LAPACK's dpotrf rejects a non-positive pivot; whether it rejects a NaN one
        Lf = np.linalg.cholesky(A)                                                              # or hands the NaN on depends on the build behind NumPy
        assert where.startswith("nan") and np.isnan(Lf[p, p]) and not np.any(np.isnan(Lf[:p, :p]))
    except np.linalg.LinAlgError:
        pass
    if p > 0:
        np.linalg.cholesky(A[:p, :p])                                                           # everything before the pivot factors
    good = D.spd(n, "cma", 40)
    Lg = np.linalg.cholesky(good[:p + 1, :p + 1].astype(np.float64))
    piv = A[p, p] - np.sum(Lg[p, :p].astype(LD) ** 2) if where != "nan_off" else np.nan         # nan_off: row p of L holds the NaN, so its pivot does
    assert not (piv > 0)
    assert list(c["active"]) == [1, 0, 1] and c["status"][0] == D.NOTPD_STATUS[where]
    np.linalg.cholesky(c["A"][2])


# ---- SOLVE / TRTRI --------------------------------------------------------------------------------------------------------------------------------
def test_solve_and_gvec_references():
    assert {c[0] for c in D.SOLVE_CASES} == set(D.SOLVE_NS) and {c[0] for c in D.GVEC_CASES} == set(D.SOLVE_NS)
    for k in range(2, 6):
        assert {c[k] for c in D.SOLVE_CASES} == {False, True}
    for n in (255, 257):
        assert sorted({c[2] for c in D.SOLVE_CASES if c[0] == n}) == [False, True]
    c = D.solve_case(40, "graded", False, True, True, True)
    for b in (0, 2):
        L = c["L"][b]
        y = np.linalg.solve(L, c["gamma"][b] * c["U"][b])
        g = np.linalg.solve(L.T, y) / c["isc"][b]
        err, bound = D.solve_residual(L, c["gamma"][b], c["U"][b], g, c["isc"][b])
        assert np.all(err <= bound)
        if b == 0:
            gw = g.copy(); gw[3] *= 1 + 1e-8
            e2, _ = D.solve_residual(L, c["gamma"][b], c["U"][b], gw, c["isc"][b])
            assert np.any(e2 > bound)
    assert c["gamma"][2] == 0.0 and not np.any(g)
    a, b = D.gvec_case(33, True), D.gvec_case(33, True, single=True)
    assert np.array_equal(a["U"][2], b["U"][0]) and a["gamma"][2] == b["gamma"][0] == 2.0 and a["gamma"][1] == 0.0 and np.array_equal(a["S"], b["S"])
    assert len(set(D.GVEC_CASES)) == len(D.GVEC_CASES)
    c = D.gvec_case(33, True)
    ref, terms = D.gvec_reference(c["S"], c["U"][0], c["gamma"][0])
    got = (c["gamma"][0] * c["U"][0]) @ c["S"]
    assert np.all(np.abs(got - ref) <= D.sum_bound(33, terms)) and np.all(np.abs(ref) <= terms)


def test_trtri_shapes_and_reference():
    t = {n: D.trtri_blocks(n) for n in D.TRTRI_NS}
    assert {v[0] for v in t.values()} >= {1, 2, 3} and t[1] == (1, 1, True, 1) and t[17] == (2, 1, False, 1) and t[33] == (3, 2, True, 1)
    assert t[48] == (3, 2, True, 16) and t[100] == (7, 4, True, 4) and t[300] == (19, 10, True, 12) and t[301] == (19, 10, True, 13) and t[400] == (25, 13, True, 16)
    assert t[15][3] == 15 and t[16] == (1, 1, True, 16) and t[31] == (2, 1, False, 15) and t[32] == (2, 1, False, 16)
    assert {c[0] for c in D.TRTRI_CASES} == set(D.TRTRI_NS) and len(set(D.TRTRI_CASES)) == len(D.TRTRI_CASES)
    for n in D.TRTRI_NS:
        cs = [c for c in D.TRTRI_CASES if c[0] == n]
        assert {c[1] for c in cs} == {"random", "graded"} and {c[3] for c in cs} == {False, True} and len({c[4] for c in cs}) == 2
    assert {c[4] for c in D.TRTRI_CASES} == {0, 1, 2} and {c[2] for c in D.TRTRI_CASES} == {False, True} and {c[5] for c in D.TRTRI_CASES} == {False, True}
    n = 37
    L = D.potri_factor(n, "graded", 31)
    part, bound = D.trtri_reference(L)
    X = np.linalg.inv(L)
    got = np.array([np.sum(X[16 * J:, 16 * J:16 * J + 16] ** 2) for J in range(3)])
    assert np.all(np.abs(got - part) <= bound) and np.all(bound < 1e-9 * part)
    assert abs(float(np.sum(part)) - np.trace(np.linalg.inv(L @ L.T))) < 1e-9 * float(np.sum(part))
    d = np.diag(L)
    assert d.max() / d.min() > 1e3                                                               # graded: standard deviations over 4 decades


def test_quadrature_reference():
    """the float64 NumPy evaluation equals the header's formulas (a C++ host build would give the same up to libm); the longdouble evaluation approximates
    x^-1/2 to the error the header states, and the tolerance built from the two is small"""
    for m, M in ((0.01, 1.0), (3e-9, 2.5), (2e-13, 7.0)):
        s64, w64 = D.quad_nodes(m, M, np.float64)
        sl, wl = D.quad_nodes(m, M, LD)
        assert np.all(s64 > 0) and np.all(w64 > 0) and np.all(np.diff(s64) > 0)
        xs = D.quad_xs(m, M)
        assert float(xs[0]) == pytest.approx(m) and float(xs[-1]) == pytest.approx(M) and len(xs) == 200
        trunc = float(np.max(np.abs(D.quad_eval(sl, wl, xs))))
        assert trunc < (1e-15 if M / m <= 1e12 else 1e-13), (m, M, trunc)
        tol, meas = D.quad_tolerance(m, M)
        assert 64 * D.U <= tol < 1e-9 and tol >= 8 * meas
        bad = w64.copy(); bad[17] *= 1 + 1e-6
        assert np.max(np.abs(D.quad_eval(s64, bad, xs))) > 10 * tol
    c = D.trtri_case(17, "graded", False, True, 2, True)
    assert set(c["quad_tol"]) == {0, 2}


# ---- A^-1/2 and sqrt(A) ---------------------------------------------------------------------------------------------------------------------------
def _distinct_invsqrt():
    seen, out = set(), []
    for n, spectra, coop, regions, in_vec, scaled in D.INVSQRT_CASES:
        for slot, spec in ((0, spectra[0]), (2, spectra[1])):
            if (n, spec, slot) not in seen:
                seen.add((n, spec, slot)); out.append((n, spec, slot))
    return out


@pytest.mark.parametrize("n,spec,slot", _distinct_invsqrt())
def test_invsqrt_references_are_certified(n, spec, slot):
    """Y symmetric positive definite with Y A Y = I to 1 / 100 of the relative tolerance: Y is A^-1/2.  The float64 eigh route, which is what the
    reference's Sigma^-0.5 does, is further from it than the tolerance's first term by construction (factor 8)."""
    c = D.invsqrt_case(n, (spec, spec) if slot == 0 else ("cluster", spec))
    r = D.invsqrt_reference(c, slot)
    Y, A = r["Y"], c["A"][slot].astype(LD)
    assert np.array_equal(Y, Y.T) and np.array_equal(c["A"][slot], c["A"][slot].T)
    np.linalg.cholesky(Y.astype(np.float64))
    np.linalg.cholesky(c["A"][slot])
    tol, (t1, t2) = D.invsqrt_tolerance(r, r["Minf"])
    resid = float(np.max(np.abs(Y @ A @ Y - np.eye(n, dtype=LD))))
    print("n %d %s: residual %.2e, eigh64 off by %.2e relative, tolerance %.2e relative (terms %.2e %.2e)" % (n, spec, resid, r["eigh_err"] / r["ny"], tol / r["ny"],
                                                                                                            t1, t2))
    assert resid <= tol / r["ny"] / 100
    assert t2 > 0 and tol / r["ny"] < (1e-4 if spec == "dec12" else 1e-7 if spec == "dec8" else 1e-10)
    lam = c["lam"][slot]
    assert lam.min() > 0
    fro, M = float(np.sum(1 / lam.astype(LD))), r["Minf"]
    assert min(1 / fro, M / 2) / M > 1e-14                                                       # inside the quadrature's range: the Lanczos path, not the dense one
    if spec.startswith("dec") and n > 2:
        assert 10 ** (float(spec[3:]) - 1) < lam.max() / lam.min() <= 10 ** float(spec[3:]) * 1.01


def test_invsqrt_case_lists_reach_their_edges():
    assert {c[0] for c in D.INVSQRT_CASES} == set(D.INVSQRT_NS)
    for n in D.INVSQRT_NS:
        specs = {s for c in D.INVSQRT_CASES if c[0] == n for s in c[1]}
        assert specs >= {"cluster", "dec4", "dec8"} and (("dec12" in specs) == (n == 160))
        assert {c[4] for c in D.INVSQRT_CASES if c[0] == n} == {False, True} and {c[5] for c in D.INVSQRT_CASES if c[0] == n} == {False, True}
    g = {n: D.lanczos_groups(3, n) for n in D.INVSQRT_NS}
    assert g == {1: 1, 2: 1, 17: 1, 64: 1, 100: 1, 159: 1, 160: 8, 161: 8, 300: 8, 304: 8, 400: 1}          # n = 400: the column slab no longer fits
    assert [-(-n // 8) for n in (160, 161, 300, 304)] == [20, 21, 38, 38] and [n % 8 for n in (160, 161, 300, 304)] == [0, 1, 4, 0]
    assert D.lanczos_groups(3, 300, coop=False) == 1 and D.lanczos_groups(3, 300, regions=False) == 1 and D.lanczos_groups(9, 300) == 1
    for n, spectra, coop, regions, in_vec, scaled in D.INVSQRT_CASES:
        if n in (160, 161, 300, 304) and spectra != ("dec12", "cluster"):
            assert D.lanczos_groups(3, n, coop, regions) == 8
    for n, spectra, coop, regions in D.INVSQRT_SOLO:
        assert D.lanczos_groups(3, n) == 8 and D.lanczos_groups(3, n, coop, regions) == 1
        assert any(c[0] == n and c[1] == spectra for c in D.INVSQRT_CASES)
    assert {(c[2], c[3]) for c in D.INVSQRT_SOLO} == {(False, True), (True, False)}
    for n, spectra, in_vec, scaled in D.INVSQRT_NOACTIVE:                                        # nullptr active: every slot computed, matrices certified above
        c = D.invsqrt_case(n, spectra, True, True, in_vec, scaled, use_active=False)
        assert list(c["computed"]) == [1, 1, 1] and D.unpack_case(c["data"])[2][1] == 0 and np.array_equal(c["A"][1], c["A"][0]) and not np.array_equal(c["b"][1], c["b"][0])
        assert any(k[0] == n and k[1][0] == spectra[0] for k in D.INVSQRT_CASES) and any(k[0] == n and k[1][1] == spectra[1] for k in D.INVSQRT_CASES)
    assert sorted(D.lanczos_groups(3, c[0]) for c in D.INVSQRT_NOACTIVE) == [1, 8, 8]
    for n, dec in ((20, 16), (20, 18), (300, 16), (300, 18)):
        A = D.dense_case(n, dec)["A"][0]
        M = np.max(np.sum(np.abs(A), axis=0))
        fro = float(np.sum(1 / np.diag(A).astype(LD)))                                           # tr(A^-1) >= sum 1 / a_ii
        assert min(1 / fro, M / 2) / M < 1e-14                                                   # beyond the quadrature: the dense fall-back


@pytest.mark.parametrize("n,spec", D.SYM_SQRT_CASES)
def test_sym_sqrt_references_are_certified(n, spec):
    c = D.sym_sqrt_case(n, spec)
    S, tol, (t1, t2) = D.sym_sqrt_reference(c)
    assert np.array_equal(S, S.T)
    np.linalg.cholesky(S.astype(np.float64))
    resid = float(np.sqrt(np.sum((S @ S - c["A"].astype(LD)) ** 2)))
    nS = float(np.sqrt(np.sum(S * S)))
    print("n %d %s: ||S S - A||_F %.2e, tolerance %.2e (8 x eigh64 %.2e, floor %.2e), ||S||_F %.2e" % (n, spec, resid, tol, t1, t2, nS))
    # S S - A = S dS + dS S: ||dS||_F <= resid / (2 sqrt(lambda_min)); held to 1 / 100 of the tolerance
    assert resid / (2 * np.sqrt(c["lam"].min())) <= tol / 100
    assert tol < 1e-8 * nS


def test_sym_sqrt_bad_inputs():
    assert {c[0] for c in D.SYM_SQRT_CASES} == set(D.SYM_SQRT_NS)
    for bad, lo, hi in (("indefinite", -1.1e-3, -0.9e-3), ("singular", -1e-15, 1e-15)):
        for n in (16, 17, 100):
            c = D.sym_sqrt_case(n, "cluster", bad=bad)
            w = np.linalg.eigvalsh(c["A"])
            assert lo < w[0] < hi and w[1] > 0.01 and np.array_equal(c["A"], c["A"].T)
            if bad == "singular":                                                                # exactly singular: a zero row and column, whatever the arithmetic
                assert not np.any(c["A"][n // 2]) and not np.any(c["A"][:, n // 2]) and np.count_nonzero(np.diag(c["A"])) == n - 1
