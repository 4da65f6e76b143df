"""CPU side of the direct tests of the adaptation kernels (tests/test_gpu_adapt_harness.py): the inputs and references of tests/helpers/adapt_cases.py
are what they claim.  The file format round-trips; the NES references agree with tests/helpers/nes_ref.py; the CMA references, chained for one update,
reproduce the oracle's :cmamppi; every h_sigma and early-break case sits on its intended side in longdouble; and every shape of the case lists reaches
the pair-block, empty-split and columns-per-workgroup counts its table names, computed from constants that are read back from the kernel sources --
a constant that moves fails here instead of dropping an edge from the GPU file."""
import os
import re
import numpy as np
import pytest
from tests.helpers import adapt_cases as A
from tests.helpers import nes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = A.LD


def _src(name):
    with open(os.path.join(ROOT, "mpopis_amd", "csrc", name)) as f:
        return f.read()


def _cases():
    return [A.break_case(257), A.break_nonfinite_case(), A.scatter_case(17, 33, 3, "zero"), A.potri_case(3, "graded", True, True),
            A.update_case(3, True, False, True), A.cma_begin_case(1, True), A.cma_paths_case(20, 192, 38, 3, "zero"), A.cma_sigma_case(16, 0)]


def test_case_files_round_trip():
    for c in _cases():
        op, B, ipar, dpar, arrays = A.unpack_case(c["data"])
        assert B == c["B"] and arrays[0][0] == A.I32 and arrays[0][1].size == B
        again = A.pack_case(op, B, ipar, dpar, [(t, a if a.size else None) for t, a in arrays])
        assert again == c["data"]
    c = A.update_case(17, False, True, False)
    op, B, ipar, dpar, arrays = A.unpack_case(c["data"])
    assert op == A.OP_UPDATE and ipar == [17, A.UPDATE_K, A.UPDATE_KSPLIT, 0, 17 * 17] and dpar == [c["a_scale"][0], c["u_scale"][0]]
    assert arrays[3][1].size == 17 * 17 and arrays[4][1].size == 3 * 17 * 17 and arrays[6][1].size == 0 and arrays[7][1].size == 0
    assert np.array_equal(A.cm(arrays[4][1][2 * 289:], 17), c["A"][2])


def test_result_files_round_trip():
    rng = np.random.default_rng(0)
    body = rng.standard_normal((3, 5))
    body[1] = A.POISON_F64
    arr = np.concatenate([body.reshape(-1), np.full(A.GUARD, A.POISON_F64)])
    flags = np.concatenate([np.array([1, 0, A.POISON_I32], dtype=np.int32), np.full(A.GUARD, A.POISON_I32, dtype=np.int32)])
    out = A.unpack_result(A.pack_result([(A.F64, arr), (A.I32, flags)]))
    b, g = A.split_guard(out[0], (3, 5))
    assert np.array_equal(A.bits(b), A.bits(body)) and np.all(A.is_poison(g)) and np.all(A.is_poison(b[1])) and not np.any(A.is_poison(b[0]))
    f, g = A.split_guard(out[1], (3,))
    assert list(A.is_poison(f)) == [False, False, True] and np.all(A.is_poison(g))
    M = rng.standard_normal((4, 4))
    assert np.array_equal(A.cm(A.to_cm(M), 4), M) and A.to_cm(M)[1] == M[1, 0]


def test_single_slot_cases_carry_slot_two():
    """the determinism check compares slot 2 of B = 3 with B = 1: both must hold the same inputs"""
    a, b = A.update_case(17, True, True, True), A.update_case(17, True, True, True, single=True)
    for k in ("E", "cost", "S", "A", "U0", "a_scale", "u_scale"):
        assert np.array_equal(a[k][2], b[k][0]), k
    a, b = A.update_case(16, False, False, False), A.update_case(16, False, False, False, single=True)
    assert np.array_equal(a["S"][0], b["S"][0]) and a["a_scale"][2] == b["a_scale"][0] and a["u_scale"][2] == b["u_scale"][0]
    assert list(a["active"]) == [1, 0, 1] and list(b["active"]) == [1]


# ---- references -----------------------------------------------------------------------------------------------------------------------------------
def test_nes_references_agree_with_the_policy_reference():
    cs, K = 6, 40
    E, c = A.slot_samples(cs, K, "generic", 3)
    L = A.potri_factor(cs, "random", 1)
    X, S = A.potri_reference(L)
    Sinv = nes_ref.inv_from_chol(L)
    assert np.allclose(S.astype(np.float64), Sinv, rtol=1e-11, atol=0)
    err, bound = A.trtri_residual(L, X.astype(np.float64))
    assert np.all(err <= bound)
    assert np.all(np.triu(X, 1) == 0)
    G, Sg = A.nes_gradients_ld(E, c, Sinv)
    G64, Sg64 = nes_ref.nes_gradients(E, c, Sinv)
    assert np.allclose(G.astype(np.float64), G64, rtol=0, atol=1e-11 * np.abs(G64).max())
    assert np.allclose(Sg.astype(np.float64), Sg64, rtol=0, atol=1e-11 * np.abs(Sg64).max())
    # the staged references of the GPU file, chained, are the same G
    (M, g, C), (tM, tg, tC) = A.scatter_reference(E, c)
    T, _ = A.gemm_reference(Sinv, M)
    G2, _ = A.gemm_reference(T, Sinv, 1.0, D=Sinv, beta=-C)
    assert np.allclose(G2.astype(np.float64), G64, rtol=0, atol=1e-11 * np.abs(G64).max())
    assert np.all(np.abs(M) <= tM) and np.all(np.abs(g) <= tg) and abs(C) <= tC
    # the cancelling costs cancel
    _, cc = A.slot_samples(cs, K, "cancel", 0)
    assert np.any(cc > 0) and np.any(cc < 0) and abs(cc.sum()) < 1e-6 * np.abs(cc).sum()
    assert not np.any(A.slot_samples(cs, K, "zero", 0)[1])


def test_cma_references_chain_to_the_oracle(oracle):
    """one :cmamppi update (N = 2) on a mountaincar env at K = 32, T = 4: Sigma_last = sigma'^2 Sigma' and U_last of the oracle against the paths and
    Sigma references chained, with the constants and weights restated from init_cma_constants"""
    K, T, sigma0 = 32, 4, 0.7
    env = oracle.OracleEnv("mountaincar")
    env.state = [0.4, 0.05]                     # close to the goal: the elite costs differ by more than the early-break tolerance
    pol = oracle.OraclePolicy("cmamppi", env, K, T, lam=1.0, cov=[0.5], N=2, elite_threshold=0.5, cma_sigma=sigma0)
    cs, m_elite = pol.cs, int(pol.p.m_elite)
    assert cs == 4 and m_elite == 16
    consts, ws = A.cma_constants(cs, K, m_elite)
    assert np.allclose(ws, pol.cma_ws, rtol=1e-14, atol=0)
    assert np.allclose(consts, [pol.p.mu_eff, pol.p.c_sigma, pol.p.d_sigma, pol.p.c_Sigma, pol.p.c1, pol.p.c_mu, pol.p.E_cma], rtol=1e-14, atol=0)
    Sig0, U0 = pol.Sigma, pol.U
    Z = np.random.default_rng(5).standard_normal((2, K, cs))
    out = pol(env.copy(), Z)
    assert out["status"] == 0 and out["iters_run"] == 2
    # iteration 1 as the policy runs it: E = chol(sigma^2 Sigma) Z, costs, sortperm, dw (:550-576); C = Sigma^-0.5 (:580)
    E = np.linalg.cholesky(sigma0 * sigma0 * Sig0) @ Z[0].T
    cost = pol.simulate_model(U0, E, None, U0)
    order = np.argsort(cost, kind="stable").astype(np.int32)
    dw = E[:, order[:m_elite]] @ ws[:m_elite]
    lam, V = np.linalg.eigh(Sig0)
    C = (V / np.sqrt(lam)) @ V.T
    c = dict(cs=cs, K=K, n_iter=1, consts=consts, ws=ws, E=E[None], order=order[None], y=(C @ dw)[None], fro=np.array([np.sum(C * C)]), U0=U0[None],
             scal=np.array([[sigma0, 0, 0, 0, 0, 0, 0, 0.0]]), vec=np.concatenate([np.zeros(2 * cs), dw])[None])
    r = A.cma_paths_reference(c, 0)
    S1, _ = A.cma_sigma_reference(Sig0, r["ts"][0], r["h"], r["pS"][0], consts)
    assert np.isfinite(float(r["ts"][0])) and float(r["sigma"][0]) != sigma0
    got = (r["sig2"][0] * S1).astype(np.float64)
    assert np.allclose(got, out["Sigma_last"], rtol=1e-12, atol=1e-13 * np.abs(got).max()), np.abs(got - out["Sigma_last"]).max()
    assert np.allclose(r["U"][0].astype(np.float64), out["U_last"], rtol=1e-12, atol=1e-14)
    assert np.any(r["U"][0] != U0)


def test_temp_sum_zero_sample_is_nan_only_under_a_negative_weight():
    c = A.cma_paths_case(20, 192, 38, 3, "zero")
    for b in range(c["B"]):
        t = A.temp_sum_terms(c["E"][b], c["order"][b], c["ws"], c["scal"][b, 0], c["fro"][b], 3)
        assert np.sum(np.isnan(t)) == 1 and c["ws"][np.flatnonzero(np.isnan(t))[0]] < 0
        assert np.isnan(A.cma_paths_reference(c, b)["ts"][0])
    ws = np.array([0.5, -0.25]); E = np.array([[0.0, 2.0]])
    t = A.temp_sum_terms(E, np.array([0, 1], dtype=np.int32), ws, 2.0, 3.0, 5)           # d = 0 under w >= 0: 0;  d = 1 under w < 0: n w / fro
    assert t[0] == 0 and abs(t[1] - LD(5) * LD(-0.25) / 3) < 1e-18
    t = A.temp_sum_terms(E, np.array([1, 0], dtype=np.int32), ws, 2.0, 3.0, 5)           # linear index 1 -> column order[1] = 0: the zero again under w >= 0
    assert t[0] == 0 and abs(t[1] - LD(5) * LD(-0.25) / 3) < 1e-18
    t = A.temp_sum_terms(E, np.array([0, 1], dtype=np.int32), ws[::-1], 2.0, 3.0, 5)     # the zero under the negative weight: -inf 0 0
    assert np.isnan(t[0]) and t[1] == 0.5


# ---- the cases sit where they claim ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs,K,m,n_iter,kind", A.CMA_PATHS_CASES)
def test_h_sigma_cases_sit_on_their_side(cs, K, m, n_iter, kind):
    assert cs * m >= K
    c = A.cma_paths_case(cs, K, m, n_iter, kind)
    assert all(sorted(o) == list(range(K)) for o in c["order"])
    for b in range(c["B"]):
        r = A.cma_paths_reference(c, b)
        if kind == "h_below":
            assert r["h"] == 1 and -1.5 * A.H_REL < r["h_margin"] < -0.5 * A.H_REL
        elif kind == "h_above":
            assert r["h"] == 0 and 0.5 * A.H_REL < r["h_margin"] < 1.5 * A.H_REL
        else:
            assert abs(r["h_margin"]) > 1e-3                    # far from the threshold: no rounding decides it
        # the threshold in the form the kernel evaluates it and in the form the cases are placed with agree
        nps = float(r["nps"][0])
        assert (nps < A.h_threshold(cs, n_iter, c["consts"])) == bool(r["h"])
    if kind == "plain":
        hs = {A.cma_paths_reference(A.cma_paths_case(*s, n, "plain"), 0)["h"] for s in A.CMA_PATHS_SHAPES for n in (1, 3)}
        assert hs == {0, 1}                                     # the plain cases alone already take both sides


@pytest.mark.parametrize("K", A.BREAK_KS)
def test_break_cases_sit_on_their_side(K):
    c = A.break_case(K)
    below = np.nextafter(A.BREAK_TOL, 0.0)
    act, st = A.break_ref(c["cost"], c["active"], c["status"])
    assert np.array_equal(st, c["status"])
    seen = set()
    for b, intent in enumerate(c["intent"]):
        d = np.abs(np.diff(c["cost"][b].astype(LD)))
        d64 = np.abs(np.diff(c["cost"][b]))                                     # what the device forms: the rounding decides nothing
        assert (d64.max() < A.BREAK_TOL) == (d.max() < LD(A.BREAK_TOL)) and np.argmax(d64) == np.argmax(d)
        assert d64.max() == d.max() or abs(d.max() / LD(A.BREAK_TOL) - 1) > 0.09
        if intent == "inactive":
            assert act[b] == 0 and c["active"][b] == 0
            continue
        assert act[b] == (1 if intent == "stay" else 0), (b, intent)
        mx, at = d.max(), int(np.argmax(d))
        assert (mx >= LD(A.BREAK_TOL)) == (intent == "stay")
        if mx in (LD(A.BREAK_TOL), LD(below)):
            assert np.sum(d > 2.1e-3) == 1
            seen.add((at, float(mx)))
    want = {(p, float(v)) for p in {0, K - 2} | ({255} if K >= 257 else set()) for v in (A.BREAK_TOL, below)}
    assert seen == want
    assert "inactive" in c["intent"] or K == 1000                               # (K = 1000 spends all eight slots on the three pairs)


def test_break_nonfinite_case():
    c = A.break_nonfinite_case()
    act, st = A.break_ref(c["cost"], c["active"], c["status"])
    assert list(act) == [0, 0, 0, 0, 0, 0, 0, 1]
    assert list(st) == [A.ERR_ACTION, A.ERR_ACTION, A.ERR_ACTION, A.ERR_HIP, A.ERR_ACTION, A.ERR_ARG, A.ERR_NUMERIC, A.ERR_NOT_PD]


def test_kernel_constants_are_the_ones_the_tables_assume():
    nes, cma, eng = _src("kernels_nes.hip"), _src("kernels_cma.hip"), _src("engine.h")
    m = re.search(r"constexpr int kNesKC = (\d+), kNesS = kNesKC \+ 1, kNesPW = (\d+), kNesPB = (\d+) \* kNesPW;", nes)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (A.NES_KC, A.NES_PW, A.NES_WAVES)
    assert "static int nes_nt(int cs) { return cs / 16 + 1; }" in nes
    assert "const int per = ((K + ksplit - 1) / ksplit + kNesKC - 1) / kNesKC * kNesKC;" in nes
    m = re.search(r"nes_trtri_cpb\(int n\) \{ return std::max\(1, std::min\((\d+), \((\d+) \* 1024 / 8\) / n\)\); \}", nes)
    assert m and int(m.group(1)) == A.TRTRI_MAX_CPB and int(m.group(2)) * 1024 // 8 == A.TRTRI_LDS_DOUBLES
    assert "m < 10e-3" in nes
    m = re.search(r"constexpr int kCmaThreads = (\d+)", cma)
    assert m and int(m.group(1)) == A.CMA_THREADS and "i0 += 4 * kCmaThreads" in cma
    ranks = re.search(r"return c == MPOPIS_ERR_HIP \? 4 : c == MPOPIS_ERR_ACTION \? 3 : c == MPOPIS_ERR_NOT_PD \? 2 : c == MPOPIS_ERR_NUMERIC \? 1 : c < 0 \? 5 : 0;", eng)
    assert ranks
    with open(os.path.join(ROOT, "include", "mpopis.h")) as f:
        assert "MPOPIS_OK = 0, MPOPIS_ERR_ARG = -1, MPOPIS_ERR_NOT_PD = -2, MPOPIS_ERR_ACTION = -3, MPOPIS_ERR_HIP = -4, MPOPIS_ERR_NUMERIC = -5" in f.read()


def test_shapes_reach_the_edges_their_tables_name():
    for cs in A.SCATTER_CS:
        assert A.nes_tiles(cs) == A.SCATTER_TILES[cs], cs
    assert A.SCATTER_TILES[16][0] == A.SCATTER_TILES[15][0] + 1                  # a multiple of 16: the ones row opens a tile of its own
    assert A.SCATTER_TILES[111][2:] == (1, 0) and A.SCATTER_TILES[112][2:] == (2, 2)   # 28 -> 36 pairs: a second pair-block whose last two waves own no pair
    shapes = {(K, ks) for _, K, ks, _ in A.SCATTER_CASES}
    assert shapes == set(A.SCATTER_SPLITS)
    for K, ks in shapes:
        assert A.nes_splits(K, ks) == A.SCATTER_SPLITS[(K, ks)], (K, ks)
    assert A.SCATTER_SPLITS[(40, 4)][1] == 2 and A.SCATTER_SPLITS[(33, 32)][1] == 30
    assert any(v[2] != A.NES_KC for v in A.SCATTER_SPLITS.values()) and any(v[2] == A.NES_KC for v in A.SCATTER_SPLITS.values())
    # the case list: every cs at (100, 3), every K x ksplit at cs = 17 and 112, both slot-0 kinds at every cs of the cross
    assert {cs for cs, K, ks, _ in A.SCATTER_CASES if (K, ks) == (100, 3)} == set(A.SCATTER_CS)
    for cs in (17, 112):
        assert {(K, ks) for c, K, ks, _ in A.SCATTER_CASES if c == cs} >= {(K, ks) for K in A.SCATTER_KS for ks in A.SCATTER_KSPLITS} | {(40, 4), (33, 32)}
        assert {k for c, _, _, k in A.SCATTER_CASES if c == cs} == {"cancel", "zero"}
    for n in A.POTRI_NS:
        assert A.trtri_cpb(n) == A.POTRI_CPB[n], n
    assert sorted(set(A.POTRI_CPB.values())) == [48, 63, 64]
    assert {n for n, *_ in A.POTRI_CASES} == set(A.POTRI_NS)
    for n in A.POTRI_NS:
        mine = [c for c in A.POTRI_CASES if c[0] == n]
        assert {c[1] for c in mine} == {"random", "graded"} and {c[2] for c in mine} == {False, True}
    assert {c[3] for c in A.POTRI_CASES} == {False, True}
    d = np.diag(A.potri_factor(100, "graded", 5)) ** 2
    assert d.max() / d.min() > 1e7
    assert {c[0] for c in A.UPDATE_CASES} == set(A.UPDATE_CS)
    for cs in (17, 112):
        assert {(s, a) for c, s, a, _ in A.UPDATE_CASES if c == cs} == {(False, False), (False, True), (True, False), (True, True)}
        assert {p for c, _, _, p in A.UPDATE_CASES if c == cs} == {False, True}
    assert A.UPDATE_K % 4 == 0 and any(cs % 4 for cs in A.UPDATE_CS)                # the GEMM's k loop: n not a multiple of 4
    for cs, K, m in A.CMA_PATHS_SHAPES:
        assert cs * m >= K
        assert {n for c, k, _, n, kind in A.CMA_PATHS_CASES if (c, k) == (cs, K) and kind == "plain"} == {1, 3}
    assert any(K > 4 * A.CMA_THREADS for _, K, _ in A.CMA_PATHS_SHAPES) and any(K == 4 * A.CMA_THREADS for _, K, _ in A.CMA_PATHS_SHAPES)
    assert {k for *_, k in A.CMA_PATHS_CASES} == {"plain", "h_below", "h_above", "zero"}
    c = A.cma_sigma_case(17, 1)
    assert not np.allclose(np.tril(c["Sig"][0], -1), np.triu(c["Sig"][0], 1).T)
    ref, _ = A.cma_sigma_reference(c["Sig"][0], c["scal"][0, 1], 1, c["vec"][0, 17:34], c["consts"])
    assert np.array_equal(ref, ref.T)
