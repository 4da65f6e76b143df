"""The inputs and references of tests/test_gpu_mfma_harness.py are what they claim -- shown on the CPU with NumPy and the oracle alone
(tests/helpers/mfma_cases.py holds what both files share): for every case a plain float64 evaluation of the operation, in the kernel's own plan, stays
within a quarter of the case's derived bound against the longdouble reference, so the bound tests the kernel and not the input; the transcription of
wcov_form reaches every named form over the case lists; the edge shapes (empty K splits, repeated and left-out columns, +inf costs, one dominant
weight, intensities inside (0, 1) and clamped at either end) are really there; the longdouble transcription of the shrinkage formulas is the oracle's;
the harness's files round-trip."""
import numpy as np
import pytest
from tests.helpers import mfma_cases as M

LD = M.LD


def _worst(got, ref, bound):
    err = np.abs(np.asarray(got).astype(LD) - ref)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(np.where(bound == 0, 0, err / np.where(bound == 0, 1, bound))))


def test_files_round_trip():
    c = M.wcov_case(17, 64, 2, "cost")
    op, B, ipar, dpar, arrays = M.unpack_case(c["data"])
    assert (op, B, ipar) == (M.OP_WCOV, 3, [17, 64, 64, 2, 0, 1]) and dpar == [0.0, M.RIDGE, -1 / 20.0]
    assert [a.size for _, a in arrays] == [3, 3 * 17 * 64, 0, 0, 0, 0, 0, 3 * 64, 0, 3 * 17]
    assert np.array_equal(arrays[1][1].reshape(3, 17, 64), c["X"]) and np.array_equal(arrays[0][1], [1, 0, 1])
    outs = [(M.F64, np.arange(10.0 + M.GUARD)), (M.U64, np.array([1, 2 ** 64 - 1], dtype=np.uint64))]
    form, arrs = M.unpack_result(M.pack_result(513, outs))
    assert form == 513 and np.array_equal(arrs[0], outs[0][1]) and arrs[1][1] == 2 ** 64 - 1
    body, guard = M.split_guard(arrs[0], (2, 5))
    assert body.shape == (2, 5) and guard.size == M.GUARD
    assert np.all(M.is_poison(np.frombuffer(b"\xa5" * 16, dtype=np.float64))) and not np.any(M.is_poison(np.zeros(2)))


def test_cost_key_orders_like_the_costs():
    v = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-300, 2.0, 1e300, np.inf])
    keys = [M.cost_key(x) for x in v]
    assert keys == sorted(keys) and len(set(keys)) >= len(v) - 1 and all(0 <= k < 2 ** 64 for k in keys)
    assert M.cost_key(np.nan) > M.cost_key(np.inf)                      # NaN sorts last


# ---- sampler ---------------------------------------------------------------------------------------------------------------------------
def test_sampler_cases_reach_every_row_group_count_and_stay_within_the_bound():
    groups = {M.sampler_groups(n) for n in M.TRMM_NS}
    assert {g for g, _ in groups} == {1, 2, 3, 7} and (2, 5) in groups and (3, 7) in groups and (7, 8) in groups      # 129: 5 + 4, 300: 7 + 7 + 5, 800: 8 x 6 + 2
    assert {n for n, K, _, _ in M.TRMM_CASES if K == 65} == set(M.TRMM_NS) and all({K for n, K, _, _ in M.TRMM_CASES if n == nn} >= set(M.TRMM_KS) for nn in (17, 129))
    assert {(sh, o) for _, _, sh, o in M.TRMM_CASES} == {(False, False), (False, True), (True, False), (True, True)}
    worst = 0.0
    for n, K, shared, osc in M.TRMM_CASES:
        if n > 304 and K > 17:
            continue                                                      # (the 800-row case is checked at K = 17: the same bound, a fourth of the arithmetic)
        c = M.trmm_case(n, K, shared=shared, osc=osc)
        L = c["L"][0]
        assert np.all(np.abs(L[np.tril_indices(n, -1)]) <= 0.1) and np.all((np.diag(L) >= 0.25) & (np.diag(L) <= 1.0))
        o = c["osc"][0] if osc else None
        ref, bound = M.sampler_reference(L, c["Z"][0], o)
        worst = max(worst, _worst(M.sampler_emulation(L, c["Z"][0], o), ref, bound))
    assert worst <= 0.25, worst


def test_fused_cases_and_the_panel_layout():
    assert all(M.fusable(n) for n in M.FUSED_NS) and not M.fusable(102) and not M.fusable(132)
    assert {n <= 112 for n in M.FUSED_NS} == {True, False}
    assert {(sh, o) for _, _, sh, o in M.FUSED_CASES} == {(False, False), (False, True), (True, False), (True, True)}
    for n in (4, 20, 116):
        c = M.fused_case(M.OP_FUSED, n, 17)
        A = c["A"][0]
        assert np.array_equal(A, A.T) and np.all(np.linalg.eigvalsh(A) > 0)
        L = c["L0"][0]
        P = M.panel_of(L).reshape(-1, 16, M.PANEL_ROWS)
        assert P.size == M.panel_doubles(n)
        for j in range(P.shape[0] * 16):                                 # k_trmm_LZ_mfma reads column j0 + 4 lk + q of L from LDS row 4 q + lk
            col = P[j // 16, ((j % 16) & 3) * 4 + ((j % 16) >> 2)]
            want = np.zeros(M.PANEL_ROWS)
            if j < n:
                want[j:n] = L[j:, j]
            assert np.array_equal(col, want)


# ---- scatter ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scatter_cases():
    return M.scatter_cases()


def test_scatter_cases_reach_every_form(scatter_cases):
    seen = {M.case_form(c, env) for c, env in scatter_cases}
    partials = {(p, sq) for p, sq, _, _ in seen}
    assert partials >= {(M.WCOV_PAIR64, False), (M.WCOV_PAIR16, False), (M.WCOV_ROWS, False), (M.WCOV_TALL, False), (M.WCOV_PAIR64, True), (M.WCOV_PAIR16, True),
                        (M.WCOV_TALL, True)}
    for p in (M.WCOV_PAIR64, M.WCOV_PAIR16, M.WCOV_ROWS, M.WCOV_TALL):   # every form with the ones row and without, with the weights from the costs
        assert {aug for q, sq, aug, _ in seen if q == p and not sq} == {True, False}, p
        assert any(fc for q, _, _, fc in seen if q == p), p
    # the row form's own edges: the ones row first guarded / last staged / absent; a last workgroup whose second half is all padding
    rows = [c for c, env in scatter_cases if M.case_form(c, env)[0] == M.WCOV_ROWS]
    # the row form's grid: cs x ksplit x m with m = 64, 65, 257 contiguous and 819 of 1000 gathered, the latter also weighted
    assert {(c["cs"], c["ksplit"], c["m"]) for c in rows} == {(cs, ks, m) for cs in (97, 100, 111, 112) for ks in (2, 6) for m in (64, 65, 257, 819)}
    assert all(c["idx"] is not None and c["K"] == 1000 for c in rows if c["m"] == 819) and any(c["w"] is not None for c in rows if c["m"] == 819)
    for cs in (97, 100, 111, 112):                                        # every weight source at every (cs, ksplit) and every (cs, m)
        src = lambda c: "cost" if c["variant"] == "cost" else "w" if c["w"] is not None else "none"
        for ks in (2, 6):
            assert {src(c) for c in rows if (c["cs"], c["ksplit"]) == (cs, ks) and c["idx"] is None} == {"cost", "w", "none"}
        for m in (64, 65, 257):
            assert {src(c) for c in rows if (c["cs"], c["m"]) == (cs, m)} == {"cost", "w", "none"}
    # cs & 15 of the ones-row cases: the decode of the mean in the finish kernel sees every il = 1 .. 15
    il = {c["cs"] & 15 for c, env in scatter_cases if M.case_form(c, env)[2]}
    assert il == set(range(1, 16)), il


def test_scatter_default_rule_cases():
    for cs, ksplit, sel_batch, rscale, partial in M.RULE_CASES:
        assert M.wcov_form(cs, 130, 130, ksplit, sel_batch, rscale, rscale, not rscale, False)[0] == partial
    prods = {sb * (ks // 2) for _, ks, sb, _, p in M.RULE_CASES if sb > 0 and ks % 2 == 0}
    assert {190, 192, 189, 191} <= prods


def test_scatter_edge_shapes_are_what_they_claim(scatter_cases):
    empt = [c for c, _ in scatter_cases if c["K"] == 64 and c["ksplit"] == 32]
    assert len(empt) == 6 and all(len(M.empty_splits(c["cs"], c["m"], 32)) >= 28 for c in empt)
    assert any(M.empty_splits(c["cs"], c["m"], c["ksplit"]) for c, _ in scatter_cases if c["variant"] == "plain")
    assert {c["ksplit"] for c, _ in scatter_cases} >= {1, 2, 5, 6, 8, 9, 32}
    for c, _ in scatter_cases:
        if c["idx"] is not None:
            for b in range(c["B"]):
                cols = c["idx"][b, :c["m"]]
                assert len(set(cols.tolist())) <= c["K"] // 2                 # at least half of the columns are left out
                assert c["m"] < 4 or len(set(cols.tolist())) < c["m"]        # repeats
                assert c["m"] < 2 or len(set(cols.tolist())) >= 2
        if c["cost"] is not None:
            assert np.all(np.isinf(c["cost"]).sum(axis=1) >= 1)
            for b in range(c["B"]):
                w = M._wcov_inputs(dict(c, w=None), b)[1]                 # the weights of the costs themselves
                if c["w"] is not None:                                    # the weights that ride along are the normalised ones of the same costs
                    assert c["cs"] % 16 == 0 and np.max(np.abs(c["w"][b] - (w / w.sum()).astype(np.float64))) <= 1e-15
                assert np.all(w[np.isinf(c["cost"][b])] == 0) and w.max() == 1
                if c["variant"] == "cost_dominant":
                    assert np.sum(w == 1) == 1 and np.all(np.sort(w)[:-1] < 1e-300)
        if c["variant"] == "pmc":
            assert np.all(c["X"][:, :, 0] == 0) and np.max(np.abs(c["shift"])) > 500          # shifted by the first column; the offsets of 1e3 are gone from X
            assert len(set(c["X"][0][0].tolist())) < c["K"]                                   # resampled: repeats


def test_scatter_float64_emulation_is_well_inside_the_bound(scatter_cases):
    """the one-pass uncentred form with 8 interleaved partials in plain float64 against the longdouble reference: <= 0.25 of the bound (one active slot
    per case)"""
    worst = {"S": 0.0, "mu": 0.0}
    for c, _ in scatter_cases:
        b = int(np.flatnonzero(c["active"])[0])
        ref = M.wcov_reference(c, b)
        S, mu = M.wcov_emulation(c, b)
        assert np.all(ref["S_bound"] >= 0) and np.all(np.isfinite(ref["S"].astype(np.float64)))
        worst["S"] = max(worst["S"], _worst(S, ref["S"], ref["S_bound"]))
        if mu is not None and ref["mu"] is not None and c["mu"] is None:
            worst["mu"] = max(worst["mu"], _worst(mu, ref["mean"], ref["mean_bound"]))
            if c["shift"] is not None:                                    # adding the shift back rounds once more: inside the bound, which has that rounding as a term
                assert _worst(mu + c["shift"][b], ref["mu"], ref["mu_bound"]) <= 1.0
    print("worst emulation error / bound:", worst)
    assert worst["S"] <= 0.25 and worst["mu"] <= 0.25, worst


# ---- shrinkage and CE --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ["ss", "lw", "rblw", "oas"])
@pytest.mark.parametrize("cs,m", M.SHRINK_SHAPES)
def test_shrinkage_inputs(oracle, est, cs, m):
    rng = np.random.default_rng([cs, m, M.EST[est]])
    for _ in range(3):
        X = M.elite_data(cs, m, rng)
        tol, hi = M.lam_tolerance(X, est)
        assert 0.05 < hi["lam_raw"] < 0.95, float(hi["lam_raw"])
        assert tol < 1e-10
        mean, S = oracle.cov_estimate(X, est)
        want = (1 - hi["lam"]) * hi["S"] + hi["lam"] * hi["F"]
        assert np.max(np.abs(S.astype(LD) - want)) <= 1e-13 * float(np.max(np.abs(want))) and np.max(np.abs(mean.astype(LD) - hi["mean"])) <= 1e-14
        # the moments the kernels are handed reproduce the intensity
        Sm, Q, rs = M.moments_for_shrink(X, est)
        raw = M.ss_lambda_f64(Sm, Q, rs, m)[0] if est in ("ss", "lw") else M.common_lambda_f64(Sm, m, est == "oas")[0]
        assert abs(raw - float(hi["lam_raw"])) <= tol


def test_shrinkage_clamp_cases():
    cs, m = 20, 30
    want = {"ss_zero": 0.0, "lw_zero": 0.0, "ss_one": 1.0, "ss_no_offdiag": 1.0, "rblw_one": 1.0, "oas_one": 1.0, "rblw_no_spread": 1.0}
    for kind, lam in want.items():
        S, Q, est = M.clamp_case(kind, cs, m)
        if est in ("ss", "lw"):
            rs = 1.0 / np.sqrt(np.diag(S)) if est == "ss" else np.ones(cs)
            raw, cl = M.ss_lambda_f64(S, Q, rs, m)
        else:
            raw, cl = M.common_lambda_f64(S, m, est == "oas")
        if kind in ("ss_no_offdiag", "rblw_no_spread"):                  # the guarded quotient: its denominator is exactly 0
            assert cl == 1.0 and raw in (1.0, np.inf), (kind, raw)
        else:
            assert cl == lam and (raw < -0.03 if lam == 0 else raw > 1.5), (kind, raw)


@pytest.mark.parametrize("est,cs,m", M.CE_CASES + [(e, cs, m) for e in M.ESTS for cs, m in M.CE_BEYOND])
def test_ce_inputs(oracle, est, cs, m):
    assert M.ce_small_ok(cs, m) == (cs <= 128 and m <= 64)
    c = M.ce_case(M.OP_CE_SMALL, cs, 150, m, est)
    for b in (0, 2):
        assert sorted(c["order"][b].tolist()) == list(range(150))
        X = c["E"][b][:, c["order"][b, :m]]
        tol, hi = c["lam"][b]                                             # the tolerance on lambda* the GPU test will use: stored in the case
        assert tol < 1e-10, tol
        mean, S = oracle.cov_estimate(X, est)
        want = (1 - hi["lam"]) * hi["S"] + hi["lam"] * hi["F"]
        assert np.max(np.abs(S.astype(LD) - want)) <= np.max(M.shrunk_tolerance(X, est, tol, hi))


def test_ce_case_list_is_the_full_cross():
    assert sorted(M.CE_CASES) == sorted((e, cs, m) for e in ("mle", "ss", "lw", "rblw", "oas") for cs in (4, 20, 100, 128) for m in (2, 3, 30, 63, 64))
    assert len(set(M.CE_CASES)) == 100 and all(M.ce_small_ok(cs, m) for _, cs, m in M.CE_CASES) and not any(M.ce_small_ok(cs, m) for cs, m in M.CE_BEYOND)
    assert sorted(M.WMEAN_MODES) == [(0, False), (0, True), (1, False), (1, True)]


# ---- gather / weighted mean --------------------------------------------------------------------------------------------------------------
def test_gather_and_wmean_references():
    for K, m in ((257, 257), (2049, 2048), (257, 30)):
        c = M.gather_case(2, 17, K, m=m)
        assert c["idx"].max() < max(1, K // 2)
        ref, bound = M.gather_mean_reference(c, 0)
        got = c["X"][0][:, c["idx"][0, :m]].sum(axis=1) / m
        assert _worst(got, ref, bound) <= 0.25
    for K in (1, 257, 2050):
        for norm, sp in M.WMEAN_MODES:
            c = M.gather_case(3, 17, K, normalize=norm, shift_pair=sp)
            ref, bound = M.wmean_reference(c, 2)
            sft = (c["sa"][2] - c["sb"][2]) if sp else np.zeros(17)
            got = ((c["X"][2] + sft[:, None]) * c["w"][2]).sum(axis=1)
            assert _worst(got / c["w"][2].sum() if norm else got, ref, bound) <= 0.25
