"""The inputs of tests/test_gpu_select_harness.py are what they claim -- shown on the CPU with the oracle and NumPy alone (tests/helpers/select_cases.py
holds the generators both files share): the literal transcription of make_alias_table! reproduces the oracle bit for bit and the case list reaches the
loop's `dry` exit, leftover smalls, chains of exhausted larges longer than a 64-entry batch and exact ties; the early-break vectors sit on the side of
10e-3 they are named for; the weight inputs meet the test's tolerance with the oracle's own double arithmetic; the harness's files round-trip."""
import struct
import numpy as np
import pytest
from tests.helpers import select_cases as S

ALIAS_KS = (2, 63, 64, 65, 1000, 4096, 7168, 7169, 8192, 8193, 16384)
WEIGHT_KS = (1, 255, 256, 1023, 1024, 2048, 8192, 8193, 20000)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("K", ALIAS_KS)
def test_transcription_is_the_oracle_and_the_cases_reach_every_branch(oracle, K):
    rng = np.random.default_rng(1000 + K)
    seen = {"dry": 0, "leftover": 0, "chain": 0, "ties": 0, "eq_one": 0, "no_large": 0}
    vecs = S.alias_weight_vectors(K, rng, oracle)
    assert all(k in vecs for k in S.GENERIC_ALIAS_KINDS)
    for name, w in vecs.items():
        assert w.shape == (K,) and np.all(w >= 0) and abs(w.sum() - 1.0) < 1e-9, name
        a, al, info = S.alias_table_traced(w)
        ra, ral = oracle.make_alias_table(w)
        assert np.array_equal(_bits(a), _bits(ra)) and np.array_equal(al, ral), name
        assert np.all((al >= 0) & (al < K)) and np.all(np.isfinite(a)), name          # a table the draw kernel may be given
        seen["dry"] += info["dry"]; seen["leftover"] += info["leftover_smalls"] > 0; seen["ties"] += info["ties"] > 0
        seen["chain"] = max(seen["chain"], info["pending_chain"]); seen["eq_one"] += info["eq_one"] > 0; seen["no_large"] += info["n_large"] == 0
        if name.startswith("larges_"):
            assert info["n_large"] == int(name.split("_")[1]), (name, info)
        if name.startswith("smalls_"):
            assert info["n_small"] == int(name.split("_")[1]), (name, info)
        if name.startswith("onehot"):
            assert info["n_large"] == 1 and info["n_small"] == K - 1
        if name == "slight_larges" and K >= 4:
            assert info["n_small"] == 1 and info["n_large"] == K - 1 and info["pending_chain"] >= K - 3, info
        if name == "slight_smalls" and K >= 4:
            assert info["n_large"] == 1 and info["n_small"] == K - 1, info
        if name in ("half_blocked", "half_interleaved") and K & (K - 1) == 0:
            assert info["ties"] > 0, (name, info)                                       # 1.5 and 0.5 are exact: every pairing lands on 1.0
    assert seen["ties"] > 0
    if K >= 1000:
        assert seen["dry"] > 0 and seen["chain"] > 64, seen
    if K & (K - 1) == 0:
        assert seen["no_large"] > 0                                                     # exactly uniform: nothing to pair
        assert K < 8 or seen["leftover"] > 0, seen                                      # scaling by a power of two is exact: the pairs cancel, index 0 is left


@pytest.mark.parametrize("K,m,p", [(200, 40, 0), (200, 40, 20), (200, 40, 38), (200, 40, 39), (4096, 3000, 2500), (4096, 3000, 2998), (4096, 3000, 2999),
                                   (9000, 3000, 2999), (256, 64, 63), (2, 2, 0), (50, 50, 48)])
def test_break_vectors_sit_where_they_claim(K, m, p):
    rng = np.random.default_rng(K + p)
    for over in (False, True):
        c = S.break_vector(K, m, p, over, rng)
        order = S.canonical_order(c)
        assert np.array_equal(order, np.argsort(c, kind="stable"))
        s = c[order]
        d = np.abs(np.diff(s))
        assert (d[p] < S.BREAK_THRESHOLD) == (not over)
        nb = np.nextafter(s[p + 1], -np.inf if over else np.inf)                      # the neighbouring double lies on the other side
        assert ((nb - s[p]) < S.BREAK_THRESHOLD) == over
        assert np.all(np.delete(d, p) <= 2.0 ** -8)                                    # every other gap is far from the threshold
        inside = p + 1 < m
        assert S.host_break(c, order, m) == (not over if inside else True)
        assert S.host_break(c, order, 0) is False and S.host_break(c, order, 1) is False


def test_host_break_propagates_non_finite_keys():
    rng = np.random.default_rng(5)
    for name, c in S.nonfinite_vectors(150, rng).items():
        order = S.canonical_order(c)
        assert sorted(order.tolist()) == list(range(150))
        nfin = int(np.isfinite(c).sum())
        assert np.all(np.isfinite(c[order[:nfin]])) and not np.any(np.isfinite(c[order[nfin:]]))
        assert np.array_equal(order[:nfin], np.flatnonzero(np.isfinite(c))[np.argsort(c[np.isfinite(c)], kind="stable")])
        assert S.host_break(c, order, 150) is False, name                              # the elite set reaches a non-finite key
        if name.endswith("equal_base"):
            assert S.host_break(c, order, 75) is True, name                            # ... and breaks while it holds equal finite keys only


def test_sort_vectors_have_the_ties_they_claim():
    rng = np.random.default_rng(9)
    for K in (1, 2, 63, 257, 4097, 12289):
        v = S.sort_vectors(K, rng)
        assert all(x.shape == (K,) and np.all(np.isfinite(x)) for x in v.values())
        assert len(np.unique(v["distinct"])) == K and len(np.unique(v["distinct2"])) == K
        assert len(np.unique(v["equal"])) == 1 and len(np.unique(v["alternating"])) == min(K, 2)
        for p in S.DUP_BOUNDARIES:
            if p < K:
                assert v["dup_blocks"][p - 1] == v["dup_blocks"][p]


@pytest.mark.parametrize("K", WEIGHT_KS)
def test_weight_inputs_meet_the_tolerance_with_the_oracle_alone(oracle, K):
    assert np.finfo(np.longdouble).nmant > 52, "np.longdouble carries no extra precision here: the reference would be no better than the kernel"
    rng = np.random.default_rng(2000 + K)
    for name, (lam, vecs) in S.weight_cost_cases(K, rng).items():
        for c in vecs:
            tol, ref = S.weights_tol(c, lam)
            w = oracle.compute_weights(lam, c)
            assert np.all(np.abs(w.astype(np.longdouble) - ref) <= tol), name
            assert abs(w.sum() - 1.0) <= K * 2.0 ** -52, name
        if name == "underflow" and K >= 1023:
            assert np.mean(w == 0.0) > 0.9


def test_case_files_round_trip():
    rng = np.random.default_rng(3)
    B, K = 3, 37
    cost = rng.standard_normal((B, K)); cost[1, 4] = np.nan; cost[2, 0] = -np.inf
    c = S.unpack_case(S.pack_case(S.OP_SORT, B, K, [1, 0, 1], m_elite=7, no_ws=True, cost=cost))
    assert (c["op"], c["B"], c["K"], c["m_elite"], c["no_ws"]) == (S.OP_SORT, B, K, 7, True)
    assert np.array_equal(_bits(c["cost"]), _bits(cost).reshape(B, K)) and c["active"].tolist() == [1, 0, 1]
    c = S.unpack_case(S.pack_case(S.OP_WEIGHTS, B, K, [1, 1, 0], lam=1e-6, status0=[0, 0, S.POISON_I32], cost=cost))
    assert c["lam"] == 1e-6 and c["status0"].tolist() == [0, 0, S.POISON_I32] and not c["no_ws"]
    # per-slot λ: the second double of the header and bit 1 of flags, beside bit 0 and without disturbing it
    for no_ws in (False, True):
        buf = S.pack_case(S.OP_WEIGHTS, B, K, [1, 1, 0], lam=(10.0, 0.7), no_ws=no_ws, cost=cost)
        assert struct.unpack_from("<q", buf, 8 + 4 * 8)[0] == (2 | int(no_ws)) and struct.unpack_from("<2d", buf, 64) == (10.0, 0.7)
        c = S.unpack_case(buf)
        assert c["lam"] == (10.0, 0.7) and c["no_ws"] == no_ws and np.array_equal(_bits(c["cost"]), _bits(cost).reshape(B, K))
    assert struct.unpack_from("<2d", S.pack_case(S.OP_WEIGHTS, B, K, [1, 1, 0], lam=3.0, cost=cost), 64) == (3.0, 0.0)
    acc, al = rng.random((B, K)), rng.integers(0, K, (B, K))
    di, du = rng.integers(0, K, (B, K + 5)), rng.random((B, K + 5))
    c = S.unpack_case(S.pack_case(S.OP_ALIAS_SAMPLE, B, K, [1, 1, 1], accept=acc, alias=al, di=di, du=du, di_stride=K + 5, log_stride=K + 3))
    assert np.array_equal(c["accept"], acc) and np.array_equal(c["alias"], al) and np.array_equal(c["di"], di) and np.array_equal(c["du"], du)
    assert (c["di_stride"], c["log_stride"]) == (K + 5, K + 3)
    # results: guards split off, poison recognised
    order = np.full(B * K + S.GUARD, S.POISON_I32, dtype=np.int32); order[:K] = np.arange(K)
    r = S.unpack_result(S.pack_result(S.OP_SORT, S.SORT_RANK, [], [order, [1, 0, 0], [0, 0, 0]]), S.OP_SORT, B, K)
    assert r["form"] == S.SORT_RANK and np.array_equal(r["order"][0], np.arange(K)) and np.all(S.is_poison(r["order"][1:])) and np.all(S.is_poison(r["order_guard"]))
    w = np.frombuffer(b"\xa5" * 8 * (B * K + S.GUARD), dtype=np.float64)
    r = S.unpack_result(S.pack_result(S.OP_WEIGHTS, S.WEIGHTS_REG_256, [w, [1.0, 1.0, 1.0]], [[0, -3, 0]]), S.OP_WEIGHTS, B, K)
    assert np.all(S.is_poison(r["w"])) and r["status"].tolist() == [0, -3, 0] and r["wsum"].tolist() == [1.0, 1.0, 1.0]
    r = S.unpack_result(S.pack_result(S.OP_ALIAS_BUILD, S.ALIAS_SEQ_LDS, [w], [order, [0, 1, 2]]), S.OP_ALIAS_BUILD, B, K)
    assert r["need"].tolist() == [0, 1, 2] and r["alias"].shape == (B, K)
    r = S.unpack_result(S.pack_result(S.OP_ALIAS_SAMPLE, 0, [], [order, np.zeros(B * (K + 3) + S.GUARD, dtype=np.int32)]), S.OP_ALIAS_SAMPLE, B, K, log_stride=K + 3)
    assert r["log"].shape == (B, K + 3)
