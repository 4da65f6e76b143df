"""The selection kernels -- the six sort forms and the CE kernel's fused sort with their elite early break, the three alias-table constructions, the
alias draw and both forms of k_weights -- exercised directly, below the policy level, through the C++ harness tools/kbench_select.hip: one process
per launch, inputs written by the test, raw device outputs read back.  Shapes sit on both sides of every threshold of launch_sortperm /
launch_alias_build / launch_weights and every case asserts the form the launcher reported, so a threshold that moves fails a test instead of
dropping a form from coverage.  References are NumPy and the oracle (tests/helpers/select_cases.py; tests/test_select_cases_cpu.py shows on the CPU
that the inputs are what they claim), never the engine.  The harness poisons every output first: inactive slots and the entries past K must stay
untouched.

Not asserted: the relative order of +0.0 and -0.0.  The device and the oracle compare numerically (equal keys, index decides) where Julia's isless
puts -0.0 first; no input here holds a negative zero."""
import os
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import select_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness():
    return HR.build("select")


def _run(exe, tmp_path, case, op, B, K, env=None, log_stride=0):
    return S.unpack_result(HR.run_case(exe, tmp_path, case, env=dict(os.environ, **(env or {}))), op, B, K, log_stride=log_stride)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ================================================================ sort + early break ===========================================================
def _check_sort(exe, tmp_path, K, m_elite, vecs, form, op=S.OP_SORT, no_ws=False, env=None):
    """vecs: one cost vector per slot, None = the inactive slot.  -> the orders of the active slots"""
    B = len(vecs)
    rng = np.random.default_rng(K)
    cost = np.stack([rng.standard_normal(K) if v is None else v for v in vecs])
    active = np.array([0 if v is None else 1 for v in vecs], dtype=np.int32)
    r = _run(exe, tmp_path, S.pack_case(op, B, K, active, m_elite=m_elite, no_ws=no_ws, cost=cost), op, B, K, env=env)
    assert r["form"] == form, (r["form"], form)
    assert np.all(S.is_poison(r["order_guard"])) and np.all(r["done"] == 0)          # nothing past B K; the arrival counters are back at zero
    orders = []
    for b in range(B):
        if not active[b]:
            assert np.all(S.is_poison(r["order"][b])) and r["active"][b] == 0, b
            continue
        want = S.canonical_order(cost[b])
        got = r["order"][b]
        fin = np.isfinite(cost[b])
        assert sorted(got.tolist()) == list(range(K)), ("not a permutation", b, K - len(set(got.tolist())))        # (a)
        nf = int(fin.sum())
        assert np.array_equal(got[:nf], np.flatnonzero(fin)[np.argsort(cost[b][fin], kind="stable")]), b             # (b); all of it when finite
        if nf == K:
            assert np.array_equal(got, np.argsort(cost[b], kind="stable")), b
        assert np.array_equal(got, want), b                                           # NaN placed like +inf, index breaks ties: the same in every form
        brk = S.host_break(cost[b], want, m_elite)
        assert r["active"][b] == (0 if brk else 1), (b, m_elite, brk)
        orders.append(got)
    return orders


def _generic_slots(K, rng, inactive_at):
    v = list(S.sort_vectors(K, rng).values())
    v.insert(inactive_at % (len(v) + 1), None)
    return v                                                                          # 8 vectors + the inactive slot: B = 9


def _m_generic(K):
    return min(K, max(2, K // 5))


@pytest.mark.parametrize("K,form", [(k, S.SORT_RANK) for k in (1, 2, 63, 64, 255, 256)] + [(k, S.SORT_LDS) for k in (257, 512, 513, 1024)] +
                         [(k, S.SORT_BITONIC4) for k in (1025, 2047, 2048, 4095, 4096)] + [(k, S.SORT_BITONIC8) for k in (4097, 8191, 8192)])
def test_sort_one_workgroup_forms(harness, tmp_path, K, form):
    """B = 9: too many slots for the chip-wide rank sort (9 K^2 > 2 x 4096^2 from K = 2048), so the workspace is there and the bitonic forms still run"""
    _check_sort(harness, tmp_path, K, _m_generic(K), _generic_slots(K, np.random.default_rng(K), K), form)


def _few_slots(B, K, kinds, rng):
    v = S.sort_vectors(K, rng)
    slots = [v[k] for k in kinds]
    if B > 1:
        slots.insert(1, None)
    assert len(slots) == B
    return slots


MULTI_CASES = [(1, 2048, ("dup_blocks",)), (1, 2048, ("small_ints",)), (1, 4096, ("dup_blocks",)), (1, 4096, ("small_ints",)), (2, 4096, ("dup_blocks",)),
               (3, 4096, ("small_ints", "dup_blocks")), (1, 5792, ("dup_blocks",)), (1, 5793, ("dup_blocks",)), (1, 5793, ("alternating",))]


@pytest.mark.parametrize("B,K,kinds", MULTI_CASES)
def test_sort_rank_multi_rule(harness, tmp_path, B, K, kinds):
    """k_sortperm_rank_multi takes K >= 2048 while B K^2 <= 2 x 4096^2 (5792^2 is the last square below it); MPOPIS_SORT_MULTI=0 and a missing workspace
    both send the same inputs through the bitonic network, with the same result"""
    multi = B * K * K <= 2 * 4096 * 4096
    bitonic = S.SORT_BITONIC8 if K > 4096 else S.SORT_BITONIC4
    slots = _few_slots(B, K, kinds, np.random.default_rng(B * K))
    m = K // 5
    o1 = _check_sort(harness, tmp_path, K, m, slots, S.SORT_RANK_MULTI if multi else bitonic)
    o2 = _check_sort(harness, tmp_path, K, m, slots, bitonic, env={"MPOPIS_SORT_MULTI": "0"})
    o3 = _check_sort(harness, tmp_path, K, m, slots, bitonic, no_ws=True)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(o1, o2, o3))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [8193, 9001, 12288, 12289, 20000])
def test_sort_rank_big(harness, tmp_path, B, K):
    """beyond 8192: the slot's costs go through LDS in chunks of 4096 (two to five, the last one ragged)"""
    slots = _few_slots(B, K, ("dup_blocks",) if B == 1 else ("small_ints", "dup_blocks"), np.random.default_rng(B * K))
    _check_sort(harness, tmp_path, K, K // 5, slots, S.SORT_RANK_BIG)


@pytest.mark.parametrize("K,m", [(2, 2), (150, 30), (256, 64)])
def test_sort_fused_into_the_ce_kernel(harness, tmp_path, K, m):
    _check_sort(harness, tmp_path, K, m, _generic_slots(K, np.random.default_rng(K), K + 3), S.SORT_CE_FUSED, op=S.OP_CE_SORT)


BREAK_CASES = [  # op, K, m_elite, positions p of the deciding pair (p, p+1), form
    (S.OP_SORT, 200, 40, (0, 20, 38, 39), S.SORT_RANK),
    (S.OP_SORT, 200, 200, (0, 130, 198), S.SORT_RANK),                     # m_elite = K; pair 130 sits in the third wave
    (S.OP_SORT, 300, 2, (0, 1), S.SORT_LDS),                               # m_elite = 2: one pair
    (S.OP_SORT, 1000, 900, (0, 700, 898, 899), S.SORT_LDS),                # 512 threads: pair 700 is a second-stride entry of a late wave
    (S.OP_SORT, 4096, 3000, (0, 2500, 2998, 2999), S.SORT_BITONIC4),       # 1024 threads, third stride
    (S.OP_SORT, 1500, 1500, (1498,), S.SORT_BITONIC4),
    (S.OP_SORT, 6000, 5000, (0, 4500, 4998, 4999), S.SORT_BITONIC8),
    (S.OP_SORT, 2048, 1500, (700, 1498, 1499), S.SORT_RANK_MULTI),         # the slot's last workgroup reduces with 256 threads
    (S.OP_SORT, 9000, 3000, (0, 2500, 2998, 2999), S.SORT_RANK_BIG),
    (S.OP_CE_SORT, 256, 64, (0, 30, 62, 63), S.SORT_CE_FUSED),
]


@pytest.mark.parametrize("op,K,m,positions,form", BREAK_CASES)
def test_early_break_at_its_threshold_and_its_elite_boundary(harness, tmp_path, op, K, m, positions, form):
    """Sorted costs whose gaps are all <= 2^-9 except one pair, whose difference is the last double below 10e-3 or the first one not below it (strict <);
    the pair sits first, deep inside (beyond a thread stride / in a late wave), on the last elite pair (m-2, m-1) and on the first pair outside
    (m-1, m), where it must not count.  The host rule is evaluated on the same doubles, so the comparison is exact."""
    rng = np.random.default_rng(K + m)
    slots = [S.break_vector(K, m, p, over, rng) for p in positions if p < K - 1 for over in (False, True)]
    slots.insert(len(slots) // 2, None)
    _check_sort(harness, tmp_path, K, m, slots, form, op=op)


@pytest.mark.parametrize("K,m,form", [(200, 0, S.SORT_RANK), (200, 1, S.SORT_RANK), (700, 1, S.SORT_LDS), (3000, 1, S.SORT_BITONIC4), (3000, 0, S.SORT_BITONIC4),
                                      (5000, 1, S.SORT_BITONIC8), (2048, 1, S.SORT_RANK_MULTI), (9000, 1, S.SORT_RANK_BIG), (9000, 0, S.SORT_RANK_BIG)])
def test_no_break_below_two_elites(harness, tmp_path, K, m, form):
    rng = np.random.default_rng(K)
    _check_sort(harness, tmp_path, K, m, [np.full(K, 3.0), None, S.break_vector(K, 2, 0, False, rng), rng.integers(0, 3, K).astype(float)], form)


NONFINITE_CASES = [(S.OP_SORT, 150, S.SORT_RANK, S.SORT_RANK), (S.OP_SORT, 700, S.SORT_LDS, S.SORT_LDS), (S.OP_SORT, 1500, S.SORT_BITONIC4, S.SORT_BITONIC4),
                   (S.OP_SORT, 2100, S.SORT_RANK_MULTI, S.SORT_BITONIC4), (S.OP_SORT, 3000, S.SORT_BITONIC4, S.SORT_BITONIC4),
                   (S.OP_SORT, 4096, S.SORT_BITONIC4, S.SORT_BITONIC4), (S.OP_SORT, 5000, S.SORT_BITONIC8, S.SORT_BITONIC8),
                   (S.OP_SORT, 9001, S.SORT_RANK_BIG, None), (S.OP_CE_SORT, 60, S.SORT_CE_FUSED, None)]


@pytest.mark.parametrize("op,K,form,form_bitonic", NONFINITE_CASES)
def test_sort_with_non_finite_costs(harness, tmp_path, op, K, form, form_bitonic):
    """One +inf; several +inf at a K that is no power of two (a real (+inf, i < K) meets the padding's (+inf, i >= K)); one NaN, a few, all; NaN and +inf
    mixed.  (a) order is a permutation, (b) the finite entries come first in stable order, (c) every form that takes the shape gives the same order
    (with the workspace, without it, with MPOPIS_SORT_MULTI=0), (d) an elite set that reaches a non-finite key does not break -- m_elite = K; at
    m_elite = K/2 the vectors on an all-equal base break, the others follow the host rule.
    Before the NaN canonicalisation in k_sortperm<EPT> / k_sortperm_lds and the NaN-propagating maximum in the break helpers this failed: a NaN made
    both partners of a shuffle / LDS compare-exchange keep the same element, so order[] lost indices and repeated others (a), and fmax dropped the
    NaN of inf - inf / NaN - x, so an all-NaN elite set (every form) and a NaN among equal costs (rank sort, CE kernel) broke the slot (d)."""
    rng = np.random.default_rng(K)
    slots = list(S.nonfinite_vectors(K, rng).values())
    slots.insert(K % 7, None)                                                          # B = 7: 7 x 2100^2 <= 2 x 4096^2 still takes the chip-wide rank sort
    m_all = K if op == S.OP_SORT else min(K, 64)
    o1 = _check_sort(harness, tmp_path, K, m_all, slots, form, op=op)
    if form_bitonic is None:
        _check_sort(harness, tmp_path, K, m_all // 2, slots, form, op=op)
        return
    o2 = _check_sort(harness, tmp_path, K, K // 2, slots, form_bitonic, no_ws=True)
    o3 = _check_sort(harness, tmp_path, K, m_all, slots, form_bitonic, env={"MPOPIS_SORT_MULTI": "0"})
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(o1, o2, o3))


# ================================================================ alias table ==================================================================
ALIAS_KS = (2, 63, 64, 65, 1000, 4096, 7168, 7169, 8192, 8193, 16384)


def _check_alias(exe, tmp_path, oracle, K, named, form, no_ws=False, env=None):
    """named: list of (name, weight vector) per slot, (None, None) = the inactive slot"""
    B = len(named)
    w = np.stack([np.full(K, 1.0 / K) if v is None else v for _, v in named])
    active = np.array([0 if v is None else 1 for _, v in named], dtype=np.int32)
    r = _run(exe, tmp_path, S.pack_case(S.OP_ALIAS_BUILD, B, K, active, no_ws=no_ws, w=w), S.OP_ALIAS_BUILD, B, K, env=env)
    assert r["form"] == form, (r["form"], form)
    assert np.all(S.is_poison(r["accept_guard"])) and np.all(S.is_poison(r["alias_guard"]))
    par = form == S.ALIAS_PAR_THEN_SEQ_LDS
    certified = []
    for b, (name, v) in enumerate(named):
        if v is None:
            assert np.all(S.is_poison(r["accept"][b])) and np.all(S.is_poison(r["alias"][b])) and S.is_poison(r["need"][b])
            continue
        ra, ral, info = S.alias_table_traced(v)
        oa, oal = oracle.make_alias_table(v)
        assert np.array_equal(_bits(ra), _bits(oa)) and np.array_equal(ral, oal)
        assert np.array_equal(r["alias"][b], oal), (name, int(np.sum(r["alias"][b] != oal)))
        if not par:
            assert S.is_poison(r["need"][b]), name                                    # the sequential forms take no flag
        if not par or r["need"][b] != 0:                                               # sequential construction: the reference's operations in its order
            bad = np.flatnonzero(_bits(r["accept"][b]) != _bits(oa))
            assert bad.size == 0, (name, bad[:5], r["accept"][b][bad[:5]], oa[bad[:5]])
        else:
            certified.append(name)
            scaled = v * float(K)
            le1 = scaled <= 1.0
            assert np.array_equal(_bits(r["accept"][b][le1]), _bits(oa[le1])), name
            dev = np.abs(r["accept"][b][~le1] - oa[~le1])
            assert np.all(dev <= S.alias_par_bound(K)), (name, dev.max(), S.alias_par_bound(K))
        if par and info["ties_inner"] > 0:
            assert r["need"][b] != 0, (name, info)                                     # an exact tie is a decision the scans cannot certify
    return certified


def _alias_slots(K, oracle, which):
    vecs = S.alias_weight_vectors(K, np.random.default_rng(1000 + K), oracle)
    if which == "all":
        named = list(vecs.items())
        named.insert(K % len(named), (None, None))
    elif which == "one":
        named = [("softmax20_a", vecs["softmax20_a"])]
    else:
        named = [("softmax20_b", vecs["softmax20_b"]), (None, None), ("half_blocked", vecs["half_blocked"])]
    return named


@pytest.mark.parametrize("which", ["all", "one", "three"])
@pytest.mark.parametrize("K", ALIAS_KS)
def test_alias_default_route(harness, tmp_path, oracle, K, which):
    """As the engine calls it (need_ws and, beyond the LDS form's K, the stacks' workspace): the parallel construction first, the sequential one on the
    slots it flagged; beyond K = 7168 the sequential construction on global arrays.  Condition of this test: on the generic inputs (two softmax vectors
    at lambda = 20, one random normalised vector) at least one slot per case is NOT flagged -- otherwise the parallel kernel's results would all have
    been overwritten and nothing of it tested."""
    glob = K > 7168
    named = _alias_slots(K, oracle, which)
    certified = _check_alias(harness, tmp_path, oracle, K, named, S.ALIAS_SEQ_GLOBAL if glob else S.ALIAS_PAR_THEN_SEQ_LDS)
    if not glob:
        assert any(n in S.GENERIC_ALIAS_KINDS for n in certified) or not any(n in S.GENERIC_ALIAS_KINDS for n, _ in named), certified


@pytest.mark.parametrize("K", ALIAS_KS)
def test_alias_sequential_forms_are_bit_exact(harness, tmp_path, oracle, K):
    """k_alias_build<false> (no need_ws, and MPOPIS_ALIAS_PAR=0 with it) and k_alias_build<true>: accept and alias bit-equal to the oracle, every entry"""
    named = _alias_slots(K, oracle, "all")
    form = S.ALIAS_SEQ_GLOBAL if K > 7168 else S.ALIAS_SEQ_LDS
    _check_alias(harness, tmp_path, oracle, K, named, form, no_ws=True)
    if K in (65, 4096, 7168, 8192):
        _check_alias(harness, tmp_path, oracle, K, named, form, env={"MPOPIS_ALIAS_PAR": "0"})


@pytest.mark.parametrize("K", [64, 1000])
def test_alias_sample_on_both_sides_of_accept(harness, tmp_path, oracle, K):
    """u just below accept[i], equal to it (strict <: the alias is taken) and just above, for every index i, plus random draws; di / du rows and the log
    carry strides of their own.  The table is the oracle's (the harness refuses a table with an index outside [0, K) or a non-finite accept)."""
    rng = np.random.default_rng(K)
    acc, al = oracle.make_alias_table(oracle.compute_weights(20.0, rng.standard_normal(K) * 30.0))
    B, ds, ls = 5, K + 7, K + 3
    di, du = np.zeros((B, ds), dtype=np.int32), np.zeros((B, ds))
    for b, u in enumerate((np.nextafter(acc, 0.0), acc, np.nextafter(acc, 2.0))):
        di[b, :K], du[b, :K] = np.arange(K), u
    di[3, :K], du[3, :K] = rng.integers(0, K, K), rng.random(K)
    di[4, :K], du[4, :K] = rng.integers(0, K, K), rng.random(K)
    active = np.array([1, 1, 1, 1, 0], dtype=np.int32)
    case = S.pack_case(S.OP_ALIAS_SAMPLE, B, K, active, accept=np.tile(acc, (B, 1)), alias=np.tile(al, (B, 1)), di=di, du=du, di_stride=ds, log_stride=ls)
    r = _run(harness, tmp_path, case, S.OP_ALIAS_SAMPLE, B, K, log_stride=ls)
    assert np.all(S.is_poison(r["out_guard"])) and np.all(S.is_poison(r["log_guard"])) and np.all(S.is_poison(r["log"][:, K:]))
    for b in range(4):
        want = oracle.alias_sample(acc, al, di[b, :K], du[b, :K])
        assert np.array_equal(r["out"][b], want) and np.array_equal(r["log"][b, :K], want), b
    assert np.array_equal(r["out"][1], al)                                             # u == accept[i]: never i itself (unless it is its own alias)
    assert np.all(S.is_poison(r["out"][4])) and np.all(S.is_poison(r["log"][4]))


# ================================================================ weights ======================================================================
WEIGHT_KS = (1, 255, 256, 1023, 1024, 2048, 8192, 8193, 20000)


def _weights_form(K):
    return S.WEIGHTS_REG_256 if K < 1024 else S.WEIGHTS_REG_1024 if K <= 8192 else S.WEIGHTS_3PASS_1024


def _run_weights(exe, tmp_path, K, lam, vecs):
    """lam: one λ for every slot, or a pair (λ_even, λ_odd) = the per-slot form of the same launcher"""
    B = len(vecs)
    cost = np.stack([np.zeros(K) if v is None else v for v in vecs])
    active = np.array([0 if v is None else 1 for v in vecs], dtype=np.int32)
    status0 = np.where(active == 1, 0, S.POISON_I32).astype(np.int32)
    r = _run(exe, tmp_path, S.pack_case(S.OP_WEIGHTS, B, K, active, lam=lam, status0=status0, cost=cost), S.OP_WEIGHTS, B, K)
    assert r["form"] == _weights_form(K)
    assert np.all(S.is_poison(r["w_guard"]))
    for b in range(B):
        if not active[b]:
            assert np.all(S.is_poison(r["w"][b])) and S.is_poison(r["wsum"][b:b + 1])[0] and r["status"][b] == S.POISON_I32
    return r


@pytest.mark.parametrize("kind", ["generic", "equal", "underflow", "huge_lambda", "lane_penalty"])
@pytest.mark.parametrize("K", WEIGHT_KS)
def test_weights_against_long_double(harness, tmp_path, oracle, K, kind):
    """k_weights (register form at both workgroup sizes, three-pass form) against compute_weights in np.longdouble: per weight
    4 2^-52 (|x_k| + log2 K + 4) w_ref with x_k = -(c_k - min c) / lambda (rounding of the exponent's argument, summation depth, a 1-ulp exp), floor =
    the smallest subnormal; the sum of the weights within K 2^-52 of 1.  The oracle's own double arithmetic is held to the same tolerance on the same
    input first, so the bound tests the kernel and not the input."""
    lam, vecs = S.weight_cost_cases(K, np.random.default_rng(2000 + K))[kind]
    slots = [vecs[0], None, vecs[1]] if K % 2 else [vecs[0], vecs[1], None]
    for c in vecs:
        tol, ref = S.weights_tol(c, lam)
        assert np.all(np.abs(oracle.compute_weights(lam, c).astype(np.longdouble) - ref) <= tol)
    r = _run_weights(harness, tmp_path, K, lam, slots)
    for b, c in enumerate(slots):
        if c is None:
            continue
        tol, ref = S.weights_tol(c, lam)
        err = np.abs(r["w"][b].astype(np.longdouble) - ref)
        worst = int(np.argmax(err / tol))
        print("K %d %s slot %d: worst error / tolerance %.3f (w_ref %.3e), |wsum - 1| = %.3e" % (K, kind, b, float(err[worst] / tol[worst]), float(ref[worst]), abs(r["wsum"][b] - 1.0)))
        assert np.all(err <= tol), (b, worst, float(err[worst]), float(tol[worst]))
        assert abs(r["wsum"][b] - 1.0) <= K * 2.0 ** -52
        assert r["status"][b] == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("K", [1000, 9000])
def test_weights_flag_a_non_finite_cost_for_its_slot_only(harness, tmp_path, K, bad):
    rng = np.random.default_rng(K)
    a, b, c = (rng.standard_normal(K) * 20.0 + 100.0 for _ in range(3))
    clean = _run_weights(harness, tmp_path, K, 10.0, [a, b, c, None])
    assert clean["status"][:3].tolist() == [0, 0, 0]
    hurt = b.copy(); hurt[K // 2] = bad
    r = _run_weights(harness, tmp_path, K, 10.0, [a, hurt, c, None])
    assert r["status"][:3].tolist() == [0, S.ERR_ACTION, 0]
    for s in (0, 2):
        assert np.array_equal(_bits(r["w"][s]), _bits(clean["w"][s])) and r["wsum"][s] == clean["wsum"][s]


LAM_EVEN, LAM_ODD = 10.0, 0.7


def _assert_slot_bits(per_slot, scalar, b):
    assert np.array_equal(_bits(per_slot["w"][b]), _bits(scalar["w"][b])), b
    assert np.array_equal(_bits(per_slot["wsum"][b:b + 1]), _bits(scalar["wsum"][b:b + 1])), b
    assert per_slot["status"][b] == scalar["status"][b], b


@pytest.mark.parametrize("K", [1, 256, 1024, 8192, 8193])
def test_weights_per_slot_lambda_is_the_scalar_run_of_that_lambda(harness, tmp_path, K):
    """The per-slot instantiation of k_weights differs from the scalar one by the load of -1/λ_b alone: each active slot's w and wsum are
    bit-equal to a scalar run with that slot's λ (smallest K, a full 256-thread register form, the first and the last 1024-thread register form,
    the first three-pass form).  _run_weights checks the form, the inactive slot and the guards of every run."""
    rng = np.random.default_rng(3000 + K)
    a, b, c = (rng.standard_normal(K) * 20.0 + 100.0 for _ in range(3))
    slots = [a, b, c, None]
    per_slot = _run_weights(harness, tmp_path, K, (LAM_EVEN, LAM_ODD), slots)
    scalar = [_run_weights(harness, tmp_path, K, lam, slots) for lam in (LAM_EVEN, LAM_ODD)]
    for s in range(3):
        _assert_slot_bits(per_slot, scalar[s % 2], s)
        assert per_slot["status"][s] == 0
    if K > 1:                                                                          # the two λ do weigh differently: the runs are not one run
        assert not np.array_equal(_bits(scalar[0]["w"][0]), _bits(scalar[1]["w"][0]))


def test_weights_per_slot_lambda_flags_a_nan_cost_for_its_slot_only(harness, tmp_path):
    K = 1000
    rng = np.random.default_rng(3000 + K)
    a, b, c = (rng.standard_normal(K) * 20.0 + 100.0 for _ in range(3))
    clean = _run_weights(harness, tmp_path, K, (LAM_EVEN, LAM_ODD), [a, b, c, None])
    hurt = b.copy(); hurt[K // 2] = np.nan
    r = _run_weights(harness, tmp_path, K, (LAM_EVEN, LAM_ODD), [a, hurt, c, None])
    assert clean["status"][:3].tolist() == [0, 0, 0] and r["status"][:3].tolist() == [0, S.ERR_ACTION, 0]
    for s in (0, 2):
        _assert_slot_bits(r, clean, s)
