"""Inputs, file format, host-side rules and references for the direct tests of the two adaptation steps (tools/kbench_adapt.hip: kernels_nes.hip
and kernels_cma.hip): shared by tests/test_adapt_cases_cpu.py (which proves on the CPU that the inputs and the references are what they claim) and
tests/test_gpu_adapt_harness.py.  Nothing here touches the engine.  References are np.longdouble evaluations of the exact float64 inputs, written
from the formulas in the two kernel files' headers and the oracle.  The error bounds are derived, not measured (u = 2^-53):

  sums of products   |got - ref| <= 2 (n + 8) u sum|terms|   for an n-term sum (scatter entries: n = K; every GEMM entry, S g, ||p_sigma||^2: n = the
                     matrix order; temp_sum: n = K).  (n - 1) u sum|terms| is the forward bound of an n-term sum in ANY order, with or without FMA;
                     the + 8 covers the roundings inside a term (c_k x_ak, the alpha / beta scalings and the D term of a GEMM, the nine operations
                     of a temp_sum term), the factor 2 the second-order terms and the rounding of the longdouble reference itself.
  triangular inverse |L X - I| <= 2 (n + 2) u |L| |X| componentwise: forward substitution is backward stable, (L + dL) x = e_j with |dL| <= n u |L|
                     whatever the order of the row's sum; the row's two accumulators, their sum and the division are the + 2.
  elementwise        |got - ref| <= 16 u sum|terms| for the closed formulas of the CMA kernels (p_sigma, p_Sigma, U += sigma dw, the Sigma update):
                     no term passes through more than 12 roundings (the Sigma update's middle term: eight to form the factor, the products, the adds).
  exp / sqrt / pow   the sum bound of ||p_sigma||^2 propagated to first order through the reference formula, + 8 u relative per library function
                     (the HIP math API reference lists 1 ULP for the double-precision exp, pow and sqrt: below 8 u = 4 ULP, so 8 u stands).
A structural error -- a dropped column, a wrong row, a stale partial, a missing mirror -- moves an entry by about sum|terms| / n, 1e12 bounds away."""
import numpy as np
from tests.helpers import harness_io as IO
from tests.helpers.harness_io import F64, I32, GUARD, LD, U, bits, is_poison, split_guard                # (re-exported: the tests read them as A.<name>)

OP_BREAK, OP_SCATTER, OP_POTRI, OP_UPDATE, OP_CMA_BEGIN, OP_CMA_PATHS, OP_CMA_SIGMA = range(7)
OPS = ("BREAK", "SCATTER", "POTRI", "UPDATE", "CMA_BEGIN", "CMA_PATHS", "CMA_SIGMA")
MAGIC_IN, MAGIC_OUT = b"ADPCASE1", b"ADPRES01"
POISON_I32 = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]
POISON_F64_BITS = np.frombuffer(b"\xa5" * 8, dtype=np.uint64)[0]
POISON_F64 = np.frombuffer(b"\xa5" * 8, dtype=np.float64)[0]
ELEM = 16                                                  # roundings allowed to an elementwise formula (see above)
LIBM = 8                                                   # u per exp / sqrt / pow
# include/mpopis.h
OK, ERR_ARG, ERR_NOT_PD, ERR_ACTION, ERR_HIP, ERR_NUMERIC = 0, -1, -2, -3, -4, -5
BREAK_TOL = np.float64(10e-3)                              # the reference writes it this way (:868)
# kernels_nes.hip / kernels_cma.hip (tests/test_adapt_cases_cpu.py reads them back from the sources)
NES_KC, NES_PW, NES_WAVES = 32, 7, 4
NES_PB = NES_WAVES * NES_PW
TRTRI_LDS_DOUBLES, TRTRI_MAX_CPB = 150 * 1024 // 8, 64
CMA_THREADS = 1024


# ---- the case lists of tests/test_gpu_adapt_harness.py (the CPU file proves what they reach) ----------------------------------------------------
BREAK_KS = (2, 255, 256, 257, 1000)
SCATTER_CS = (1, 15, 16, 17, 32, 100, 111, 112, 300)
SCATTER_KS = (1, 31, 32, 33, 100, 1024)
SCATTER_KSPLITS = (1, 3, 32)
# (cs, K, ksplit, slot 0: "cancel" costs of both signs that nearly cancel | "zero" all-zero costs): every cs at (100, 3), every K and ksplit at cs = 17
# and cs = 112, and the two shapes whose whole splits are empty
SCATTER_CASES = [(cs, 100, 3, ("cancel", "zero")[i % 2]) for i, cs in enumerate(SCATTER_CS)] + \
                [(cs, K, ks, ("cancel", "zero")[(i + j) % 2]) for cs in (17, 112) for i, K in enumerate(SCATTER_KS) for j, ks in enumerate(SCATTER_KSPLITS)] + \
                [(17, 40, 4, "cancel"), (112, 40, 4, "zero"), (17, 33, 32, "zero"), (112, 33, 32, "cancel")]
SCATTER_CASES = list(dict.fromkeys(SCATTER_CASES))
# what the shapes reach: cs -> (tiles per side, tile pairs, pair-blocks, waves of the last pair-block that own no pair)
SCATTER_TILES = {1: (1, 1, 1, 3), 15: (1, 1, 1, 3), 16: (2, 3, 1, 3), 17: (2, 3, 1, 3), 32: (3, 6, 1, 3), 100: (7, 28, 1, 0), 111: (7, 28, 1, 0),
                 112: (8, 36, 2, 2), 300: (19, 190, 7, 0)}
# (K, ksplit) -> (columns per split, empty splits, length of the last non-empty split's last chunk: 32 = exact)
SCATTER_SPLITS = {(1, 1): (32, 0, 1), (1, 3): (32, 2, 1), (1, 32): (32, 31, 1), (31, 1): (32, 0, 31), (31, 3): (32, 2, 31), (31, 32): (32, 31, 31),
                  (32, 1): (32, 0, 32), (32, 3): (32, 2, 32), (32, 32): (32, 31, 32), (33, 1): (64, 0, 1), (33, 3): (32, 1, 1), (33, 32): (32, 30, 1),
                  (100, 1): (128, 0, 4), (100, 3): (64, 1, 4), (100, 32): (32, 28, 4), (1024, 1): (1024, 0, 32), (1024, 3): (352, 0, 32),
                  (1024, 32): (32, 0, 32), (40, 4): (32, 2, 8)}
POTRI_NS = (1, 3, 16, 17, 100, 300, 301, 400)
POTRI_CPB = {1: 64, 3: 64, 16: 64, 17: 64, 100: 64, 300: 64, 301: 63, 400: 48}
# (n, "random" | "graded" factor, shared factor (Lstride 0), active given): every n with both kinds between them, both strides and both forms of active
POTRI_CASES = [(1, "random", False, False), (1, "graded", True, True), (3, "graded", True, True), (3, "random", False, False), (16, "random", True, False),
               (16, "graded", False, True), (17, "graded", False, True), (17, "random", True, False), (100, "random", False, True), (100, "graded", True, False),
               (300, "random", True, True), (300, "graded", False, True), (301, "graded", False, False), (301, "random", True, True), (400, "random", False, True),
               (400, "graded", True, True)]
UPDATE_CS = (3, 16, 17, 100, 112)
UPDATE_K, UPDATE_KSPLIT = 100, 3
# (cs, S per slot, A per slot, per-slot scales): the four stride combinations with both scale forms at cs = 17 and 112, one combination each elsewhere
UPDATE_CASES = [(cs, s, a, (i + s + a) % 2 == 1) for i, cs in enumerate((17, 112)) for s in (False, True) for a in (False, True)] + \
               [(3, True, False, True), (16, False, True, False), (100, True, True, True), (16, True, False, True), (3, False, False, False)]
CMA_BEGIN_CASES = [(cs, per_slot) for cs in (1, 100) for per_slot in (False, True)]
CMA_PATHS_SHAPES = ((1, 5, 5), (20, 192, 38), (7, 4097, 820), (100, 4096, 819), (300, 1024, 205))
# (cs, K, m_elite, n_iter, kind): "plain" | "h_below" / "h_above" (||p_sigma|| 1e-6 relative below / above the h_sigma threshold) | "zero" (an exact zero
# of E under a negative weight)
CMA_PATHS_CASES = [(cs, K, m, (1, 3)[i % 2], "plain") for i, (cs, K, m) in enumerate(CMA_PATHS_SHAPES)] + \
                  [(cs, K, m, (3, 1)[i % 2], "plain") for i, (cs, K, m) in enumerate(CMA_PATHS_SHAPES)] + \
                  [(20, 192, 38, 1, "h_below"), (20, 192, 38, 1, "h_above"), (7, 4097, 820, 3, "h_below"), (7, 4097, 820, 3, "h_above"), (20, 192, 38, 3, "zero"),
                   (100, 4096, 819, 1, "zero")]
H_REL = 1e-6
CMA_SIGMA_CASES = [(cs, h) for cs in (1, 16, 17, 300) for h in (0, 1)]


# ---- the harness's files ---------------------------------------------------------------------------------------------------------------------
def pack_case(op, B, ipar, dpar, arrays):
    """arrays: list of (type, array or None) in the op's fixed order (None = not given)"""
    return IO.pack_case(MAGIC_IN, op, B, ipar, dpar, arrays)


def unpack_case(buf):
    return IO.unpack_case(MAGIC_IN, buf)


def pack_result(arrays):
    """what the harness writes (used by the CPU round-trip test); arrays: list of (type, array with its guard entries)"""
    return IO.pack_result(MAGIC_OUT, 0, arrays)


def unpack_result(buf):
    """-> [arrays as written, guard entries included]"""
    return IO.unpack_result(MAGIC_OUT, buf)[1]


def cm(flat, n):
    """the column-major n x n matrix in `flat` as a NumPy matrix (A[i, j] = flat[i + j n])"""
    return np.asarray(flat).reshape(n, n).T


def to_cm(A):
    return np.ascontiguousarray(np.asarray(A).T).reshape(-1)


def sum_bound(n, terms):
    return 2 * (n + 8) * LD(U) * np.asarray(terms, dtype=LD)


def elem_bound(terms):
    return ELEM * LD(U) * np.asarray(terms, dtype=LD)


# ---- host rules (restated from the launchers) ---------------------------------------------------------------------------------------------------
def nes_tiles(cs):
    """-> (tiles per side incl. the ones row, tile pairs, pair-blocks, waves of the last pair-block without a pair)"""
    nt = cs // 16 + 1
    npairs = nt * (nt + 1) // 2
    blocks = (npairs + NES_PB - 1) // NES_PB
    idle = sum(1 for w in range(NES_WAVES) if (blocks - 1) * NES_PB + w * NES_PW >= npairs)
    return nt, npairs, blocks, idle


def nes_splits(K, ksplit):
    """-> (columns per split, empty splits, columns in the last chunk of the last non-empty split)"""
    per = ((K + ksplit - 1) // ksplit + NES_KC - 1) // NES_KC * NES_KC
    empty = sum(1 for s in range(ksplit) if s * per >= K)
    last = [min(K, s * per + per) - s * per for s in range(ksplit) if s * per < K][-1]
    return per, empty, (last - 1) % NES_KC + 1


def trtri_cpb(n):
    return max(1, min(TRTRI_MAX_CPB, TRTRI_LDS_DOUBLES // n))


def status_rank(c):
    return 4 if c == ERR_HIP else 3 if c == ERR_ACTION else 2 if c == ERR_NOT_PD else 1 if c == ERR_NUMERIC else 5 if c < 0 else 0


def cma_constants(cs, K, m_elite):
    """init_cma_constants (CMAMPPI_Policy's constructor, :513-525) in float64 -> (consts7 = mu_eff, c_sigma, d_sigma, c_Sigma, c1, c_mu, E_cma; ws[K])"""
    m, n = K, float(cs)
    ws = np.array([np.log((m + 1) / 2.0) - np.log(float(i)) for i in range(1, m + 1)])
    s = 0.0
    for i in range(m_elite):
        s += ws[i]
    ws[:m_elite] = ws[:m_elite] / s
    s2 = 0.0
    for i in range(m_elite):
        s2 += ws[i] * ws[i]
    mu_eff = 1 / s2
    c_sigma = (mu_eff + 2) / (n + mu_eff + 5)
    d_sigma = 1 + 2 * max(0.0, np.sqrt(max(0.0, (mu_eff - 1) / (n + 1))) - 1) + c_sigma          # (fmax(0, NaN) = 0 in the C form)
    c_Sigma = (4 + mu_eff / n) / (n + 4 + 2 * mu_eff / n)
    c1 = 2 / ((n + 1.3) * (n + 1.3) + mu_eff)
    c_mu = min(1 - c1, 2 * (mu_eff - 2 + 1 / mu_eff) / ((n + 2) * (n + 2) + mu_eff))
    if m_elite < m:
        st = 0.0
        for i in range(m_elite, m):
            st += ws[i]
        ws[m_elite:] = ws[m_elite:] * (-(1 + c1 / c_mu) / st)
    E_cma = np.sqrt(n) * (1 - 1 / (4 * n) + 1 / (21 * (n * n)))
    return np.array([mu_eff, c_sigma, d_sigma, c_Sigma, c1, c_mu, E_cma]), ws


def actives(B, inactive):
    a = np.ones(B, dtype=np.int32)
    if inactive is not None:
        a[inactive] = 0
    return a


# ================================================================ BREAK ========================================================================
def break_ref(cost, active, status):
    """k_nes_break (:868-870): a non-finite cost raises MPOPIS_ERR_ACTION and stops the slot; else max |c_k+1 - c_k| < 10e-3 stops it (NaN never)"""
    active, status = active.copy(), status.copy()
    for b in range(len(active)):
        if not active[b]:
            continue
        c = cost[b].astype(LD)
        if not np.all(np.isfinite(cost[b])):
            if status_rank(ERR_ACTION) > status_rank(status[b]):
                status[b] = ERR_ACTION
            active[b] = 0
        elif len(c) < 2 or np.max(np.abs(np.diff(c))) < LD(BREAK_TOL):        # K = 1: Julia's maximum of an empty collection throws; the engine needs K >= 2
            active[b] = 0
    return active, status


def break_slot(K, pos, diff, seed):
    """costs whose largest consecutive difference is exactly `diff`, at pair (pos, pos + 1); every other difference stays below 2.1e-3"""
    rng = np.random.default_rng(seed)
    c = 1e-3 * rng.random(K)
    c[pos + 1:] += diff
    c[pos], c[pos + 1] = 0.0, diff
    if pos + 2 < K:
        c[pos + 2] = diff + 1e-3 * rng.random()
    return c


def break_case(K):
    """8 slots: the deciding pair first / across the 256-thread stride / last, each at exactly 0.01 (strict <: the slot stays active) and at the next
    double below (stops); the remaining slots: an inactive one (keeps active and status), random large differences (stays), constant costs (stops)"""
    below = np.nextafter(BREAK_TOL, 0.0)
    pos = [p for p in dict.fromkeys((0, 255, K - 2)) if 0 <= p <= K - 2]
    slots = [(p, d) for p in pos for d in (BREAK_TOL, below)]
    cost, intent = [], []
    for i, (p, d) in enumerate(slots):
        cost.append(break_slot(K, p, d, 100 * K + i)); intent.append("stay" if d == BREAK_TOL else "stop")
    rng = np.random.default_rng(K)
    extra = [("inactive", 5.0 * rng.standard_normal(K)), ("stay", 5.0 * rng.standard_normal(K)), ("stop", np.full(K, -3.25)), ("stop", 7.0 + 9e-3 * rng.random(K)),
             ("stay", break_slot(K, K // 2 if K > 2 else 0, 0.5, K + 7))]
    for name, c in extra[:8 - len(slots)]:
        cost.append(c); intent.append(name)
    B = len(cost)
    cost = np.array(cost)
    active = np.array([0 if s == "inactive" else 1 for s in intent], dtype=np.int32)
    status = np.array([(OK, ERR_NUMERIC, OK, ERR_NOT_PD)[b % 4] for b in range(B)], dtype=np.int32)          # a break never touches status
    return dict(K=K, B=B, cost=cost, active=active, status=status, intent=intent,
                data=pack_case(OP_BREAK, B, [K], [], [(I32, active), (F64, cost), (I32, status)]))


def break_nonfinite_case(K=257):
    """+inf, NaN and -inf costs -> MPOPIS_ERR_ACTION and active 0; a status that already ranks higher (MPOPIS_ERR_HIP, MPOPIS_ERR_ARG) stays, a lower
    one (NOT_PD, NUMERIC) is replaced; an inactive slot with a non-finite cost keeps both; the bad cost sits first, last and across the thread stride"""
    rng = np.random.default_rng(31)
    cost = 5.0 * rng.standard_normal((8, K))
    cost[0, 0] = np.inf; cost[1, K - 1] = np.nan; cost[2, 256] = -np.inf; cost[3, 100] = np.inf; cost[4, 3] = np.nan; cost[5, 255] = np.inf; cost[6, 7] = np.nan
    active = np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    status = np.array([OK, OK, ERR_NUMERIC, ERR_HIP, ERR_NOT_PD, ERR_ARG, ERR_NUMERIC, ERR_NOT_PD], dtype=np.int32)
    return dict(K=K, B=8, cost=cost, active=active, status=status, intent=["error"] * 6 + ["inactive", "stay"],
                data=pack_case(OP_BREAK, 8, [K], [], [(I32, active), (F64, cost), (I32, status)]))


# ================================================================ SCATTER / UPDATE ==============================================================
def slot_samples(cs, K, kind, seed):
    """(E [cs][K], cost [K]) of one slot; the data depends on (cs, K, kind, seed) alone, so the same slot can sit in batches of different size"""
    rng = np.random.default_rng([seed, cs, K])
    E = rng.standard_normal((cs, K)) * (0.25 + rng.random((cs, 1)))
    if kind == "zero":
        c = np.zeros(K)
    elif kind == "cancel":                       # both signs, the sum cancels to ~1e-8 of sum|c|
        c = 100.0 * np.where(np.arange(K) % 2 == 0, 1.0, -1.0) * (1.0 + 1e-8 * rng.standard_normal(K))
        if K % 2:
            c[-1] = 1e-6
    else:
        c = 50.0 * rng.standard_normal(K) + 20.0
    return E, c


def scatter_case(cs, K, ksplit, slot0="cancel", single=False):
    """B = 3: slot 0 `slot0`, slot 1 inactive, slot 2 generic signed costs; single: slot 2 alone (B = 1, the same data)"""
    kinds = ["generic"] if single else [slot0, "generic", "generic"]
    seeds = [2] if single else [0, 1, 2]
    B = len(kinds)
    sl = [slot_samples(cs, K, k, s) for k, s in zip(kinds, seeds)]
    E = np.array([s[0] for s in sl]); cost = np.array([s[1] for s in sl])
    active = actives(B, None if single else 1)
    return dict(cs=cs, K=K, ksplit=ksplit, B=B, E=E, cost=cost, active=active, kinds=kinds,
                data=pack_case(OP_SCATTER, B, [cs, K, ksplit], [], [(I32, active), (F64, E), (F64, cost)]))


def scatter_reference(E, c):
    """-> (M, g, C) and the sums of |terms| (tM, tg, tC) in longdouble: M = sum_k c_k E_k E_k', g = sum_k c_k E_k, C = sum_k c_k"""
    El, cl = E.astype(LD), c.astype(LD)
    Ec = El * cl
    M, g, C = Ec @ El.T, Ec.sum(axis=1), cl.sum()
    aE = np.abs(El); aEc = np.abs(Ec)
    return (M, g, C), (aEc @ aE.T, aEc.sum(axis=1), np.abs(cl).sum())


def update_case(cs, s_per_slot, a_per_slot, per_slot_scale, single=False, K=UPDATE_K, ksplit=UPDATE_KSPLIT):
    """launch_nes_update on the scatter case's samples; S: a symmetric positive definite matrix (Sigma^-1), A: a general matrix, U: a vector;
    scales -sf_b / K^2 and sf_b / K with another step factor in every slot.  single: slot 2 alone, with slot 2's matrices and scales"""
    sc = scatter_case(cs, K, ksplit, "cancel", single)
    B = sc["B"]
    ids = [2] if single else [0, 1, 2]

    def mats(seed):
        rng = np.random.default_rng([seed, cs])
        G = rng.standard_normal((cs, cs))
        S = G @ G.T / cs + 0.5 * np.eye(cs)
        S = 0.5 * (S + S.T)
        A = 0.3 * rng.standard_normal((cs, cs)) + np.eye(cs)
        return S, A, rng.standard_normal(cs)
    ms = [mats(10 + i) for i in ids]
    shared = mats(10)
    S = np.array([m[0] for m in ms]) if s_per_slot else shared[0][None]
    A = np.array([m[1] for m in ms]) if a_per_slot else shared[1][None]
    U0 = np.array([m[2] for m in ms])
    sf = np.array([0.01 * (1 + 0.5 * i) for i in ids])
    a_b, u_b = -sf / K / K, sf / K
    if per_slot_scale:
        dpar, arr_a, arr_u = [1.0, 1.0], a_b, u_b                   # (the scalar is unused with a per-slot array)
    else:
        a_b, u_b = np.full(B, a_b[-1]), np.full(B, u_b[-1])
        dpar, arr_a, arr_u = [a_b[0], u_b[0]], None, None
    nn = cs * cs
    arrays = [(I32, sc["active"]), (F64, sc["E"]), (F64, sc["cost"]), (F64, np.array([to_cm(x) for x in S])), (F64, np.array([to_cm(x) for x in A])), (F64, U0),
              (F64, arr_a), (F64, arr_u)]
    out = dict(sc)
    out.update(S=S, A=A, U0=U0, a_scale=a_b, u_scale=u_b, s_per_slot=s_per_slot, a_per_slot=a_per_slot, per_slot_scale=per_slot_scale, scatter_data=sc["data"],
               data=pack_case(OP_UPDATE, B, [cs, K, ksplit, nn if s_per_slot else 0, nn if a_per_slot else 0], dpar, arrays))
    return out


def gemm_reference(A, Bm, alpha=1.0, D=None, beta=0.0):
    """alpha A B + beta D and the sum of |terms|, longdouble"""
    Al, Bl = np.asarray(A).astype(LD), np.asarray(Bm).astype(LD)
    ref, terms = LD(alpha) * (Al @ Bl), abs(LD(alpha)) * (np.abs(Al) @ np.abs(Bl))
    if D is not None:
        ref = ref + LD(beta) * np.asarray(D).astype(LD)
        terms = terms + np.abs(LD(beta) * np.asarray(D).astype(LD))
    return ref, terms


def nes_gradients_ld(E, c, Sinv):
    """(G, Sigma^-1 g) of kernels_nes.hip's header in longdouble: G = S M S - C S"""
    (M, g, C), _ = scatter_reference(E, c)
    S = Sinv.astype(LD)
    return S @ M @ S - C * S, S @ g


# ================================================================ POTRI ========================================================================
def potri_factor(n, kind, seed):
    """the Cholesky factor of a random SPD matrix; "graded": variances graded over 8 decades"""
    rng = np.random.default_rng([seed, n])
    G = rng.standard_normal((n, n + 3))
    A = G @ G.T / (n + 3) + 0.05 * np.eye(n)
    if kind == "graded":
        d = 10.0 ** (np.linspace(-2.0, 2.0, n) if n > 1 else np.array([2.0]))           # standard deviations 1e-2 .. 1e2: variances 1e-4 .. 1e4
        A = A * d[:, None] * d[None, :]
    return np.linalg.cholesky(0.5 * (A + A.T))


def potri_case(n, kind, shared, use_active):
    """B = 2; with `active` given slot 0 is inactive"""
    B = 2
    L = np.array([potri_factor(n, kind, 5 + b) for b in range(1 if shared else B)])
    active = actives(B, 0 if use_active else None)
    return dict(n=n, B=B, L=L, shared=shared, use_active=use_active, active=active, computed=active if use_active else np.ones(B, dtype=np.int32),
                data=pack_case(OP_POTRI, B, [n, 0 if shared else n * n, int(use_active)], [], [(I32, active), (F64, np.array([to_cm(x) for x in L]))]))


def trtri_residual(L, X):
    """|L X - I| and its bound 2 (n + 2) u |L| |X|, longdouble"""
    n = L.shape[0]
    Ll, Xl = L.astype(LD), X.astype(LD)
    return np.abs(Ll @ Xl - np.eye(n, dtype=LD)), 2 * (n + 2) * LD(U) * (np.abs(Ll) @ np.abs(Xl))


def potri_reference(L):
    """(X = L^-1 by forward substitution, S = X'X) in longdouble"""
    n = L.shape[0]
    Ll = L.astype(LD)
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        r = -(Ll[i, :i] @ X[:i, :])
        r[i] += 1
        X[i] = r / Ll[i, i]
    return X, X.T @ X


# ================================================================ CMA ==========================================================================
def cma_begin_case(cs, per_slot):
    B = 3
    s0 = np.array([0.7, 1.0, 1.9])
    return dict(cs=cs, B=B, sigma0=s0 if per_slot else np.full(B, 1.3),
                data=pack_case(OP_CMA_BEGIN, B, [cs], [1.3], [(I32, actives(B, None)), (F64, s0 if per_slot else None)]))


def h_threshold(cs, n_iter, consts):
    """h_sigma = ||p_sigma|| < this (:585 solved for the norm), longdouble"""
    c_s, E_cma = LD(consts[1]), LD(consts[6])
    return (LD(1.4) + LD(2.0) / (cs + 1)) * E_cma * np.sqrt(1 - (1 - c_s) ** (2 * n_iter))


def cma_paths_case(cs, K, m_elite, n_iter, kind="plain", use_active=True):
    """B = 3 with the middle slot inactive (use_active False: B = 2, nullptr).  Slot state as after an earlier iteration (p_sigma, p_Sigma nonzero,
    sigma != 1) except in the h_sigma cases, which start from p_sigma = 0 so that ||p_sigma|| = sc ||y|| can be placed; `order` a random permutation"""
    B = 3 if use_active else 2
    consts, ws = cma_constants(cs, K, m_elite)
    rng = np.random.default_rng([cs, K, n_iter, len(kind)])
    E = rng.standard_normal((B, cs, K)) * 0.4
    order = np.array([rng.permutation(K) for _ in range(B)], dtype=np.int32)
    sigma = np.array([0.8, 1.0, 1.25])[:B]
    ps = 0.5 * rng.standard_normal((B, cs)); pS = 0.3 * rng.standard_normal((B, cs)); dw = 0.2 * rng.standard_normal((B, cs))
    y = rng.standard_normal((B, cs)) * np.sqrt(cs / (cs + 1.0))
    fro = cs * (1.0 + rng.random(B))
    U0 = rng.standard_normal((B, cs))
    if kind in ("h_below", "h_above"):
        ps[:] = 0.0
        sc = np.sqrt(consts[1] * (2 - consts[1]) * consts[0])
        target = float(h_threshold(cs, n_iter, consts)) * (1 - H_REL if kind == "h_below" else 1 + H_REL)
        y = y * (target / (sc * np.sqrt(np.sum(y.astype(LD) ** 2, axis=1)).astype(np.float64)))[:, None]
    if kind == "zero":
        for b in range(B):
            ii = int(np.flatnonzero(ws < 0)[b])                                   # a negative weight
            j = int(order[b, ii])
            E[b, j % cs, order[b, j // cs]] = 0.0
    scal = np.tile(np.array([0.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0, 17.0]), (B, 1)); scal[:, 0] = sigma
    vec = np.concatenate([ps, pS, dw], axis=1)
    active = actives(B, 1 if use_active else None)
    arrays = [(I32, active), (F64, y), (F64, fro), (F64, E), (I32, order), (F64, ws), (F64, U0), (F64, scal), (F64, vec)]
    return dict(cs=cs, K=K, m_elite=m_elite, n_iter=n_iter, kind=kind, B=B, consts=consts, ws=ws, E=E, order=order, y=y, fro=fro, U0=U0, scal=scal, vec=vec,
                active=active, computed=active if use_active else np.ones(B, dtype=np.int32),
                data=pack_case(OP_CMA_PATHS, B, [cs, K, n_iter, m_elite, int(use_active)], consts, arrays))


def temp_sum_terms(E, order, ws, sigma_old, fro, n_iter):
    """the K terms of temp_sum (:588-596) in longdouble, IEEE results included: ds[order[ii]] indexes ds = elite_E / sigma (cs x m_elite) linearly;
    a negative weight is rescaled by n / norm(C ds)^2 with norm(C d)^2 = d^2 ||C||_F^2 -- at d = 0 that is -inf 0 0 = NaN"""
    cs, K = E.shape
    j = order.astype(np.int64)
    d = E[j % cs, order[j // cs]].astype(LD) / LD(sigma_old)
    w = ws.astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        nc = np.sqrt((d * d) * LD(fro))
        w0 = np.where(w >= 0, w, n_iter * w / (nc * nc))
        return w0 * d * d


def cma_paths_reference(c, b, ps_dev=None):
    """slot b of launch_cma_paths in longdouble -> dict of (ref, bound) per output.  ps_dev: the device's new p_sigma; ||p_sigma|| and what follows
    from it (sigma, sigma^2) are then taken from those bits, as that stage received them"""
    cs, K, n = c["cs"], c["K"], c["n_iter"]
    mu_eff, c_s, d_s, c_S, c1, c_mu, E_cma = [LD(v) for v in c["consts"]]
    sig = LD(c["scal"][b, 0])
    ps, pS, dw = [c["vec"][b, i * cs:(i + 1) * cs].astype(LD) for i in range(3)]
    y = c["y"][b].astype(LD)
    out = {}
    out["U"] = (c["U0"][b].astype(LD) + sig * dw, elem_bound(np.abs(c["U0"][b].astype(LD)) + np.abs(sig * dw)))                # :577
    sc = np.sqrt(c_s * (2 - c_s) * mu_eff)
    pn = (1 - c_s) * ps + sc * y                                                                                             # :581
    out["ps"] = (pn, elem_bound(np.abs((1 - c_s) * ps) + np.abs(sc * y)))
    pin = pn if ps_dev is None else ps_dev.astype(LD)
    nps2 = np.sum(pin * pin)
    rel2 = 2 * (cs + 8) * LD(U)                                              # relative sum bound of ||p_sigma||^2 (all terms positive)
    nps = np.sqrt(nps2)
    rel_nps = rel2 / 2 + LIBM * LD(U)
    out["nps"] = (nps, nps * rel_nps)
    a = c_s / d_s
    x = a * (nps / E_cma - 1)                                                                                                # :582
    dx = a * nps / E_cma * rel_nps + ELEM * LD(U) * a * (nps / E_cma + 1)
    sig_new = sig * np.exp(x)
    rel_sig = dx + LIBM * LD(U) + 2 * LD(U)
    out["sigma"] = (sig_new, sig_new * rel_sig)
    out["sig2"] = (sig_new * sig_new, sig_new * sig_new * (2 * rel_sig + 2 * LD(U)))
    lhs = nps / np.sqrt(1 - (1 - c_s) ** (2 * n))
    thr = (LD(1.4) + LD(2.0) / (cs + 1)) * E_cma
    h = 1 if lhs < thr else 0                                                                                                # :585
    out["h"] = h
    out["h_margin"] = float(lhs / thr - 1)
    sS = h * np.sqrt(c_S * (2 - c_S) * mu_eff)
    out["pS"] = ((1 - c_S) * pS + sS * dw, elem_bound(np.abs((1 - c_S) * pS) + np.abs(sS * dw)))                              # :586
    t = temp_sum_terms(c["E"][b], c["order"][b], c["ws"], c["scal"][b, 0], c["fro"][b], n)
    out["ts"] = (np.sum(t), sum_bound(K, np.sum(np.abs(t))))
    return out


def cma_sigma_case(cs, h, use_active=True):
    """B = 3 with the middle slot inactive; the input Sigma's strict lower triangle holds other values than its upper"""
    B = 3 if use_active else 2
    consts, _ = cma_constants(cs, 1024, 205)
    rng = np.random.default_rng([cs, h])
    G = rng.standard_normal((B, cs, cs))
    Sig = np.array([g @ g.T / cs + np.eye(cs) for g in G])
    Sig = np.triu(Sig) + np.tril(7.0 + rng.standard_normal((B, cs, cs)), -1)
    scal = np.tile(np.array([1.1, 0.0, float(h), 3.0, 4.0, 5.0, 6.0, 7.0]), (B, 1)); scal[:, 1] = 0.05 * rng.standard_normal(B)
    vec = rng.standard_normal((B, 3 * cs))
    active = actives(B, 1 if use_active else None)
    arrays = [(I32, active), (F64, np.array([to_cm(s) for s in Sig])), (F64, scal), (F64, vec)]
    return dict(cs=cs, h=h, B=B, consts=consts, Sig=Sig, scal=scal, vec=vec, active=active, computed=active if use_active else np.ones(B, dtype=np.int32),
                data=pack_case(OP_CMA_SIGMA, B, [cs, 1, int(use_active)], consts, arrays))


def cma_sigma_reference(Sig, ts, h, pS, consts):
    """:598-599 in longdouble: Sigma = (1 - c1 - c_mu) Sigma + c1 (p p' + (1 - h) c_S (2 - c_S) Sigma) .+ c_mu temp_sum, then the upper triangle
    mirrored (triu(S) + triu(S, 1)') -> (ref, bound)"""
    mu_eff, c_s, d_s, c_S, c1, c_mu, E_cma = [LD(v) for v in consts]
    S = np.triu(Sig.astype(LD)); S = S + np.triu(S, 1).T
    p = pS.astype(LD)
    t1, t2, t3, t4 = (1 - c1 - c_mu) * S, c1 * np.outer(p, p), c1 * ((1 - h) * c_S * (2 - c_S)) * S, c_mu * LD(ts)
    return t1 + t2 + t3 + t4, elem_bound(np.abs(t1) + np.abs(t2) + np.abs(t3) + np.abs(t4))
