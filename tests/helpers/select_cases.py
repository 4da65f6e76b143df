"""Inputs, file format and host-side rules for the direct tests of the selection kernels (tools/kbench_select.hip): shared by
tests/test_select_cases_cpu.py (which proves on the CPU that the inputs are what they claim) and tests/test_gpu_select_harness.py.
Nothing here touches the engine; references are NumPy and the oracle."""
import struct
import numpy as np
from tests.helpers.harness_io import GUARD, is_poison      # (re-exported: the tests read them under this module's name)

OP_SORT, OP_ALIAS_BUILD, OP_ALIAS_SAMPLE, OP_WEIGHTS, OP_CE_SORT = 0, 1, 2, 3, 4
MAGIC_IN, MAGIC_OUT = b"SELCASE1", b"SELRES01"
POISON_I32 = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]
POISON_F64_BITS = np.frombuffer(b"\xa5" * 8, dtype=np.uint64)[0]
# enums of mpopis_amd/csrc/engine.h
SORT_RANK, SORT_LDS, SORT_BITONIC4, SORT_BITONIC8, SORT_RANK_MULTI, SORT_RANK_BIG, SORT_CE_FUSED = 0, 1, 2, 3, 4, 5, 100
ALIAS_SEQ_LDS, ALIAS_SEQ_GLOBAL, ALIAS_PAR_THEN_SEQ_LDS = 0, 1, 2
WEIGHTS_REG_256, WEIGHTS_REG_1024, WEIGHTS_3PASS_1024 = 0, 1, 2
ERR_ACTION = -3
BREAK_THRESHOLD = 10e-3                                    # the reference writes it this way (:458-461)


# ---- the harness's files ---------------------------------------------------------------------------------------------------------------
def pack_case(op, B, K, active, m_elite=0, no_ws=False, lam=1.0, status0=None, cost=None, w=None, accept=None, alias=None, di=None, du=None,
              di_stride=0, log_stride=0):
    """lam: one λ, or (OP_WEIGHTS) a pair (λ_even, λ_odd): the per-slot mode, even slots weigh with the first and odd slots with the second"""
    lam_pair = np.ndim(lam) > 0
    lam_even, lam_odd = (float(lam[0]), float(lam[1])) if lam_pair else (float(lam), 0.0)
    assert not lam_pair or (op == OP_WEIGHTS and len(lam) == 2)
    active = np.ascontiguousarray(active, dtype=np.int32)
    status0 = np.zeros(B, dtype=np.int32) if status0 is None else np.ascontiguousarray(status0, dtype=np.int32)
    assert active.shape == (B,) and status0.shape == (B,)
    out = [MAGIC_IN, struct.pack("<7q", op, B, K, m_elite, (1 if no_ws else 0) | (2 if lam_pair else 0), di_stride, log_stride), struct.pack("<2d", lam_even, lam_odd),
           active.tobytes(), status0.tobytes()]
    f64 = lambda x, n: _arr(x, np.float64, n).tobytes()
    i32 = lambda x, n: _arr(x, np.int32, n).tobytes()
    if op in (OP_SORT, OP_CE_SORT, OP_WEIGHTS):
        out.append(f64(cost, B * K))
    elif op == OP_ALIAS_BUILD:
        out.append(f64(w, B * K))
    else:
        out += [f64(accept, B * K), f64(du, B * di_stride), i32(alias, B * K), i32(di, B * di_stride)]
    return b"".join(out)


def _arr(x, dt, n):
    x = np.ascontiguousarray(x, dtype=dt).reshape(-1)
    assert x.size == n, (x.size, n)
    return x


def unpack_case(buf):
    """inverse of pack_case (what the harness parses)"""
    assert buf[:8] == MAGIC_IN
    op, B, K, m_elite, flags, di_stride, log_stride = struct.unpack_from("<7q", buf, 8)
    lam, lam_odd = struct.unpack_from("<2d", buf, 64)
    if flags & 2:
        lam = (lam, lam_odd)
    off = 80
    def take(dt, n):
        nonlocal off
        a = np.frombuffer(buf, dtype=dt, count=n, offset=off).copy()
        off += a.nbytes
        return a
    c = dict(op=op, B=B, K=K, m_elite=m_elite, no_ws=bool(flags & 1), di_stride=di_stride, log_stride=log_stride, lam=lam)
    c["active"], c["status0"] = take(np.int32, B), take(np.int32, B)
    if op in (OP_SORT, OP_CE_SORT, OP_WEIGHTS):
        c["cost"] = take(np.float64, B * K).reshape(B, K)
    elif op == OP_ALIAS_BUILD:
        c["w"] = take(np.float64, B * K).reshape(B, K)
    else:
        c["accept"], c["du"] = take(np.float64, B * K).reshape(B, K), take(np.float64, B * di_stride).reshape(B, di_stride)
        c["alias"], c["di"] = take(np.int32, B * K).reshape(B, K), take(np.int32, B * di_stride).reshape(B, di_stride)
    assert off == len(buf)
    return c


def pack_result(op, form, f64s, i32s):
    """what the harness writes (used by the CPU round-trip test)"""
    return b"".join([MAGIC_OUT, struct.pack("<3q", form, GUARD, 0)] + [np.ascontiguousarray(a, np.float64).tobytes() for a in f64s] +
                    [np.ascontiguousarray(a, np.int32).tobytes() for a in i32s])


def unpack_result(buf, op, B, K, log_stride=0):
    """-> dict; arrays keep their guard entries as name + '_guard' (all poison if the launch wrote nothing past the end)"""
    assert buf[:8] == MAGIC_OUT, buf[:8]
    form, guard, _ = struct.unpack_from("<3q", buf, 8)
    assert guard == GUARD
    off = 32
    def take(dt, n):
        nonlocal off
        a = np.frombuffer(buf, dtype=dt, count=n, offset=off).copy()
        off += a.nbytes
        return a
    r = {"form": form}
    def guarded(name, dt, rows, cols):
        a = take(dt, rows * cols + GUARD)
        r[name], r[name + "_guard"] = a[:rows * cols].reshape(rows, cols), a[rows * cols:]
    if op in (OP_SORT, OP_CE_SORT):
        guarded("order", np.int32, B, K); r["active"] = take(np.int32, B); r["done"] = take(np.int32, B)
    elif op == OP_ALIAS_BUILD:
        guarded("accept", np.float64, B, K); guarded("alias", np.int32, B, K); r["need"] = take(np.int32, B)
    elif op == OP_ALIAS_SAMPLE:
        guarded("out", np.int32, B, K); guarded("log", np.int32, B, log_stride)
    else:
        guarded("w", np.float64, B, K); r["wsum"] = take(np.float64, B); r["status"] = take(np.int32, B)
    assert off == len(buf), (off, len(buf))
    return r


# ---- sort: host rules --------------------------------------------------------------------------------------------------------------------
def canonical_order(cost):
    """the device's total order: (cost, index) ascending with NaN placed like +inf.  For finite costs this is np.argsort(kind='stable') == Julia's
    sortperm; with non-finite costs the finite entries come first in stable order and every index appears once."""
    c = np.asarray(cost, dtype=np.float64)
    return np.argsort(np.where(np.isnan(c), np.inf, c), kind="stable").astype(np.int32)


def host_break(cost, order, m_elite):
    """maximum(abs.(diff(cost[order][1:m_elite]))) < 10e-3 (:458-461); np.max propagates NaN like Julia's maximum, so a non-finite elite key never breaks.
    No check below two elites (the engine's rule)."""
    if m_elite < 2:
        return False
    with np.errstate(invalid="ignore"):
        d = np.abs(np.diff(np.asarray(cost, dtype=np.float64)[np.asarray(order)[:m_elite]]))
        return bool(np.max(d) < BREAK_THRESHOLD)


def sort_vectors(K, rng):
    """name -> cost vector of length K: the generic finite cases"""
    v = {}
    v["distinct"] = rng.permutation(K) * 0.25 + 3.0
    v["distinct2"] = -rng.permutation(K) * 1.5 + 7.0
    v["equal"] = np.full(K, 2.5)
    v["alternating"] = np.where(np.arange(K) % 2 == 1, 1.0, -1.0)
    v["small_ints"] = rng.integers(0, 8, K).astype(np.float64)              # CartPole-like
    v["ascending"] = np.arange(K) * 0.5
    v["descending"] = (K - np.arange(K)) * 0.5
    d = rng.standard_normal(K) * 10.0
    if K > 70:
        d[K - 1] = d[30]; d[0] = d[30]; d[K // 2] = d[30]                   # equal keys far apart
    for p in DUP_BOUNDARIES:                                                # ... and blocks of exact duplicates straddling p-1 / p
        if p < K:
            d[max(p - 3, 0):min(p + 3, K)] = d[max(p - 3, 0)]
    v["dup_blocks"] = d
    return v


DUP_BOUNDARIES = (4, 8, 64, 256, 512, 1024, 4096, 8192, 12288)             # EPT = 4 / 8 register runs, a wave, thread blocks, the 4096-chunks of rank_big


def break_vector(K, m_elite, p, over, rng):
    """A cost vector whose sorted form has every adjacent gap <= 2^-9 except the pair (p, p+1); that gap is the largest double below 10e-3 as the
    subtraction computes it (over = False) or the smallest one not below it (over = True).  Returned shuffled.  With p + 1 < m_elite the pair alone
    decides the break; with p = m_elite - 1 it lies just outside the elite set and must not matter."""
    assert 0 <= p < K - 1
    gaps = rng.integers(0, 3, K - 1) * 2.0 ** -10                           # 0, 2^-10, 2^-9: exact ties included
    s = np.empty(K)
    s[0] = 1.0
    s[1:p + 1] = 1.0 + np.cumsum(gaps[:p])                                  # multiples of 2^-10: these differences are exact
    hi = s[p] + BREAK_THRESHOLD
    while not (hi - s[p] < BREAK_THRESHOLD):
        hi = np.nextafter(hi, -np.inf)
    if over:
        while hi - s[p] < BREAK_THRESHOLD:
            hi = np.nextafter(hi, np.inf)
    s[p + 1] = hi
    if p + 2 < K:                                                           # the tail restarts on the grid, one to two steps above hi
        s[p + 2:] = np.ceil(hi * 1024 + 1) / 1024 + np.concatenate([[0.0], np.cumsum(gaps[p + 2:])])
    perm = rng.permutation(K)
    c = np.empty(K)
    c[perm] = s
    return c


def nonfinite_vectors(K, rng):
    """name -> cost vector with non-finite entries (K >= 16)"""
    v = {}
    e = np.full(K, 1.0); e[K // 3] = np.inf; v["one_inf_equal_base"] = e
    r = rng.standard_normal(K) * 5.0; r[[1, K // 2, K // 2 + 1, K - 2, K - 1]] = np.inf; v["several_inf"] = r
    e = np.full(K, 1.0); e[(2 * K) // 3] = np.nan; v["one_nan_equal_base"] = e
    r = rng.standard_normal(K) * 5.0; r[[0, 5, K // 2, K - 3, K - 1]] = np.nan; v["few_nan"] = r
    v["all_nan"] = np.full(K, np.nan)
    e = np.full(K, 1.0); e[[2, K // 2, K - 1]] = np.nan; e[[3, K // 4, K - 2]] = np.inf; v["mixed_equal_base"] = e
    return v


# ---- alias table -------------------------------------------------------------------------------------------------------------------------
def alias_table_traced(w, wsum=1.0):
    """StatsBase.make_alias_table!(w, wsum, a, alias), transcribed literally (0-based), plus what the loop went through:
    n_large / n_small (after classification), dry (the loop ended because the smalls ran out while a large stayed > 1), leftover_smalls (original smalls
    never paired: the larges ran out), pending_chain (longest run of consecutive iterations whose small was the large exhausted just before), ties
    (updates that landed exactly on 1.0; ties_inner: those of any large but the one popped last) and eq_one (entries classified as neither)."""
    n = len(w)
    ac = n / wsum
    a = [float(x) * ac for x in w]
    alias = list(range(n))
    larges, smalls = [], []
    for i in range(n):
        if a[i] > 1.0:
            larges.append(i)
        elif a[i] < 1.0:
            smalls.append(i)
    info = {"n_large": len(larges), "n_small": len(smalls), "eq_one": n - len(larges) - len(smalls), "ties": 0, "ties_inner": 0, "pending_chain": 0}
    last_large = larges[0] if larges else -1                                # popped last; the parallel construction exempts its final tie
    was_large = set()
    chain = 0
    while larges and smalls:
        s = smalls.pop()
        l = larges.pop()
        chain = chain + 1 if s in was_large else 0
        info["pending_chain"] = max(info["pending_chain"], chain)
        alias[s] = l
        a[l] = (a[l] - 1.0) + a[s]
        if a[l] == 1.0:
            info["ties"] += 1
            info["ties_inner"] += l != last_large
        if a[l] > 1.0:
            larges.append(l)
        else:
            smalls.append(l); was_large.add(l)
    info["dry"] = bool(larges)
    info["leftover_smalls"] = sum(1 for s in smalls if s not in was_large)
    for s in smalls:
        a[s] = 1.0
    return np.array(a), np.array(alias, dtype=np.int32), info


def alias_weight_vectors(K, rng, oracle):
    """name -> weight vector of length K (sums to 1 up to rounding).  Kinds that need more room than K gives are left out."""
    v = {}
    v["softmax20_a"] = oracle.compute_weights(20.0, rng.standard_normal(K) * 30.0 + 100.0)
    v["softmax20_b"] = oracle.compute_weights(20.0, rng.random(K) * 200.0)
    r = rng.random(K) + 0.05; v["random_normalised"] = r / r.sum()
    v["uniform"] = np.full(K, 1.0 / K)
    for name, i in (("onehot_first", 0), ("onehot_mid", K // 2), ("onehot_last", K - 1)):
        o = np.zeros(K); o[i] = 1.0; v[name] = o
    if K >= 8:                                                              # collapsed softmax: exact zeros, a few denormals, one entry carrying the mass
        c = np.zeros(K); c[K // 3] = 1.0; c[[1, K // 2, K - 1]] = [5e-324, 3e-320, 1e-310]; v["collapsed"] = c
    h = K // 2
    blk = np.full(K, 1.0 / K); blk[:h] = 1.5 / K; blk[K - h:] = 0.5 / K; v["half_blocked"] = blk
    il = np.full(K, 1.0 / K); il[0:2 * h:2] = 1.5 / K; il[1:2 * h:2] = 0.5 / K; v["half_interleaved"] = il
    if K >= 8:                                                              # 1.5 / 0.5 pairs that cancel exactly (at a power-of-two K) and one small just
        g = (K - 1) // 2                                                    # below 1 at index 0, popped last: the larges run out first and it is left over
        lo = np.full(K, 1.0 / K); lo[0] = (1.0 - 2.0 ** -30) / K; lo[1:1 + g] = 1.5 / K; lo[1 + g:1 + 2 * g] = 0.5 / K; v["leftover_small"] = lo
    if K >= 3:
        d = 0.5 / K
        sl = np.full(K, (1.0 + d) / K); sl[0] = (1.0 - (K - 1) * d) / K; v["slight_larges"] = sl          # K-1 larges just above 1, one small: a chain of
        ss = np.full(K, (1.0 - d) / K); ss[K - 1] = (1.0 + (K - 1) * d) / K; v["slight_smalls"] = ss      # exhausted larges / one large absorbing everything
    for nl in (64, 65, 128):
        if K >= 4 * nl:
            x = np.full(K, (1.0 - nl / (K - nl)) / K); x[rng.permutation(K)[:nl]] = 2.0 / K; v["larges_%d" % nl] = x
    for ns in (64, 65):
        if K >= 2 * ns:
            x = np.full(K, (1.0 + 0.5 * ns / (K - ns)) / K); x[rng.permutation(K)[:ns]] = 0.5 / K; v["smalls_%d" % ns] = x
    return v


GENERIC_ALIAS_KINDS = ("softmax20_a", "softmax20_b", "random_normalised")


def alias_par_bound(K):
    """|accept - oracle| allowed on the entries the parallel construction takes from its scans (scaled weight > 1): at most 2K additions of
    magnitude at most K, each rounded to 2^-53 relative: 4 K^2 2^-52 with the factor of two of the analysis in kernels_select.hip"""
    return 4.0 * K * K * 2.0 ** -52


# ---- weights -----------------------------------------------------------------------------------------------------------------------------
def weights_ref(cost, lam):
    """compute_weights (utils.jl:79-86) in np.longdouble -> (w_ref, x) with x_k = -(c_k - min c) / lam"""
    c = np.asarray(cost, dtype=np.longdouble)
    x = -(c - c.min()) / np.longdouble(lam)
    e = np.exp(x)
    return e / e.sum(), x


def weights_tol(cost, lam):
    """per-weight tolerance 4 2^-52 (|x_k| + log2 K + 4) w_ref -- rounding of the exponent's argument, summation depth, a 1-ulp exp -- with the
    smallest subnormal as the absolute floor"""
    w, x = weights_ref(cost, lam)
    K = len(w)
    return np.maximum(4 * np.longdouble(2.0) ** -52 * (np.abs(x) + np.log2(K) + 4) * w, np.longdouble(2.0) ** -1074), w


def weight_cost_cases(K, rng):
    """name -> (lambda, [two different cost vectors])"""
    two = lambda f: [f(), f()]
    return {
        "generic": (10.0, two(lambda: rng.standard_normal(K) * 50.0 + 300.0)),
        "equal": (1.0, [np.full(K, 41.5), np.full(K, -3.0)]),
        "underflow": (1e-6, two(lambda: 10.0 + rng.random(K))),                       # x down to -1e6: most weights underflow, a few land among the subnormals
        "huge_lambda": (1e12, two(lambda: rng.standard_normal(K) * 50.0 + 300.0)),
        "lane_penalty": (10.0, two(lambda: 1e6 + rng.random(K) * 40.0)),
    }
