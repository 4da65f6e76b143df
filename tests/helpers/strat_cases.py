"""Inputs, file format, restatements and bounds for the antithetic and Latin-hypercube draws (mpopis_amd/csrc/strat.h, kernels_strat.hip,
tools/kbench_strat.hip): shared by tests/test_strat_cases_cpu.py, tests/test_gpu_strat_harness.py and tests/test_gpu_noise_kinds.py.  Nothing
here touches the engine.

Integer part (bit for bit): round keys, jitter word, the Feistel permutation with cycle walking.  Floating-point part: phi_inv_f64 restates
strat_phi_inv operation by operation (fma where the device has one; 1 / sqrt in double stands in for the v_rsq_f64 seed), phi_inv_mp is the
definition at 40 digits, phi_inv_bound the absolute bound on |device - definition|.

The bound is derived, not tuned; every term is a step strat.h documents.  With u = 2^-53, z the result and phi its density:
  p:       the numerator j 2^33 + xi 2^33 is an integer below 2^53 (exact), the division by K rounds once: u p, through dz/dp = 1/phi(z).
           p/phi(z) <= sqrt(pi/2) for p <= 1/2 and falls like 1/|z|: this is what the small-side evaluation buys -- evaluated from the far
           side the same rounding of 1 - p would cost u / phi(z), unbounded in the tail.
  centre (p > exp(-2)):  y = p - 1/2 rounds to u |y| (exact for p >= 1/4); y2 = y y rounds once; P0, Q0: Horner with fma, each step's result s_i
           rounds to u |s_i| and is multiplied by y2 from there on (running error), plus the polynomial's slope times the error of y2; the
           product y2 P0, the quotient, the final fma and the product with sqrt(2 pi) (constant within u) round once each.
  tail:    L = log_unit(p) (philox.h) with the terms bm_bound of sample_cases.py lists -- table entries within 1 ulp, r = fma(m, inv, -1),
           remainder r^6 / 6, Horner roundings, k ln2 with the constant 2.4e-17 off, two roundings of the sum --; v = -2 L exact;
           t = strat_sqrt(v): dv / (2 sqrt(v - dv)) + 1 ulp; log_unit(t) likewise, plus dt / t; the quotient log(t) / t, t0 = t - ., 1 / t,
           P, Q (running error, slope times the error of 1 / t), product, quotient and the final difference round once each.
  approximation: the rational functions are not the function.  TRUNC[region] is the largest |formula in exact arithmetic - Phi^-1| found at 40
           digits on 4000 points per region over the range a K <= 2^20 can reach (p >= 2^-53), doubled: 1.76e-16 / 7.2e-18 / 7.7e-18 measured
           (centre / 2 <= t < 8 / t >= 8; tests/test_strat_cases_cpu.py repeats the measurement on a coarser grid).
No device-library function is involved, so no term rests on an unmeasured accuracy figure."""
import numpy as np
from tests.helpers.harness_io import F64, I32, U64, GUARD, U, is_poison, pack_case as _pack_case, unpack_result as _unpack_result, ulp_of
from tests.helpers.sample_cases import TAB_LOG, fma, lin_map, philox_np, table_f64

PHILOX, ANTITHETIC, LHS = 0, 1, 2                          # MPOPIS_NOISE_* of include/mpopis.h
KIND_IDS = {"philox": PHILOX, "antithetic": ANTITHETIC, "lhs": LHS}
TAG_KEYS, TAG_JITTER = 0x10000000, 0x20000000               # kStratTagKeys, kStratTagJitter of strat.h
MAX_K = 1 << 20
OP_PERM, OP_JITTER, OP_PHIINV, OP_GEN = range(4)
MAGIC_IN, MAGIC_OUT = b"STRCASE1", b"STRRES01"
M32 = np.uint64(0xffffffff)


# ---- the harness's files (tools/kbench_strat.hip) ---------------------------------------------------------------------------------------------
def case_rows(op, B, cs, K, seeds, active, step, it):
    """PERM / JITTER over every (slot, row, sample)"""
    return _pack_case(MAGIC_IN, op, B, [cs, K, step, it], [], [(I32, np.asarray(active, dtype=np.int32)), (U64, np.asarray(seeds, dtype=np.uint64))])


def case_phi_inv(j, x, K):
    j, x = np.asarray(j, dtype=np.uint32), np.asarray(x, dtype=np.uint32)
    return _pack_case(MAGIC_IN, OP_PHIINV, 1, [K, j.size], [], [(I32, np.ones(1, dtype=np.int32)), (I32, j.view(np.int32)), (I32, x.view(np.int32))])


def case_gen(B, cs, K, as_, mppi, kind, seeds, active, step, it, no_active=False):
    return _pack_case(MAGIC_IN, OP_GEN, B, [cs, K, as_, mppi, kind, step, it, 0 if no_active else 1], [],
                      [(I32, np.asarray(active, dtype=np.int32)), (U64, np.asarray(seeds, dtype=np.uint64))])


def unpack_result(buf):
    """-> (body, guard) of the launch's one output array"""
    _, arrays = _unpack_result(MAGIC_OUT, buf)
    assert len(arrays) == 1
    return arrays[0][:-GUARD], arrays[0][-GUARD:]


# ---- integer part ----------------------------------------------------------------------------------------------------------------------------
def half_bits(K):
    """strat_half_bits: half the width of the Feistel domain (the bits of K - 1, rounded up to an even count, halved; at least 1)"""
    nb = int(K - 1).bit_length()
    return 1 if nb < 1 else (nb + 1) // 2


def _philox_rows(c0, c1, step, tag_iter, seed):
    c0 = np.asarray(c0, dtype=np.uint64).reshape(-1)
    s = np.empty((c0.size, 6), dtype=np.uint64)
    s[:, 0], s[:, 1], s[:, 2], s[:, 3] = c0, c1, step, tag_iter
    s[:, 4], s[:, 5] = int(seed) & 0xffffffff, int(seed) >> 32
    return philox_np(s)


def round_keys(seed, step, it, r):
    """[rows, 4] uint32: the Philox call (r, 0, step, TAG_KEYS | it) under the slot's seed"""
    return _philox_rows(r, 0, step, TAG_KEYS | it, seed)


def jitter_words(seed, step, it, r, K):
    """[K] uint32 of row r: word 0 of the Philox call (k, r, step, TAG_JITTER | it)"""
    return _philox_rows(np.arange(K), r, step, TAG_JITTER | it, seed)[:, 0].copy()


def _round(x, key, half):
    t = ((x ^ key) * np.uint64(0x9E3779B1)) & M32
    t ^= t >> np.uint64(15)
    t = (t * np.uint64(0x85EBCA6B)) & M32
    t ^= t >> np.uint64(13)
    return t >> np.uint64(32 - half)


def perm(K, keys):
    """pi(k) for k = 0 .. K - 1 under one row's four round keys -> [K] int64; also returns the largest number of walks any k needed"""
    if K == 1:
        return np.zeros(1, dtype=np.int64), 0
    half = half_bits(K)
    mask, dom = np.uint64((1 << half) - 1), 1 << (2 * half)
    key = [np.uint64(int(v)) for v in keys]
    y = np.arange(K, dtype=np.uint64)
    todo = np.ones(K, dtype=bool)
    walks = 0
    while todo.any():
        walks += 1
        assert walks <= dom
        v = y[todo]
        L, R = v >> np.uint64(half), v & mask
        for i in range(4):
            L, R = R, L ^ _round(R, key[i], half)
        v = (L << np.uint64(half)) | R
        y[todo] = v
        todo[todo] = v >= np.uint64(K)
    return y.astype(np.int64), walks


def perm_rows(seed, step, it, cs, K):
    """[cs, K] strata of a slot"""
    keys = round_keys(seed, step, it, np.arange(cs))
    return np.stack([perm(K, keys[r])[0] for r in range(cs)])


def jitter_rows(seed, step, it, cs, K):
    return np.stack([jitter_words(seed, step, it, r, K) for r in range(cs)])


def xi_of(x):
    """(x + 0.5) 2^-32, exact in double"""
    return (np.asarray(x, dtype=np.float64) + 0.5) * 2.0 ** -32


# ---- floating-point part ---------------------------------------------------------------------------------------------------------------------
P0 = (-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1, 1.39312609387279679503E1, -1.23916583867381258016E0)
Q0 = (1.00000000000000000000E0, 1.95448858338141759834E0, 4.67627912898881538453E0, 8.63602421390890590575E1, -2.25462687854119370527E2,
      2.00260212380060660359E2, -8.20372256168333339912E1, 1.59056225126211695515E1, -1.18331621121330003142E0)
P1 = (4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1, 4.40805073893200834700E1, 1.46849561928858024014E1,
      2.18663306850790267539E0, -1.40256079171354495875E-1, -3.50424626827848203418E-2, -8.57456785154685413611E-4)
Q1 = (1.00000000000000000000E0, 1.57799883256466749731E1, 4.53907635128879210584E1, 4.13172038254672030440E1, 1.50425385692907503408E1,
      2.50464946208309415979E0, -1.42182922854787788574E-1, -3.80806407691578277194E-2, -9.33259480895457427372E-4)
P2 = (3.23774891776946035970E0, 6.91522889068984211695E0, 3.93881025292474443415E0, 1.33303460815807542389E0, 2.01485389549179081538E-1,
      1.23716634817820021358E-2, 3.01581553508235416007E-4, 2.65806974686737550832E-6, 6.23974539184983293730E-9)
Q2 = (1.00000000000000000000E0, 6.02427039364742014255E0, 3.67983563856160859403E0, 1.37702099489081330271E0, 2.16236993594496635890E-1,
      1.34204006088543189037E-2, 3.28014464682127739104E-4, 2.89247864745380683936E-6, 6.79019408009981274425E-9)
EXP_M2 = 0.13533528323661269189
S2PI = 2.50662827463100050242E0
_LN2 = 6.93147180559945286227e-01
TRUNC = {"centre": 2 * 1.76e-16, "tail1": 2 * 7.2e-18, "tail2": 2 * 7.7e-18}      # see the module docstring


def _small_side(j, xi, K):
    """-> (flip, j, xi) of the mirrored input: strata of the upper half (and the upper half of an odd K's middle stratum) go to K - 1 - j, 1 - xi"""
    j, xi = np.broadcast_arrays(np.asarray(j, dtype=np.int64), np.asarray(xi, dtype=np.float64))
    flip = (2 * j + 1 > K) | ((2 * j + 1 == K) & (xi > 0.5))
    return flip, np.where(flip, K - 1 - j, j), np.where(flip, 1.0 - xi, xi)


def _p_of(j, xi, K):
    num = j.astype(np.float64) * 2.0 ** 33 + xi * 2.0 ** 33               # an integer below 2^53: exact
    assert np.all(num == np.floor(num)) and np.all(num < 2.0 ** 53)
    return (num * 2.0 ** -33) / float(K)


def _log_unit(u, tab):
    """log_unit of philox.h in float64"""
    m, k = np.frexp(u)
    i = ((m.view(np.int64) >> 44) & (TAB_LOG - 1)).astype(np.int64)
    inv, logc = tab[2 * i], tab[2 * i + 1]
    r = fma(m, inv, -1.0)
    p = fma(r, 1.0 / 5.0, -1.0 / 4.0)
    p = fma(p, r, 1.0 / 3.0)
    p = fma(p, r, -0.5)
    lp = fma(p * r, r, r)
    return fma(k.astype(np.float64), _LN2, logc) + lp


def _sqrt(v):
    y = 1.0 / np.sqrt(v)
    g, h = v * y, 0.5 * y
    rr = fma(-h, g, 0.5)
    g, h = fma(g, rr, g), fma(h, rr, h)
    return fma(fma(-g, g, v), h, g)


def _horner(x, c):
    """-> (value, running bound on its rounding error, bound on |slope|)"""
    s, e, d = np.full_like(x, c[0]), np.zeros_like(x), np.zeros_like(x)
    ax = np.abs(x)
    for ci in c[1:]:
        d = d * ax + np.abs(s)
        s = fma(s, x, ci)
        e = e * ax + U * np.abs(s)
    return s, e, d


def _ratio(x, dx, P, Q):
    """x P(x) / Q(x) as the device forms it -> (value, bound on its error given |error of x| <= dx)"""
    p, ep, sp = _horner(x, P)
    q, eq, sq = _horner(x, Q)
    ep, eq = ep + sp * dx, eq + sq * dx
    n = x * p
    en = U * np.abs(n) + np.abs(p) * dx + np.abs(x) * ep
    val = n / q
    aq = np.abs(q) - eq
    return val, U * np.abs(val) + en / aq + np.abs(val) * eq / aq


def phi_inv_f64(j, xi, K, tab=None):
    """strat_phi_inv restated in float64 for stratum j and jitter xi (a multiple of 2^-33 in (0, 1); the device's are xi_of(x))"""
    tab = table_f64() if tab is None else tab
    flip, js, xs = _small_side(j, xi, K)
    p = _p_of(js, xs, K)
    centre = p > EXP_M2
    y = p - 0.5
    y2 = y * y
    q = (y2 * _horner(y2, P0)[0]) / _horner(y2, Q0)[0]
    mag_c = -(fma(y, q, y) * S2PI)
    pt = np.where(centre, 0.01, p)                                       # (keeps the unused branch in range)
    t = _sqrt(-2.0 * _log_unit(pt, tab))
    t0 = t - _log_unit(t, tab) / t
    z = 1.0 / t
    t1 = np.where(t < 8.0, (z * _horner(z, P1)[0]) / _horner(z, Q1)[0], (z * _horner(z, P2)[0]) / _horner(z, Q2)[0])
    mag = np.where(centre, mag_c, t0 - t1)
    return np.where(flip, mag, -mag)


def _log_unit_bound(u, du, tab):
    """absolute bound on |log_unit(u^) - log u| for |u^ - u| <= du (the terms of sample_cases.bm_bound's dL, for any positive normal u)"""
    m, k = np.frexp(u)
    i = ((m.view(np.int64) >> 44) & (TAB_LOG - 1)).astype(np.int64)
    inv, logc = tab[2 * i], tab[2 * i + 1]
    top = i == TAB_LOG - 1
    d_inv, d_logc = np.where(top, 0.0, ulp_of(inv)), np.where(top, 0.0, ulp_of(logc))
    r = m * inv - 1.0
    ar = np.abs(r) + d_inv
    lp, L = np.abs(np.log1p(r)), np.abs(np.log(u))
    dL = (m * d_inv + U * ar) / (1 - ar) + d_logc + ar ** 6 / (6 * (1 - ar)) + 2 * U * ar ** 2 + U * lp
    dL = dL + np.abs(k) * 2.4e-17 + U * np.abs(k * _LN2 + logc) + U * L
    return dL + du / (u - du)


def phi_inv_bound(j, xi, K):
    """absolute bound on |strat_phi_inv - Phi^-1((j + xi) / K)|; the derivation is in the module's docstring"""
    tab = table_f64()
    _, js, xs = _small_side(j, xi, K)
    p = _p_of(js, xs, K)
    zabs = np.abs(phi_inv_f64(js, xs, K, tab))
    d_p = 1.01 * U * p * np.sqrt(2 * np.pi) * np.exp(0.5 * zabs * zabs)                 # u p / phi(z)
    centre = p > EXP_M2
    # centre
    y = p - 0.5
    ey = np.where(p >= 0.25, 0.0, U * np.abs(y))
    y2 = y * y
    ey2 = U * y2 + 2 * np.abs(y) * ey
    pv, ep, sp = _horner(y2, P0)
    qv, eq, sq = _horner(y2, Q0)
    ep, eq = ep + sp * ey2, eq + sq * ey2
    n = y2 * pv
    en = U * np.abs(n) + np.abs(pv) * ey2 + y2 * ep
    q = n / qv
    aq = np.abs(qv) - eq
    e_q = U * np.abs(q) + en / aq + np.abs(q) * eq / aq
    w = np.abs(y) * (1 + np.abs(q))
    ew = U * w + ey * (1 + np.abs(q)) + np.abs(y) * e_q
    b_c = 2 * U * w * S2PI + S2PI * ew + TRUNC["centre"]
    # tail
    pt = np.where(centre, 0.01, p)
    L = np.abs(np.log(pt))
    dv = 2 * _log_unit_bound(pt, 0.0, tab)
    v = 2 * L
    t = np.sqrt(v)
    dt = dv / (2 * np.sqrt(v - dv)) + ulp_of(t)
    lt = np.log(t)
    dlt = _log_unit_bound(t, dt, tab)
    d = lt / t
    dd = 1.0001 * (U * d + dlt / t + d * dt / t)
    t0 = t - d
    dt0 = U * t0 + dt + dd
    z = 1.0 / t
    dz = 1.0001 * (U * z + dt / (t * t))
    t1a, e1a = _ratio(z, dz, P1, Q1)
    t1b, e1b = _ratio(z, dz, P2, Q2)
    near8 = np.abs(t - 8.0) <= dt                                        # either pair may be taken there
    lo = t < 8.0
    e1 = np.where(near8, np.maximum(e1a, e1b), np.where(lo, e1a, e1b))
    tr = np.where(near8, max(TRUNC["tail1"], TRUNC["tail2"]), np.where(lo, TRUNC["tail1"], TRUNC["tail2"]))
    b_t = U * np.abs(t0 - np.where(lo, t1a, t1b)) + dt0 + e1 + tr
    return d_p + np.where(centre, b_c, b_t)


def phi_inv_mp(j, xi, K, digits=40):
    """Phi^-1((j + xi) / K) at `digits` digits -> list of mpmath.mpf.  Newton on log Phi from the float64 restatement; the last step is checked to
    be below 10^-30, so the value does not depend on where the iteration started."""
    import mpmath as mp
    flip, js, xs = _small_side(j, xi, K)
    z0 = -np.abs(np.atleast_1d(phi_inv_f64(js, xs, K)))
    flip, js, xs = np.atleast_1d(flip), np.atleast_1d(js), np.atleast_1d(xs)
    out = []
    with mp.workdps(digits):
        for f, a, b, g in zip(flip.ravel(), js.ravel(), xs.ravel(), z0.ravel()):
            p = (mp.mpf(int(a)) + mp.mpf(float(b))) / K
            lp = mp.log(p)
            z = mp.mpf(float(g))
            for _ in range(6):
                c = mp.ncdf(z)
                dz = (mp.log(c) - lp) * c / mp.npdf(z)
                z -= dz
                if abs(dz) < mp.mpf(10) ** -30:
                    break
            assert abs(dz) < mp.mpf(10) ** -30, (a, b, K, dz)
            out.append(-z if f else z)
    return out


def mp_err(got, ref_mp):
    """|got - ref| per element as float64 (the difference is formed at the reference's precision)"""
    import mpmath as mp
    with mp.workdps(40):
        return np.array([float(abs(mp.mpf(float(g)) - r)) for g, r in zip(np.asarray(got, dtype=np.float64).ravel(), ref_mp)])


def formula_mp(p, region):
    """the documented formula of one region in exact arithmetic (40 digits) at p -> mpf: what TRUNC measures against Phi^-1"""
    import mpmath as mp
    hor = lambda x, c: sum(mp.mpf(ci) * x ** (len(c) - 1 - i) for i, ci in enumerate(c))
    if region == "centre":
        y = p - mp.mpf(0.5)
        return (y + y * (y * y * hor(y * y, P0) / hor(y * y, Q0))) * mp.mpf(S2PI)
    t = mp.sqrt(-2 * mp.log(p))
    P, Q = (P1, Q1) if region == "tail1" else (P2, Q2)
    return -(t - mp.log(t) / t - (1 / t) * hor(1 / t, P) / hor(1 / t, Q))


def trunc_points(region, n):
    """n values of p spread over a region (uniform in p in the centre, uniform in t = sqrt(-2 log p) in the tails down to p = 2^-53) -> mpf list"""
    import mpmath as mp
    if region == "centre":
        return [mp.mpf(EXP_M2) + (mp.mpf(0.5) - mp.mpf(EXP_M2)) * (i + mp.mpf(0.5)) / n for i in range(n)]
    a, b = (mp.mpf(2), mp.mpf(8)) if region == "tail1" else (mp.mpf(8), mp.sqrt(2 * 53 * mp.log(2)))
    return [mp.exp(-(a + (b - a) * (i + mp.mpf(0.5)) / n) ** 2 / 2) for i in range(n)]


def truth_mp(p):
    """Phi^-1(p) for an mpf p in (0, 1/2]: Newton on log Phi from the asymptotic start"""
    import mpmath as mp
    z = -mp.sqrt(-2 * mp.log(p)) if p < mp.mpf("0.4") else mp.mpf(S2PI) * (p - mp.mpf(0.5))
    lp = mp.log(p)
    for _ in range(60):
        c = mp.ncdf(z)
        dz = (mp.log(c) - lp) * c / mp.npdf(z)
        z -= dz
        if abs(dz) < mp.mpf(10) ** -32:
            return z
    raise AssertionError("no convergence at p = %s" % p)


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------
def antithetic_source(cs, K, as_, mppi):
    """(k0 [K], sign [K], lin [cs, K]): column k is sign[k] times the Philox kind's normal number lin[r, k0[k]]"""
    h = (K + 1) // 2
    k = np.arange(K)
    return np.where(k < h, k, k - h), np.where(k < h, 1.0, -1.0), lin_map(cs, K, as_, mppi)


def lhs_inputs(seeds, active, step, it, cs, K):
    """(j, x) [B, cs, K] of the Latin-hypercube draw (inactive slots included: the caller masks them)"""
    j = np.stack([perm_rows(s, step, it, cs, K) for s in seeds])
    x = np.stack([jitter_rows(s, step, it, cs, K) for s in seeds])
    return j, x


GEN_SEEDS = (20240001, (1 << 32) + 77, 0xfedcba9876543210)              # distinct, two of them >= 2^32
GEN_ACTIVE = (1, 0, 1)                                                   # one inactive slot in the middle
GEN_STREAM = (11, 2)                                                     # (MPC step, AIS iteration)


def gen_shapes():
    """(mppi, cs, K, as) of the issue's table: cs in {1, 2, 5}, K in {1, 2, 3, 5, 64, 65, 257}, both orders, as = 1 and 2 (as | cs)"""
    out = []
    for cs in (1, 2, 5):
        for K in (1, 2, 3, 5, 64, 65, 257):
            for as_ in (1, 2):
                if cs % as_ == 0:
                    out += [(0, cs, K, as_), (1, cs, K, as_)]
    return out
