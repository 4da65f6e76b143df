"""Inputs, file format, references and bounds for the direct tests of the Philox sampling kernels and the step's read-out tail
(tools/kbench_sample.hip): shared by tests/test_sample_cases_cpu.py (which proves helpers, references and the bound on the CPU) and
tests/test_gpu_sample_harness.py.  Nothing here touches the engine; references are NumPy (np.longdouble where arithmetic is involved) and the oracle.

The Box-Muller bound (bm_bound) is derived, not tuned; every term is one that mpopis_amd/csrc/philox.h documents.  With u = 2^-53:
  log:   r = fma(m, inv, -1) carries the table's error in 1/c (<= 1 ulp of the entry, times m < 1) and one rounding (u |r|), both through
         d log1p / dr = 1 / (1 + r); log c carries <= 1 ulp of the entry; the polynomial stops before r^6 / 6 (remainder <= |r|^6 / (6 (1 - |r|)));
         its Horner steps round to <= 2 u r^2 in all (they are multiplied by r^2) and its last fma to u |log1p r|; k ln2 + log c: the constant is
         within 2^-54 of ln 2, the fma rounds to u |k ln2 + log c|, the final sum to u |log u1|.
         In the top interval (k = 0, c = 1: table entry exactly (1, 0)) r = m - 1, the fma gives 0 and 0 + log1p r are all exact: what is left is
         the remainder and the polynomial's own rounding, relative to |log u1| -- nothing blows up at u1 -> 1.
  sqrt:  v = -2 log u1 is exact; R = sqrt(v): dR <= dv / (2 sqrt(v - dv)) + 1 ulp(R).
  angle: x = f (2 pi / 128) with f exact: the constant and the product round (2 u |x|); sin: remainder x^7 / 5040, last fma u |x|, the
         error of x itself, and the inner terms' rounding (<= 2 u |x|^3); cos: remainder x^8 / 40320, last fma u, z = x x and the inner steps 5 u x^2.
  rotation by the sector centre: each table entry <= 1 ulp; one product and one fma round.
  z = R t: |dz| <= dR (|t| + dt) + R dt + u |z|, plus 2^-59 R for the long double reference itself (2 pi u2 rounded at 2^-63 relative)."""
import os
import re
import struct
from fractions import Fraction
import numpy as np
from tests.helpers.harness_io import GUARD, LD, U, bits, is_poison, ulp_of      # (re-exported: the tests read them under this module's name)

OP_TAB, OP_WORDS, OP_BOXMULLER, OP_NORMALQ, OP_NORMALS, OP_DRAWS, OP_FINALIZE, OP_T_IN, OP_T_OUT = range(9)
MAGIC_IN, MAGIC_OUT = b"SMPCASE1", b"SMPRES01"
MAX_AS = 16                                                # kMaxAs of engine.h
POISON_I32 = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]
POISON_U32 = np.frombuffer(b"\xa5" * 4, dtype=np.uint32)[0]
POISON_F64_BITS = np.frombuffer(b"\xa5" * 8, dtype=np.uint64)[0]
SINGLE, PAIR, QUAD = 0, 1, 2                               # enum SampleNormalForm of engine.h
RNG_TOL = 1e-13                                            # tests/test_gpu_parity.py::test_device_rng_normals_full_size: the outer contract
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def table_sizes():
    """(kRngTabLog, kRngTabSc, kRngTabDoubles) read back from philox.h"""
    with open(os.path.join(ROOT, "mpopis_amd", "csrc", "philox.h")) as f:
        m = re.search(r"constexpr int kRngTabLog = (\d+), kRngTabSc = (\d+), kRngTabDoubles = 2 \* \(kRngTabLog \+ kRngTabSc\);", f.read())
    n_log, n_sc = int(m.group(1)), int(m.group(2))
    return n_log, n_sc, 2 * (n_log + n_sc)


TAB_LOG, TAB_SC, TAB_DOUBLES = 256, 128, 768               # what the directed sets and the restatement are written for; the CPU test holds them to philox.h


# ---- the harness's files ---------------------------------------------------------------------------------------------------------------
def pack_case(op, B=1, cs=1, K=1, as_=1, T=1, mppi=0, flags=0, n=0, slo=0, shi=0, src_stride=0, src_off=0, arrays=()):
    """arrays: the op's payload in file order, already of the right dtype"""
    out = [MAGIC_IN, struct.pack("<15q", op, B, cs, K, as_, T, mppi, flags, n, slo, shi, src_stride, src_off, 0, 0)]
    out += [np.ascontiguousarray(a).tobytes() for a in arrays]
    return b"".join(out)


def case_words(sets):
    sets = np.ascontiguousarray(sets, dtype=np.uint32).reshape(-1, 6)
    return pack_case(OP_WORDS, n=len(sets), arrays=[sets])


def case_box_muller(wr, wa, from_global=False):
    w = np.stack([np.asarray(wr, dtype=np.uint32), np.asarray(wa, dtype=np.uint32)], axis=1)
    return pack_case(OP_BOXMULLER, n=len(w), flags=1 if from_global else 0, arrays=[w])


def case_normalq(entries):
    """entries: (seed, slo, shi, q)"""
    a = np.array([[s, lo | (hi << 32), q] for s, lo, hi, q in entries], dtype=np.uint64)
    return pack_case(OP_NORMALQ, n=len(a), arrays=[a])


def case_normals(B, cs, K, as_, T, mppi, seeds, slo, shi, active, dscale=None, no_active=False):
    arr = [np.asarray(seeds, dtype=np.uint64), np.asarray(active, dtype=np.int32)]
    assert arr[0].shape == (B,) and arr[1].shape == (B,)
    if dscale is not None:
        arr.append(_arr(dscale, np.float64, B * cs))
    return pack_case(OP_NORMALS, B, cs, K, as_, T, mppi, (1 if dscale is not None else 0) | (2 if no_active else 0), 0, slo, shi, arrays=arr)


def case_draws(B, K, seeds, slo, shi, active, no_active=False):
    return pack_case(OP_DRAWS, B, 1, K, flags=2 if no_active else 0, slo=slo, shi=shi, arrays=[_arr(seeds, np.uint64, B), _arr(active, np.int32, B)])


def case_finalize(B, as_, T, lo, hi, Uin, wn):
    cs = as_ * T
    return pack_case(OP_FINALIZE, B, cs, 1, as_, T, arrays=[_arr(lo, np.float64, MAX_AS), _arr(hi, np.float64, MAX_AS), _arr(Uin, np.float64, B * cs), _arr(wn, np.float64, B * cs)])


def case_transpose_in(B, cs, K, src, src_stride=0, src_off=0):
    src = np.ascontiguousarray(src, dtype=np.float64).reshape(-1)
    return pack_case(OP_T_IN, B, cs, K, n=src.size, src_stride=src_stride, src_off=src_off, arrays=[src])


def case_transpose_out(B, cs, K, src, shiftA=None, shiftB=None):
    arr = [_arr(src, np.float64, B * cs * K)]
    if shiftA is not None:
        arr += [_arr(shiftA, np.float64, B * cs), _arr(shiftB, np.float64, B * cs)]
    return pack_case(OP_T_OUT, B, cs, K, flags=1 if shiftA is not None else 0, arrays=arr)


def _arr(x, dt, n):
    x = np.ascontiguousarray(x, dtype=dt).reshape(-1)
    assert x.size == n, (x.size, n)
    return x


def unpack_case_header(buf):
    """what the harness parses first -> dict, payload bytes"""
    assert buf[:8] == MAGIC_IN
    names = ("op", "B", "cs", "K", "as", "T", "mppi", "flags", "n", "slo", "shi", "src_stride", "src_off")
    return dict(zip(names, struct.unpack_from("<13q", buf, 8))), buf[128:]


def result_layout(op, B=1, cs=1, K=1, as_=1, n=0):
    """[(name, dtype, entries before the guard)] in file order"""
    if op == OP_TAB:
        return [("tab", np.float64, TAB_DOUBLES)]
    if op == OP_WORDS:
        return [("out", np.uint32, 4 * n)]
    if op == OP_BOXMULLER:
        return [("z", np.float64, 2 * n)]
    if op == OP_NORMALQ:
        return [("z", np.float64, 8 * n)]
    if op == OP_NORMALS:
        return [("Z", np.float64, B * cs * K)]
    if op == OP_DRAWS:
        return [("du", np.float64, B * K), ("di", np.int32, B * K)]
    if op == OP_FINALIZE:
        return [("U", np.float64, B * cs), ("control", np.float64, B * as_), ("wn", np.float64, B * cs)]
    return [("dst", np.float64, B * cs * K)]


def pack_result(form, arrays):
    """what the harness writes (used by the CPU round-trip test); arrays come with their guard entries"""
    return b"".join([MAGIC_OUT, struct.pack("<3q", form, GUARD, 0)] + [np.ascontiguousarray(a).tobytes() for a in arrays])


def unpack_result(buf, op, **shape):
    """-> dict; arrays are flat and keep their guard entries as name + '_guard' (all poison if the launch wrote nothing past the end)"""
    assert buf[:8] == MAGIC_OUT, buf[:8]
    form, guard, _ = struct.unpack_from("<3q", buf, 8)
    assert guard == GUARD
    off = 32
    r = {"form": form}
    for name, dt, cnt in result_layout(op, **shape):
        a = np.frombuffer(buf, dtype=dt, count=cnt + GUARD, offset=off).copy()
        off += a.nbytes
        r[name], r[name + "_guard"] = a[:cnt], a[cnt:]
    assert off == len(buf), (off, len(buf))
    return r


# ---- Philox4x32-10 ------------------------------------------------------------------------------------------------------------------------
KAT = [  # Random123 kat_vectors, philox4x32-10 (tests/test_oracle_kat.py): counter, key, output
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
]


def philox_np(sets):
    """Philox4x32-10 on n x {c0, c1, c2, c3, k0, k1} -> n x 4 words; the rounds restated on uint64 arrays (no Python loop over the sets)"""
    s = np.asarray(sets, dtype=np.uint64).reshape(-1, 6)
    c0, c1, c2, c3, k0, k1 = (s[:, i].copy() for i in range(6))
    M = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & M, n2, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def directed_philox_sets(rng):
    """The KAT inputs, then each of the six input words at 0, 1, 2^31, 2^32 - 1 with the others random (nine draws each: 216 sets)"""
    sets = [c + k for c, k, _ in KAT]
    for pos in range(6):
        for val in (0, 1, 1 << 31, 0xffffffff):
            for _ in range(9):
                s = [int(x) for x in rng.integers(0, 1 << 32, 6)]
                s[pos] = val
                sets.append(s)
    return np.array(sets, dtype=np.uint64).astype(np.uint32)


def stream_call_sets(seed, slo, shi, q):
    """the Philox input of call q (array) of a normal stream: counter = (q lo, q hi, slo, shi), key = seed (philox.h)"""
    q = np.asarray(q, dtype=np.uint64).reshape(-1)
    s = np.empty((q.size, 6), dtype=np.uint64)
    s[:, 0], s[:, 1], s[:, 2], s[:, 3] = q & np.uint64(0xffffffff), q >> np.uint64(32), slo, shi
    s[:, 4], s[:, 5] = seed & 0xffffffff, seed >> 32
    return s


def stream_words(seed, slo, shi, n_normals):
    """(wr, wa) of the Box-Muller pairs behind normals 0 .. n_normals - 1 (rounded up to whole calls): pair p gives normals 2p, 2p + 1"""
    w = philox_np(stream_call_sets(seed, slo, shi, np.arange((n_normals + 3) // 4))).reshape(-1, 2)
    return w[:, 0].copy(), w[:, 1].copy()


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def table_ref():
    """the documented nodes in np.longdouble: [1/c_i, log c_i] x 256 with c_i = (1 + (i + 0.5)/256)/2 (last: c = 1), then [sin, cos](2 pi (j + 0.5)/128) x 128"""
    i = np.arange(TAB_LOG, dtype=LD)
    c = (1 + (i + LD(0.5)) / TAB_LOG) / 2
    c[-1] = 1
    n = 2 * np.arange(TAB_SC, dtype=np.int64) + 1
    t = np.empty(TAB_DOUBLES, dtype=LD)
    t[0:2 * TAB_LOG:2], t[1:2 * TAB_LOG:2] = 1 / c, np.log(c)
    t[2 * TAB_LOG::2], t[2 * TAB_LOG + 1::2] = _sin_pi_over(n, TAB_SC), _sin_pi_over(n + TAB_SC // 2, TAB_SC)
    return t


def _sin_pi_over(n, d):
    """sin(pi n / d) for integers n, 4 | d, in np.longdouble with a small RELATIVE error everywhere: the argument is reduced to the first octant in
    integers, so that nothing is lost next to the axes (sin and cos of an argument <= pi/4 rounded at 2^-63)"""
    n = np.asarray(n, dtype=np.int64) % (2 * d)
    sign = np.where(n >= d, -1, 1)
    n = np.where(n >= d, n - d, n)
    n = np.where(n > d // 2, d - n, n)                                   # 0 .. d/2
    pi = 4 * np.arctan(LD(1))
    return sign * np.where(n <= d // 4, np.sin(pi * n.astype(LD) / d), np.cos(pi * (d // 2 - n).astype(LD) / d))


def table_f64():
    """table_ref rounded to double: the table a correctly rounding host would make (the CPU restatement's table)"""
    return table_ref().astype(np.float64)


# ---- Box-Muller: directed words -------------------------------------------------------------------------------------------------------------
BM_EXPONENTS = (0, -1, -2, -8, -16, -31)


def log_interval(wr):
    """(k, i) of u1 = (wr + 0.5) 2^-32 = m 2^k: the exponent and the table index log_unit takes (top 8 fraction bits of m)"""
    u1 = (np.asarray(wr, dtype=np.float64) + 0.5) * 2.0 ** -32
    m, k = np.frexp(u1)
    return k, ((m.view(np.int64) >> 44) & (TAB_LOG - 1)).astype(np.int64)


def interval_ends(k):
    """{i: (first wr, last wr)} of the table intervals that hold a word at exponent k: (wr + 0.5) 2^(-32-k) in [(256 + i)/512, (257 + i)/512)"""
    out = {}
    e = Fraction(2) ** (23 + k)
    for i in range(TAB_LOG):
        lo, hi = -((-((TAB_LOG + i) * e - Fraction(1, 2))) // 1), -((-((TAB_LOG + 1 + i) * e - Fraction(1, 2))) // 1) - 1       # ceil, ceil - 1
        lo, hi = max(int(lo), 0), min(int(hi), 0xffffffff)
        if lo <= hi:
            out[i] = (lo, hi)
    return out


def directed_wr():
    w = {0, 1, 0xfffffffe, 0xffffffff}
    for k in BM_EXPONENTS:
        for lo, hi in interval_ends(k).values():
            w.update((lo, hi))
    for e in range(33):
        w.update(x for x in ((1 << e) - 1, 1 << e) if 0 <= x <= 0xffffffff)
    return np.array(sorted(w), dtype=np.uint32)


def reduced_wr():
    w = {0, 1, 0xfffffffe, 0xffffffff}
    for k in (0, -1, -8):
        ends = interval_ends(k)
        for i in (0, 1, 127, 128, 254, 255):
            w.update(ends[i])
    return np.array(sorted(w), dtype=np.uint32)


def directed_wa():
    j = np.arange(TAB_SC, dtype=np.int64)[:, None] << 25
    return (j + np.array([0, 1, (1 << 24) - 1, 1 << 24, (1 << 25) - 1], dtype=np.int64)[None, :]).reshape(-1).astype(np.uint32)


def reduced_wa():
    j = np.array([0, 31, 32, 63, 64, 127], dtype=np.int64)[:, None] << 25
    return (j + np.array([1 << 24, 0], dtype=np.int64)[None, :]).reshape(-1).astype(np.uint32)


def directed_pairs():
    """reduced wr x all wa, then all wr x reduced wa"""
    a, b = np.meshgrid(reduced_wr(), directed_wa(), indexing="ij")
    c, d = np.meshgrid(directed_wr(), reduced_wa(), indexing="ij")
    return np.concatenate([a.ravel(), c.ravel()]), np.concatenate([b.ravel(), d.ravel()])


def random_pairs(n=1 << 18, seed=20250):
    w = np.random.default_rng(seed).integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    return w[:, 0].copy(), w[:, 1].copy()


# ---- Box-Muller: reference, bound, float64 restatement -----------------------------------------------------------------------------------
def bm_ref(wr, wa):
    """the definition in np.longdouble -> (z0, z1): u = (w + 1/2) 2^-32, R = sqrt(-2 log u1), theta = 2 pi u2, z0 = R cos, z1 = R sin"""
    u1 = (np.asarray(wr).astype(LD) + LD(0.5)) * LD(2.0) ** -32
    u2 = (np.asarray(wa).astype(LD) + LD(0.5)) * LD(2.0) ** -32
    R = np.sqrt(-2 * np.log(u1))
    th = 8 * np.arctan(LD(1)) * u2
    return R * np.cos(th), R * np.sin(th)


_LN2 = 6.93147180559945286227e-01
_SECTOR = 4.90873852123405193510e-02


def bm_bound(wr, wa):
    """absolute bounds (dz0, dz1) on |device - bm_ref| per pair; the derivation is in the module's docstring"""
    wr, wa = np.asarray(wr), np.asarray(wa)
    t = table_f64()
    u1 = (wr.astype(np.float64) + 0.5) * 2.0 ** -32
    m, k = np.frexp(u1)
    _, i = log_interval(wr)
    inv, logc = t[2 * i], t[2 * i + 1]
    top_entry = i == TAB_LOG - 1                                       # exactly (1, 0): no table error
    d_inv, d_logc = np.where(top_entry, 0.0, ulp_of(inv)), np.where(top_entry, 0.0, ulp_of(logc))
    r = m * inv - 1.0
    ar = np.abs(r) + d_inv
    lp, L = np.abs(np.log1p(r)), np.abs(np.log(u1))
    exact_sum = top_entry & (k == 0)                                   # fma(0, ln2, 0) = 0 and 0 + lp = lp: no rounding
    dL = (m * d_inv + U * ar) / (1 - ar) + d_logc + ar ** 6 / (6 * (1 - ar)) + 2 * U * ar ** 2 + U * lp
    dL = dL + np.where(exact_sum, 0.0, np.abs(k) * 2.0 ** -54 + U * np.abs(k * _LN2 + logc) + U * L)
    v, dv = 2 * L, 2 * dL
    R = np.sqrt(v)
    dR = dv / (2 * np.sqrt(v - dv)) + ulp_of(R)
    j = (wa >> 25).astype(np.int64)
    f = (wa & 0x1ffffff).astype(np.float64) * 2.0 ** -25 + (2.0 ** -26 - 0.5)
    ax = np.abs(f * _SECTOR)
    ds = ax ** 7 / 5040 + U * ax + 2 * U * ax + 2 * U * ax ** 3
    dc = ax ** 8 / 40320 + U + 5 * U * ax ** 2
    S, C = t[2 * TAB_LOG + 2 * j], t[2 * TAB_LOG + 2 * j + 1]
    dS, dC = ulp_of(S), ulp_of(C)
    th = 2 * np.pi * (wa.astype(np.float64) + 0.5) * 2.0 ** -32
    sn, cn = np.abs(np.sin(th)), np.abs(np.cos(th))
    d_sn = dS + np.abs(S) * dc + dC * ax + np.abs(C) * ds + dS * dc + dC * ds + U * np.abs(C) * ax + U * sn
    d_cn = dC + np.abs(C) * dc + dS * ax + np.abs(S) * ds + dC * dc + dS * ds + U * np.abs(S) * ax + U * cn
    ref_err = 2.0 ** -59 * R
    dz0 = dR * (cn + d_cn) + R * d_cn + U * (R + dR) * (cn + d_cn) + ref_err
    dz1 = dR * (sn + d_sn) + R * d_sn + U * (R + dR) * (sn + d_sn) + ref_err
    return dz0, dz1


def bm_ratio(z0, z1, wr, wa):
    """error / bound per pair (the larger of the two outputs) and the errors in ulp of a unit normal (2^-52)"""
    r0, r1 = bm_ref(wr, wa)
    e0, e1 = np.abs(np.asarray(z0).astype(LD) - r0).astype(np.float64), np.abs(np.asarray(z1).astype(LD) - r1).astype(np.float64)
    b0, b1 = bm_bound(wr, wa)
    return np.maximum(e0 / b0, e1 / b1), np.maximum(e0, e1) / 2.0 ** -52


def _split(a):
    c = 134217729.0 * a                                                 # Veltkamp, 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def fma(a, b, c):
    """a b + c rounded once, vectorised: the product exactly as a sum of two doubles (Dekker), the three-term sum in np.longdouble, one rounding
    to double (Python's math.fma appears in 3.13; where the long double sum is inexact the result can differ from a true fma in the last bit)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return ((p.astype(LD) + c.astype(LD)) + e.astype(LD)).astype(np.float64)


MUTATIONS = ("r5_dropped", "z120_dropped", "index_shifted")


def bm_device_f64(wr, wa, tab, mutate=None):
    """box_muller_u32 of philox.h restated in float64, operation by operation (fma where the device has one); 1 / sqrt in double stands in for
    the v_rsq_f64 seed.  mutate: one of MUTATIONS -- a subtly wrong variant the bound must be able to see."""
    wr, wa = np.asarray(wr), np.asarray(wa)
    u1 = fma(wr.astype(np.float64), 2.0 ** -32, 2.0 ** -33)
    m, k = np.frexp(u1)
    _, i = log_interval(wr)
    if mutate == "index_shifted":
        i = i + 1                                                       # (255 + 1 reads the first sector's sine and cosine, as the device would)
    inv, logc = tab[2 * i], tab[2 * i + 1]
    r = fma(m, inv, -1.0)
    p = np.full_like(r, -1.0 / 4.0) if mutate == "r5_dropped" else fma(r, 1.0 / 5.0, -1.0 / 4.0)
    p = fma(p, r, 1.0 / 3.0)
    p = fma(p, r, -0.5)
    lp = fma(p * r, r, r)
    v = -2.0 * (fma(k.astype(np.float64), _LN2, logc) + lp)
    y = 1.0 / np.sqrt(v)
    g, h = v * y, 0.5 * y
    rr = fma(-h, g, 0.5)
    g, h = fma(g, rr, g), fma(h, rr, h)
    R = fma(fma(-g, g, v), h, g)
    j = (wa >> 25).astype(np.int64)
    f = fma((wa & 0x1ffffff).astype(np.float64), 2.0 ** -25, 2.0 ** -26 - 0.5)
    x = f * _SECTOR
    z = x * x
    ps = np.full_like(z, -1.0 / 6.0) if mutate == "z120_dropped" else fma(z, 1.0 / 120.0, -1.0 / 6.0)
    s = fma(z * x, ps, x)
    pc = fma(z, -1.0 / 720.0, 1.0 / 24.0)
    pc = fma(z, pc, -0.5)
    c = fma(z, pc, 1.0)
    S, C = tab[2 * TAB_LOG + 2 * j], tab[2 * TAB_LOG + 2 * j + 1]
    sn, cs = fma(S, c, C * s), fma(C, c, -(S * s))
    return R * cs, R * sn


# ---- the normals' placement ----------------------------------------------------------------------------------------------------------------
def lin_map(cs, K, as_, mppi):
    """[cs, K] -> the index of entry (r, k) in the reference's linear draw order (kernels_sample.hip):
    G order lin = k cs + r; :mppi order lin = (t K + k) as + a with r = t as + a"""
    r, k = np.meshgrid(np.arange(cs, dtype=np.int64), np.arange(K, dtype=np.int64), indexing="ij")
    if mppi:
        t, a = r // as_, r % as_
        return (t * K + k) * as_ + a
    return k * cs + r


def predicted_form(cs, as_, mppi):
    if not mppi and cs % 4 == 0:
        return QUAD
    return PAIR if (as_ if mppi else cs) % 2 == 0 else SINGLE


def normals_shapes():
    """(mppi, cs, K, as, T) of every NORMALS case of the issue's table; G order runs with as = 2 where cs is even and as = 1 otherwise (unused there)"""
    g = [(cs, K) for cs in (1, 2, 3, 4, 5, 6, 7, 8, 12, 21, 22) for K in (1, 257)] + [(cs, K) for cs in (3, 6, 8) for K in (2, 255, 256, 513)]
    out = [(0, cs, K, 2 if cs % 2 == 0 else 1, cs // (2 if cs % 2 == 0 else 1)) for cs, K in g]
    out += [(1, a * T, K, a, T) for a, T in ((1, 1), (1, 5), (2, 1), (2, 3), (3, 2), (3, 3), (4, 2), (16, 2)) for K in (1, 2, 257)]
    return out


CROSS_FORM_N = 3084
CROSS_FORM_SHAPES = [(0, 4, 771, 2, 2), (0, 2, 1542, 2, 1), (0, 1, 3084, 1, 1), (0, 3, 1028, 1, 3), (0, 6, 514, 2, 3), (0, 12, 257, 2, 6),
                     (1, 4, 771, 2, 2), (1, 4, 771, 1, 4)]                    # (mppi, cs, K, as, T)
NORMALS_SEEDS = (20240001, (1 << 32) + 77, 0xfedcba9876543210)              # distinct, two of them >= 2^32
NORMALS_STREAM = (11, 0x80000002)
NORMALS_ACTIVE = (1, 0, 1)


def normals_dscale(B, cs, rng):
    d = rng.uniform(0.25, 2.0, B * cs)
    d[0], d[-1] = -0.75, 0.0                                            # a negative and a zero, both in active slots
    if B * cs > 4:
        d[B * cs - 2] = -d[B * cs - 2]
    return d.reshape(B, cs)


# ---- finalize -------------------------------------------------------------------------------------------------------------------------------
FINALIZE_SHAPES = ((1, 1), (2, 1), (2, 2), (2, 50), (2, 150), (4, 64), (16, 1), (16, 17))          # (as, T)


FINALIZE_KINDS = ("below", "lo", "between", "hi", "above", "+inf", "-inf", "nan", "-0")


def finalize_inputs(as_, T, B, rng):
    """lo, hi, U, wn, {(b, a): kind} with wc = U + wn below, at, between and above the bounds, +-inf, NaN and -0.0 in the first `as` entries of the
    slots: the kinds rotate through the B as control entries, starting where the shape before it in FINALIZE_SHAPES stopped"""
    cs = as_ * T
    lo, hi = np.zeros(MAX_AS), np.zeros(MAX_AS)
    lo[:as_], hi[:as_] = -1.0 - 0.125 * np.arange(as_), 0.5 + 0.25 * np.arange(as_)
    Uin, wn = rng.standard_normal((B, cs)), rng.standard_normal((B, cs)) * 0.5
    kinds = FINALIZE_KINDS
    start = sum(B * a for a, t in FINALIZE_SHAPES[:FINALIZE_SHAPES.index((as_, T))]) if (as_, T) in FINALIZE_SHAPES else 0
    want = {}
    for b in range(B):
        for a in range(as_):
            kind = kinds[(start + b * as_ + a) % len(kinds)]
            u = {"below": lo[a] - 1.5, "lo": lo[a], "between": 0.25 * (lo[a] + hi[a]), "hi": hi[a], "above": hi[a] + 2.0,
                 "+inf": np.inf, "-inf": -np.inf, "nan": np.nan, "-0": -0.0}[kind]
            Uin[b, a], wn[b, a] = (u, 0.0) if kind in ("+inf", "-inf", "nan") else (-0.0, -0.0) if kind == "-0" else (u - 0.25, 0.25)   # u and u - 0.25 are multiples of 2^-5: exact
            want[(b, a)] = kind
    if cs > as_:                                                        # non-finite and signed-zero entries in the part that is rolled, too
        Uin[0, cs - 1], wn[B - 1, as_] = -0.0, np.inf
        wn[0, cs - 1] = -0.0
    return lo, hi, Uin, wn, want


def finalize_ref(as_, T, lo, hi, Uin, wn):
    """weighted_controls = U + wn; control = clamp(wc[1:as]); roll (the last `as` entries of U never change); T == 1: U' = wc.  -> U', control"""
    wc = Uin + wn
    a = wc[:, :as_]
    with np.errstate(invalid="ignore"):
        control = np.where(a > hi[:as_], hi[:as_], np.where(a < lo[:as_], lo[:as_], a))       # Julia's clamp / clampd: NaN stays NaN
    Uo = Uin.copy()
    if T > 1:
        Uo[:, :as_ * T - as_] = wc[:, as_:]
    else:
        Uo[:] = wc
    return Uo, control


# ---- transposes -----------------------------------------------------------------------------------------------------------------------------
TRANSPOSE_CS, TRANSPOSE_K = (1, 2, 31, 32, 33, 100), (1, 31, 32, 33, 257)
SENTINEL = -7.7e77


def transpose_values(B, cs, K, rng):
    """[B][K][cs] (cs x K column-major per slot), every entry distinct, none equal to the sentinel"""
    return (np.arange(B * cs * K, dtype=np.float64).reshape(B, K, cs) + 1.0) * (1.0 + 2.0 ** -30) + rng.integers(0, 2, (B, K, cs)) * 2.0 ** -20


def transpose_in_ref(x):
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1)))             # [B][cs][K]


def transpose_out_ref(y, A=None, Bv=None):
    """[B][cs][K] -> [B][K][cs], with dst = src + (A - B) evaluated in that order"""
    if A is not None:
        y = y + (A - Bv)[:, :, None]
    return np.ascontiguousarray(np.transpose(y, (0, 2, 1)))


def tab_log_device_f64(c):
    """rng_tab_log of kernels_sample.hip restated in float64: log c = 2 atanh(s), s = (c - 1)/(c + 1) carried as sh + sl"""
    c = np.asarray(c, dtype=np.float64)
    num, den = c - 1.0, c + 1.0
    sh = num / den
    sl = fma(-sh, den, num) / den
    z = sh * sh
    p = np.zeros_like(c)
    for n in range(20, 0, -1):
        p = fma(p, z, 1.0 / (2 * n + 1))
    return 2.0 * (sh + fma(sh * z, p, sl))
