"""Inputs, file format, long-double references and error bounds for the risk kernel (mpopis_amd/csrc/kernels_risk.hip) as tools/kbench_risk.hip
launches it, and the bounds tests/test_gpu_scenarios.py holds the engine's aggregate to.

References.  mpopis_amd.scenarios.aggregate(..., dtype=np.longdouble) -- the written definition, evaluated with a 64-bit significand, so its own
rounding (2^-64 relative per operation) is 2^-11 of the double-precision bounds below and is not budgeted separately.

Bounds, with u = 2^-53 (the unit roundoff of binary64) and exact binary64 inputs c_m:

  tail mean, n = tail terms.  Any summation order of n terms errs by at most (n - 1) u sum|c_(i)| to first order (Higham, Accuracy and Stability of
  Numerical Algorithms, (4.4)); the division by n adds one rounding, u |J|.  n = 1 is a copy: the bound is 0 and the test asks for equality.

  entropic, J = c* + log(s / M) / theta with s = sum exp(e_m), e_m = theta (c_m - c*) <= 0, one e_m = 0.  Device exp and log in double are taken to
  be accurate to 2 ulp each: the ROCm device-library documentation is not part of the toolchain's installed files, so this is an assumption, chosen
  on the loose side of the 1 ulp commonly quoted for both OCML functions.  To first order: c_m - c* and the product with theta round once each, which
  moves exp(e_m) by at most 2 u |e_m| exp(e_m) <= 0.74 u; exp itself adds 2 u exp(e_m); the sum adds (M - 1) u s in the worst order; s / M one u.
  Relative to s >= 1 that is at most (1.74 (M - 1) + 3) u in the argument of log, i.e. the same absolute error in log(s / M), plus 2 u |log(s / M)|
  from log and u |log(s / M)| from the division by theta, with |log(s / M)| <= ln M < 2.78; the final addition rounds once more, u |J|.  The worst
  case is therefore u |J| + (1.74 (M - 1) + 3 + 3 ln M) u / |theta|.  The figure the tests ASSERT is the smaller one the feature was specified with,
        3 u |J| + (M + 12) u / |theta|,
  which counts the summation at its typical rather than its worst-case growth; it is the stricter of the two for M >= 4 wherever the 1 / |theta|
  term dominates (every case here), and a result that misses it fails the test."""
import numpy as np

from mpopis_amd import scenarios

U53 = 2.0 ** -53


def tail_bound(costs, tail):
    """costs (M, ...) -> per-column bound for the mean of the `tail` largest; 0 where tail == 1"""
    c = np.asarray(costs, dtype=np.longdouble)
    if tail == 1:
        return np.zeros(c.shape[1:], dtype=np.longdouble)
    s = -np.sort(-c, axis=0)[:tail]
    J = s.sum(axis=0) / tail
    return (tail - 1) * U53 * np.abs(s).sum(axis=0) + U53 * np.abs(J)


def entropic_bound(J, M, theta):
    return 3 * U53 * np.abs(np.asarray(J, dtype=np.longdouble)) + (M + 12) * U53 / abs(theta)


def ratio(got, ref, bound):
    """worst |got - ref| / bound over the finite entries (0 / 0 counts as 0: an exact case met exactly); the non-finite ones must agree in kind"""
    got, ref = np.asarray(got, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    err = np.abs(got[fin] - ref[fin])
    b = np.broadcast_to(bound, ref.shape)[fin]
    r = np.where(err == 0, 0.0, err / np.where(b == 0, np.longdouble(1e-300), b))
    return float(r.max()) if r.size else 0.0


def check_aggregate(got, sc, kind, tail=0, theta=0.0):
    """got (..., K) against aggregate(sc (..., M, K)) in long double; returns the worst error / bound (asserted <= 1 by the caller)"""
    sc = np.asarray(sc, dtype=np.float64)
    M = sc.shape[-2]
    ref = scenarios.aggregate(sc, kind, tail, theta, dtype=np.longdouble)
    rk, tl, th = scenarios.resolve_risk(kind, M, tail, theta)
    if rk == scenarios.RISK_TAIL_MEAN:
        with np.errstate(invalid="ignore"):
            bound = tail_bound(np.moveaxis(np.where(np.isfinite(sc), sc, 0.0), -2, 0), tl)
    else:
        bound = entropic_bound(np.where(np.isfinite(ref), ref, 0.0), M, th)
    return ratio(got, ref, bound)


# ---- the kernel harness (tools/kbench_risk.hip) ---------------------------------------------------------------------------------------------------
from tests.helpers.harness_io import F64, I32, U64, GUARD, is_poison, split_guard, pack_case, unpack_result as _unpack_result  # noqa: E402

CASE_MAGIC, RESULT_MAGIC = b"RSKCASE1", b"RSKRES01"
KS = (1, 63, 64, 65, 200)
MS = (1, 2, 3, 7, 16)
THETAS = (1e-3, -1e-3, 1.0, -1.0)
B, B_FULL, B0, INACTIVE = 3, 5, 1, 1    # a view of 3 slots (the batch's slots 1..3) inside planes laid out for 5: a scenario stride taken from B
                                        # reads the wrong plane from scenario 1 on; the view's slot 1 is inactive
NAN_SLOT = 2                            # the view's slot that holds the one NaN
ERR_ACTION = -3                         # MPOPIS_ERR_ACTION
CMIN_EMPTY = np.uint64(0xffffffffffffffff)


def tails(M):
    """tail in {1, 2, M - 1, M}, as far as they exist for this M"""
    return sorted({t for t in (1, 2, M - 1, M) if 1 <= t <= M})


def make_costs(M, K, seed):
    """[M][B_FULL][K] scenario planes.  In the view's slots: O(1) costs with 1e6-penalty entries beside them, an all-equal column, a tie between
    scenarios 0 and 1, a -0.0 that is its column's maximum, and one NaN in one scenario of one sample of NAN_SLOT.  The batch's slots outside the
    view hold a constant no result may show."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 4.0, (M, B_FULL, K))
    pen = rng.random((M, B_FULL, K)) < 0.2
    c[pen] += 1e6 * rng.integers(1, 3, int(pen.sum()))
    v = c[:, B0:B0 + B]                                          # (a view: writes go through)
    v[:, 0, 0] = 2.5
    if M >= 2:
        v[1, :, K // 2] = v[0, :, K // 2]
    if M >= 2 and K > 1:                                         # (K = 1: the one column stays the all-equal one)
        v[0, 0, K - 1] = -0.0
        v[1:, 0, K - 1] = -1.0 - rng.random(M - 1)
    v[M // 2, NAN_SLOT, K // 3] = np.nan
    c[:, :B0] = 12345.0
    c[:, B0 + B:] = 12345.0
    return c


def view_costs(c):
    """the view's costs as aggregate takes them: (B, M, K)"""
    return np.ascontiguousarray(np.moveaxis(c[:, B0:B0 + B], 0, 1))


def active_flags():
    a = np.ones(B, dtype=np.int32)
    a[INACTIVE] = 0
    return a


def risk_case(c, kind, tail, theta, cmin0=None, status0=None, use_active=True, use_status=True):
    """the case file of one launch; cmin0 None: launched without cmin"""
    M, _, K = c.shape
    status0 = np.zeros(B, dtype=np.int32) if status0 is None else status0
    return pack_case(CASE_MAGIC, 0, B, [M, B_FULL, B0, K, kind, tail, int(use_active), int(use_status)], [theta],
                     [(I32, active_flags()), (F64, c), (U64, cmin0), (I32, status0)])


def unpack_result(buf, K, with_cmin):
    """-> cost (B, K) and its guard, cmin (B,) or None, status (B,); the guards of cmin and status are checked here"""
    _, arrs = _unpack_result(RESULT_MAGIC, buf)
    cost, guard = split_guard(arrs[0], (B, K))
    cmin = None
    if with_cmin:
        cmin, g = split_guard(arrs[1], (B,))
        assert np.all(is_poison(g))
    else:
        assert arrs[1].size == 0
    status, g = split_guard(arrs[2], (B,))
    assert np.all(is_poison(g))
    return cost, guard, cmin, status


def cost_key(v):
    """engine.h cost_key: order-preserving double -> uint64 (unsigned comparison == numeric comparison), every NaN last"""
    v = np.float64(v)
    if np.isnan(v):
        return np.uint64(0xfff8000000000000)
    u = int(np.array([v]).view(np.uint64)[0])
    return np.uint64((~u) & 0xffffffffffffffff) if u >> 63 else np.uint64(u | 0x8000000000000000)
