"""The inputs, references and bounds of tests/helpers/risk_cases.py are what tests/test_gpu_risk_harness.py and tests/test_gpu_scenarios.py take them
for -- shown on the CPU, without the kernel: the inputs hold the cases they claim, the long-double reference agrees with an independent
evaluation, the bounds are zero exactly where equality is asked and are not met by a wrong answer, and the case file round-trips."""
import math
from fractions import Fraction

import numpy as np
import pytest

from mpopis_amd import scenarios
from tests.helpers import harness_io as IO
from tests.helpers import risk_cases as R


@pytest.mark.parametrize("M", R.MS)
@pytest.mark.parametrize("K", R.KS)
def test_inputs_hold_what_they_claim(M, K):
    c = R.make_costs(M, K, seed=100 * M + K)
    v = R.view_costs(c)
    assert c.shape == (M, R.B_FULL, K) and v.shape == (R.B, M, K) and R.B_FULL > R.B and R.B0 > 0
    assert np.all(c[:, :R.B0] == 12345.0) and np.all(c[:, R.B0 + R.B:] == 12345.0)      # outside the view: a value no result may show
    assert np.array_equal(v[1], c[:, R.B0 + 1], equal_nan=True)
    assert np.all(v[0, :, 0] == 2.5)                                                        # the all-equal column
    nan = np.argwhere(np.isnan(v))
    assert len(nan) == 1 and nan[0][0] == R.NAN_SLOT and R.NAN_SLOT != R.INACTIVE           # one NaN, in an active slot
    fin = v[np.isfinite(v)]
    assert (fin > 9e5).any() or M * K < 8
    assert (fin < 5).any()
    if M >= 2 and K > 1:                                                                    # (K = 1: the one column also holds the NaN)
        assert np.all(v[:, 0, K // 2] == v[:, 1, K // 2])                                   # a tie between scenarios 0 and 1
    if M >= 2 and K > 1:
        col = v[0, :, K - 1]
        assert col[0] == 0.0 and np.signbit(col[0]) and np.all(col[1:] < 0)                 # -0.0 is its column's maximum
    assert R.active_flags().tolist() == [1, 0, 1]
    assert R.tails(M) == sorted({t for t in (1, 2, M - 1, M) if 1 <= t <= M}) and 1 in R.tails(M) and M in R.tails(M)


def _exact_tail_mean(col, tail):
    s = sorted((Fraction(float(x)) for x in col), reverse=True)[:tail]
    return sum(s) / tail


def test_long_double_tail_mean_against_exact_rationals():
    rng = np.random.default_rng(3)
    c = R.view_costs(R.make_costs(7, 65, seed=3))[0]                                        # (7, 65), no NaN in slot 0
    for tail in R.tails(7):
        ref = scenarios.aggregate(c, "cvar", tail, dtype=np.longdouble)
        bound = R.tail_bound(c, tail)
        for k in rng.choice(65, 12, replace=False):
            exact = _exact_tail_mean(c[:, k], tail)
            err = abs(Fraction(float(ref[k])) - exact)                                      # (float(): the long double rounded to double, 2^-53 |J| at most)
            assert err <= Fraction(2.0 ** -52) * abs(exact) + Fraction(1, 10 ** 300), (tail, k)
            if tail == 1:
                assert bound[k] == 0 and float(ref[k]) == max(c[:, k])
            else:
                assert bound[k] > 0
                got64 = scenarios.aggregate(c, "cvar", tail)[k]                             # the same order in double: inside its own bound
                assert abs(Fraction(float(got64)) - exact) <= Fraction(float(bound[k]))


def test_long_double_entropic_against_math_module():
    c = np.array([[0.3], [1.7], [0.9], [1.7]])
    for theta in R.THETAS:
        ref = float(scenarios.aggregate(c, "entropic", theta=theta, dtype=np.longdouble)[0])
        cs = max(c[:, 0]) if theta > 0 else min(c[:, 0])
        want = cs + math.log(math.fsum(math.exp(theta * (x - cs)) for x in c[:, 0]) / 4.0) / theta
        assert abs(ref - want) <= float(R.entropic_bound(want, 4, theta))
        lo, hi = c.min(), c.max()
        assert lo <= ref <= hi and (ref > c.mean()) == (theta > 0)                          # risk-averse above the mean, risk-seeking below


def test_bounds_reject_a_wrong_answer():
    c = R.view_costs(R.make_costs(3, 64, seed=9))[[0]]                                      # (1, 3, 64)
    good = scenarios.aggregate(c, "mean")
    assert R.check_aggregate(good, c, "mean") <= 1.0
    wrong = np.sort(c, axis=1)[:, 1]                                                        # the median is not the mean
    assert R.check_aggregate(wrong, c, "mean") > 1e6
    assert R.check_aggregate(good * (1 + 2.0 ** -40), c, "mean") > 1.0                      # nor is the mean 2^-40 off
    worst = scenarios.aggregate(c, "worst")
    assert R.check_aggregate(worst, c, "worst") == 0.0
    assert R.check_aggregate(np.nextafter(worst, np.inf), c, "worst") > 1e100               # tail = 1 asks for equality
    ent = scenarios.aggregate(c, "entropic", theta=1e-3)
    assert R.check_aggregate(ent, c, "entropic", theta=1e-3) <= 1.0
    assert R.check_aggregate(ent + 1e-9, c, "entropic", theta=1e-3) > 1.0
    with pytest.raises(AssertionError):
        R.check_aggregate(np.where(np.arange(64) == 5, np.nan, good), c, "mean")            # a NaN where the reference has a number


def test_entropic_bound_is_the_stated_formula():
    u = 2.0 ** -53
    assert float(R.entropic_bound(10.0, 16, 1e-3)) == pytest.approx(3 * u * 10.0 + 28 * u / 1e-3, rel=1e-15)
    assert float(R.entropic_bound(-10.0, 1, -1.0)) == pytest.approx(3 * u * 10.0 + 13 * u, rel=1e-15)


def test_cost_key_orders_like_the_numbers():
    vals = [-np.inf, -1e6, -1.0, -0.0, 0.0, 1e-300, 2.5, 1e6, np.inf]
    keys = [int(R.cost_key(v)) for v in vals]
    assert keys == sorted(keys) and keys[3] < keys[4]                                       # (-0.0 sorts just before +0.0)
    assert int(R.cost_key(np.nan)) > keys[-1] and int(R.cost_key(-np.nan)) == int(R.cost_key(np.nan))
    assert int(R.CMIN_EMPTY) > int(R.cost_key(np.nan))


def test_case_file_round_trips():
    c = R.make_costs(3, 65, seed=1)
    cmin0 = np.full(R.B, R.CMIN_EMPTY)
    data = R.risk_case(c, scenarios.RISK_TAIL_MEAN, 2, 0.0, cmin0=cmin0)
    op, B, ipar, dpar, arrays = IO.unpack_case(R.CASE_MAGIC, data)
    assert (op, B) == (0, R.B) and ipar == [3, R.B_FULL, R.B0, 65, 0, 2, 1, 1] and dpar == [0.0]
    assert [t for t, _ in arrays] == [IO.I32, IO.F64, IO.U64, IO.I32]
    assert np.array_equal(arrays[1][1].reshape(c.shape), c, equal_nan=True) and np.array_equal(arrays[2][1], cmin0)
    data = R.risk_case(c, scenarios.RISK_ENTROPIC, 3, -1e-3)
    _, _, ipar, dpar, arrays = IO.unpack_case(R.CASE_MAGIC, data)
    assert ipar[4:6] == [1, 3] and dpar == [-1e-3] and arrays[2][1].size == 0               # launched without cmin
    res = IO.pack_result(R.RESULT_MAGIC, 0, [(IO.F64, IO.poisoned((R.B * 65 + IO.GUARD,))), (IO.U64, None), (IO.I32, IO.poisoned((R.B + IO.GUARD,), IO.I32))])
    cost, guard, cmin, status = R.unpack_result(res, 65, False)
    assert cost.shape == (R.B, 65) and np.all(R.is_poison(cost)) and np.all(R.is_poison(guard)) and cmin is None and status.shape == (R.B,)
