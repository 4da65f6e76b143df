"""The risk kernel of a scenario handle (mpopis_amd/csrc/kernels_risk.hip: launch_risk) exercised directly through the C++
harness tools/kbench_risk.hip: one process per launch, inputs written by the test, raw device outputs read back.

Shapes: K on both sides of a wave and of the 256-thread workgroup (1, 63, 64, 65, 200); three slots with the middle one inactive, launched as a
VIEW of a five-slot batch (the scenario planes are strided by the batch, not by the view); M = 1, 2, 3, 7, 16 -- five of the sixteen template
instances, the smallest, the largest, odd and even pass counts of the sorting network; tail = 1, 2, M - 1, M; theta = +-1e-3, +-1.
Inputs (tests/helpers/risk_cases.py: make_costs): 1e6-penalty costs beside O(1) ones, ties, an all-equal column, a -0.0 that is its column's
maximum, one NaN in one scenario of one sample.  References are mpopis_amd.scenarios.aggregate in np.longdouble, never the engine; the bounds are
derived in the helper.  The harness poisons the cost output: the inactive slot and the guard entries must stay untouched and no active entry
may keep the poison.

Every check prints `RATIO <op> <worst error / bound>`; DESIGN.md section 19 records the worst per op."""
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import risk_cases as R
from mpopis_amd import scenarios

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness():
    return HR.build("risk")


def _launch(harness, tmp_path, c, kind, tail, theta, cmin0, status0=None):
    K = c.shape[2]
    buf = HR.run_case(harness, tmp_path, R.risk_case(c, kind, tail, theta, cmin0=cmin0, status0=status0))
    cost, guard, cmin, status = R.unpack_result(buf, K, cmin0 is not None)
    assert np.all(R.is_poison(guard)), "guard entries of cost written"
    assert np.all(R.is_poison(cost[R.INACTIVE])), "the inactive slot's costs written"
    for b in range(R.B):
        if b != R.INACTIVE:
            assert not np.any(R.is_poison(cost[b])), "slot %d keeps untouched entries" % b
    return cost, cmin, status


def _check_side_outputs(J, cmin, cmin0, status, status0):
    """cmin: the key of the minimum aggregate merged into what was there (an all-NaN-free slot: its minimum finite J; NaN sorts last, so the NaN
    slot's key is still that of its smallest number); status: raised in exactly the slots with a non-finite aggregate; the inactive slot keeps both"""
    for b in range(R.B):
        if b == R.INACTIVE:
            assert cmin is None or cmin[b] == cmin0[b]
            assert status[b] == status0[b]
            continue
        fin = J[b][np.isfinite(J[b])]
        if cmin is not None:
            want = min(R.cost_key(fin.min() if fin.size else np.nan), cmin0[b])
            assert cmin[b] == want, (b, hex(int(cmin[b])), hex(int(want)))
        bad = not np.all(np.isfinite(J[b]))
        assert status[b] == (R.ERR_ACTION if bad else status0[b]), (b, status[b])
        assert bad == (b == R.NAN_SLOT)


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("M", R.MS)
def test_tail_mean(harness, tmp_path, M, K):
    c = R.make_costs(M, K, seed=100 * M + K)
    v = R.view_costs(c)
    worst = 0.0
    for tail in R.tails(M):
        cmin0 = np.full(R.B, R.CMIN_EMPTY)
        status0 = np.zeros(R.B, dtype=np.int32)
        cost, cmin, status = _launch(harness, tmp_path, c, scenarios.RISK_TAIL_MEAN, tail, 0.0, cmin0, status0)
        act = [b for b in range(R.B) if b != R.INACTIVE]
        if tail == 1:                                            # the worst case: equal as doubles to the maximum
            mx = np.where(np.isnan(v).any(axis=1), np.nan, np.where(np.isnan(v), -np.inf, v).max(axis=1))
            assert np.array_equal(cost[act], mx[act], equal_nan=True)
        r = R.check_aggregate(cost[act], v[act], "cvar", tail)
        print("RATIO tail_mean %.4f  (M %d K %d tail %d)" % (r, M, K, tail))
        assert r <= 1.0, (M, K, tail, r)
        worst = max(worst, r)
        _check_side_outputs(cost, cmin, cmin0, status, status0)
        assert cost[0, 0] == 2.5                                 # the all-equal column: every tail mean of equal numbers is that number


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("M", R.MS)
def test_entropic(harness, tmp_path, M, K):
    c = R.make_costs(M, K, seed=7 + 100 * M + K)
    v = R.view_costs(c)
    act = [b for b in range(R.B) if b != R.INACTIVE]
    for theta in R.THETAS:
        cmin0 = np.full(R.B, R.CMIN_EMPTY)
        status0 = np.zeros(R.B, dtype=np.int32)
        cost, cmin, status = _launch(harness, tmp_path, c, scenarios.RISK_ENTROPIC, M, theta, cmin0, status0)
        r = R.check_aggregate(cost[act], v[act], "entropic", theta=theta)
        print("RATIO entropic %.4f  (M %d K %d theta %g)" % (r, M, K, theta))
        assert r <= 1.0, (M, K, theta, r)
        _check_side_outputs(cost, cmin, cmin0, status, status0)
        lo, hi = np.nanmin(v[0], axis=0), np.nanmax(v[0], axis=0)
        assert np.all(cost[0] >= lo - 1e-6) and np.all(cost[0] <= hi + 1e-6)      # a mean of sorts: between the extremes


def test_cmin_and_status_merge_with_what_is_there(harness, tmp_path):
    """cmin is a running minimum and status merges by precedence: an earlier smaller key stays, NOT_PD (-2) is overridden by ACTION (-3) and an
    earlier HIP error (-4) is not; launched without cmin / status nothing but cost is written"""
    M, K = 3, 65
    c = R.make_costs(M, K, seed=5)
    cmin0 = np.array([R.cost_key(-1e9), R.CMIN_EMPTY, R.CMIN_EMPTY], dtype=np.uint64)
    status0 = np.array([-2, -2, -4], dtype=np.int32)
    cost, cmin, status = _launch(harness, tmp_path, c, scenarios.RISK_TAIL_MEAN, M, 0.0, cmin0, status0)
    assert cmin[0] == cmin0[0] and cmin[1] == cmin0[1] and cmin[2] == R.cost_key(np.nanmin(cost[2]))
    assert list(status) == [-2, -2, -4]                          # slot 0 finite: kept; slot 1 inactive; slot 2: the HIP error outranks ACTION
    status0 = np.array([0, 0, -2], dtype=np.int32)
    cost, cmin, status = _launch(harness, tmp_path, c, scenarios.RISK_TAIL_MEAN, M, 0.0, None, status0)
    assert cmin is None and list(status) == [0, 0, R.ERR_ACTION]
    buf = HR.run_case(harness, tmp_path, R.risk_case(c, scenarios.RISK_TAIL_MEAN, M, 0.0, status0=status0, use_status=False, use_active=False))
    cost2, guard, _, status = R.unpack_result(buf, K, False)
    assert list(status) == [0, 0, -2] and np.all(R.is_poison(guard))
    assert not np.any(R.is_poison(cost2))                        # without `active` every slot of the view is aggregated
    assert np.array_equal(cost2[[0, 2]], cost[[0, 2]], equal_nan=True)


def test_non_finite_inputs_follow_the_documented_rule(harness, tmp_path):
    """tail mean: a NaN gives NaN, infinities take part in the sort and the sum; entropic: the IEEE sum of the non-finite inputs"""
    M, K = 3, 64
    c = np.ones((M, R.B_FULL, K))
    v = c[:, R.B0:R.B0 + R.B]
    v[:, 0, 0] = [np.inf, 1.0, 2.0]
    v[:, 0, 1] = [-np.inf, 1.0, 2.0]
    v[:, 0, 2] = [np.inf, -np.inf, 2.0]
    v[:, 0, 3] = [np.nan, np.inf, 2.0]
    vc = R.view_costs(c)
    for kind, tail, theta, name in ((scenarios.RISK_TAIL_MEAN, 2, 0.0, "cvar"), (scenarios.RISK_TAIL_MEAN, 3, 0.0, "cvar"),
                                    (scenarios.RISK_ENTROPIC, 3, 1.0, "entropic"), (scenarios.RISK_ENTROPIC, 3, -1.0, "entropic")):
        cost, _, status = _launch(harness, tmp_path, c, kind, tail, theta, None)
        ref = scenarios.aggregate(vc, name, tail, theta)
        assert np.array_equal(cost[0, :4], ref[0, :4], equal_nan=True), (name, tail, theta, cost[0, :4], ref[0, :4])
        assert status[0] == R.ERR_ACTION and status[2] == 0
    assert np.isnan(ref[0, 2]) and np.isnan(ref[0, 3]) and ref[0, 1] == -np.inf       # (entropic, theta < 0, of the last round)
