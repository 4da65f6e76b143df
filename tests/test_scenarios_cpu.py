"""CPU-side checks of the scenario seam (mpopis_set_scenarios, mpopis_set_risk, mpopis_get_scenarios, mpopis_get_scenario_costs): the four entry
points are declared and exported and refuse a NULL handle, mpopis_amd.scenarios.aggregate gives the known answers of its definition, the Python
side refuses what the library would refuse before reaching it, and the harnesses' split hands every rank the blocks of its own trials.
No compute on a device."""
import os
import re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpopis_set_scenarios", "mpopis_set_risk", "mpopis_get_scenarios", "mpopis_get_scenario_costs")


@pytest.fixture(scope="module")
def L():
    from mpopis_amd import build, _lib
    build.build()
    return _lib.lib()


def test_header_declares_the_four_calls_and_keeps_the_version():
    hdr = open(os.path.join(ROOT, "include", "mpopis.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    src = re.sub(r"\s+", " ", src)
    assert "#define MPOPIS_ABI_VERSION 5" in src
    assert "#define MPOPIS_MAX_SCENARIOS 16" in src
    assert re.search(r"enum \{ MPOPIS_RISK_TAIL_MEAN = 0, MPOPIS_RISK_ENTROPIC = 1 \}", src)
    for proto in ("int mpopis_set_scenarios(mpopis_handle *h, int32_t M, const double *p , int32_t n, int32_t per_slot);",
                  "int mpopis_set_risk(mpopis_handle *h, int32_t kind, int32_t tail, double theta);",
                  "int mpopis_get_scenarios(mpopis_handle *h, int32_t *M, int32_t *kind, int32_t *tail, double *theta);",
                  "int mpopis_get_scenario_costs(mpopis_handle *h, double *out );"):
        assert proto in src, proto


def test_symbols_exported(L):
    from mpopis_amd import _lib, scenarios
    for name in NAMES:
        assert name in _lib.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert L.mpopis_abi_version() == 5                      # support is detected by the symbol, not by the version
    assert (scenarios.RISK_TAIL_MEAN, scenarios.RISK_ENTROPIC, scenarios.MAX_SCENARIOS) == (0, 1, 16)


def test_null_handle_is_an_argument_error(L):
    assert L.mpopis_set_scenarios(None, 1, None, 20, 0) == -1
    assert L.mpopis_set_risk(None, 0, 0, 0.0) == -1
    assert L.mpopis_get_scenarios(None, None, None, None, None) == -1
    assert L.mpopis_get_scenario_costs(None, None) == -1


# ---- aggregate: the written definition ---------------------------------------------------------------------------------------------------------

def test_aggregate_known_answers():
    from mpopis_amd.scenarios import aggregate
    c = np.array([3.0, 1.0, 2.0])[:, None]                  # (M, K) = (3, 1)
    assert aggregate(c, "worst")[0] == 3.0 and aggregate(c, "cvar", tail=1)[0] == 3.0
    assert aggregate(c, "cvar", tail=2)[0] == 2.5
    assert aggregate(c, "cvar", tail=3)[0] == 2.0 and aggregate(c, "mean")[0] == 2.0 and aggregate(c, "cvar", tail=0)[0] == 2.0
    e = aggregate(np.array([[0.0], [1.0]]), "entropic", theta=np.log(2.0))
    assert abs(e[0] - np.log2(1.5)) < 4e-16                 # 1 + log2((1/2 + 1) / 2)
    e = aggregate(np.array([[0.0], [1.0]]), "entropic", theta=-np.log(2.0))
    assert abs(e[0] - (-np.log2(0.75))) < 4e-16             # theta < 0 takes the minimum: 0 - log2((1 + 1/2) / 2)
    big = aggregate(np.array([[1e6], [1e6 + 1.0]]), "entropic", theta=-800.0)
    assert np.isfinite(big[0]) and 1e6 <= big[0] < 1e6 + 1e-2            # exp(-800) underflows harmlessly only because c* is the MINIMUM here
    big = aggregate(np.array([[1e6], [1e6 + 1.0]]), "entropic", theta=800.0)
    assert np.isfinite(big[0]) and 1e6 + 0.99 < big[0] <= 1e6 + 1.0
    # the scenario axis is the second to last; leading axes are slots
    c3 = np.arange(24.0).reshape(2, 3, 4)
    assert np.array_equal(aggregate(c3, "worst"), c3[:, 2]) and np.array_equal(aggregate(c3, "mean"), c3[:, 1])
    assert aggregate(c3, "mean", dtype=np.longdouble).dtype == np.longdouble


def test_aggregate_worst_returns_the_bits_of_the_input():
    from mpopis_amd.scenarios import aggregate
    rng = np.random.default_rng(0)
    c = rng.standard_normal((5, 7, 33)) * 10.0 ** rng.integers(-3, 7, (5, 7, 33))
    assert np.array_equal(aggregate(c, "worst"), c.max(axis=1))
    z = aggregate(np.array([[-0.0], [-1.0]]), "worst")
    assert z[0] == 0.0 and np.signbit(z[0])


def test_aggregate_non_finite():
    from mpopis_amd.scenarios import aggregate
    nan, inf = np.nan, np.inf
    c = np.array([[1.0, nan, inf, -inf, inf], [2.0, 5.0, 1.0, 1.0, -inf], [3.0, inf, 2.0, 2.0, 0.0]])
    for kind, kw in (("mean", {}), ("worst", {}), ("cvar", dict(tail=2))):
        J = aggregate(c, kind, **kw)
        assert np.isfinite(J[0]) and np.isnan(J[1])                      # NaN propagates, whatever else the column holds
    assert np.array_equal(aggregate(c, "worst")[2:], [inf, 2.0, inf])
    assert np.array_equal(aggregate(c, "cvar", tail=2)[2:4], [inf, 1.5])
    assert aggregate(c, "mean")[3] == -inf and np.isnan(aggregate(c, "mean")[4])            # inf + 0 + -inf
    for theta in (1.0, -1.0):
        J = aggregate(c, "entropic", theta=theta)
        assert np.isfinite(J[0]) and np.isnan(J[1]) and J[2] == inf and J[3] == -inf and np.isnan(J[4])


# ---- the Python-side refusals ------------------------------------------------------------------------------------------------------------------

def test_python_side_refusals():
    from mpopis_amd import scenarios as S
    from mpopis_amd._lib import MPOPISError, ERR_ARG

    def refused(f, *a, **k):
        with pytest.raises(MPOPISError) as ei:
            f(*a, **k)
        assert ei.value.code == ERR_ARG
    refused(S.resolve_risk, "median", 3)
    refused(S.resolve_risk, "mean", 0)
    refused(S.resolve_risk, "cvar", 3, tail=4)
    refused(S.resolve_risk, "cvar", 3, tail=-1)
    refused(S.resolve_risk, "cvar", 3, tail=1.5)
    for th in (0.0, np.inf, -np.inf, np.nan):
        refused(S.resolve_risk, "entropic", 3, theta=th)
    assert S.resolve_risk("mean", 4) == (0, 4, 0.0) and S.resolve_risk("worst", 4) == (0, 1, 0.0)
    assert S.resolve_risk("cvar", 4, tail=0) == (0, 4, 0.0) and S.resolve_risk(":cvar", 4, tail=3) == (0, 3, 0.0)
    assert S.resolve_risk("entropic", 4, theta=-0.5) == (1, 4, -0.5)
    refused(S.check_scenarios, np.zeros((17, 20)), 2, 20)
    refused(S.check_scenarios, np.zeros((3, 19)), 2, 20)
    refused(S.check_scenarios, np.zeros((2, 3, 20)), 2, 20)                # three axes without per_slot
    refused(S.check_scenarios, np.zeros((3, 20)), 2, 20, True)             # two axes with it
    refused(S.check_scenarios, np.zeros((3, 3, 20)), 2, 20, True)          # not one block per slot
    assert S.check_scenarios(None, 2, 20) is None and S.check_scenarios(np.zeros((0, 20)), 2, 20) is None
    assert S.check_scenarios(np.zeros((16, 8)), 2, 8).shape == (16, 8)
    refused(S.aggregate, np.zeros(5))
    assert S.parse_risk("mean") == ("mean", 0, 0.0) and S.parse_risk(("cvar", 2)) == ("cvar", 2, 0.0)
    assert S.parse_risk(("entropic", 0.25)) == ("entropic", 0, 0.25) and S.parse_risk("worst") == ("worst", 0, 0.0)
    refused(S.parse_risk, "cvar")
    refused(S.parse_risk, ("median", 2))
    refused(S.parse_risk, 3)


def test_harnesses_take_the_keywords():
    import inspect
    from mpopis_amd import examples
    sig = inspect.signature(examples.simulate_car_racing).parameters
    assert sig["model_params"].default is None and sig["risk"].default == "mean"
    assert examples._SIMPLE_KW["model_params"] is None and examples._SIMPLE_KW["risk"] == "mean"
    from mpopis_amd._lib import MPOPISError
    with pytest.raises(MPOPISError):
        examples.simulate_car_racing(num_trials=1, risk="cvar", quiet=True)               # refused before a handle exists
    with pytest.raises(ValueError):
        examples.simulate_car_racing(num_trials=1, num_cars=2, model_params=np.zeros((2, 20)), car_fleet=np.zeros((2, 20)), quiet=True)


# ---- sharding ----------------------------------------------------------------------------------------------------------------------------------

def test_split_model_params_per_trial_over_ranks():
    from mpopis_amd.examples import split_model_params_per_trial, shard_trials
    n_trials, M, n = 7, 3, 20                               # not a multiple of 3: ranks hold 3, 2, 2 trials
    shared = np.arange(M * n, dtype=np.float64).reshape(M, n)
    per = np.arange(n_trials * M * n, dtype=np.float64).reshape(n_trials, M, n)
    seen = []
    for rank in range(3):
        p, per_slot = split_model_params_per_trial(shared, n, n_trials, rank, 3)
        assert per_slot is False and np.array_equal(p, shared)
        p, per_slot = split_model_params_per_trial(per, n, n_trials, rank, 3)
        mine = shard_trials(n_trials, rank, 3)
        assert per_slot is True and p.shape == (len(mine), M, n)
        assert np.array_equal(p, per[[k - 1 for k in mine]])                # trial k (1-based) gets block k - 1, in slot order
        seen += mine
    assert sorted(seen) == list(range(1, n_trials + 1))
    assert split_model_params_per_trial(None, n, n_trials) == (None, False)
    p, per_slot = split_model_params_per_trial(per, n, n_trials)
    assert per_slot and np.array_equal(p, per)
    for bad in (np.zeros((M, n + 1)), np.zeros((n_trials + 1, M, n)), np.zeros(n), np.zeros((n_trials, M, n - 1))):
        with pytest.raises(ValueError):
            split_model_params_per_trial(bad, n, n_trials)
