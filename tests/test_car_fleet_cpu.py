"""A fleet -- every car of a multi-car slot with its own parameter vector (mpopis_set_env_params_cars) -- the parts that
need no device: the expectation tests/helpers/car_fleet_ref.py composes from the oracle's per-car pieces against the oracle's own multi-car
simulate_model at equal parameters; that the fleet the GPU tests drive moves every car far enough to tell the cars apart; the prototype, the
exported symbol and the Python-side refusals; MultiCarRacingEnv's car_params list; simulate_car_racing's two exclusive keywords."""
import os
import re
import types

import numpy as np
import pytest

from tests.helpers import car_fleet_ref as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(oracle, track, ncars, K, T, seed):
    """shaped as tests/test_gpu_many_cars.test_rollout_costs_against_the_oracle shapes them (slot 0: the reset grid, five far-out samples)"""
    rng = np.random.default_rng(seed)
    cs = 2 * ncars * T
    env = oracle.OracleEnv("car", ncars, track=track)
    U = rng.uniform(-0.3, 0.3, cs)
    U[1::2] += 0.3
    E = rng.standard_normal((K, cs)) * np.tile([0.25, 0.32], ncars * T)
    E[:5] *= 8.0
    return env, U, E


@pytest.mark.parametrize("ncars", [2, 3, 5, 8])
def test_helper_reproduces_the_oracle_at_equal_parameters(oracle, track, ncars):
    K, T = 24, 9
    env, U, E = _inputs(oracle, track, ncars, K, T, 100 + ncars)
    pol = oracle.OraclePolicy("gmppi", env, K, T, lam=10.0, U0=np.zeros(2 * ncars), cov=np.tile([0.0625, 0.1], ncars), N=1)
    ref, ref_tr = pol.simulate_model(U, E.T, log=True)
    fleet = np.tile(oracle.car_default_params(), (ncars, 1))
    got, got_tr = fref.fleet_rollout(oracle, fleet, track, env.state, U, E, log=True)
    assert np.max(np.abs(got - ref) / np.abs(ref)) <= 1e-12
    assert np.max(np.abs(got_tr - ref_tr) / (np.abs(ref_tr) + 1e-9)) <= 1e-12


def test_helper_control_cost_at_equal_parameters(oracle, track):
    ncars, K, T, alpha = 3, 16, 5, 0.8
    env, U, E = _inputs(oracle, track, ncars, K, T, 7)
    rng = np.random.default_rng(8)
    cs = 2 * ncars * T
    A = rng.standard_normal((cs, cs))
    Sinv, Uo = A @ A.T / cs + np.eye(cs), rng.uniform(-0.3, 0.3, cs)
    pol = oracle.OraclePolicy("gmppi", env, K, T, lam=10.0, alpha=alpha, U0=np.zeros(2 * ncars), cov=np.tile([0.0625, 0.1], ncars), N=1)
    ref = pol.simulate_model(U, E.T, Sigma_inv=Sinv, U_orig=Uo)
    fleet = np.tile(oracle.car_default_params(), (ncars, 1))
    got = fref.fleet_rollout(oracle, fleet, track, env.state, U, E, gamma=10.0 * (1 - alpha), Sigma_inv=Sinv, U_orig=Uo)
    assert np.max(np.abs(got - ref) / np.abs(ref)) <= 1e-12


@pytest.mark.parametrize("ncars", [2, 3, 5, 8])
def test_the_graded_fleet_moves_every_car_but_the_first(oracle, track, ncars):
    """what lets the GPU cases tell the cars apart: against the default-parameter trajectory, some state of every car c >= 1 moves by > 0.1"""
    K, T = 16, 9
    env, U, E = _inputs(oracle, track, ncars, K, T, 200 + ncars)
    base = oracle.car_default_params()
    fleet = fref.graded_fleet(ncars, base)
    assert np.array_equal(fleet[0], base) and np.all(fleet[:, 18:] == base[18:])
    _, tr0 = fref.fleet_rollout(oracle, np.tile(base, (ncars, 1)), track, env.state, U, E, log=True)
    _, tr1 = fref.fleet_rollout(oracle, fleet, track, env.state, U, E, log=True)
    moved = np.max(np.abs(tr1 - tr0).reshape(K * T, ncars, 8), axis=(0, 2))
    assert moved[0] == 0.0                                           # (car 0 keeps the defaults, and no car's dynamics see another car)
    assert np.all(moved[1:] > 0.1), moved


def test_prototype_symbol_and_null_handle():
    from mpopis_amd import build, _lib
    hdr = open(os.path.join(ROOT, "include", "mpopis.h")).read()
    assert re.search(r"int\s+mpopis_set_env_params_cars\(mpopis_handle \*h, const double \*p[^,]*, int32_t n[^,]*, int32_t per_slot\);", hdr)
    assert "#define MPOPIS_ABI_VERSION 5" in hdr
    assert "mpopis_set_env_params_cars" in _lib.ABI_SYMBOLS
    build.build()
    L = _lib.lib()
    assert L.mpopis_set_env_params_cars(None, None, 20, 0) == _lib.ERR_ARG


def _bare_engine(L, B=2, ncars=3, kind="car"):
    from mpopis_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.L, e.B, e.as_, e.env_kind, e._h = L, B, 2 * ncars, kind, None
    return e


def test_python_refusals_come_before_the_library():
    from mpopis_amd._lib import MPOPISError, ERR_ARG

    def reached(*a):
        raise AssertionError("the library was reached")
    with pytest.raises(MPOPISError, match="predates per-car env parameters") as ei:
        _bare_engine(types.SimpleNamespace()).set_env_params_cars(np.ones((3, 20)))
    assert ei.value.code == ERR_ARG
    L = types.SimpleNamespace(mpopis_set_env_params_cars=reached)
    for bad in (np.ones(20), np.ones((2, 20)), np.ones((3, 19)), np.ones((3, 3, 20)), np.ones((2, 3, 20, 1)), np.ones((2, 2, 20))):
        with pytest.raises(MPOPISError, match="shape") as ei:
            _bare_engine(L).set_env_params_cars(bad)
        assert ei.value.code == ERR_ARG
    with pytest.raises(MPOPISError, match="car handle"):
        _bare_engine(L, kind="mountaincar").set_env_params_cars(np.ones((3, 20)))
    for good in (np.ones((3, 20)), np.ones((2, 3, 20))):              # the accepted shapes do reach it
        with pytest.raises(AssertionError, match="reached"):
            _bare_engine(L).set_env_params_cars(good)


def test_multicar_env_car_params_list():
    from mpopis_amd.envs import fleet_from_car_params, CarRacingEnvParams, MultiCarRacingEnv
    from mpopis_amd._lib import MPOPISError
    d = CarRacingEnvParams().vector(0.1, 0.01)
    assert fleet_from_car_params(3, [], 0.1, 0.01) is None
    heavy = CarRacingEnvParams(m=3000.0)
    v = d.copy()
    v[9] = 0.5
    fl = fleet_from_car_params(4, [heavy, v], 0.1, 0.01)
    assert fl.shape == (4, 20)
    assert fl[0, 0] == 3000.0 and np.array_equal(fl[0, 1:], d[1:])
    assert np.array_equal(fl[1], v)
    assert np.array_equal(fl[2], d) and np.array_equal(fl[3], d)      # the cars past the list: the defaults
    assert np.array_equal(fleet_from_car_params(2, [heavy], 0.2, 0.02)[:, 18:], [[0.2, 0.02]] * 2)
    with pytest.raises(MPOPISError, match="Car parameters must be ≤ # cars"):
        fleet_from_car_params(2, [d, d, d], 0.1, 0.01)
    with pytest.raises(MPOPISError, match="20 values"):
        fleet_from_car_params(2, [d[:18]], 0.1, 0.01)
    with pytest.raises(MPOPISError, match="Car parameters must be ≤ # cars"):     # refused before any engine is made
        MultiCarRacingEnv(2, car_params=[d, d, d])


def test_simulate_car_racing_takes_one_of_the_two_keywords():
    from mpopis_amd import simulate_car_racing
    from mpopis_amd.examples import split_fleet_per_trial, shard_trials
    with pytest.raises(ValueError, match="car_params and car_fleet"):
        simulate_car_racing(num_trials=2, num_cars=3, car_params=np.ones(20), car_fleet=np.ones((3, 20)), seed=1, quiet=True)
    with pytest.raises(ValueError, match="car_fleet"):
        simulate_car_racing(num_trials=2, num_cars=3, car_fleet=np.ones((2, 20)), seed=1, quiet=True)
    assert split_fleet_per_trial(None, 3, 5) is None
    one = np.arange(60.0).reshape(3, 20)
    assert split_fleet_per_trial(one, 3, 5) is not None and np.array_equal(split_fleet_per_trial(one, 3, 5), one)
    per = np.arange(5 * 60.0).reshape(5, 3, 20)
    seen = []
    for rank in range(2):
        mine = shard_trials(5, rank, 2)
        assert np.array_equal(split_fleet_per_trial(per, 3, 5, rank, 2), per[[k - 1 for k in mine]])
        seen += mine
    assert sorted(seen) == [1, 2, 3, 4, 5]
