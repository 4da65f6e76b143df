"""A fleet on the device: every car of a multi-car slot with its own parameter vector (mpopis_set_env_params_cars).

The expectation is tests/helpers/car_fleet_ref.py: the oracle's per-car step and reward composed in the reference's order (with equal vectors it
reproduces the oracle's own multi-car simulate_model, tests/test_car_fleet_cpu.py).  The fleet of the tests grades mass, tyre grip, engine force,
steering range and β limit from car 0 (the defaults) to the last car; costs alone can hide a car reading another car's vector (the pair distances
dominate them), so every rollout case also compares the LOGGED TRAJECTORIES, which move by 0.3 .. 1.7 per car.
Tolerances are those of tests/test_gpu_parity.py and tests/test_gpu_many_cars.py: 1e-8 relative on costs and trajectories (floor 1e-9), 1e-9 on env
states and rewards, 1e-7 on a policy step's costs (run_case), integers exact."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from tests.test_gpu_baseline_shapes import start_states
from tests.test_gpu_trace import host_loop, check_steps, check_plans
from tests.helpers import slot_env_cases as SC
from tests.helpers import car_fleet_ref as fref

pytestmark = pytest.mark.gpu

RTOL = 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV = (0.0625, 0.1)


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-9)))


def two_fleets(oracle, ncars):
    """slot 0: the graded fleet; slot 1: the same cars in reverse order, integrating with δt = 0.02 (dt / δt is per slot)"""
    f0 = fref.graded_fleet(ncars, oracle.car_default_params())
    f1 = f0[::-1].copy()
    f1[:, 19] = 0.02
    return np.stack([f0, f1])


def close_starts(oracle, track, ncars, B=2):
    """as tests/test_gpu_many_cars.close_starts (slot 1: cars 0 / 1 coincident, car 2 three metres from car 0: the -11000 term), for 2 cars too"""
    env = oracle.OracleEnv("car", ncars, track=track)
    x0 = np.stack([env.state for _ in range(B)])
    x0[1, 8:10] = x0[1, 0:2]
    if ncars > 2:
        x0[1, 16] = x0[1, 0] + 3.0
        x0[1, 17] = x0[1, 1]
    for c in range(3, ncars):
        x0[1, 8 * c + 1] += 1.5 * c
        x0[1, 8 * c + 3] = 13.0
    return x0


def bounds(ncars):
    """asymmetric, different for every action of every car"""
    return -np.linspace(0.45, 1.0, 2 * ncars), np.linspace(1.0, 0.55, 2 * ncars)


def level1_inputs(rng, B, ncars, K, T):
    cs = 2 * ncars * T
    U = rng.uniform(-0.3, 0.3, (B, cs))
    U[:, 1::2] += 0.3
    E = rng.standard_normal((B, K, cs)) * np.tile([0.25, 0.32], ncars * T)
    E[0, :5] *= 8.0                                       # far-out samples: clamps, off-track, each car's own β penalty
    return U, E


def fleet_engine(eng_mod, track, fleet, ncars, K, T, B, kind="gmppi", log=False, alpha=1.0, N=1, seed=0, lo=None, hi=None):
    eng = eng_mod.Engine("car", ncars, kind, K, T, batch=B, lam=10.0, alpha=alpha, ais_its=N, lam_ais=20.0, cov=np.tile(COV, ncars), track=track,
                         log_trajectories=log, seed=seed)
    if fleet is not None:
        eng.set_env_params_cars(fleet)
    if lo is not None:
        eng.set_action_bounds(lo, hi)
    return eng


# ---- 1. rollout costs and logged trajectories --------------------------------------------------------------------------------------------------

# every num_cars in {2, 3, 5, 8}, every K in {1, 63, 64, 65, 131} (a workgroup holds 64 samples), every T in {1, 5, 9} (renormalisation every 4th step)
ROLLOUT_CASES = [(2, 1, 1, 1.0), (2, 65, 9, 1.0), (2, 131, 5, 1.0), (3, 63, 5, 1.0), (3, 64, 1, 1.0), (3, 131, 9, 0.8), (5, 64, 9, 1.0),
                 (5, 65, 5, 1.0), (5, 1, 9, 1.0), (8, 63, 1, 1.0), (8, 64, 5, 1.0), (8, 131, 9, 1.0)]


@pytest.mark.parametrize("ncars,K,T,alpha", ROLLOUT_CASES)
def test_rollout_costs_and_trajectories(eng_mod, oracle, track, ncars, K, T, alpha):
    rng = np.random.default_rng(1700 + 100 * ncars + K + T)
    B, cs = 2, 2 * ncars * T
    fleets = two_fleets(oracle, ncars)
    lo, hi = bounds(ncars)
    U, E = level1_inputs(rng, B, ncars, K, T)
    x0 = close_starts(oracle, track, ncars)
    kw, hkw = {}, [{}, {}]
    if alpha != 1.0:
        A = rng.standard_normal((cs, cs))
        kw = dict(U_orig=rng.uniform(-0.3, 0.3, (B, cs)), Sigma_inv=A @ A.T / cs + np.eye(cs))
        hkw = [dict(gamma=10.0 * (1 - alpha), Sigma_inv=kw["Sigma_inv"], U_orig=kw["U_orig"][b]) for b in range(B)]
    ref = [fref.fleet_rollout(oracle, fleets[b], track, x0[b], U[b], E[b], lo=lo, hi=hi, log=True, **hkw[b]) for b in range(B)]
    assert np.all(ref[1][0] > 10000.0)                    # the contact term is in every rollout of slot 1
    for log in (False, True):
        eng = fleet_engine(eng_mod, track, fleets, ncars, K, T, B, log=log, alpha=alpha, lo=lo, hi=hi)
        got = eng.rollout_costs(U, E, x0=x0, **kw)
        tr = eng.get_trajectories() if log else None
        eng.close()
        for b in range(B):
            ec = rel_err(got[b], ref[b][0])
            et = rel_err(tr[b], ref[b][1]) if log else 0.0
            print("[fleet level 1] cars %d K %d T %d log %d slot %d: cost %.2e traj %.2e" % (ncars, K, T, log, b, ec, et))
            assert ec < RTOL, (ncars, K, T, log, b, ec)
            assert et < RTOL, (ncars, K, T, b, et)         # fails when a car reads another car's vector


def test_the_trajectory_comparison_tells_the_cars_apart(oracle, track):
    """the premise of the case above, at the sizes it runs: a fleet whose cars 1 and 2 swap vectors is far outside the tolerance"""
    ncars, K, T = 3, 8, 9
    fleets = two_fleets(oracle, ncars)
    U, E = level1_inputs(np.random.default_rng(3), 1, ncars, K, T)
    x0 = close_starts(oracle, track, ncars)
    _, good = fref.fleet_rollout(oracle, fleets[0], track, x0[0], U[0], E[0], log=True)
    _, swapped = fref.fleet_rollout(oracle, fleets[0][[0, 2, 1]], track, x0[0], U[0], E[0], log=True)
    assert rel_err(swapped, good) > 1e-3


# ---- 2. a fleet with per-slot tracks, and a track beyond 190 points ----------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", ["small", "ring_only"])
def test_fleet_with_per_slot_tracks(eng_mod, oracle, track, sizes):
    ncars, K, T, B = 3, 65, 5, 2
    tracks = [SC.tracks3(track)[0], SC.ring(12, 80.0, 50.0)] if sizes == "small" else [SC.mixed_tracks([200])[0], SC.tracks3(track)[0]]
    tos = [1, 0]
    fleets = two_fleets(oracle, ncars)
    U, E = level1_inputs(np.random.default_rng(21), B, ncars, K, T)
    x0 = np.stack([SC.start_state(tracks[tos[b]], ncars, b) for b in range(B)])
    for order in ("fleet_first", "tracks_first"):          # the two setters are independent of each other
        eng = fleet_engine(eng_mod, None, fleets if order == "fleet_first" else None, ncars, K, T, B, log=True)
        eng.set_tracks(tracks, tos)
        if order == "tracks_first":
            eng.set_env_params_cars(fleets)
        got = eng.rollout_costs(U, E, x0=x0)
        tr = eng.get_trajectories()
        eng.close()
        for b in range(B):
            cost, traj = fref.fleet_rollout(oracle, fleets[b], tracks[tos[b]], x0[b], U[b], E[b], log=True)
            ec, et = rel_err(got[b], cost), rel_err(tr[b], traj)
            print("[fleet tracks] %s %s slot %d (P %d): cost %.2e traj %.2e" % (sizes, order, b, len(tracks[tos[b]][0]), ec, et))
            assert ec < RTOL and et < RTOL, (sizes, order, b, ec, et)


# ---- 3. an equal fleet against the oracle and against a shared handle --------------------------------------------------------------------------

@pytest.mark.parametrize("ncars", [3, 8])
def test_equal_fleet_against_the_oracle(eng_mod, oracle, track, ncars):
    K, T, B = 131, 9, 2
    U, E = level1_inputs(np.random.default_rng(31 + ncars), B, ncars, K, T)
    x0 = close_starts(oracle, track, ncars)
    env = oracle.OracleEnv("car", ncars, track=track)
    pol = oracle.OraclePolicy("gmppi", env, K, T, lam=10.0, U0=np.zeros(2 * ncars), cov=np.tile(COV, ncars), N=1, nthreads=8)
    eng = fleet_engine(eng_mod, track, np.tile(oracle.car_default_params(), (ncars, 1)), ncars, K, T, B)
    got = eng.rollout_costs(U, E, x0=x0)
    eng.close()
    eng = fleet_engine(eng_mod, track, None, ncars, K, T, B)
    shared = eng.rollout_costs(U, E, x0=x0)
    eng.close()
    for b in range(B):
        env.state = x0[b]
        assert rel_err(got[b], pol.simulate_model(U[b], E[b].T)) < RTOL, (ncars, b)
    # (not a pass condition: the two handles run different rollout bodies)
    print("[fleet equal] cars %d: costs of the equal fleet %s those of a handle without one (max rel %.2e)"
          % (ncars, "EQUAL bit for bit" if np.array_equal(got, shared) else "DIFFER in the last bits from", rel_err(got, shared)))


# ---- 4. env_step / env_query -------------------------------------------------------------------------------------------------------------------

def test_env_step_and_query_heterogeneous_eight_cars(eng_mod, oracle, track):
    ncars, B = 8, 2
    rng = np.random.default_rng(8)
    fleets = two_fleets(oracle, ncars)
    eng = fleet_engine(eng_mod, track, fleets, ncars, 16, 4, B)
    x0 = close_starts(oracle, track, ncars)
    x0[1, 8 * 7] += 40.0                                  # car 7 of slot 1 off the track
    eng.set_state(x0)
    s = [x0[b].reshape(ncars, 8).copy() for b in range(B)]
    for step in range(6):
        a = np.clip(rng.uniform(-0.5, 0.9, (B, 2 * ncars)), -1, 1)
        rew = eng.env_step(a)
        r_q, within, dist, beta = eng.env_query()
        xs = eng.get_state()[0]
        for b in range(B):
            s[b] = fref.fleet_step(oracle, fleets[b], s[b], a[b])
            ref_rew = fref.fleet_reward(oracle, fleets[b], track, s[b])
            assert abs(rew[b] - ref_rew) <= 1e-9 * max(1.0, abs(ref_rew)), (step, b, rew[b], ref_rew)
            assert abs(r_q[b] - ref_rew) <= 1e-9 * max(1.0, abs(ref_rew))
            assert np.max(np.abs(xs[b] - s[b].reshape(-1))) < 1e-9
            win = [oracle.within_track(track, s[b][c, :2]) for c in range(ncars)]
            assert bool(within[b]) == all(w[0] for w in win)
            assert np.max(np.abs(dist[b] - [w[1] for w in win])) < 1e-9
            assert np.max(np.abs(beta[b] - np.arctan2(s[b][:, 4], s[b][:, 3]))) < 1e-12
    assert not within[1]
    eng.close()


def test_env_step_and_query_equal_fleet_returns_the_bits_of_a_shared_handle(eng_mod, oracle, track):
    ncars, B = 8, 2
    x0 = close_starts(oracle, track, ncars)
    out = []
    for fleet in (None, np.tile(oracle.car_default_params(), (B, ncars, 1))):
        rng = np.random.default_rng(9)
        eng = fleet_engine(eng_mod, track, fleet, ncars, 16, 4, B)
        eng.set_state(x0)
        rec = []
        for step in range(4):
            rec.append(eng.env_step(np.clip(rng.uniform(-0.5, 0.9, (B, 2 * ncars)), -1, 1)))
            rec += list(eng.env_query()) + [eng.get_state()[0]]
        eng.close()
        out.append(rec)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 5. policy steps with injected noise -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["gmppi", "musigmaaismppi"])
def test_policy_step_and_plan(eng_mod, oracle, track, kind):
    ncars, K, T, N, B, top = 3, 160, 8, 3, 2, 4
    cs = 2 * ncars * T
    fleets = two_fleets(oracle, ncars)
    x0 = start_states(oracle, track, ncars, B)
    eng = fleet_engine(eng_mod, track, fleets, ncars, K, T, B, kind=kind, N=N, seed=5)
    eng.set_state(x0)
    rng = np.random.default_rng(55)
    Neff = 1 if kind == "gmppi" else N
    for step in range(2):
        U_orig = eng.get_U()
        Z = rng.standard_normal((B, Neff, K, cs))
        got = eng.policy_step(Z, want_E=True)
        plan = eng.get_plan(top)
        for b in range(B):
            E_out = got["E"][b]                                                    # (K, cs): the last iteration rolled out U_orig + E_out[k]
            cost, traj = fref.fleet_rollout(oracle, fleets[b], track, x0[b], U_orig[b], E_out, log=True)
            ec = rel_err(got["cost"][b], cost)
            wc = U_orig[b] + got["weights"][b] @ E_out
            eu = float(np.max(np.abs(got["control"][b] - np.clip(wc[:2 * ncars], -1.0, 1.0))))
            assert ec < 1e-7 and eu < 1e-9, (kind, step, b, ec, eu)
            _, ptraj = fref.fleet_rollout(oracle, fleets[b], track, x0[b], plan["controls"][b], np.zeros((1, cs)), log=True)
            e0 = rel_err(plan["traj"][b, 0], ptraj[0])
            ej = max(rel_err(plan["traj"][b, j], traj[plan["idx0"][b, j - 1]]) for j in range(1, top + 1))
            print("[fleet policy] %s step %d slot %d: cost %.2e control %.2e plan %.2e samples %.2e" % (kind, step, b, ec, eu, e0, ej))
            assert e0 < RTOL and ej < RTOL, (kind, step, b, e0, ej)
            assert np.max(np.abs(plan["controls"][b] - wc)) < 1e-9
        eng.env_step(got["control"])
        x0 = eng.get_state()[0]
    eng.close()


# ---- 6. the closed loop ------------------------------------------------------------------------------------------------------------------------

def test_closed_loop_trace_and_own_beta_limits(eng_mod, oracle, track):
    ncars, K, T, N, B, ns, top = 3, 64, 8, 3, 2, 12, 2
    fleets = two_fleets(oracle, ncars)
    fleets[1, 1, 17] = 0.03                                # car 1 of slot 1: a β limit its side slip passes while far below the default 0.785
    x0 = start_states(oracle, track, ncars, B)
    x0[1, 8 + 4] = 2.0                                    # ... Vy = 2 m/s at 15 m/s: β is 0.075 .. 0.14 after the first step whatever the action

    def make(overlap):
        eng = fleet_engine(eng_mod, track, fleets, ncars, K, T, B, kind="musigmaaismppi", N=N, seed=61)
        eng.set_overlap(overlap)
        eng.set_state(x0)
        return eng

    eng = make(4)
    rec, acts, tr = eng.run_trials(num_steps=ns, laps=2, log_actions=True, trace=dict(plan_every=4, top=top))
    eng.close()
    eng = make(1)
    rec0, acts0 = eng.run_trials(num_steps=ns, laps=2, log_actions=True)
    eng.close()
    eng = make(1)
    ref = host_loop(eng, ns, top, plan_every=4)
    eng.close()
    assert np.all(rec[:, 15] == 0) and np.array_equal(rec, rec0) and np.array_equal(acts, acts0)
    for b in range(B):
        n = int(tr["steps_run"][b])
        assert np.array_equal(acts[b, :n], ref["actions"][b, :n])
    check_steps(tr, ref, "fleet")
    check_plans(tr, ref, top, "fleet")
    # the driven steps against the helper (1e-9, as env_step above)
    for b in range(B):
        for s in range(int(tr["steps_run"][b])):
            nxt = fref.fleet_step(oracle, fleets[b], tr["states"][b, s].reshape(ncars, 8), np.clip(acts[b, s], -1.0, 1.0))
            assert np.max(np.abs(tr["states"][b, s + 1] - nxt.reshape(-1))) < 1e-9, (b, s)
    # car 1 of slot 1 passed ITS limit below the default one, and records[11] counts by every car's own limit
    n1 = int(tr["steps_run"][1])
    b1 = np.abs(tr["beta"][1, :n1, 1])
    assert np.any((b1 > 0.03) & (b1 < oracle.car_default_params()[17])), b1
    for b in range(B):
        n = int(tr["steps_run"][b])
        over = np.any(np.abs(tr["beta"][b, :n]) > fleets[b][:, 17], axis=1)
        assert rec[b, 11] == np.sum(over & (tr["rewards"][b, :n] < -4000)), (b, rec[b, 11])
    assert rec[1, 11] >= 1
    default_over = np.any(np.abs(tr["beta"][1, :n1]) > oracle.car_default_params()[17], axis=1)
    assert rec[1, 11] > np.sum(default_over & (tr["rewards"][1, :n1] < -4000))          # the shared limit would have counted fewer


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals_and_the_way_back(eng_mod, oracle, track):
    from mpopis_amd import build, _lib
    from mpopis_amd._lib import MPOPISError, ERR_ARG
    ncars, K, T, B = 3, 64, 5, 2
    cs = 2 * ncars * T
    fleets = two_fleets(oracle, ncars)
    x0 = start_states(oracle, track, ncars, B)
    Z = np.random.default_rng(7).standard_normal((B, 1, K, cs))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def step(eng):
        eng.set_state(x0)
        eng.set_U(np.zeros((B, cs)))
        g = eng.policy_step(Z, want_E=True)
        return g["control"].copy(), g["cost"].copy(), g["weights"].copy()

    eng = fleet_engine(eng_mod, track, fleets, ncars, K, T, B)
    first = step(eng)

    def refused(word, p, n=20, per_slot=1):
        assert eng.L.mpopis_set_env_params_cars(eng._h, None if p is None else dp(p), n, per_slot) == ERR_ARG
        msg = eng.L.mpopis_last_error(eng._h).decode()
        assert word in msg, msg

    flat = np.ascontiguousarray(fleets)
    refused("p is NULL", None)
    refused("20 parameters", flat, n=19)
    bad = flat.copy()
    bad[1, 2, 18] = 0.2                                   # dt of slot 1, car 2
    refused("slot 1, car 2", bad)
    bad = flat.copy()
    bad[0, 1, 19] = 0.02                                  # δt of slot 0, car 1
    refused("slot 0, car 1", bad)
    refused("slot 0, car 1", np.ascontiguousarray(bad[0]), per_slot=0)
    with pytest.raises(MPOPISError) as ei:
        eng.set_env_params_cars(bad)
    assert ei.value.code == ERR_ARG
    for a, b in zip(step(eng), first):                    # every refused call left the handle as it was
        assert np.array_equal(a, b)
    # a fleet really is in force (the defaults give other costs), per_slot = 0 gives every slot the same fleet, and set_env_params leads back
    eng.set_env_params_cars(fleets[0])
    same = step(eng)
    assert np.array_equal(same[1][0], first[1][0]) and not np.array_equal(same[1][1], first[1][1])
    eng.set_env_params(oracle.car_default_params())
    back = step(eng)
    fresh_eng = fleet_engine(eng_mod, track, None, ncars, K, T, B)
    fresh = step(fresh_eng)
    for a, b in zip(back, fresh):
        assert np.array_equal(a, b)
    assert not np.array_equal(fresh[1], first[1])
    # set_env_params_slots leads back as well: one vector per slot, the bits of a handle that never had a fleet
    per_slot = np.stack([fleets[0, 1], fleets[0, 2]])
    eng.set_env_params_cars(fleets)
    eng.set_env_params_slots(per_slot)
    fresh_eng.set_env_params_slots(per_slot)
    for a, b in zip(step(eng), step(fresh_eng)):
        assert np.array_equal(a, b)
    eng.close()
    fresh_eng.close()
    # other env kinds and a custom handle
    mc = eng_mod.Engine("mountaincar", 0, "gmppi", 16, 4, batch=1, lam=1.0, cov=[1.5])
    assert mc.L.mpopis_set_env_params_cars(mc._h, dp(flat), 20, 0) == ERR_ARG and "not a car handle" in mc.L.mpopis_last_error(mc._h).decode()
    mc.close()
    from tests.helpers import pointmass_ref as PM
    cenv = types.SimpleNamespace(code_object=build.build_env(os.path.join(ROOT, "tests", "helpers", "envs", "pointmass_sdk.hip")), state_size=PM.SS,
                                 action_size=PM.AS, params=np.array(PM.PARAMS, dtype=np.float64), lo=PM.LO, hi=PM.HI, reset_state=None)
    cu = eng_mod.Engine("custom", 0, "gmppi", 16, 4, batch=1, lam=1.0, cov=[0.3, 0.3, 0.1], custom_env=cenv)
    assert cu.L.mpopis_set_env_params_cars(cu._h, dp(flat), 20, 0) == ERR_ARG and "custom handle" in cu.L.mpopis_last_error(cu._h).decode()
    cu.close()


def test_one_car_handle_takes_the_existing_forms(eng_mod, oracle, track):
    K, T, B = 65, 5, 2
    p = np.stack([oracle.car_default_params() for _ in range(B)])
    p[1, 0] *= 1.3
    p[1, 9] = 0.7
    U, E = level1_inputs(np.random.default_rng(71), B, 1, K, T)
    x0 = start_states(oracle, track, 1, B)
    res = []
    for how in ("cars", "slots", "cars_shared", "shared"):
        eng = fleet_engine(eng_mod, track, None, 1, K, T, B)
        if how == "cars":
            eng.set_env_params_cars(p[:, None, :])
        elif how == "slots":
            eng.set_env_params_slots(p)
        elif how == "cars_shared":
            eng.set_env_params_cars(p[1][None, :])
        else:
            eng.set_env_params(p[1])
        res.append(eng.rollout_costs(U, E, x0=x0))
        eng.close()
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[2], res[3])
    assert not np.array_equal(res[0][0], res[2][0])


# ---- 8. the Python harness ---------------------------------------------------------------------------------------------------------------------

def test_simulate_car_racing_with_a_fleet(eng_mod, oracle):
    from mpopis_amd import examples
    fleet = fref.graded_fleet(3, oracle.car_default_params())
    kw = dict(num_trials=2, num_steps=10, num_cars=3, policy_type=":cemppi", num_samples=64, horizon=8, ais_its=2, seed=5, quiet=True)
    rec, summ = examples.simulate_car_racing(car_fleet=fleet, **kw)
    assert rec.shape == (2, 18) and np.all(rec[:, 2] >= 1)
    assert summ["AVE"].shape == (3 + 2 + 6 + 1 + 1,)
    rec2, _ = examples.simulate_car_racing(car_fleet=np.stack([fleet, fleet[::-1]]), **kw)
    assert np.array_equal(rec2[0, 1:17], rec[0, 1:17]) and not np.array_equal(rec2[1, 1:17], rec[1, 1:17])     # trial 2 drove the other fleet
    rec0, _ = examples.simulate_car_racing(**kw)
    assert not np.array_equal(rec0[:, 1:17], rec[:, 1:17])                                                      # ... and the defaults drive differently
