"""Scenario rollouts and risk costs (mpopis_set_scenarios / mpopis_set_risk / mpopis_get_scenario_costs) at the engine level.

What is compared.  (1) every scenario's costs against rollout_costs of a PLAIN handle given that scenario's vectors through
set_env_params_slots -- the per-slot kernels that exist without the feature -- bit for bit, and for the one-car case against the CPU oracle under
each scenario's parameters (RTOL = 1e-8, the Level-1 tolerance of tests/test_gpu_parity.py); (2) the `cost` output against
mpopis_amd.scenarios.aggregate of those scenario costs in long double, to the bounds derived in tests/helpers/risk_cases.py; (3) a handle whose
scenarios are copies of each slot's own parameters against the plain per-slot handle, bit for bit, on all nine policies; (4) weights and control
of a step with distinct scenarios against the oracle's compute_weights and the clamped U + E w (1e-9 and 1e-8, the tolerances of
tests/test_gpu_parity.py::test_level2_policy_step for those two quantities); (5) plan and closed loop with model != plant against handles that
hold the model and the plant separately; (6) both schedules; (7) the setter's refusals and its way back."""
import numpy as np
import pytest

from tests.helpers import risk_cases as R
from tests.helpers import slot_env_cases as SC

pytestmark = pytest.mark.gpu

RTOL = 1e-8          # tests/test_gpu_parity.py: Level-1 costs against the oracle
POLICIES = ["mppi", "gmppi", "imppi", "cemppi", "cmamppi", "muaismppi", "musigmaaismppi", "pmcmppi", "nesmppi"]


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


def car_models(oracle, B, M):
    """(B, M, 20): scenario 0 the defaults, 1 a car 20 % heavier, 2 one 20 % lighter on tyres with 0.7 of the friction, later ones in between;
    C_alpha_f grows by 3 % per slot so that the slots differ too"""
    base = oracle.car_default_params()
    p = np.tile(base, (B, M, 1))
    for m in range(M):
        if m % 3 == 1:
            p[:, m, 0] *= 1.2 - 0.02 * (m // 3)
        if m % 3 == 2:
            p[:, m, 0] *= 0.8 + 0.02 * (m // 3)
            p[:, m, 9] *= 0.7
            p[:, m, 10] *= 0.7
    for b in range(B):
        p[b, :, 7] *= 1.0 + 0.03 * b
    return p


def _car_engine(eng_mod, nc, K, T, B, track, kind="gmppi", alpha=1.0, **kw):
    return eng_mod.Engine("car", nc, kind, K, T, batch=B, lam=10.0, alpha=alpha, cov=np.tile(SC.COV, nc), track=track, **kw)


def _car_case(eng_mod, track, nc, K, T, B, p, per_slot, seed, tracks=None, alpha=1.0):
    """rollout_costs of a scenario handle and, per scenario, of a plain handle given that scenario's vectors per slot: everything the tests of
    (1) and (2) look at, computed once"""
    rng = np.random.default_rng(seed)
    U, E = SC.level1_inputs(rng, B, nc, K, T)
    trk_of = (lambda b: tracks[b]) if tracks else (lambda b: track)
    x0 = np.stack([SC.start_state(trk_of(b), nc, b) for b in range(B)])
    extra = {}
    if alpha != 1.0:
        cs = 2 * nc * T
        A = rng.standard_normal((cs, cs))
        extra = dict(U_orig=rng.uniform(-0.3, 0.3, (B, cs)), Sigma_inv=A @ A.T / cs + np.eye(cs))
    pfull = p if per_slot else np.tile(p, (B, 1, 1))
    M = pfull.shape[1]

    def make():
        eng = _car_engine(eng_mod, nc, K, T, B, None if tracks else track, alpha=alpha)
        if tracks:
            eng.set_tracks(tracks)
        return eng
    eng = make()
    eng.set_scenarios(p, per_slot=per_slot)
    out = dict(U=U, E=E, x0=x0, p=pfull, M=M, agg={})
    out["cost_mean"] = eng.rollout_costs(U, E, x0=x0, **extra)
    out["sc"] = eng.get_scenario_costs()
    for name, kw in (("worst", {}), ("cvar", dict(tail=2)), ("entropic", dict(theta=1e-3)), ("entropic", dict(theta=-1e-3))):
        if name == "cvar" and M < 3:
            continue
        eng.set_risk(name, **kw)
        c = eng.rollout_costs(U, E, x0=x0, **extra)
        assert np.array_equal(eng.get_scenario_costs(), out["sc"])          # the risk changes the aggregate, never the scenario costs
        out["agg"][(name, kw.get("tail", 0), kw.get("theta", 0.0))] = c
    eng.close()
    plain = make()
    out["ref"] = []
    for m in range(M):
        plain.set_env_params_slots(pfull[:, m])
        out["ref"].append(plain.rollout_costs(U, E, x0=x0, **extra))
    plain.close()
    return out


def _check_case(c, label):
    assert c["sc"].shape == c["cost_mean"].shape[:1] + (c["M"],) + c["cost_mean"].shape[1:]
    for m in range(c["M"]):
        assert np.array_equal(c["sc"][:, m], c["ref"][m]), (label, m)
    worst = {}
    r = R.check_aggregate(c["cost_mean"], c["sc"], "mean")
    worst["mean"] = r
    for (name, tail, theta), got in c["agg"].items():
        if name == "worst":
            assert np.array_equal(got, c["sc"].max(axis=1)), label                       # exact: the bits of the largest input
        worst["%s %s" % (name, tail or theta)] = R.check_aggregate(got, c["sc"], name, tail, theta)
    for k, r in worst.items():
        print("RATIO engine_%s %.4f  (%s)" % (k.split()[0], r, label))
        assert r <= 1.0, (label, k, r)


# ---- 1 + 2. scenario costs are the per-slot kernels' costs; the aggregate ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def one_car(eng_mod, oracle, track):
    return _car_case(eng_mod, track, 1, 96, 6, 3, car_models(oracle, 3, 3), True, seed=41)


def test_one_car_scenarios_are_the_per_slot_costs(one_car):
    _check_case(one_car, "car x1 K 96 T 6 B 3 M 3 per slot")
    sc = one_car["sc"]
    for b in range(3):                                           # the scenarios really differ: mass and friction move a good part of the costs
        assert np.mean(sc[b, 0] != sc[b, 1]) > 0.5 and np.mean(sc[b, 0] != sc[b, 2]) > 0.5
        assert np.max(np.abs(sc[b, 0] - sc[b, 2]) / (np.abs(sc[b, 0]) + 1e-9)) > 1e-3
    assert not np.array_equal(sc[0], sc[1])


def test_one_car_scenarios_against_the_oracle(one_car, oracle, track):
    c = one_car
    for b in range(3):
        for m in range(3):
            env = oracle.OracleEnv("car", 1, params=c["p"][b, m], track=track)
            env.state = c["x0"][b]
            pol = oracle.OraclePolicy("gmppi", env, 96, 6, lam=10.0, U0=np.zeros(2), cov=np.array(SC.COV))
            ref = pol.simulate_model(c["U"][b], c["E"][b].T)
            assert SC.rel_err(c["sc"][b, m], ref) < RTOL, (b, m, SC.rel_err(c["sc"][b, m], ref))


def test_two_cars_shared_scenarios(eng_mod, oracle, track):
    _check_case(_car_case(eng_mod, track, 2, 70, 5, 2, car_models(oracle, 1, 2)[0], False, seed=42), "car x2 K 70 T 5 B 2 M 2 shared")


def test_scenarios_on_two_per_slot_tracks(eng_mod, oracle, track):
    tracks = [tuple(np.ascontiguousarray(v, dtype=np.float64) for v in track), SC.ring(12, 80.0, 50.0)]
    _check_case(_car_case(eng_mod, track, 1, 65, 5, 2, car_models(oracle, 2, 3), True, seed=43, tracks=tracks), "car x1 two tracks")


def test_scenarios_with_a_control_cost(eng_mod, oracle, track):
    _check_case(_car_case(eng_mod, track, 1, 65, 5, 2, car_models(oracle, 2, 2), True, seed=44, alpha=0.5), "car x1 alpha 0.5 with Sigma_inv")


def _simple_models(oracle, kind, B, M):
    base = oracle.mountaincar_default_params() if kind == "mountaincar" else oracle.cartpole_default_params()
    p = np.tile(base, (B, M, 1))
    for m in range(M):
        if kind == "mountaincar":
            p[:, m, 5] *= 1.0 + 0.15 * m                         # power
            p[:, m, 6] *= 1.0 - 0.05 * m                         # gravity
        else:
            p[:, m, 6] *= 1.0 + 0.2 * m                          # force_mag
            p[:, m, 2] *= 1.0 + 0.3 * m                          # masspole
            p[:, m, 3] = p[:, m, 1] + p[:, m, 2]
            p[:, m, 5] = p[:, m, 2] * p[:, m, 4]
    for b in range(B):
        p[b, :, 5 if kind == "mountaincar" else 6] *= 1.0 + 0.02 * b
    return p


@pytest.mark.parametrize("kind", ["mountaincar", "cartpole"])
def test_simple_env_scenarios(eng_mod, oracle, kind):
    K, T, B, M = 65, 8, 2, 4
    rng = np.random.default_rng(45)
    p = _simple_models(oracle, kind, B, M)
    x0 = np.array([[-0.5, 0.0], [-0.45, 0.01]]) if kind == "mountaincar" else 0.05 * rng.standard_normal((B, 4))
    U = rng.uniform(-0.3, 0.3, (B, T))
    E = rng.standard_normal((B, K, T)) * 1.2
    make = lambda: eng_mod.Engine(kind, 0, "gmppi", K, T, batch=B, lam=0.1, cov=[1.5])
    eng = make()
    eng.set_scenarios(p, per_slot=True)
    c = dict(M=M, agg={})
    c["cost_mean"] = eng.rollout_costs(U, E, x0=x0)
    c["sc"] = eng.get_scenario_costs()
    eng.set_risk("cvar", tail=2)
    c["agg"][("cvar", 2, 0.0)] = eng.rollout_costs(U, E, x0=x0)
    eng.close()
    plain = make()
    c["ref"] = []
    for m in range(M):
        plain.set_env_params_slots(p[:, m])
        c["ref"].append(plain.rollout_costs(U, E, x0=x0))
    plain.close()
    _check_case(c, kind)
    assert not np.array_equal(c["sc"][:, 0], c["sc"][:, M - 1])


# ---- 3 + 6. identical scenarios change nothing, on every policy and in both schedules -----------------------------------------------------------

def _policy_engine(eng_mod, track, kind, B=2, K=96, T=5, N=3, **kw):
    return eng_mod.Engine("car", 1, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cma_sigma=0.75,
                          cov=[0.0625, 0.1], track=track, seed=515, **kw)


def _steps_and_trials(eng, x0, kind):
    eng.set_state(x0)
    res = []
    for _ in range(2):
        g = eng.policy_step(None)
        res += [g["control"].copy(), g["cost"].copy(), g["weights"].copy(), eng.get_U(), g["iters_run"].copy()]
        if kind != "mppi":
            res.append(eng.get_Sigma())
    rec, act = eng.run_trials(6, 2, log_actions=True)
    return res + [rec[:, :15], act]


def _slot_params(oracle, B):
    p = np.tile(oracle.car_default_params(), (B, 1))
    for b in range(B):
        p[b, 0] *= 1.0 + 0.1 * b
        p[b, 9] *= 1.0 - 0.1 * b
    return p


VARIANTS = [("mean", 1, {}), ("mean", 2, {}), ("mean", 4, {}), ("worst", 3, {}), ("entropic", 2, dict(theta=0.5))]


@pytest.mark.parametrize("kind", POLICIES)
def test_identical_scenarios_change_nothing(eng_mod, oracle, track, kind):
    B = 2
    ps = _slot_params(oracle, B)
    x0 = np.stack([SC.start_state(track, 1, b) for b in range(B)])
    overlaps = (4, 1) if kind == "musigmaaismppi" else (0,)     # (6): the two settings of tests/test_gpu_persistent_chains.py
    for overlap in overlaps:
        plain = _policy_engine(eng_mod, track, kind)
        plain.set_overlap(overlap)
        plain.set_env_params_slots(ps)
        ref = _steps_and_trials(plain, x0, kind)
        plain.close()
        assert np.all(np.isfinite(ref[0])) and not np.array_equal(ref[1][0], ref[1][1])
        for risk, M, kw in VARIANTS:
            eng = _policy_engine(eng_mod, track, kind)
            eng.set_overlap(overlap)
            eng.set_env_params_slots(ps)
            eng.set_scenarios(np.repeat(ps[:, None, :], M, axis=1), per_slot=True)
            eng.set_risk(risk, **kw)
            got = _steps_and_trials(eng, x0, kind)
            eng.close()
            # (entropic: c* + log(mean(exp(0))) / theta = c* + log(1) / theta = c*, exact as well)
            for i, (a, b) in enumerate(zip(got, ref)):
                assert np.array_equal(a, b), (kind, overlap, risk, M, i)


# ---- 4. distinct scenarios steer the step -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mppi", "gmppi"])
def test_distinct_scenarios_steer_the_step(eng_mod, oracle, track, kind):
    B, K, T, M, lam = 2, 96, 6, 3, 10.0
    cs = 2 * T
    rng = np.random.default_rng(46)
    p = car_models(oracle, B, M)
    x0 = np.stack([SC.start_state(track, 1, b) for b in range(B)])
    Z = rng.standard_normal((B, T, K, 2)) if kind == "mppi" else rng.standard_normal((B, 1, K, cs))
    outs = {}
    for risk in ("mean", "worst"):
        eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, lam=lam, cov=[0.0625, 0.1], track=track, seed=3)
        eng.set_scenarios(p, per_slot=True)
        eng.set_risk(risk)
        eng.set_state(x0)
        U0 = rng.uniform(-0.2, 0.2, (B, cs))
        U0[:, 1::2] += 0.3
        eng.set_U(U0)
        g = eng.policy_step(Z, want_E=True)
        sc = eng.get_scenario_costs()
        eng.close()
        assert R.check_aggregate(g["cost"], sc, risk) <= 1.0
        for b in range(B):
            w = oracle.compute_weights(lam, g["cost"][b])
            assert np.max(np.abs(g["weights"][b] - w)) < 1e-9
            E = g["E"][b].reshape(-1, cs) if kind != "mppi" else g["E"][b].transpose(1, 0, 2).reshape(K, cs)     # (K, cs): sample k's noise
            ctrl = np.clip((U0[b] + w @ E)[:2], -1.0, 1.0)
            assert np.max(np.abs(g["control"][b] - ctrl)) < 1e-8, (kind, risk, b, g["control"][b], ctrl)
        outs[risk] = g
    assert not np.array_equal(outs["mean"]["control"], outs["worst"]["control"])       # the risk steers: same noise, another control


# ---- 5. model != plant ----------------------------------------------------------------------------------------------------------------------------

def test_plan_rolls_under_scenario_zero_not_under_the_plant(eng_mod, oracle, track):
    B = 2
    p0 = _slot_params(oracle, B)
    q = p0.copy()
    q[:, 0] *= 1.3
    q[:, 9] *= 0.6
    q[:, 10] *= 0.6
    x0 = np.stack([SC.start_state(track, 1, b) for b in range(B)])
    S = _policy_engine(eng_mod, track, "cemppi")
    S.set_env_params_slots(q)
    S.set_scenarios(np.repeat(p0[:, None, :], 2, axis=1), per_slot=True)
    P = _policy_engine(eng_mod, track, "cemppi")
    P.set_env_params_slots(p0)
    Q = _policy_engine(eng_mod, track, "cemppi")
    Q.set_env_params_slots(q)
    res = []
    for eng in (S, P, Q):
        eng.set_state(x0)
        g = eng.policy_step(None)
        plan = eng.get_plan(top=2)
        res.append((g, plan))
        eng.close()
    (gS, plS), (gP, plP), (gQ, plQ) = res
    for k in ("control", "cost", "weights", "iters_run"):
        assert np.array_equal(gS[k], gP[k]), k
    for k in plP:
        assert np.array_equal(plS[k], plP[k]), k
    assert not np.array_equal(plS["traj"], plQ["traj"]) and not np.array_equal(gS["cost"], gQ["cost"])     # q would have shown


def test_traced_closed_loop_plans_with_the_model_and_drives_the_plant(eng_mod, oracle, track):
    """run_trials(trace=...) on S (plant q, scenarios {p0, p0}) against the host loop: policy_step on P (parameters p0) at the state the plant is in,
    env_step on Q (parameters q) -- the way tests/test_gpu_trace.py compares the resident loop with the host loop, with model and plant on two handles"""
    B, ns = 2, 6
    p0 = _slot_params(oracle, B)
    q = p0.copy()
    q[:, 0] *= 1.3
    q[:, 9] *= 0.6
    q[:, 10] *= 0.6
    x0 = np.stack([SC.start_state(track, 1, b) for b in range(B)])
    S = _policy_engine(eng_mod, track, "musigmaaismppi")
    S.set_env_params_slots(q)
    S.set_scenarios(np.repeat(p0[:, None, :], 2, axis=1), per_slot=True)
    S.set_state(x0)
    rec, acts, tr = S.run_trials(num_steps=ns, laps=2, log_actions=True, trace=dict(plan_every=3, top=2))
    S.close()
    P = _policy_engine(eng_mod, track, "musigmaaismppi")
    P.set_env_params_slots(p0)
    Q = _policy_engine(eng_mod, track, "musigmaaismppi")
    Q.set_env_params_slots(q)
    x = x0.copy()
    Q.set_state(x)
    n_run = tr["steps_run"]
    assert np.all(n_run == ns + 1)                               # nobody leaves the track in seven steps: every slot is compared at every step
    for s in range(ns + 1):
        assert np.array_equal(tr["states"][:, s], x), s
        P.set_state(x)
        g = P.policy_step(None)
        if s % 3 == 0:
            plan = P.get_plan(top=2)
            j = s // 3
            assert np.array_equal(tr["plan_traj"][:, j], plan["traj"]) and np.array_equal(tr["plan_controls"][:, j], plan["controls"]), s
            assert np.array_equal(tr["plan_cost"][:, j], plan["cost"]) and np.array_equal(tr["plan_idx0"][:, j], plan["idx0"]), s
        assert np.array_equal(acts[:, s], g["control"]), s
        assert np.array_equal(tr["iters"][:, s], g["iters_run"]), s
        rew = Q.env_step(g["control"])
        assert np.array_equal(tr["rewards"][:, s], rew), s
        x = Q.get_state()[0]
    assert np.array_equal(tr["states"][:, ns + 1], x)
    P.close()
    # ... and the plant is q, not p0: the same controls on P's parameters drive elsewhere
    P2 = _policy_engine(eng_mod, track, "musigmaaismppi")
    P2.set_env_params_slots(p0)
    P2.set_state(x0)
    P2.env_step(acts[:, 0])
    assert not np.array_equal(P2.get_state()[0], tr["states"][:, 1])
    P2.close()
    Q.close()


# ---- 7. the setter ----------------------------------------------------------------------------------------------------------------------------------

def test_setter_refusals_and_the_way_back(eng_mod, oracle, track):
    from mpopis_amd import _lib
    from mpopis_amd._lib import MPOPISError
    import ctypes as C
    B = 2
    ps = _slot_params(oracle, B)
    x0 = np.stack([SC.start_state(track, 1, b) for b in range(B)])
    never = _policy_engine(eng_mod, track, "cemppi")
    never.set_env_params_slots(ps)
    ref = _steps_and_trials(never, x0, "cemppi")
    never.close()

    eng = _policy_engine(eng_mod, track, "cemppi")
    eng.set_env_params_slots(ps)
    L, h = eng.L, eng._h
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    p3 = np.ascontiguousarray(car_models(oracle, B, 3))

    def refused(rc, word):
        assert rc == _lib.ERR_ARG, rc
        assert word in L.mpopis_last_error(h).decode(), L.mpopis_last_error(h)
    # before any scenarios: set_risk and the getter refuse
    refused(L.mpopis_set_risk(h, 0, 1, 0.0), "no scenarios")
    refused(L.mpopis_get_scenario_costs(h, dp(np.zeros(B * 3 * 96))), "no scenarios")
    assert eng.scenarios()["M"] == 0
    refused(L.mpopis_set_scenarios(h, 17, dp(p3), 20, 1), "M must be")
    refused(L.mpopis_set_scenarios(h, -1, dp(p3), 20, 1), "M must be")
    refused(L.mpopis_set_scenarios(h, 3, dp(p3), 19, 1), "expects 20")
    refused(L.mpopis_set_scenarios(h, 3, None, 20, 1), "NULL")
    assert eng.scenarios()["M"] == 0

    eng.set_scenarios(p3, per_slot=True)
    eng.set_risk("worst")
    assert eng.scenarios() == dict(M=3, kind="worst", tail=1, theta=0.0)
    refused(L.mpopis_set_risk(h, 2, 0, 0.0), "unknown kind")
    refused(L.mpopis_set_risk(h, 0, 4, 0.0), "tail")
    refused(L.mpopis_set_risk(h, 0, -1, 0.0), "tail")
    refused(L.mpopis_set_risk(h, 1, 0, 0.0), "theta")
    refused(L.mpopis_set_risk(h, 1, 0, float("inf")), "theta")
    refused(L.mpopis_set_risk(h, 1, 0, float("nan")), "theta")
    refused(L.mpopis_set_scenarios(h, 17, dp(p3), 20, 1), "M must be")
    refused(L.mpopis_set_env_params_cars(h, dp(ps), 20, 1), "scenario")
    assert eng.scenarios() == dict(M=3, kind="worst", tail=1, theta=0.0)                  # every refusal left the handle as it was
    eng.set_scenarios(p3[:, :2], per_slot=True)
    assert eng.scenarios() == dict(M=2, kind="mean", tail=2, theta=0.0)                   # the call resets the risk to the mean
    eng.set_state(x0)
    steered = eng.policy_step(None)
    assert eng.get_scenario_costs().shape == (B, 2, 96)
    assert not np.array_equal(steered["cost"], ref[1])

    # M = 0: back to the bits of a handle that never switched -- Level 1 on the handle that has stepped under scenarios ...
    rng = np.random.default_rng(47)
    U, E = SC.level1_inputs(rng, B, 1, 96, 5)
    eng.set_scenarios(None)
    assert eng.scenarios()["M"] == 0
    back = eng.rollout_costs(U, E, x0=x0)
    eng.close()
    never = _policy_engine(eng_mod, track, "cemppi")
    never.set_env_params_slots(ps)
    assert np.array_equal(back, never.rollout_costs(U, E, x0=x0))
    never.close()
    # ... and the whole step and closed loop on a handle that switched on and off again
    eng = _policy_engine(eng_mod, track, "cemppi")
    eng.set_env_params_slots(ps)
    eng.set_scenarios(p3, per_slot=True)
    eng.set_risk("entropic", theta=2.0)
    eng.set_scenarios(None)
    got = _steps_and_trials(eng, x0, "cemppi")
    eng.close()
    for i, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(a, b), i

    for make, word in ((lambda: eng_mod.Engine("car", 1, "gmppi", 64, 5, batch=1, cov=[0.0625, 0.1], track=track, log_trajectories=True), "log_trajectories"),):
        e = make()
        refused_rc = e.L.mpopis_set_scenarios(e._h, 1, dp(np.ascontiguousarray(ps[:1])), 20, 0)
        assert refused_rc == _lib.ERR_ARG and word in e.L.mpopis_last_error(e._h).decode()
        e.close()
    fleet = eng_mod.Engine("car", 2, "gmppi", 64, 5, batch=1, cov=np.tile([0.0625, 0.1], 2), track=track)
    fleet.set_env_params_cars(np.stack([ps[0], ps[1]]))
    with pytest.raises(MPOPISError) as ei:
        fleet.set_scenarios(ps[:1])
    assert ei.value.code == _lib.ERR_ARG and "fleet" in str(ei.value)
    fleet.close()


def test_custom_handle_is_refused(eng_mod, oracle):
    """a handle on a caller's env (the mountain car of tests/helpers/envs, as tests/test_gpu_custom_env.py builds it) takes no scenarios"""
    import ctypes as C
    import os
    import types
    from mpopis_amd import build, _lib
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "envs", "mountaincar_sdk.hip")
    env = types.SimpleNamespace(code_object=build.build_env(src), state_size=2, action_size=1,
                                params=np.array(oracle.mountaincar_default_params(), dtype=np.float64), lo=None, hi=None, reset_state=None)
    eng = eng_mod.Engine("custom", 0, "gmppi", 64, 5, batch=1, lam=0.1, cov=[1.5], custom_env=env)
    with pytest.raises(_lib.MPOPISError) as ei:
        eng.set_scenarios(np.zeros((1, 8)))
    assert ei.value.code == _lib.ERR_ARG
    p = np.zeros(8)
    assert eng.L.mpopis_set_scenarios(eng._h, 1, p.ctypes.data_as(C.POINTER(C.c_double)), 8, 0) == _lib.ERR_ARG
    assert "custom" in eng.L.mpopis_last_error(eng._h).decode()
    eng.close()


@pytest.mark.parametrize("risk", ["mean", "worst", "entropic"])
def test_nan_action_is_an_action_error_as_on_a_plain_handle(eng_mod, oracle, track, risk):
    from mpopis_amd._lib import MPOPISError
    for kind, K in (("gmppi", 64), ("musigmaaismppi", 4096)):   # k_weights reports it / the risk kernel does (weights folded into the moments kernel)
        T = 10
        eng = eng_mod.Engine("car", 1, kind, K, T, batch=2, lam=10.0, ais_its=2, cov=[0.0625, 0.1], track=track, seed=11)
        eng.set_scenarios(car_models(oracle, 1, 3)[0])
        eng.set_risk(risk, theta=1.0)
        assert np.all(np.isfinite(eng.policy_step(None)["cost"]))
        U = np.zeros((2, 2 * T))
        U[1, 1] = np.nan                                         # slot 1 only
        eng.set_U(U)
        with pytest.raises(MPOPISError) as ei:
            eng.policy_step(None)
        assert ei.value.code == -3, str(ei.value)
        eng.set_U(np.zeros((2, 2 * T)))                          # the handle keeps working
        g = eng.policy_step(None)
        assert np.all(np.isfinite(g["cost"])) and np.all(np.isfinite(g["control"]))
        eng.close()
