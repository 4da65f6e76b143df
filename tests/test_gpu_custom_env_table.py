"""GPU tests of custom envs with a data table (MPOPIS_DEFINE_ENV_TABLE of include/mpopis_env.h, mpopis_set_env_table):
  - mapnav (tests/helpers/envs/mapnav_sdk.hip = the shipped example: waypoints + a cost map in the table, read at wave-uniform and at per-lane
    run-time indices) against the NumPy restatement tests/helpers/mapnav_ref.py, on tables of 3, 4096 (the last size staged in LDS), 4097 (the
    first read from global memory) and 20 000 doubles, at K on both sides of the 256-thread workgroup;
  - the LDS kernel against the global one, per-slot tables, replacing the table on a live handle, the closed loop, the empty table, errors;
  - cartpole_tab (the built-in CartPole's parameters in the table) against the built-in CartPole under the device RNG, all nine policies, and
    against the oracle with injected noise;
  - the Python mirror (CustomEnv(..., table=...) under the policy classes).
Comparisons with NumPy stand on the edge-margin condition that tests/test_custom_env_table_cpu.py checks for the same seeds; it is asserted
here again on the reference before the device is compared."""
import os
import types
import numpy as np
import pytest

from tests.helpers import mapnav_ref as MN
from tests.helpers import mapnav_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = os.path.join(ROOT, "tests", "helpers", "envs")
ALL_POLICIES = ["mppi", "gmppi", "imppi", "cemppi", "cmamppi", "muaismppi", "musigmaaismppi", "pmcmppi", "nesmppi"]
MAX_TABLE = 1 << 20


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


@pytest.fixture(scope="module")
def sdk(oracle):
    from mpopis_amd import build

    def desc(name, ss, as_, params, lo=None, hi=None, table=None, table_per_slot=False):
        return types.SimpleNamespace(code_object=build.build_env(os.path.join(ENVS, name + ".hip")), state_size=ss, action_size=as_,
                                     params=np.array(params, dtype=np.float64), lo=lo, hi=hi, reset_state=None, table=table, table_per_slot=table_per_slot)
    return types.SimpleNamespace(desc=desc, cartpole_params=np.array(oracle.cartpole_default_params(), dtype=np.float64))


def mapnav_env(sdk, p, table=None, table_per_slot=False):
    return sdk.desc("mapnav_sdk", MN.SS, MN.AS, p, lo=MN.LO, hi=MN.HI, table=table, table_per_slot=table_per_slot)


def cartpole_tab_env(sdk, pad=0):
    return sdk.desc("cartpole_tab_sdk", 4, 1, [], table=np.concatenate([sdk.cartpole_params, np.full(pad, np.nan)]))


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-9)))


def custom_engine(eng_mod, env, kind, K, T, **kw):
    return eng_mod.Engine("custom", 0, kind, K, T, custom_env=env, **kw)


@pytest.fixture(scope="module")
def level1_cache(eng_mod, sdk):
    """(table, K) -> (case, NumPy reference, device costs, device trajectories): every rollout is run once and shared by tests 1 and 2"""
    cache = {}

    def get(table, K):
        if (table, K) not in cache:
            case = MC.level1_case(table, K)
            ref = MC.level1_reference(case)
            eng = custom_engine(eng_mod, mapnav_env(sdk, case["p"], table=case["tab"]), "gmppi", K, MC.LEVEL1_T, batch=MC.LEVEL1_B, lam=1.0,
                                cov=[0.3, 0.3], log_trajectories=True)
            cost = eng.rollout_costs(case["U"], case["E"], x0=case["x0"])
            traj = eng.get_trajectories()
            eng.close()
            cache[(table, K)] = (case, ref, cost, traj)
        return cache[(table, K)]
    return get


# ---- 1. rollout costs and logger, mapnav against NumPy -----------------------------------------------------------------------------------

@pytest.mark.parametrize("K", MC.LEVEL1_K)
@pytest.mark.parametrize("table", list(MC.TABLES))
def test_level1_mapnav_against_numpy(level1_cache, table, K):
    case, (ref_cost, ref_traj, margin, outside), cost, traj = level1_cache(table, K)
    assert case["tab"].size == MC.TABLE_SIZES[table]
    assert margin >= MN.MARGIN and outside > 0                   # the condition the comparison stands on; some rollouts leave the map
    assert rel_err(cost, ref_cost) < 1e-10, rel_err(cost, ref_cost)          # 1e-10 relative, as test_level1_pointmass
    assert rel_err(traj, ref_traj) < 1e-10, rel_err(traj, ref_traj)


# ---- 2. the LDS kernel against the global one --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", MC.LEVEL1_K)
def test_lds_form_equals_global_form(level1_cache, K):
    """The 4096-double table goes through mpopis_env_rollout_tab (LDS), the same content padded by one double through
    mpopis_env_rollout_gtab (global memory): the same functions on the same numbers.  Required: 1e-12.  Measured on one MI355X: bit-identical
    for every K (costs and logged trajectories)."""
    _, _, cost_lds, traj_lds = level1_cache("g64", K)
    _, _, cost_g, traj_g = level1_cache("g64pad", K)
    print("LDS vs global, K = %d: bit-identical costs %s, trajectories %s" % (K, np.array_equal(cost_lds, cost_g), np.array_equal(traj_lds, traj_g)))
    assert rel_err(cost_lds, cost_g) <= 1e-12 and rel_err(traj_lds, traj_g) <= 1e-12


# ---- 3. per-slot tables ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,G", [(2, 3), (50, 64)])               # 13 doubles; 4196 doubles: past the LDS limit
def test_per_slot_tables(eng_mod, sdk, P, G):
    rng = np.random.default_rng(300 + G)
    B, K, T = 3, 130, 9
    cs = MN.AS * T
    p = MN.params(P, G)
    tabs = np.stack([MN.make_table(P, G, rng) for _ in range(B)])
    assert (tabs.shape[1] > 4096) == (G == 64)
    x0 = np.concatenate([rng.uniform(-0.8, 0.8, (B, 2)), rng.uniform(-0.3, 0.3, (B, 2))], axis=1)
    U, E = rng.uniform(-0.3, 0.3, (B, cs)), rng.standard_normal((B, K, cs)) * 0.8
    eng = custom_engine(eng_mod, mapnav_env(sdk, p, table=tabs, table_per_slot=True), "gmppi", K, T, batch=B, lam=1.0, cov=[0.3, 0.3])
    per_slot = eng.rollout_costs(U, E, x0=x0)
    eng.set_env_table(tabs[1])                                   # ... and one table shared by the three slots
    shared = eng.rollout_costs(U, E, x0=x0)
    eng.close()
    one = custom_engine(eng_mod, mapnav_env(sdk, p), "gmppi", K, T, batch=1, lam=1.0, cov=[0.3, 0.3])
    for b in range(B):
        one.set_env_table(tabs[b])
        assert np.array_equal(per_slot[b], one.rollout_costs(U[b:b + 1], E[b:b + 1], x0=x0[b:b + 1])[0]), b
        one.set_env_table(tabs[1])
        assert np.array_equal(shared[b], one.rollout_costs(U[b:b + 1], E[b:b + 1], x0=x0[b:b + 1])[0]), b
    one.close()
    assert not np.array_equal(per_slot[0], shared[0]) and np.array_equal(per_slot[1], shared[1])      # the tables do differ, and are seen


# ---- 4. replacing the table on a live handle ---------------------------------------------------------------------------------------------

def test_replacing_the_table_on_a_live_handle(eng_mod, sdk):
    """policy step, small table -> step -> 20 000 doubles -> step -> n = 0 -> step -> the small table again -> step, with the batch as three
    part-chains on their own streams; every step equals a fresh handle put into the same state with that table.  Injected noise, so that the
    fresh handle needs nothing but state, pol.U and the table (the device RNG also counts the MPC steps a handle has taken)."""
    rng = np.random.default_rng(44)
    B, K, T, N = 4, 256, 6, 3
    cs = MN.AS * T
    small, big = (MN.params(2, 3), MN.make_table(2, 3, rng)), (MN.params(5000, 100), MN.make_table(5000, 100, rng))
    assert big[1].size == 20000
    kw = dict(batch=B, lam=1.0, ais_its=N, elite_threshold=0.8, cov=[0.3, 0.3], seed=4)
    live = custom_engine(eng_mod, mapnav_env(sdk, small[0], table=small[1]), "cemppi", K, T, **kw)
    live.set_overlap(3)
    x0 = np.concatenate([rng.uniform(-0.8, 0.8, (B, 2)), rng.uniform(-0.3, 0.3, (B, 2))], axis=1)
    live.set_state(x0)
    outs = []
    for i, (p, tab) in enumerate([small, small, big, (big[0], None), small]):
        if i > 0:
            live.set_env_params(p)                                # (with n = 0 the parameters still promise a table: the env reads none of it)
            live.set_env_table(tab)
        U_before = live.get_U()
        Z = rng.standard_normal((B, N, K, cs))
        got = live.policy_step(Z)
        fresh = custom_engine(eng_mod, mapnav_env(sdk, p, table=tab), "cemppi", K, T, **kw)
        fresh.set_overlap(3)
        fresh.set_state(x0); fresh.set_U(U_before)
        ref = fresh.policy_step(Z)
        for key in ("control", "cost", "weights", "iters_run"):
            assert np.array_equal(got[key], ref[key]), (i, key)
        assert np.array_equal(live.get_U(), fresh.get_U()), i
        fresh.close()
        outs.append(got["cost"])
    live.close()
    assert not np.array_equal(outs[1], outs[2]) and not np.array_equal(outs[2], outs[3]) and not np.array_equal(outs[3], outs[4])


# ---- 5. cartpole_tab against the built-in CartPole, device RNG, all nine policies -------------------------------------------------------

def _steps_or_error(eng, n):
    from mpopis_amd._lib import MPOPISError
    out = []
    try:
        for _ in range(n):
            out.append(eng.policy_step())
    except MPOPISError as e:
        out.append(e.code)
    return out


@pytest.fixture(scope="module")
def builtin_cartpole_steps(eng_mod):
    """two policy steps of the built-in CartPole per policy, computed once for both table sizes"""
    cache = {}

    def get(kind, K, T, x0, kw):
        if kind not in cache:
            a = eng_mod.Engine("cartpole", 0, kind, K, T, **kw)
            a.set_state(x0)
            ra = _steps_or_error(a, 2)
            ok = not isinstance(ra[-1], int)
            cache[kind] = (ra, a.get_U() if ok else None, a.get_Sigma() if ok and kind != "mppi" else None)
            a.close()
        return cache[kind]
    return get


@pytest.mark.parametrize("pad", [0, 4097 - 11])
@pytest.mark.parametrize("kind", ALL_POLICIES)
def test_cartpole_tab_equals_builtin_cartpole_under_device_rng(eng_mod, sdk, builtin_cartpole_steps, kind, pad):
    """shapes and assertions of test_sdk_cartpole_equals_builtin_cartpole_under_device_rng; the 11-double table runs the LDS kernel, the same
    table padded to 4097 the global one"""
    B, K, T, N = 3, 128, 20, 3
    x0 = np.array([[0.03, 0.0, -0.04, 0.1], [-0.02, 0.1, 0.05, -0.1], [0.0, -0.05, 0.01, 0.02]])
    kw = dict(batch=B, lam=0.1, ais_its=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75, cov=[1.5], seed=77)
    ra, Ua, Sa = builtin_cartpole_steps(kind, K, T, x0, kw)
    env = cartpole_tab_env(sdk, pad)
    assert env.table.size == 11 + pad
    b = custom_engine(eng_mod, env, kind, K, T, **kw)
    b.set_state(x0)
    rb = _steps_or_error(b, 2)
    assert len(ra) == len(rb) and not isinstance(ra[0], int)
    for sa, sb in zip(ra, rb):
        if isinstance(sa, int) or isinstance(sb, int):
            assert sa == sb
            continue
        assert np.array_equal(sa["cost"], sb["cost"]) and np.array_equal(sa["iters_run"], sb["iters_run"])
        assert np.max(np.abs(sa["control"] - sb["control"])) <= 1e-12
    if not isinstance(ra[-1], int):
        assert np.max(np.abs(Ua - b.get_U())) <= 1e-12
        if kind != "mppi":
            assert np.max(np.abs(Sa - b.get_Sigma())) <= 1e-12
    b.close()


# ---- 6. cartpole_tab against the oracle: the cold kernels too ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["cemppi", "cmamppi", "pmcmppi"])
def test_level2_cartpole_tab_against_the_oracle(eng_mod, oracle, sdk, kind):
    """as test_level2_sdk_cartpole: closed loop for 4 MPC steps with injected noise; mpopis_env_step / mpopis_env_query run the two cold table kernels"""
    from mpopis_amd._lib import MPOPISError
    rng = np.random.default_rng(33)
    K, T, N = 20, 15, 5
    x0 = np.array([0.03, 0.0, -0.04, 0.1])
    env = oracle.OracleEnv("cartpole"); env.state = x0
    pol = oracle.OraclePolicy(kind, env, K, T, lam=0.1, U0=[0.0], cov=[1.5], N=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75)
    eng = custom_engine(eng_mod, cartpole_tab_env(sdk), kind, K, T, batch=1, lam=0.1, ais_its=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75, cov=[1.5])
    eng.set_state(x0[None])
    Neff = pol.n_iters()
    for step in range(4):
        Z = rng.standard_normal((Neff, K, T))
        ri = rng.integers(0, K, (max(1, Neff - 1), K)).astype(np.int32); ru = rng.random((max(1, Neff - 1), K))
        ref = pol(env, Z, ri, ru)
        if ref["status"]:
            with pytest.raises(MPOPISError) as ei:
                eng.policy_step(Z[None], ri[None], ru[None])
            assert ei.value.code == ref["status"]
            break
        got = eng.policy_step(Z[None], ri[None], ru[None])
        assert got["iters_run"][0] == ref["iters_run"]
        assert np.array_equal(got["cost"][0], ref["cost"])
        assert np.max(np.abs(got["weights"][0] - ref["weights"])) < 1e-12
        assert abs(got["control"][0, 0] - ref["control"][0]) < 1e-9
        env.step(ref["control"])
        r = eng.env_step(ref["control"][None])
        assert r[0] == env.reward()
        x, t, done = eng.get_state()
        assert np.max(np.abs(x[0] - env.state)) < 1e-13 and t[0] == env.e.t and done[0] == env.e.done
        assert eng.env_query()[0][0] == env.reward() and bool(eng.env_query()[1][0])
        eng.set_U(pol.U[None])
    eng.close()


# ---- 7. closed loop, per-slot tables ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mppi", "cemppi"])
def test_level3_run_trials_mapnav_with_per_slot_tables(eng_mod, sdk, kind):
    rng = np.random.default_rng(70)
    K, T, N, steps = 64, 8, 3, 12
    p = MN.params(4, 16)
    tabs = np.stack([MN.make_table(4, 16, rng) for _ in range(2)])
    x0s = np.array([[0.2, -0.3, 0.1, 0.0], [-0.5, 0.4, 0.0, -0.1]])
    kw = dict(batch=2, lam=1.0, ais_its=N, elite_threshold=0.8, cov=[0.3, 0.3], seed=21)
    eng = custom_engine(eng_mod, mapnav_env(sdk, p, table=tabs, table_per_slot=True), kind, K, T, **kw)
    eng.set_state(x0s)
    rec, acts = eng.run_trials(num_steps=steps, laps=0, log_actions=True)
    eng.close()
    host = custom_engine(eng_mod, mapnav_env(sdk, p, table=tabs, table_per_slot=True), kind, K, T, **kw)
    host.set_state(x0s)
    logged = np.zeros_like(acts)
    for s in range(steps + 1):
        c = host.policy_step(minimal=True)["control"]
        logged[:, s] = c
        host.env_step(c)
    host.close()
    for b in range(2):
        n = int(rec[b, 1]) + 1                               # actions the slot took while it was alive
        assert n >= steps and np.array_equal(acts[b, :n], logged[b, :n])      # (max_steps = 200: nobody is done inside 12 steps)
    assert np.ptp(acts[0]) > 0.0 and not np.array_equal(acts[0], acts[1])


# ---- 8. errors and the empty table -------------------------------------------------------------------------------------------------------

def test_set_env_table_errors(eng_mod, sdk):
    import ctypes as C
    from mpopis_amd._lib import MPOPISError
    builtin = eng_mod.Engine("cartpole", 0, "gmppi", 16, 4, batch=1, lam=1.0, cov=[1.0])
    with pytest.raises(MPOPISError) as ei:
        builtin.set_env_table(np.zeros(3))
    assert ei.value.code == -1 and "not a custom handle" in str(ei.value)
    builtin.close()
    from tests.helpers import pointmass_ref as PM
    plain = custom_engine(eng_mod, sdk.desc("pointmass_sdk", PM.SS, PM.AS, PM.PARAMS, lo=PM.LO, hi=PM.HI), "gmppi", 16, 4, batch=1, lam=1.0, cov=[0.3, 0.3, 0.1])
    with pytest.raises(MPOPISError) as ei:
        plain.set_env_table(np.zeros(3))
    assert ei.value.code == -1 and "mpopis_env_table_abi" in str(ei.value)
    plain.close()
    eng = custom_engine(eng_mod, mapnav_env(sdk, MN.params(1, 1)), "gmppi", 16, 4, batch=2, lam=1.0, cov=[0.3, 0.3])
    L, h = eng.L, eng._h
    buf = np.zeros(8)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mpopis_set_env_table(h, dp, -1, 0) == -1 and b"n must be" in L.mpopis_last_error(h)
    assert L.mpopis_set_env_table(h, dp, MAX_TABLE + 1, 0) == -1 and b"n must be" in L.mpopis_last_error(h)
    assert L.mpopis_set_env_table(h, None, 3, 0) == -1 and b"NULL" in L.mpopis_last_error(h)
    assert L.mpopis_set_env_table(h, None, 0, 0) == 0 and L.mpopis_set_env_table(h, dp, 4, 1) == 0      # clearing; B * n = 8 doubles per slot form
    assert L.mpopis_set_env_table(h, dp, 0, 1) == 0
    with pytest.raises(MPOPISError):
        eng.set_env_table(np.zeros((3, 4)), per_slot=True)       # the Python wrapper wants (B, n)
    eng.close()


def test_table_env_before_any_table_is_set(eng_mod, sdk):
    """ntab == 0: the env must not read the table, and mapnav does not with P = 0 and G = 0 (its map is then 0 everywhere)"""
    case = MC.empty_table_case()
    B, K, cs = case["E"].shape
    ref_cost, ref_traj, margin, _ = MC.level1_reference(case)
    assert margin >= MN.MARGIN
    eng = custom_engine(eng_mod, mapnav_env(sdk, case["p"]), "gmppi", K, cs // MN.AS, batch=B, lam=1.0, cov=[0.3, 0.3], log_trajectories=True)
    cost = eng.rollout_costs(case["U"], case["E"], x0=case["x0"])
    assert rel_err(cost, ref_cost) < 1e-10 and rel_err(eng.get_trajectories(), ref_traj) < 1e-10
    eng.set_env_params(MN.params(3, 5))                          # parameters that promise a table that is not there: entries past ntab read as 0
    assert rel_err(eng.rollout_costs(case["U"], case["E"], x0=case["x0"]), ref_cost) < 1e-10
    eng.close()


# ---- 9. Python mirror --------------------------------------------------------------------------------------------------------------------

def test_python_mirror_runs_the_policies_on_a_table_env(eng_mod, sdk):
    import mpopis_amd as M
    case = MC.mirror_case()
    x0, K, T = MC.MIRROR_X0, 64, 8

    def make_env():
        return M.CustomEnv(M.mapnav_source(), MN.SS, MN.AS, params=case["p"], lo=MN.LO, hi=MN.HI, reset_state=x0, table=case["tab"])
    env = make_env()
    assert np.array_equal(M.state(env), x0) and np.array_equal(env.table, case["tab"])
    pol = M.GMPPI_Policy(env, num_samples=K, horizon=T, λ=1.5, U0=np.zeros(MN.AS), cov_mat=[0.3, 0.3], seed=3)
    act = pol(env)
    eng = custom_engine(eng_mod, env, "gmppi", K, T, batch=1, lam=1.5, cov=[0.3, 0.3], seed=3)
    eng.set_state(x0[None])
    assert np.array_equal(act, eng.policy_step()["control"][0])
    eng.close()
    env(act)                                                     # env(action): the cold step kernel with the table
    s_ref, t_ref, _, m1 = MN.step(x0, 0, act, case["p"], case["tab"])
    r_ref, m2 = MN.reward(s_ref, case["p"], case["tab"])
    assert min(m1, m2) >= MN.MARGIN
    assert np.max(np.abs(env.state - s_ref)) <= 1e-14 and env.t == t_ref == 1
    assert abs(M.reward(env) - r_ref) <= 1e-13 * max(1.0, abs(r_ref))
    env.set_table(None)                                          # set_table: without the table the same state earns another reward
    assert M.reward(env) != pytest.approx(r_ref, rel=1e-6)
    pol.close()
    env2 = make_env()
    pol = M.get_policy(":cemppi", env2, K, T, 1.5, 1.0, [0.0, 0.0], [0.3, 0.3], False, 3, 5.0, 0.8, "mle", 0.75, 0.8, seed=3)
    act = pol(env2)
    eng = custom_engine(eng_mod, env2, "cemppi", K, T, batch=1, lam=1.5, ais_its=3, elite_threshold=0.8, cov=[0.3, 0.3], seed=3)
    eng.set_state(x0[None])
    assert np.array_equal(act, eng.policy_step()["control"][0])
    eng.close(); pol.close()
