"""GPU tests of the caller-supplied env seam: envs written against include/mpopis_env.h, compiled to gfx950 code objects and run through
mpopis_create_custom under every policy.
  - CartPole and MountainCar restated with the SDK (tests/helpers/envs; pinned to the oracle's envs on the host by tests/test_custom_env_cpu.py):
    the oracle checks the new path end to end -- rollout costs + logger, every policy with injected noise, the closed loop -- and the built-in
    CartPole handle must agree with the SDK one under the device RNG, all nine policies;
  - the planar point mass (SS = 5, AS = 3: sizes of no built-in env) against the NumPy restatement tests/helpers/pointmass_ref.py;
  - argument / action errors, two code objects alive together, the Python mirror (CustomEnv under the policy classes)."""
import os
import types
import numpy as np
import pytest

from tests.helpers import pointmass_ref as PM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = os.path.join(ROOT, "tests", "helpers", "envs")
ALL_POLICIES = ["mppi", "gmppi", "imppi", "cemppi", "cmamppi", "muaismppi", "musigmaaismppi", "pmcmppi", "nesmppi"]


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


@pytest.fixture(scope="module")
def sdk(oracle):
    """the three test envs as `custom_env` descriptions (code object path, sizes, parameters)"""
    from mpopis_amd import build

    def desc(name, ss, as_, params, lo=None, hi=None, reset_state=None):
        return types.SimpleNamespace(code_object=build.build_env(os.path.join(ENVS, name + ".hip")), state_size=ss, action_size=as_,
                                     params=np.array(params, dtype=np.float64), lo=lo, hi=hi, reset_state=reset_state)
    return types.SimpleNamespace(cartpole=desc("cartpole_sdk", 4, 1, oracle.cartpole_default_params()),
                                 mountaincar=desc("mountaincar_sdk", 2, 1, oracle.mountaincar_default_params()),
                                 pointmass=desc("pointmass_sdk", PM.SS, PM.AS, PM.PARAMS, lo=PM.LO, hi=PM.HI))


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-9)))


def custom_engine(eng_mod, env, kind, K, T, **kw):
    return eng_mod.Engine("custom", 0, kind, K, T, custom_env=env, **kw)


# ---- 4. Level 1, CartPole via SDK, with logger ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 64, 65, 200])
def test_level1_sdk_cartpole_with_logger(eng_mod, oracle, sdk, K):
    rng = np.random.default_rng(31)
    T = 15
    x0 = np.array([0.02, -0.1, 0.03, 0.2])
    env = oracle.OracleEnv("cartpole"); env.state = x0
    eng = custom_engine(eng_mod, sdk.cartpole, "gmppi", K, T, batch=1, lam=0.1, cov=[1.5], log_trajectories=True)
    E = rng.standard_normal((1, K, T)) * 1.2
    U = rng.uniform(-0.5, 0.5, T)
    got = eng.rollout_costs(U[None], E, x0=x0[None])
    pol = oracle.OraclePolicy("gmppi", env, K, T, lam=0.1, U0=[0.0], cov=[1.5])
    ref, tr_ref = pol.simulate_model(U, E[0].T, log=True)
    assert np.array_equal(got[0], ref)                       # costs are small integers: exact
    assert rel_err(eng.get_trajectories()[0], tr_ref) < 1e-12
    eng.close()


# ---- 5. Level 2, CartPole via SDK, every policy against the oracle ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mppi", "gmppi", "imppi", "cemppi", "cmamppi", "muaismppi", "musigmaaismppi", "pmcmppi"])
def test_level2_sdk_cartpole(eng_mod, oracle, sdk, kind):
    """pol(env) on the SDK CartPole with the simulate_cartpole defaults (cartpole_example.jl:35-50), closed loop for 4 MPC steps, injected noise."""
    from mpopis_amd._lib import MPOPISError
    rng = np.random.default_rng(33)
    K, T, N = 20, 15, 5
    x0 = np.array([0.03, 0.0, -0.04, 0.1])
    env = oracle.OracleEnv("cartpole"); env.state = x0
    pol = oracle.OraclePolicy(kind, env, K, T, lam=0.1, U0=[0.0], cov=[1.5], N=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75)
    eng = custom_engine(eng_mod, sdk.cartpole, kind, K, T, batch=1, lam=0.1, ais_its=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75, cov=[1.5])
    eng.set_state(x0[None])
    Neff = pol.n_iters()
    for step in range(4):
        Z = rng.standard_normal((T, K, 1)) if kind == "mppi" else rng.standard_normal((Neff, K, T))
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
        r = eng.env_step(ref["control"][None])               # same action on both sides keeps the loops aligned
        assert r[0] == env.reward()
        x, t, done = eng.get_state()
        assert np.max(np.abs(x[0] - env.state)) < 1e-13 and t[0] == env.e.t and done[0] == env.e.done
        assert eng.env_query()[0][0] == env.reward() and bool(eng.env_query()[1][0])
        eng.set_U(pol.U[None])
    eng.close()


# ---- 6. custom against built-in, device RNG, all nine policies ------------------------------------------------------------------------------

def _steps_or_error(eng, n):
    from mpopis_amd._lib import MPOPISError
    out = []
    try:
        for _ in range(n):
            out.append(eng.policy_step())
    except MPOPISError as e:
        out.append(e.code)
    return out


@pytest.mark.parametrize("kind", ALL_POLICIES)
def test_sdk_cartpole_equals_builtin_cartpole_under_device_rng(eng_mod, sdk, kind):
    B, K, T, N = 3, 128, 20, 3
    x0 = np.array([[0.03, 0.0, -0.04, 0.1], [-0.02, 0.1, 0.05, -0.1], [0.0, -0.05, 0.01, 0.02]])
    kw = dict(batch=B, lam=0.1, ais_its=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75, cov=[1.5], seed=77)
    a = eng_mod.Engine("cartpole", 0, kind, K, T, **kw)
    b = custom_engine(eng_mod, sdk.cartpole, kind, K, T, **kw)
    for e in (a, b):
        e.set_state(x0)
    ra, rb = _steps_or_error(a, 2), _steps_or_error(b, 2)
    assert len(ra) == len(rb) and not isinstance(ra[0], int)     # at least the first step of every policy is compared value by value
    for sa, sb in zip(ra, rb):
        if isinstance(sa, int) or isinstance(sb, int):
            assert sa == sb                                  # the same error code from both
            continue
        assert np.array_equal(sa["cost"], sb["cost"]) and np.array_equal(sa["iters_run"], sb["iters_run"])
        assert np.max(np.abs(sa["control"] - sb["control"])) <= 1e-12
    if not isinstance(ra[-1], int):
        assert np.max(np.abs(a.get_U() - b.get_U())) <= 1e-12
        if kind != "mppi":                                   # (:mppi keeps the as x as pol.Σ: mpopis_get_Sigma refuses)
            assert np.max(np.abs(a.get_Sigma() - b.get_Sigma())) <= 1e-12
    a.close(); b.close()


# ---- 7. MountainCar via SDK -----------------------------------------------------------------------------------------------------------------

def test_level1_sdk_mountaincar_and_changed_parameters(eng_mod, oracle, sdk):
    rng = np.random.default_rng(3)
    K, T = 100, 15
    eng = custom_engine(eng_mod, sdk.mountaincar, "gmppi", K, T, batch=1, lam=0.1, cov=[1.5])
    E = rng.standard_normal((1, K, T)) * 1.2
    p2 = oracle.mountaincar_default_params().copy()
    p2[5], p2[3] = 0.004, -0.42                              # power, goal_pos: some rollouts now reach the goal inside the horizon
    for params in (None, p2):
        env = oracle.OracleEnv("mountaincar", params=params)
        env.state = [-0.5, 0.0]
        if params is not None:
            eng.set_env_params(p2)
        got = eng.rollout_costs(np.zeros((1, T)), E, x0=np.array([[-0.5, 0.0]]))
        pol = oracle.OraclePolicy("gmppi", env, K, T, lam=0.1, U0=[0.0], cov=[1.5])
        ref = pol.simulate_model(np.zeros(T), E[0].T)
        assert rel_err(got[0], ref) < 1e-12
        if params is not None:
            assert np.any(ref < -50000)                      # the changed goal is reached: the parameters did arrive
    from mpopis_amd._lib import MPOPISError
    with pytest.raises(MPOPISError) as ei:
        eng.set_env_params(p2[:7])
    assert ei.value.code == -1                               # n must equal nparams
    eng.close()


# ---- 8. point mass: SS = 5, AS = 3 ----------------------------------------------------------------------------------------------------------

def test_level1_pointmass(eng_mod, sdk):
    rng = np.random.default_rng(41)
    B, K, T = 2, 130, 11
    cs = PM.AS * T
    lam, alpha = 2.0, 0.8
    eng = custom_engine(eng_mod, sdk.pointmass, "gmppi", K, T, batch=B, lam=lam, alpha=alpha, cov=[0.3, 0.3, 0.1], log_trajectories=True)
    x0 = np.array([[0.2, -0.3, 0.5, 0.1, 0.0], [-0.6, 0.4, -0.2, 0.3, 0.25]])
    U = rng.uniform(-0.3, 0.3, (B, cs))
    Uo = rng.uniform(-0.3, 0.3, (B, cs))
    A = rng.standard_normal((cs, cs))
    Sinv = A @ A.T / cs + np.eye(cs)
    E = rng.standard_normal((B, K, cs)) * 0.4
    E[:, :5] *= 8.0                                          # far out: every clamp, on both sides, is hit
    got = eng.rollout_costs(U, E, x0=x0, U_orig=Uo, Sigma_inv=Sinv)
    tr = eng.get_trajectories()
    hit_lo = hit_hi = 0
    for b in range(B):
        ref, tr_ref = PM.rollout_costs(x0[b], U[b], E[b], U_orig=Uo[b], gamma=lam * (1 - alpha), Sigma_inv=Sinv)
        assert rel_err(got[b], ref) < 1e-10, rel_err(got[b], ref)
        assert rel_err(tr[b], tr_ref) < 1e-10, rel_err(tr[b], tr_ref)
        V = (U[b][None] + E[b]).reshape(K, T, PM.AS)
        hit_lo += (V < PM.LO).any(axis=(0, 1)); hit_hi += (V > PM.HI).any(axis=(0, 1))
    assert np.all(hit_lo) and np.all(hit_hi)
    eng.close()


@pytest.mark.parametrize("kind", ["mppi", "gmppi", "cemppi", "musigmaaismppi", "pmcmppi", "nesmppi"])
def test_level2_pointmass(eng_mod, sdk, kind):
    rng = np.random.default_rng(43)
    B, K, T, N = 1, 96, 9, 3
    cs, as_ = PM.AS * T, PM.AS
    lam = 1.5
    eng = custom_engine(eng_mod, sdk.pointmass, kind, K, T, batch=B, lam=lam, ais_its=N, lam_ais=5.0, elite_threshold=0.8, cov=[0.3, 0.3, 0.1])
    x0 = np.array([0.2, -0.3, 0.5, 0.1, 0.0])
    U0 = rng.uniform(-0.3, 0.3, cs)
    eng.set_state(x0[None]); eng.set_U(U0[None])
    Neff = 1 if kind in ("mppi", "gmppi") else N
    Z = rng.standard_normal((1, T, K, as_)) if kind == "mppi" else rng.standard_normal((1, Neff, K, cs))
    ri = rng.integers(0, K, (1, max(1, Neff - 1), K)).astype(np.int32); ru = rng.random((1, max(1, Neff - 1), K))
    got = eng.policy_step(Z, ri, ru, want_E=True)
    E = got["E"][0]
    E = E.transpose(1, 0, 2).reshape(K, cs) if kind == "mppi" else E          # -> (K, cs), row k = sample k
    cost_ref, _ = PM.rollout_costs(x0, U0, E)                                 # V = U_orig + E_out is what the last iteration rolled out
    assert np.max(np.abs(got["cost"][0] - cost_ref) / np.maximum(1.0, np.abs(cost_ref))) <= 1e-12
    w = np.exp(-(got["cost"][0] - got["cost"][0].min()) / lam); w /= w.sum()
    assert np.max(np.abs(got["weights"][0] - w)) <= 1e-12
    wc = U0 + got["weights"][0] @ E
    assert np.max(np.abs(got["control"][0] - np.clip(wc[:as_], PM.LO, PM.HI))) <= 1e-10
    Unew = eng.get_U()[0]
    assert np.max(np.abs(Unew[:cs - as_] - wc[as_:])) <= 1e-10                # rolled by three ...
    assert np.array_equal(Unew[cs - as_:], U0[cs - as_:])                     # ... with its tail untouched (utils.jl:88-101)
    eng.close()


# ---- 9. closed loop -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mppi", "cemppi"])
def test_level3_run_trials_sdk_cartpole(eng_mod, oracle, sdk, kind):
    K, T, N = 20, 15, 5
    x0s = np.array([[0.01, 0.02, -0.03, 0.04], [-0.04, 0.0, 0.045, -0.02]])
    kw = dict(batch=2, lam=0.1, ais_its=N, elite_threshold=0.8, cov=[1.5], seed=21)
    eng = custom_engine(eng_mod, sdk.cartpole, kind, K, T, **kw)
    eng.set_state(x0s)
    rec = eng.run_trials(num_steps=200, laps=0)
    for b in range(2):
        env = oracle.OracleEnv("cartpole"); env.state = x0s[b]
        pol = oracle.OraclePolicy(kind, env, K, T, lam=0.1, U0=[0.0], cov=[1.5], N=N, elite_threshold=0.8)
        r = pol.run_trial(env, 21 + b + 1, num_steps=200)
        assert rec[b, 15] == r["status"]
        assert rec[b, 1] == r["steps"] and rec[b, 0] == r["rew"], (rec[b], r)
    eng.close()
    # the same loop from the host on a second handle: policy_step + env_step
    steps = 12
    eng = custom_engine(eng_mod, sdk.cartpole, kind, K, T, **kw)
    eng.set_state(x0s)
    rec, acts = eng.run_trials(num_steps=steps, laps=0, log_actions=True)
    eng.close()
    host = custom_engine(eng_mod, sdk.cartpole, kind, K, T, **kw)
    host.set_state(x0s)
    logged = np.zeros_like(acts)
    for s in range(steps + 1):
        c = host.policy_step(minimal=True)["control"]
        logged[:, s] = c
        host.env_step(c)
    host.close()
    for b in range(2):
        n = int(rec[b, 1]) + 1                               # actions the slot took while it was alive
        assert n >= 2 and np.array_equal(acts[b, :n], logged[b, :n])


# ---- 10. errors and lifetime ----------------------------------------------------------------------------------------------------------------

def test_errors_on_custom_handles(eng_mod, sdk):
    from mpopis_amd._lib import MPOPISError
    wrong = types.SimpleNamespace(**vars(sdk.cartpole)); wrong.state_size = 5
    with pytest.raises(MPOPISError) as ei:
        custom_engine(eng_mod, wrong, "gmppi", 16, 4)
    assert ei.value.code == -1 and "state_size 4" in str(ei.value)
    K, T = 64, 6
    eng = custom_engine(eng_mod, sdk.pointmass, "gmppi", K, T, batch=2, lam=1.0, cov=[0.3, 0.3, 0.1], seed=2)
    U = np.zeros((2, PM.AS * T)); U[1, 4] = np.nan
    eng.set_U(U)
    with pytest.raises(MPOPISError) as ei:
        eng.policy_step()
    assert ei.value.code == -3                               # a NaN action poisons the rollout's cost: "Action is not in action space"
    eng.set_U(np.zeros((2, PM.AS * T)))
    assert np.all(np.isfinite(eng.policy_step()["control"]))
    eng.env_step(np.array([[0.7, 1.0, 0.0], [-1.0, -0.5, 1.0]]))                 # the bounds themselves are inside
    with pytest.raises(MPOPISError) as ei:
        eng.env_step(np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -0.1]]))             # brake below its own lower bound 0
    assert ei.value.code == -3
    eng.reset()
    x, t, done = eng.get_state()
    assert np.array_equal(x, np.zeros((2, PM.SS))) and not t.any() and not done.any()
    eng.close()


@pytest.mark.parametrize("first", ["cartpole", "pointmass"])
def test_two_code_objects_alive_together(eng_mod, sdk, first):
    rng = np.random.default_rng(6)
    K, T = 70, 5
    cp = custom_engine(eng_mod, sdk.cartpole, "gmppi", K, T, batch=1, lam=0.1, cov=[1.5])
    pm = custom_engine(eng_mod, sdk.pointmass, "gmppi", K, T, batch=1, lam=1.0, cov=[0.3, 0.3, 0.1])
    Ecp, Epm = rng.standard_normal((1, K, T)), rng.standard_normal((1, K, PM.AS * T)) * 0.4
    xcp, xpm = np.array([[0.02, -0.1, 0.03, 0.2]]), np.array([[0.2, -0.3, 0.5, 0.1, 0.0]])
    ref_pm, _ = PM.rollout_costs(xpm[0], np.zeros(PM.AS * T), Epm[0])
    first_cp = cp.rollout_costs(np.zeros((1, T)), Ecp, x0=xcp)
    for _ in range(2):                                       # alternately
        assert rel_err(pm.rollout_costs(np.zeros((1, PM.AS * T)), Epm, x0=xpm)[0], ref_pm) < 1e-10
        assert np.array_equal(cp.rollout_costs(np.zeros((1, T)), Ecp, x0=xcp), first_cp)
    assert np.all(first_cp <= 0) and np.all(first_cp >= -T)  # CartPole: minus the steps survived
    if first == "cartpole":
        cp.close()
        assert rel_err(pm.rollout_costs(np.zeros((1, PM.AS * T)), Epm, x0=xpm)[0], ref_pm) < 1e-10
        pm.close()
    else:
        pm.close()
        assert np.array_equal(cp.rollout_costs(np.zeros((1, T)), Ecp, x0=xcp), first_cp)
        cp.close()


# ---- 11. Python mirror ----------------------------------------------------------------------------------------------------------------------

def test_python_mirror_runs_the_policies_on_a_custom_env(eng_mod, sdk):
    import mpopis_amd as M
    x0 = np.array([0.2, -0.3, 0.5, 0.1, 0.0])
    K, T = 64, 8

    def make_env():
        return M.CustomEnv(M.pointmass_source(), PM.SS, PM.AS, params=PM.PARAMS, lo=PM.LO, hi=PM.HI, reset_state=x0)
    env = make_env()
    assert np.array_equal(M.state(env), x0) and not M.is_terminated(env)
    lo, hi = M.action_space(env)
    assert np.array_equal(lo, PM.LO) and np.array_equal(hi, PM.HI)
    pol = M.GMPPI_Policy(env, num_samples=K, horizon=T, λ=1.5, U0=np.zeros(PM.AS), cov_mat=[0.3, 0.3, 0.1], seed=3)
    act = pol(env)
    eng = custom_engine(eng_mod, env, "gmppi", K, T, batch=1, lam=1.5, cov=[0.3, 0.3, 0.1], seed=3)
    eng.set_state(x0[None])
    assert np.array_equal(act, eng.policy_step()["control"][0])
    eng.close()
    env(act)                                                 # env(action): the device step kernel
    s_ref, t_ref, _ = PM.step(x0, 0, act)
    assert np.max(np.abs(env.state - s_ref)) <= 1e-14 and env.t == t_ref == 1
    assert abs(M.reward(env) - PM.reward(s_ref)) <= 1e-13
    pol.close()
    env2 = make_env()
    pol = M.get_policy(":cemppi", env2, K, T, 1.5, 1.0, [0.0, 0.0, 0.0], [0.3, 0.3, 0.1], False, 3, 5.0, 0.8, "mle", 0.75, 0.8, seed=3)
    act = pol(env2)
    eng = custom_engine(eng_mod, env2, "cemppi", K, T, batch=1, lam=1.5, ais_its=3, elite_threshold=0.8, cov=[0.3, 0.3, 0.1], seed=3)
    eng.set_state(x0[None])
    assert np.array_equal(act, eng.policy_step()["control"][0])
    eng.close(); pol.close()


# ---- 12. the rest of the ABI on a custom handle ---------------------------------------------------------------------------------------------

def test_step_and_reward_named_env_without_parameters(eng_mod):
    """functions named `step` / `reward`, NP = 0 (no parameter call at all): the generated kernels against the env's host build"""
    from tests.test_custom_env_cpu import compare_pendulum_device_with_host
    compare_pendulum_device_with_host()


def test_timing_bench_and_policy_call_on_a_custom_handle(eng_mod, sdk):
    B, K, T, N = 2, 96, 7, 3
    x0 = np.array([[0.03, 0.0, -0.04, 0.1], [-0.02, 0.1, 0.05, -0.1]])
    kw = dict(batch=B, lam=0.1, ais_its=N, lam_ais=0.1, cov=[1.5], seed=9)
    eng = custom_engine(eng_mod, sdk.cartpole, "musigmaaismppi", K, T, **kw)
    eng.set_state(x0)
    eng.timing_enable(True)
    eng.timing_reset()
    first = eng.policy_step()
    tm = eng.timing_read()
    assert tm["rollout"][1] == N and tm["rollout"][0] > 0.0     # the custom rollout counts under the "rollout" class, once per AIS iteration
    eng.timing_enable(False)
    ms, rollouts = eng.bench_policy_steps(3)
    assert ms > 0.0 and rollouts == 3 * B * N * K
    eng.close()
    # mpopis_policy_call == set_state + set_U + policy_step + get_U
    U0 = np.random.default_rng(2).uniform(-0.2, 0.2, (B, T))
    one, two = custom_engine(eng_mod, sdk.cartpole, "musigmaaismppi", K, T, **kw), custom_engine(eng_mod, sdk.cartpole, "musigmaaismppi", K, T, **kw)
    U = U0.copy()
    got = one.policy_call(x0, [3, 4], [0, 0], U, want_cost=True)
    two.set_state(x0, [3, 4], [0, 0]); two.set_U(U0)
    ref = two.policy_step()
    assert np.array_equal(got["control"], ref["control"]) and np.array_equal(got["cost"], ref["cost"]) and np.array_equal(got["iters_run"], ref["iters_run"])
    assert np.array_equal(U, two.get_U()) and not np.array_equal(U, U0)
    assert np.array_equal(first["cost"].shape, (B, K))
    one.close(); two.close()
