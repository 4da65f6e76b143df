"""GPU parity tests: the HIP engine (through the C ABI) against the CPU oracle on the same seeded
inputs.  Tolerances: BASELINE.json asks for 1e-5 relative on controls / per-step cost; the engine
is held to 1e-8 here (observed ~1e-12), bit-exact for integer results (resampling indices,
iteration counts)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-8


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-9)))


def make_oracle(oracle, track, kind, ncars, K, T, **kw):
    env = oracle.OracleEnv("car", ncars, track=track)
    cov = np.tile([0.0625, 0.1], ncars)
    pol = oracle.OraclePolicy(kind, env, K, T, lam=kw.get("lam", 10.0), alpha=kw.get("alpha", 1.0),
                              U0=kw.get("U0", np.zeros(2 * ncars)), cov=cov, N=kw.get("N", 4),
                              lam_ais=kw.get("lam_ais", 20.0), elite_threshold=0.8, cma_sigma=0.75, nthreads=8)
    return env, pol


@pytest.mark.parametrize("ncars,K,T", [(1, 256, 50), (1, 150, 50), (3, 128, 50), (2, 70, 13), (1, 1100, 12), (2, 1030, 8)])
def test_level1_rollout_costs_car(eng_mod, oracle, track, ncars, K, T):
    rng = np.random.default_rng(100 + ncars)
    B = 2
    cs = 2 * ncars * T
    env, pol = make_oracle(oracle, track, "gmppi", ncars, K, T)
    eng = eng_mod.Engine("car", ncars, "gmppi", K, T, batch=B, lam=10.0, cov=np.tile([0.0625, 0.1], ncars), track=track)
    U = rng.uniform(-0.3, 0.3, (B, cs))
    U[:, 1::2] += 0.3
    E = rng.standard_normal((B, K, cs)) * np.tile([0.25, 0.32], ncars * T)
    E[0, :4] *= 8.0                                       # some samples far out: clamps, off-track, β penalties
    x0 = np.stack([env.state for _ in range(B)])
    x0[1, 0] += 2.0
    x0[1, 3] = 17.0
    got = eng.rollout_costs(U, E, x0=x0)
    for b in range(B):
        env.state = x0[b]
        ref = pol.simulate_model(U[b], E[b].T)
        assert rel_err(got[b], ref) < RTOL, (b, rel_err(got[b], ref))
    eng.close()


def test_level1_control_cost_gamma(eng_mod, oracle, track):
    rng = np.random.default_rng(7)
    K, T = 64, 20
    cs = 2 * T
    env, pol = make_oracle(oracle, track, "gmppi", 1, K, T, alpha=0.8)
    eng = eng_mod.Engine("car", 1, "gmppi", K, T, batch=1, lam=10.0, alpha=0.8, cov=[0.0625, 0.1], track=track)
    U = rng.uniform(-0.3, 0.3, cs)
    Uo = rng.uniform(-0.3, 0.3, cs)
    A = rng.standard_normal((cs, cs))
    Sinv = A @ A.T / cs + np.eye(cs)
    E = rng.standard_normal((1, K, cs)) * 0.3
    got = eng.rollout_costs(U[None], E, x0=env.state[None], U_orig=Uo[None], Sigma_inv=Sinv)
    ref = pol.simulate_model(U, E[0].T, Sigma_inv=Sinv, U_orig=Uo)
    assert rel_err(got[0], ref) < RTOL
    eng.close()


def test_level1_mountaincar(eng_mod, oracle):
    rng = np.random.default_rng(3)
    K, T = 20, 15
    env = oracle.OracleEnv("mountaincar")
    env.state = [-0.5, 0.0]
    eng = eng_mod.Engine("mountaincar", 0, "gmppi", K, T, batch=1, lam=0.1, cov=[1.5])
    E = rng.standard_normal((1, K, T)) * 1.2
    got = eng.rollout_costs(np.zeros((1, T)), E, x0=np.array([[-0.5, 0.0]]))
    pol = oracle.OraclePolicy("gmppi", env, K, T, lam=0.1, U0=[0.0], cov=[1.5])
    ref = pol.simulate_model(np.zeros(T), E[0].T)
    assert rel_err(got[0], ref) < 1e-12
    eng.close()


def test_trajectory_logger(eng_mod, oracle, track):
    rng = np.random.default_rng(5)
    K, T = 64, 12
    env, pol = make_oracle(oracle, track, "gmppi", 1, K, T)
    eng = eng_mod.Engine("car", 1, "gmppi", K, T, batch=1, lam=10.0, cov=[0.0625, 0.1], track=track, log_trajectories=True)
    E = rng.standard_normal((1, K, 2 * T)) * 0.3
    eng.rollout_costs(np.zeros((1, 2 * T)), E, x0=env.state[None])
    tr = eng.get_trajectories()[0]
    _, ref = pol.simulate_model(np.zeros(2 * T), E[0].T, log=True)
    assert rel_err(tr, ref) < RTOL
    eng.close()


@pytest.mark.parametrize("kind", ["gmppi", "imppi", "muaismppi", "musigmaaismppi", "cemppi", "pmcmppi", "cmamppi"])
@pytest.mark.parametrize("ncars", [1, 2])
def test_level2_policy_step(eng_mod, oracle, track, kind, ncars):
    """control = pol(env) with injected noise, 2 consecutive MPC steps (checks the roll of U too)."""
    rng = np.random.default_rng(11)
    B, K, T, N = 2, 192, 10, 4
    cs = 2 * ncars * T
    Neff = 1 if kind == "gmppi" else N
    eng = eng_mod.Engine("car", ncars, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8,
                         cma_sigma=0.75, cov=np.tile([0.0625, 0.1], ncars), track=track)
    envs, pols = [], []
    for b in range(B):
        e, p = make_oracle(oracle, track, kind, ncars, K, T, N=N)
        if b == 1:
            s = e.state; s[3] = 14.0; s[1] = 3.0; e.state = s
        envs.append(e); pols.append(p)
    eng.set_state(np.stack([e.state for e in envs]))
    for step in range(2):
        Z = rng.standard_normal((B, Neff, K, cs))
        di = rng.integers(0, K, (B, max(Neff - 1, 1), K)).astype(np.int32)
        du = rng.random((B, max(Neff - 1, 1), K))
        got = eng.policy_step(Z, di, du, want_E=True)
        U_dev = eng.get_U()
        for b in range(B):
            ref = pols[b](envs[b], Z[b], di[b], du[b])
            assert ref["status"] == 0
            assert got["iters_run"][b] == ref["iters_run"]
            if kind == "pmcmppi":
                assert np.array_equal(got["res_idx0"][b][:Neff - 1], ref["res_idx0"][:Neff - 1])     # bit-exact
            assert rel_err(got["cost"][b], ref["cost"]) < RTOL, (kind, step, b)
            assert np.max(np.abs(got["weights"][b] - ref["weights"])) < 1e-9
            assert np.max(np.abs(got["E"][b].T - ref["E"])) < 1e-8
            assert np.max(np.abs(got["control"][b] - ref["control"])) < 1e-8, (got["control"][b], ref["control"])
            assert np.max(np.abs(U_dev[b] - pols[b].U)) < 1e-8
    eng.close()


@pytest.mark.parametrize("T", [8, 24, 7])
def test_level2_musigma_tile_aligned_and_ragged_cs(eng_mod, oracle, track, T):
    """μΣ-AIS moments: cs = 16 / 48 (multiples of the 16-row MFMA tile: no padding row, separate weighted-mean kernel) and
    cs = 14 (ragged: mean emitted by the scatter kernel's ones row) must agree with the oracle alike."""
    rng = np.random.default_rng(T)
    B, K, N, kind = 2, 320, 4, "musigmaaismppi"
    cs = 2 * T
    eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, cov=[0.0625, 0.1], track=track)
    envs, pols = zip(*[make_oracle(oracle, track, kind, 1, K, T, N=N) for _ in range(B)])
    eng.set_state(np.stack([e.state for e in envs]))
    for step in range(2):
        Z = rng.standard_normal((B, N, K, cs))
        got = eng.policy_step(Z, want_E=True)
        U_dev = eng.get_U()
        for b in range(B):
            ref = pols[b](envs[b], Z[b])
            assert ref["status"] == 0 and got["iters_run"][b] == ref["iters_run"]
            assert rel_err(got["cost"][b], ref["cost"]) < RTOL
            assert np.max(np.abs(got["E"][b].T - ref["E"])) < 1e-8
            assert np.max(np.abs(got["control"][b] - ref["control"])) < 1e-8
            assert np.max(np.abs(U_dev[b] - pols[b].U)) < 1e-8
    eng.close()


def test_level2_mppi_mountaincar_config1(eng_mod, oracle):
    """BASELINE config 1 (plumbing): MountainCar :mppi K=20 H=15 λ=0.1 Σ=[1.5]."""
    rng = np.random.default_rng(2)
    K, T = 20, 15
    env = oracle.OracleEnv("mountaincar")
    env.state = [-0.5, 0.0]
    pol = oracle.OraclePolicy("mppi", env, K, T, lam=0.1, U0=[0.0], cov=[1.5])
    eng = eng_mod.Engine("mountaincar", 0, "mppi", K, T, batch=1, lam=0.1, cov=[1.5])
    eng.set_state(np.array([[-0.5, 0.0]]))
    for step in range(3):
        Z = rng.standard_normal((T, K, 1))
        ref = pol(env, Z)
        got = eng.policy_step(Z[None], want_E=True)
        assert rel_err(got["cost"][0], ref["cost"]) < 1e-12
        assert np.max(np.abs(got["E"][0] - ref["E"])) < 1e-13
        assert abs(got["control"][0, 0] - ref["control"][0]) < 1e-12
        assert np.max(np.abs(eng.get_U()[0] - pol.U)) < 1e-12
        env.step(ref["control"])
        r = eng.env_step(got["control"])
        assert abs(r[0] - env.reward()) < 1e-12
        x, t, done = eng.get_state()
        assert np.max(np.abs(x[0] - env.state)) < 1e-13 and t[0] == env.e.t and done[0] == env.e.done
    eng.close()


def test_level2_mppi_car(eng_mod, oracle, track):
    rng = np.random.default_rng(4)
    K, T = 128, 12
    env = oracle.OracleEnv("car", 1, track=track)
    pol = oracle.OraclePolicy("mppi", env, K, T, lam=10.0, U0=[0.0, 0.0], cov=np.array([[0.0625, 0.02], [0.02, 0.1]]))
    eng = eng_mod.Engine("car", 1, "mppi", K, T, batch=1, lam=10.0, cov=np.array([[0.0625, 0.02], [0.02, 0.1]]), track=track)
    for step in range(2):
        Z = rng.standard_normal((T, K, 2))
        ref = pol(env, Z)
        got = eng.policy_step(Z[None], want_E=True)
        assert rel_err(got["cost"][0], ref["cost"]) < RTOL
        assert np.max(np.abs(got["E"][0] - ref["E"])) < 1e-12
        assert np.max(np.abs(got["control"][0] - ref["control"])) < 1e-9
    eng.close()


def test_device_rng_matches_oracle_philox(eng_mod, oracle, track):
    """Device Philox4x32-10 + Box-Muller == the oracle's generator (same counters / streams)."""
    K, T = 256, 10
    cs = 2 * T
    eng = eng_mod.Engine("car", 1, "gmppi", K, T, batch=2, lam=10.0, cov=[0.0625, 0.1], track=track, seed=20240000)
    for step in range(2):
        got = eng.policy_step(None, want_E=True)
        for b in range(2):
            z = oracle.philox_normals(20240000 + b + 1, step, 0, cs * K).reshape(K, cs)
            E = z * np.sqrt(np.tile([0.0625, 0.1], T))
            assert np.max(np.abs(got["E"][b] - E)) < 1e-13
    eng.close()


def test_device_rng_normals_full_size(eng_mod, oracle, track):
    """400 k normals per slot through the table-based Box-Muller (philox.h): every one within 1e-13 of the oracle's libm evaluation, tails
    included, and the fused in-kernel sampler (dense Σ) gives L times the same numbers."""
    K, T = 4096, 50
    cs = 2 * T
    eng = eng_mod.Engine("car", 1, "gmppi", K, T, batch=2, lam=10.0, cov=[0.0625, 0.1], track=track, seed=99)
    got = eng.policy_step(None, want_E=True)
    zmax = 0.0
    for b in range(2):
        z = oracle.philox_normals(99 + b + 1, 0, 0, cs * K).reshape(K, cs)
        zmax = max(zmax, float(np.abs(z).max()))
        assert np.max(np.abs(got["E"][b] - z * np.sqrt(np.tile([0.0625, 0.1], T)))) < 1e-13
    assert zmax > 4.5                                                   # the sample reaches into the tails
    eng.close()
    rng = np.random.default_rng(3)
    A = rng.standard_normal((cs, cs)) * 0.05
    Sig = A @ A.T + np.diag(np.tile([0.0625, 0.1], T))
    eng = eng_mod.Engine("car", 1, "gmppi", K, T, batch=2, lam=10.0, cov=Sig, track=track, seed=99)
    got = eng.policy_step(None, want_E=True)
    Lc = np.linalg.cholesky(Sig)
    for b in range(2):
        z = oracle.philox_normals(99 + b + 1, 0, 0, cs * K).reshape(K, cs)
        assert np.max(np.abs(got["E"][b] - z @ Lc.T)) < 1e-12
    eng.close()


@pytest.mark.parametrize("ncars,K,entry", [(1, 64, 0), (1, 64, 1), (1, 4096, 1), (1, 4096, 3), (3, 512, 3), (3, 512, 4)])
def test_nan_control_in_a_rollout_is_an_action_error(eng_mod, oracle, ncars, K, entry, track):
    """A NaN in pol.U reaches every rollout as a NaN action: the reference's env(a) throws "Action is not in action space" (car_racing.jl:239) -- the engine
    must report MPOPIS_ERR_ACTION (-3), not a finite cost.  Round 6 found that a NaN PEDAL alone did not: fmax / fmin (v_max_f64 / v_min_f64) return the other
    operand for a NaN, the drive force became 0 and the rollout stayed finite (tests/test_dynamics_shim.py found it on the CPU); steering entries always
    poisoned the state.  Entries 0 / 1 / 3 / 4 = steer and pedal of the first steps (and of the second car), one-wave and two-wave rollout kernels (K)."""
    from mpopis_amd._lib import MPOPISError
    T = 10
    cs = 2 * ncars * T
    eng = eng_mod.Engine("car", ncars, "gmppi", K, T, batch=2, lam=10.0, cov=np.tile([0.0625, 0.1], ncars), track=track, seed=11)
    got = eng.policy_step(None)                               # a clean step first: finite
    assert np.all(np.isfinite(got["cost"]))
    U = np.zeros((2, cs))
    U[1, entry] = np.nan                                      # slot 1 only
    eng.set_U(U)
    with pytest.raises(MPOPISError) as ei:
        eng.policy_step(None)
    assert ei.value.code == -3, str(ei.value)
    # the oracle says the same (single car: env(a) throws; its multi-car env does not check, like the reference's functor, multi-car_racing.jl:204 --
    # there the NaN state poisons the cost and the non-finite cost is the error)
    env = oracle.OracleEnv("car", ncars, track=track)
    pol = oracle.OraclePolicy("gmppi", env, 64, T, lam=10.0, U0=np.zeros(2 * ncars), cov=np.tile([0.0625, 0.1], ncars))
    pol.U = U[1]
    assert pol(env, np.random.default_rng(0).standard_normal((1, 64, cs)))["status"] == -3
    eng.set_U(np.zeros((2, cs)))                              # the handle keeps working
    got = eng.policy_step(None)
    assert np.all(np.isfinite(got["cost"])) and np.all(np.isfinite(got["control"]))
    eng.close()


def test_env_step_and_errors(eng_mod, oracle, track):
    from mpopis_amd._lib import MPOPISError
    eng = eng_mod.Engine("car", 3, "gmppi", 64, 5, batch=2, lam=10.0, cov=np.tile([0.0625, 0.1], 3), track=track)
    env = oracle.OracleEnv("car", 3, track=track)
    a = np.array([0.3, 0.5, -0.2, 1.0, 0.9, -1.0])
    for _ in range(5):
        r = eng.env_step(np.stack([a, -a]))
        env.step(a)
        assert abs(r[0] - env.reward()) < 1e-9 * abs(env.reward())
    assert np.max(np.abs(eng.get_state()[0][0] - env.state)) < 1e-10
    eng.close()
    eng = eng_mod.Engine("car", 1, "gmppi", 64, 5, batch=1, lam=10.0, cov=[0.0625, 0.1], track=track)
    with pytest.raises(MPOPISError) as ei:
        eng.env_step([[1.5, 0.0]])                         # "Action is not in action space" car_racing.jl:239
    assert ei.value.code == -3
    Z = np.random.default_rng(5).standard_normal((1, 1, 64, 10))
    U0 = eng.get_U()
    before = eng.policy_step(Z)
    with pytest.raises(MPOPISError) as ei:
        eng.set_Sigma(np.array([[1.0, 2.0], [2.0, 1.0]]))  # PosDefException
    assert ei.value.code == -2
    eng.set_U(U0)                                          # a refused set_Sigma leaves the handle as it was: the same step gives the same bits
    after = eng.policy_step(Z)
    for key in ("control", "cost", "weights"):
        assert np.array_equal(before[key], after[key]), key
    with pytest.raises(MPOPISError) as ei:
        eng.set_Sigma(np.eye(3))                           # "Covariance matrix size problem" :79
    assert ei.value.code == -1
    eng.close()


@pytest.mark.parametrize("kind,K,T,N", [("cemppi", 150, 20, 4), ("musigmaaismppi", 256, 20, 3), ("pmcmppi", 128, 15, 3), ("gmppi", 256, 25, 1)])
def test_level3_run_trials_car(eng_mod, oracle, track, kind, K, T, N):
    """Device-resident closed loop (simulate_car_racing trial loop) vs the oracle's run_trial: same Philox
    streams, so per-step actions and the per-trial records must agree."""
    B, steps, seed = 3, 30, 20240000
    eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, cov=[0.0625, 0.1], track=track, seed=seed)
    rec, acts = eng.run_trials(num_steps=steps, laps=2, log_actions=True)
    for b in range(B):
        env, pol = make_oracle(oracle, track, kind, 1, K, T, N=N)
        r = pol.run_trial(env, seed + b + 1, num_steps=steps, laps=2, log_actions=True)
        assert r["status"] == 0 and rec[b, 15] == 0
        assert rec[b, 1] == r["steps"] and rec[b, 14] == r["rollouts"]
        assert np.max(np.abs(acts[b] - r["actions"])) < 1e-6, np.max(np.abs(acts[b] - r["actions"]))
        ref = [r["rew"], r["steps"], r["rew_per_step"]] + r["lap_t"] + [r["mean_v"], r["max_v"], r["mean_beta"], r["max_beta"],
                                                                     r["beta_viol"], r["trk_viol"], r["crash_viol"]]
        assert rel_err(rec[b, :14], ref) < 1e-6, (rec[b, :14], ref)
    x, _, _ = eng.get_state()
    assert np.all(np.isfinite(x))
    eng.close()


def test_level3_run_trials_mountaincar(eng_mod, oracle):
    K, T = 20, 15
    eng = eng_mod.Engine("mountaincar", 0, "mppi", K, T, batch=2, lam=0.1, cov=[1.5], seed=5)
    eng.set_state(np.array([[-0.5, 0.0], [-0.45, 0.0]]))
    rec = eng.run_trials(num_steps=200, laps=0)
    for b, x0 in enumerate([-0.5, -0.45]):
        env = oracle.OracleEnv("mountaincar"); env.state = [x0, 0.0]
        pol = oracle.OraclePolicy("mppi", env, K, T, lam=0.1, U0=[0.0], cov=[1.5])
        r = pol.run_trial(env, 5 + b + 1, num_steps=200)
        assert rec[b, 1] == r["steps"], (rec[b], r)
        assert abs(rec[b, 0] - r["rew"]) < 1e-6 * abs(r["rew"])
    eng.close()


def test_level3_run_trials_state_noise(eng_mod, oracle, track):
    """simulate_car_racing's state_x/y/ψ_sigma (car_example.jl:38-40,224-236): position/heading noise after each real-env
    step, velocity rotated passively; same Philox draws on both sides."""
    K, T, N = 128, 15, 3
    sig = (0.3, 0.2, 0.02)
    eng = eng_mod.Engine("car", 1, "cemppi", K, T, batch=2, lam=10.0, ais_its=N, elite_threshold=0.8, cov=[0.0625, 0.1], track=track, seed=77)
    eng.set_state_noise(*sig)
    rec, acts = eng.run_trials(num_steps=12, laps=2, log_actions=True)
    xs, _, _ = eng.get_state()
    quiet = eng_mod.Engine("car", 1, "cemppi", K, T, batch=2, lam=10.0, ais_its=N, elite_threshold=0.8, cov=[0.0625, 0.1], track=track, seed=77)
    rec0 = quiet.run_trials(num_steps=12, laps=2)
    quiet.close()
    assert not np.allclose(rec[:, 0], rec0[:, 0])                       # the noise does change the closed loop
    for b in range(2):
        env, pol = make_oracle(oracle, track, "cemppi", 1, K, T, N=N)
        r = pol.run_trial(env, 77 + b + 1, num_steps=12, laps=2, log_actions=True, state_noise=sig)
        assert r["status"] == 0 and rec[b, 1] == r["steps"]
        assert abs(rec[b, 0] - r["rew"]) < 1e-7 * abs(r["rew"])
        assert np.max(np.abs(acts[b] - r["actions"])) < 1e-7
        assert np.max(np.abs(xs[b] - env.state)) < 1e-6
    eng.close()


_FUZZ = [  # (policy, ncars, K, T, N, B)  -- ragged / tiny / awkward shapes through every kernel
    ("gmppi", 1, 1, 1, 1, 1), ("gmppi", 4, 5, 3, 1, 2), ("mppi", 1, 3, 2, 1, 3), ("mppi", 2, 65, 7, 1, 1),
    ("imppi", 3, 17, 5, 3, 2), ("muaismppi", 1, 63, 1, 4, 1), ("musigmaaismppi", 1, 33, 4, 3, 2), ("musigmaaismppi", 2, 129, 9, 2, 1),
    ("musigmaaismppi", 4, 70, 6, 3, 1), ("cemppi", 1, 10, 3, 3, 2), ("cemppi", 2, 47, 5, 4, 1), ("pmcmppi", 1, 31, 3, 3, 2),
    ("pmcmppi", 3, 90, 4, 2, 1), ("cmamppi", 1, 40, 3, 3, 1), ("cmamppi", 2, 96, 4, 2, 2),
]


@pytest.mark.parametrize("kind,ncars,K,T,N,B", _FUZZ)
def test_level2_awkward_shapes(eng_mod, oracle, track, kind, ncars, K, T, N, B):
    """Shapes no BASELINE config uses: K = 1 / below a wave / not a multiple of 64, T = 1, 4 cars, tiny elites, several slots."""
    from mpopis_amd._lib import MPOPISError
    rng = np.random.default_rng(K * 131 + T * 17 + ncars)
    cs = 2 * ncars * T
    Neff = 1 if kind in ("gmppi", "mppi") else N
    eng = eng_mod.Engine("car", ncars, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8,
                         cma_sigma=0.75, cov=np.tile([0.0625, 0.1], ncars), track=track)
    envs, pols = zip(*[make_oracle(oracle, track, kind, ncars, K, T, N=N) for _ in range(B)])
    for b in range(B):                                           # different start states per slot
        st = envs[b].state; st[3] = 10.0 + 2.0 * b; st[1] = 1.5 * b; envs[b].state = st
    eng.set_state(np.stack([e.state for e in envs]))
    for step in range(2):
        if kind == "mppi":
            Z = rng.standard_normal((B, T, K, 2 * ncars))
        else:
            Z = rng.standard_normal((B, Neff, K, cs))
        di = rng.integers(0, K, (B, max(Neff - 1, 1), K)).astype(np.int32)
        du = rng.random((B, max(Neff - 1, 1), K))
        refs = [pols[b](envs[b], Z[b], di[b], du[b]) for b in range(B)]
        worst = min(r["status"] for r in refs)
        if worst:                                                 # e.g. rank-deficient elite covariance: same error code
            with pytest.raises(MPOPISError) as ei:
                eng.policy_step(Z, di, du)
            assert ei.value.code == worst
            break
        got = eng.policy_step(Z, di, du)
        U_dev = eng.get_U()
        for b in range(B):
            assert got["iters_run"][b] == refs[b]["iters_run"], (kind, b)
            assert rel_err(got["cost"][b], refs[b]["cost"]) < 1e-7, (kind, step, b)
            assert np.max(np.abs(got["control"][b] - refs[b]["control"])) < 1e-7
            assert np.max(np.abs(U_dev[b] - pols[b].U)) < 1e-7
    eng.close()


@pytest.mark.parametrize("variant", ["heavy_fast_steer", "coarse_dt", "odd_substeps"])
def test_level1_custom_car_params(eng_mod, oracle, track, variant):
    """mpopis_set_env_params with non-default CarRacingEnvParams / dt / δt (car_racing.jl:2-21,33-34): other masses, tyres,
    a steering rate beyond the small-angle range of the per-sub-step rotation (library sin/cos path), other sub-step counts."""
    rng = np.random.default_rng(5)
    K, T = 192, 20
    p = oracle.car_default_params()
    if variant == "heavy_fast_steer":
        p[0] = 2600.0; p[1] = 4800.0; p[7] = 1.2e5; p[8] = 2.2e5; p[9] = 0.8; p[10] = 1.0
        p[12] = np.deg2rad(400.0); p[11] = np.deg2rad(25.0); p[15] = 0.5; p[16] = 0.2      # δ_dot_max, δ_max, λ_brake, λ_drive
    elif variant == "coarse_dt":
        p[18] = 0.1; p[19] = 0.02                                # 5 sub-steps
    else:
        p[18] = 0.07; p[19] = 0.01                               # 7 sub-steps (odd: remainder of the 2-per-trip loop)
    env = oracle.OracleEnv("car", 1, params=p, track=track)
    pol = oracle.OraclePolicy("gmppi", env, K, T, lam=10.0, U0=[0.0, 0.0], cov=[0.0625, 0.1])
    eng = eng_mod.Engine("car", 1, "gmppi", K, T, batch=1, lam=10.0, cov=[0.0625, 0.1], track=track, env_params=p)
    E = rng.standard_normal((1, K, 2 * T)) * np.tile([0.6, 0.4], T)
    got = eng.rollout_costs(np.zeros((1, 2 * T)), E, x0=env.state[None])
    ref = pol.simulate_model(np.zeros(2 * T), E[0].T)
    assert rel_err(got[0], ref) < RTOL
    a = np.array([[0.9, -0.3]])
    for _ in range(5):                                           # real env step with the same parameters
        env.step(a[0]); r = eng.env_step(a)
        x, _, _ = eng.get_state()
        assert np.max(np.abs(x[0] - env.state)) < 1e-10 and abs(r[0] - env.reward()) < 1e-9 * abs(env.reward())
    eng.close()


def test_level1_cartpole_with_logger(eng_mod, oracle):
    """CartPole: simulate_model + trajectory logger, ss = 4."""
    rng = np.random.default_rng(31)
    K, T = 200, 15
    x0 = np.array([0.02, -0.1, 0.03, 0.2])
    env = oracle.OracleEnv("cartpole"); env.state = x0
    eng = eng_mod.Engine("cartpole", 0, "gmppi", K, T, batch=1, lam=0.1, cov=[1.5], log_trajectories=True)
    E = rng.standard_normal((1, K, T)) * 1.2
    U = rng.uniform(-0.5, 0.5, T)
    got = eng.rollout_costs(U[None], E, x0=x0[None])
    pol = oracle.OraclePolicy("gmppi", env, K, T, lam=0.1, U0=[0.0], cov=[1.5])
    ref, tr_ref = pol.simulate_model(U, E[0].T, log=True)
    assert np.array_equal(got[0], ref)                       # costs are small integers: exact
    tr = eng.get_trajectories()[0]
    assert rel_err(tr, tr_ref) < 1e-12
    eng.close()


@pytest.mark.parametrize("kind", ["mppi", "cemppi", "musigmaaismppi", "pmcmppi", "cmamppi"])
def test_level2_cartpole(eng_mod, oracle, kind):
    """pol(env) on CartPole with the simulate_cartpole defaults (cartpole_example.jl:35-50), closed loop for 4 MPC steps."""
    rng = np.random.default_rng(33)
    K, T, N = 20, 15, 5
    x0 = np.array([0.03, 0.0, -0.04, 0.1])
    env = oracle.OracleEnv("cartpole"); env.state = x0
    pol = oracle.OraclePolicy(kind, env, K, T, lam=0.1, U0=[0.0], cov=[1.5], N=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75)
    eng = eng_mod.Engine("cartpole", 0, kind, K, T, batch=1, lam=0.1, ais_its=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75, cov=[1.5])
    eng.set_state(x0[None])
    Neff = 1 if kind == "mppi" else N
    for step in range(4):
        if kind == "mppi":
            Z = rng.standard_normal((T, K, 1)); Zo, Ze = Z, Z[None]
        else:
            Z = rng.standard_normal((Neff, K, T)); Zo, Ze = Z, Z[None]
        ri = rng.integers(0, K, (max(1, Neff - 1), K)).astype(np.int32); ru = rng.random((max(1, Neff - 1), K))
        ref = pol(env, Zo, ri, ru)
        if ref["status"]:
            from mpopis_amd._lib import MPOPISError
            with pytest.raises(MPOPISError) as ei:
                eng.policy_step(Ze, ri[None], ru[None])
            assert ei.value.code == ref["status"]
            break
        got = eng.policy_step(Ze, ri[None], ru[None])
        assert got["iters_run"][0] == ref["iters_run"]
        assert np.array_equal(got["cost"][0], ref["cost"])
        assert np.max(np.abs(got["weights"][0] - ref["weights"])) < 1e-12
        assert abs(got["control"][0, 0] - ref["control"][0]) < 1e-9
        env.step(ref["control"])
        r = eng.env_step(ref["control"][None])               # same action on both sides keeps the loops aligned
        assert r[0] == env.reward()
        x, t, done = eng.get_state()
        assert np.max(np.abs(x[0] - env.state)) < 1e-13 and t[0] == env.e.t and done[0] == env.e.done
        eng.set_U(pol.U[None])
    eng.close()


@pytest.mark.parametrize("kind", ["mppi", "cemppi"])
def test_level3_run_trials_cartpole(eng_mod, oracle, kind):
    K, T, N = 20, 15, 5
    x0s = np.array([[0.01, 0.02, -0.03, 0.04], [-0.04, 0.0, 0.045, -0.02]])
    eng = eng_mod.Engine("cartpole", 0, kind, K, T, batch=2, lam=0.1, ais_its=N, elite_threshold=0.8, cov=[1.5], seed=21)
    eng.set_state(x0s)
    rec = eng.run_trials(num_steps=200, laps=0)
    for b in range(2):
        env = oracle.OracleEnv("cartpole"); env.state = x0s[b]
        pol = oracle.OraclePolicy(kind, env, K, T, lam=0.1, U0=[0.0], cov=[1.5], N=N, elite_threshold=0.8)
        r = pol.run_trial(env, 21 + b + 1, num_steps=200)
        assert rec[b, 15] == r["status"]
        assert rec[b, 1] == r["steps"] and rec[b, 0] == r["rew"], (rec[b], r)
    eng.close()


@pytest.mark.parametrize("K", [150, 400])        # m_elite = 30: the one-launch small-elite kernel (kernels_ce.hip); 80: the general scatter path
@pytest.mark.parametrize("est", ["mle", "ss", "lw", "rblw", "oas"])
def test_level2_cemppi_shrinkage_estimators(eng_mod, oracle, track, est, K):
    """CEMPPI with the LinearShrinkage estimators (:ss is the car harness default, src/examples/car_example.jl:66): device
    shrinkage vs the oracle's restatement (third-party CovarianceEstimation.jl formulas, unpinned on both sides)."""
    rng = np.random.default_rng(17)
    T, N = 12, 4
    cs = 2 * T
    env = oracle.OracleEnv("car", 1, track=track)
    pol = oracle.OraclePolicy("cemppi", env, K, T, lam=10.0, U0=[0.0, 0.0], cov=[0.0625, 0.1], N=N, elite_threshold=0.8, sigma_est=est)
    eng = eng_mod.Engine("car", 1, "cemppi", K, T, batch=1, lam=10.0, ais_its=N, elite_threshold=0.8, sigma_est=est, cov=[0.0625, 0.1], track=track)
    for step in range(2):
        Z = rng.standard_normal((N, K, cs))
        ref = pol(env, Z)
        got = eng.policy_step(Z[None], want_E=True)
        assert got["iters_run"][0] == ref["iters_run"]
        assert rel_err(got["cost"][0], ref["cost"]) < 1e-7
        assert np.max(np.abs(got["E"][0].T - ref["E"])) < 1e-8
        assert np.max(np.abs(got["control"][0] - ref["control"])) < 1e-8
    eng.close()


def test_cma_posdef_error_matches_reference_behaviour(eng_mod, oracle, track):
    """:cmamppi 1-car K=4096 H=50: the reference's scalar rank-µ quirk (:588-598) drives Σ indefinite after a few iterations,
    MvNormal(σ²Σ) throws PosDefException (:551).  Oracle and engine must fail the same way (code -2), not silently continue."""
    from mpopis_amd._lib import MPOPISError
    K, T, N = 4096, 50, 10
    env = oracle.OracleEnv("car", 1, track=track)
    pol = oracle.OraclePolicy("cmamppi", env, K, T, lam=10.0, U0=[0.0, 0.0], cov=[0.0625, 0.1], N=N, cma_sigma=0.75, nthreads=8)
    Z = np.stack([oracle.philox_normals(20240001, 0, n, 2 * T * K).reshape(K, 2 * T) for n in range(N)])
    r = pol(env, Z)
    assert r["status"] == -2 and 1 < r["iters_run"] < N
    eng = eng_mod.Engine("car", 1, "cmamppi", K, T, batch=1, lam=10.0, ais_its=N, cma_sigma=0.75, cov=[0.0625, 0.1], track=track, seed=20240000)
    with pytest.raises(MPOPISError) as ei:
        eng.policy_step(None)                              # device Philox stream == the oracle's injected normals
    assert ei.value.code == -2 and "PosDef" in str(ei.value)
    eng.close()


@pytest.mark.parametrize("ncars,T", [(1, 10), (3, 50)])
def test_cma_beyond_the_quadrature_matches_the_oracles_eigen_path(eng_mod, oracle, track, ncars, T):
    """:cmamppi forms Σ^-0.5 δw (:580-581) with a 64-node quadrature of x^-1/2 on [m, M] (m = 1 / tr(Σ^-1), M = ||Σ||_inf) that resolves m / M down to
    1e-14.  Until round 5 a proposal covariance beyond that was reported as MPOPIS_ERR_NUMERIC (-5) where the reference's eigen-based Σ^-0.5 returns a
    value; now the Lanczos launch hands such a slot to a one-workgroup Jacobi eigen-solve (kernels_invsqrt.hip, dense_invsqrt_slot).  Here: variances
    graded over 17 decades (Cholesky factor exists; cond(Σ) ~ 1e17) against the oracle, whose Σ^-0.5 is orc_sym_pow (eigen-decomposition, like the
    reference).  N = 2 -- ONE Σ^-0.5 δw, on the well-determined graded Σ, then the CMA update and the final draw from the updated Σ: strict parity (1e-7).
    N = 3 forms a second Σ^-0.5 on the UPDATED Σ (the graded diagonal plus O(0.01) in every entry, :598): its smallest eigenvalues lie below ε ||Σ||, no
    double-precision method determines them -- the reference's LAPACK eigen() included -- and two Jacobi orderings land 1e-6 ... 1e-4 apart on the control
    (measured); what is asserted there is what IS determined: no error code, the same iteration count, finite outputs, agreement to 1e-2."""
    from mpopis_amd._lib import MPOPISError
    cs = 2 * ncars * T
    K = 256
    cov = np.tile([0.0625, 0.1], ncars)
    d = np.tile([0.0625, 0.1], cs // 2) * 10.0 ** (-17.0 * np.arange(cs) / (cs - 1.0))
    S = np.diag(d)
    for N, tol in ((2, 1e-7), (3, 1e-2)):
        eng = eng_mod.Engine("car", ncars, "cmamppi", K, T, batch=2, lam=10.0, ais_its=N, cma_sigma=0.75, cov=cov, track=track, seed=5)
        eng.set_Sigma(S)
        Z = np.random.default_rng(3).standard_normal((2, N, K, cs))
        refs = []
        for b in range(2):
            env = oracle.OracleEnv("car", ncars, track=track)
            pol = oracle.OraclePolicy("cmamppi", env, K, T, lam=10.0, U0=np.zeros(2 * ncars), cov=cov, N=N, cma_sigma=0.75, nthreads=8)
            pol.Sigma = S
            refs.append((pol, pol(env, Z[b])))
        assert min(r["status"] for _, r in refs) == 0
        got = eng.policy_step(Z)                              # raises on any error code: never -5, the dense path answers where the quadrature cannot
        U = eng.get_U(); Sg = eng.get_Sigma()
        for b, (pol, r) in enumerate(refs):
            assert got["iters_run"][b] == r["iters_run"] == N
            assert np.all(np.isfinite(got["control"][b])) and np.all(np.isfinite(Sg[b]))
            assert np.max(np.abs(got["control"][b] - r["control"])) < tol
            assert np.max(np.abs(U[b] - pol.U)) < tol
            assert np.max(np.abs(Sg[b] - r["Sigma_last"])) < tol * np.max(np.abs(r["Sigma_last"]))
        if N == 3:                                            # the handle keeps working once a usable covariance is set
            eng.reset()
            eng.set_Sigma(np.diag(np.tile([0.0625, 0.1], cs // 2)))
            got = eng.policy_step(None)
            assert np.all(np.isfinite(got["control"])) and np.all(got["iters_run"] >= 1)
        eng.close()


def test_other_track_through_loader(eng_mod, oracle, tmp_path):
    """Track(infile; width, sample_factor) with a different centre line (ellipse, 640 points, sample_factor 8, width 9):
    variable P / lane width reach the kernels through the ABI (car_racing_tracks.jl:14-34)."""
    import mpopis_amd as M
    th = np.linspace(0, 2 * np.pi, 640, endpoint=False)
    pts = np.stack([120 * np.cos(th) - 120, 70 * np.sin(th)], 1)           # passes through the origin heading +y
    f = tmp_path / "ellipse.csv"
    np.savetxt(f, pts, delimiter=",")
    trk = M.Track(str(f), width=9.0, sample_factor=8)
    assert len(trk.xp) == 80
    K, T = 128, 30
    env = M.CarRacingEnv(track=trk)
    pol = M.GMPPI_Policy(env, num_samples=K, horizon=T, λ=10.0, U0=np.zeros(2), cov_mat=[0.0625, 0.1])
    otrack = (trk.xp, trk.yp, trk.wp)
    oenv = oracle.OracleEnv("car", 1, track=otrack)
    opol = oracle.OraclePolicy("gmppi", oenv, K, T, lam=10.0, U0=[0.0, 0.0], cov=[0.0625, 0.1])
    rng = np.random.default_rng(8)
    for _ in range(4):
        Z = rng.standard_normal((1, K, 2 * T))
        a = pol(env, Z=Z); ref = opol(oenv, Z)
        assert np.max(np.abs(a - ref["control"])) < 1e-8
        env(a); oenv.step(ref["control"])
        assert abs(M.reward(env) - oenv.reward()) < 1e-8 * abs(oenv.reward())
    pol.close()


@pytest.mark.parametrize("name", ["curve1", "curve2", "curve3", "curve4", "curve5", "cubic", "cubic1", "cubic2", "cubic3", "cubic4", "cubic5"])
def test_bundled_reference_tracks(eng_mod, oracle, name):
    """The reference's other centre-line files (src/envs/car_racing_tracks/*.csv) at sample_factor 20:
    few points (P = 12..26 < the neighbour-table width for some), open and closed shapes.  Rollout costs (anchored
    nearest-point search) and reward / within_track / dist of the resident env (full search) against the oracle."""
    import mpopis_amd as M
    trk = M.Track(name, width=4.0)              # narrow lane: a good share of the 3 s rollouts leaves it
    tx, ty, tw = trk.arrays()
    P = len(tx)
    assert 12 <= P <= 26
    rng = np.random.default_rng(P)
    K, T = 256, 30
    # start on the centre line at point 1, heading along the local direction, 10 m/s
    psi = np.arctan2(ty[2] - ty[1], tx[2] - tx[1])
    x0 = np.array([tx[1], ty[1], psi, 10.0, 0.0, 0.0, 0.0, 0.0])
    oenv = oracle.OracleEnv("car", 1, track=(tx, ty, tw)); oenv.state = x0
    opol = oracle.OraclePolicy("gmppi", oenv, K, T, lam=10.0, U0=[0.0, 0.0], cov=[0.0625, 0.1])
    eng = eng_mod.Engine("car", 1, "gmppi", K, T, batch=1, lam=10.0, cov=[0.0625, 0.1], track=(tx, ty, tw))
    E = rng.standard_normal((1, K, 2 * T)) * np.tile([0.5, 0.6], T)          # wide steering noise: many rollouts leave the lane
    got = eng.rollout_costs(np.zeros((1, 2 * T)), E, x0=x0[None])
    ref = opol.simulate_model(np.zeros(2 * T), E[0].T)
    assert (ref > 1e6).sum() > 0 and (ref < 1e6).sum() > 0                   # both sides of the lane penalty are exercised
    assert rel_err(got[0], ref) < RTOL
    # resident-env queries at scattered positions around the track (inside and outside the lane)
    for _ in range(40):
        i = rng.integers(0, P)
        pos = np.array([tx[i], ty[i]]) + rng.uniform(-30, 30, 2)
        st = x0.copy(); st[:2] = pos
        oenv.state = st
        eng.set_state(st[None])
        rew, within, dist, beta = eng.env_query()
        w_ref, d_ref = oracle.within_track((tx, ty, tw), pos)
        assert bool(within[0]) == bool(w_ref) and abs(dist[0, 0] - d_ref) <= 1e-12 * max(1.0, d_ref)
        assert abs(rew[0] - oenv.reward()) <= 1e-12 * abs(oenv.reward())
    eng.close()


@pytest.mark.parametrize("kind", ["cemppi", "musigmaaismppi", "pmcmppi", "cmamppi", "muaismppi"])
def test_level2_mountaincar_default_harness_config(eng_mod, oracle, kind):
    """simulate_mountaincar's defaults (mountaincar_example.jl:49-70): K=20, H=15 (cs=15, odd), λ=0.1, Σ=[1.5], N=5,
    λ_ais=0.1 -- odd / tiny sizes through every kernel (potrf n=15, MFMA tiles with padding, bitonic sort n=32, ...)."""
    rng = np.random.default_rng(31)
    K, T, N = 20, 15, 5
    env = oracle.OracleEnv("mountaincar")
    env.state = [-0.5, 0.0]
    pol = oracle.OraclePolicy(kind, env, K, T, lam=0.1, U0=[0.0], cov=[1.5], N=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75)
    eng = eng_mod.Engine("mountaincar", 0, kind, K, T, batch=2, lam=0.1, ais_its=N, lam_ais=0.1, elite_threshold=0.8, cma_sigma=0.75, cov=[1.5])
    eng.set_state(np.array([[-0.5, 0.0], [-0.5, 0.0]]))
    for step in range(3):
        Z = rng.standard_normal((N, K, T))
        di = rng.integers(0, K, (N, K)).astype(np.int32); du = rng.random((N, K))
        ref = pol(env, Z, di, du)
        got = eng.policy_step(np.stack([Z, Z]), np.stack([di[:N - 1], di[:N - 1]]), np.stack([du[:N - 1], du[:N - 1]]), want_E=True)
        assert ref["status"] == 0
        for b in range(2):
            assert got["iters_run"][b] == ref["iters_run"]
            assert rel_err(got["cost"][b], ref["cost"]) < 1e-8, (kind, step)
            assert np.max(np.abs(got["E"][b].T - ref["E"])) < 1e-8
            assert np.max(np.abs(got["control"][b] - ref["control"])) < 1e-8
        env.step(ref["control"]); eng.env_step(got["control"])
    eng.close()


def test_level2_odd_sizes_car(eng_mod, oracle, track):
    """K not a multiple of 16/64, odd K, H giving cs not a multiple of 16."""
    rng = np.random.default_rng(33)
    for kind, K, T, N in [("musigmaaismppi", 151, 7, 3), ("cemppi", 77, 9, 3), ("pmcmppi", 101, 5, 3), ("gmppi", 65, 11, 1)]:
        cs = 2 * T
        env, pol = make_oracle(oracle, track, kind, 1, K, T, N=N)
        eng = eng_mod.Engine("car", 1, kind, K, T, batch=1, lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=[0.0625, 0.1], track=track)
        Ne = 1 if kind == "gmppi" else N
        Z = rng.standard_normal((Ne, K, cs)); di = rng.integers(0, K, (max(Ne - 1, 1), K)).astype(np.int32); du = rng.random((max(Ne - 1, 1), K))
        ref = pol(env, Z, di, du); got = eng.policy_step(Z[None], di[None], du[None], want_E=True)
        assert got["iters_run"][0] == ref["iters_run"], kind
        assert rel_err(got["cost"][0], ref["cost"]) < 1e-8, kind
        assert np.max(np.abs(got["control"][0] - ref["control"])) < 1e-8, kind
        assert np.max(np.abs(eng.get_U()[0] - pol.U)) < 1e-8, kind
        eng.close()


@pytest.mark.parametrize("kind,K", [("cemppi", 150), ("cemppi", 400), ("cmamppi", 150)])
def test_elite_early_break(eng_mod, oracle, track, kind, K):
    """The elite early break (:458-461 / :566-569: max gap of the sorted elite costs < 10e-3 => leave the AIS loop, nothing of the iteration applied):
    slot 0 gets noise so small that all its costs coincide to 1e-6 and breaks in the first iteration, slot 1 runs on.  K = 150 takes the CE kernel that
    sorts and breaks itself (kernels_ce.hip), K = 400 and :cmamppi the sort kernels' tail."""
    T, N, B = 50, 4, 2
    cs = 2 * T
    rng = np.random.default_rng(77)
    eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cma_sigma=0.75, cov=[0.0625, 0.1], track=track)
    envs, pols = zip(*[make_oracle(oracle, track, kind, 1, K, T, N=N) for _ in range(B)])
    Z = rng.standard_normal((B, N, K, cs))
    Z[0] *= 1e-9
    di = rng.integers(0, K, (B, N - 1, K)).astype(np.int32)
    du = rng.random((B, N - 1, K))
    refs = [pols[b](envs[b], Z[b], di[b], du[b]) for b in range(B)]
    got = eng.policy_step(Z, di, du)
    assert refs[0]["iters_run"] == 1 and refs[1]["iters_run"] == N          # the scenario is what it claims to be
    U_dev = eng.get_U()
    for b in range(B):
        assert got["iters_run"][b] == refs[b]["iters_run"]
        assert rel_err(got["cost"][b], refs[b]["cost"]) < 1e-7
        assert np.max(np.abs(got["control"][b] - refs[b]["control"])) < 1e-7
        assert np.max(np.abs(U_dev[b] - pols[b].U)) < 1e-7
    eng.close()
