"""MultiCarRacingEnv with 5..8 cars on the device against the CPU oracle: the rollout kernels' costs (ragged K, far-out samples, cars within
collision distance, γ != 0, the trajectory logger), one- and two-wave kernels bit for bit, every policy through the C ABI with injected noise,
the covariance scatter past 512 rows (cs = 600 and 800), device noise at 64 resident slots under every overlap schedule, and the closed loop.
Tolerances as tests/test_gpu_parity.py: 1e-8 relative on costs (the policy cases go through tests/test_gpu_baseline_shapes.run_case at its 1e-7),
integers bit-exact.  The oracle holds at most 8 cars."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

from tests.test_gpu_baseline_shapes import run_case, start_states, sig_err
from tests.test_gpu_nes import nes_case

pytestmark = pytest.mark.gpu

RTOL = 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-9)))


def make_oracle(oracle, track, kind, ncars, K, T, alpha=1.0):
    env = oracle.OracleEnv("car", ncars, track=track)
    pol = oracle.OraclePolicy(kind, env, K, T, lam=10.0, alpha=alpha, U0=np.zeros(2 * ncars), cov=np.tile([0.0625, 0.1], ncars), N=1, nthreads=8)
    return env, pol


def close_starts(env, ncars, B):
    """slot 0: the reset grid; slot 1: cars 0/1 coincident, car 2 3 m from car 0 (the -11000 contact term), the rest faster and shifted"""
    x0 = np.stack([env.state for _ in range(B)])
    x0[1, 8 * 1:8 * 1 + 2] = x0[1, 0:2]
    x0[1, 8 * 2] = x0[1, 0] + 3.0
    x0[1, 8 * 2 + 1] = x0[1, 1]
    for c in range(3, ncars):
        x0[1, 8 * c + 1] += 1.5 * c
        x0[1, 8 * c + 3] = 13.0
    return x0


@pytest.mark.parametrize("ncars,K,T,alpha", [(5, 101, 20, 1.0), (6, 70, 13, 1.0), (7, 130, 11, 0.8), (8, 53, 16, 1.0)])
def test_rollout_costs_against_the_oracle(eng_mod, oracle, track, ncars, K, T, alpha):
    rng = np.random.default_rng(500 + ncars)
    B, cs = 2, 2 * ncars * T
    env, pol = make_oracle(oracle, track, "gmppi", ncars, K, T, alpha)
    eng = eng_mod.Engine("car", ncars, "gmppi", K, T, batch=B, lam=10.0, alpha=alpha, cov=np.tile([0.0625, 0.1], ncars), track=track)
    U = rng.uniform(-0.3, 0.3, (B, cs))
    U[:, 1::2] += 0.3
    E = rng.standard_normal((B, K, cs)) * np.tile([0.25, 0.32], ncars * T)
    E[0, :5] *= 8.0                                       # far-out samples: clamps, off-track, β penalties
    x0 = close_starts(env, ncars, B)
    kw = {}
    if alpha != 1.0:
        A = rng.standard_normal((cs, cs))
        kw = dict(U_orig=rng.uniform(-0.3, 0.3, (B, cs)), Sigma_inv=A @ A.T / cs + np.eye(cs))
    got = eng.rollout_costs(U, E, x0=x0, **kw)
    for b in range(B):
        env.state = x0[b]
        if alpha != 1.0:
            ref = pol.simulate_model(U[b], E[b].T, Sigma_inv=kw["Sigma_inv"], U_orig=kw["U_orig"][b])
        else:
            ref = pol.simulate_model(U[b], E[b].T)
        assert rel_err(got[b], ref) < RTOL, (ncars, b, rel_err(got[b], ref))
        if b == 1:
            assert np.all(ref < -10000.0) or np.all(ref > 10000.0)      # the contact term is in every rollout of slot 1
    eng.close()


def test_trajectory_logger_six_cars(eng_mod, oracle, track):
    rng = np.random.default_rng(66)
    K, T, ncars = 40, 9, 6
    env, pol = make_oracle(oracle, track, "gmppi", ncars, K, T)
    eng = eng_mod.Engine("car", ncars, "gmppi", K, T, batch=1, lam=10.0, cov=np.tile([0.0625, 0.1], ncars), track=track, log_trajectories=True)
    E = rng.standard_normal((1, K, 2 * ncars * T)) * 0.3
    got = eng.rollout_costs(np.zeros((1, 2 * ncars * T)), E, x0=env.state[None])
    tr = eng.get_trajectories()[0]
    cost, ref = pol.simulate_model(np.zeros(2 * ncars * T), E[0].T, log=True)
    assert rel_err(got[0], cost) < RTOL
    assert rel_err(tr, ref) < RTOL
    eng.close()


def _duo_run(env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "many_cars_duo_case.py")], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_one_and_two_wave_kernels_agree_bit_for_bit():
    one = _duo_run({"MPOPIS_ROLLOUT_DUO": "0"})
    duo = _duo_run({"MPOPIS_ROLLOUT_DUO": "1000000"})
    assert set(one) == set(duo) == {"cars5", "cars8", "cars5_big", "cars8_big"}
    for name in one:
        assert duo[name] == one[name], name


@pytest.mark.parametrize("ncars", [5, 8])
@pytest.mark.parametrize("kind,est", [("gmppi", "mle"), ("imppi", "mle"), ("muaismppi", "mle"), ("musigmaaismppi", "mle"), ("pmcmppi", "mle"),
                                      ("cemppi", "mle"), ("cemppi", "ss"), ("cmamppi", "mle")])
def test_policy_parity(eng_mod, oracle, track, ncars, kind, est):
    """control, U, costs, weights, E, iteration counts, :pmcmppi resampling indices (bit-exact) and Σ′ of the last iteration, 2 MPC steps"""
    # (:pmcmppi: the resampled set collapses onto a few columns, Σ′ is rank-deficient up to the 1e-8 ridge, and its rounding is amplified on
    #  both sides: the wider Σ′ tolerance of tests/test_gpu_baseline_shapes.test_cs300_scatter_and_global_potrf)
    run_case(eng_mod, oracle, track, kind, ncars, K=160, T=8, N=3, B=2, steps=2, sigma_est=est, check_sigma=kind not in ("gmppi", "imppi", "muaismppi"),
             sig_tol=1e-6 if kind == "pmcmppi" else 1e-7)


@pytest.mark.parametrize("ncars", [5, 8])
def test_nes_parity(eng_mod, oracle, track, ncars):
    # (step factor 1e-7 as for 3 cars in tests/test_gpu_nes.py: the default 0.01 against multi-car costs of ~1e7 drives Σ′ to cond ~1e10, where no
    #  two FP64 evaluation orders agree)
    nes_case(eng_mod, oracle, track, ncars=ncars, K=256, T=8, N=3, B=2, steps=2, sf=1e-7)


@pytest.mark.parametrize("ncars", [6, 8])
@pytest.mark.parametrize("kind,est", [("musigmaaismppi", "mle"), ("cemppi", "ss"), ("pmcmppi", "mle")])
def test_scatter_past_512_rows(eng_mod, oracle, track, ncars, kind, est):
    """cs = 600 / 800 at H = 50: the 8-wave covariance scatter, the global Cholesky, L·Z, the :ss shrinkage, the elite gather, resampling"""
    run_case(eng_mod, oracle, track, kind, ncars, K=256, T=50, N=2, B=1, steps=1, sigma_est=est, sig_tol=1e-6 if kind == "pmcmppi" else 1e-7)


def test_device_rng_64_slots_six_cars(eng_mod, oracle, track):
    """64 resident slots, device Philox streams: slots 0, 31, 63 against the oracle fed the same streams; every overlap schedule bit-identical"""
    ncars, K, T, N, B, seed = 6, 128, 8, 3, 64, 77000
    cs = 2 * ncars * T
    cov = np.tile([0.0625, 0.1], ncars)
    x0 = np.repeat(start_states(oracle, track, ncars, 2), B // 2, axis=0)
    res = {}
    for ov in (1, 2, 4):
        eng = eng_mod.Engine("car", ncars, "musigmaaismppi", K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, cov=cov, track=track, seed=seed)
        eng.set_overlap(ov)
        eng.set_state(x0)
        got = eng.policy_step(None, want_E=True)
        res[ov] = (got["control"].copy(), got["cost"].copy(), eng.get_U().copy(), eng.get_Sigma().copy())
        eng.close()
    for ov in (2, 4):
        for a, b in zip(res[1], res[ov]):
            assert np.array_equal(a, b), ov
    control, cost, U, Sig = res[1]
    for b in (0, 31, 63):
        env = oracle.OracleEnv("car", ncars, track=track)
        env.state = x0[b]
        pol = oracle.OraclePolicy("musigmaaismppi", env, K, T, lam=10.0, U0=np.zeros(2 * ncars), cov=cov, N=N, lam_ais=20.0, nthreads=8)
        Z = np.stack([oracle.philox_normals(seed + b + 1, 0, n, cs * K).reshape(K, cs) for n in range(N)])
        ref = pol(env, Z)
        assert ref["status"] == 0
        assert rel_err(cost[b], ref["cost"]) < 1e-7, b
        assert np.max(np.abs(control[b] - ref["control"])) < 1e-7, b
        assert np.max(np.abs(U[b] - pol.U)) < 1e-7, b
        assert sig_err(Sig[b], ref["Sigma_last"]) < 1e-7, b


@pytest.mark.parametrize("ncars,kind", [(5, "musigmaaismppi"), (8, "gmppi")])
def test_closed_loop_against_the_oracle(eng_mod, oracle, track, ncars, kind):
    K, T, N, B, steps, seed = 128, 10, 3, 2, 25, 9100
    cov = np.tile([0.3, 0.4], ncars)                      # wide enough for contacts between cars (C Viol)
    eng = eng_mod.Engine("car", ncars, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, cov=cov, track=track, seed=seed)
    env0 = oracle.OracleEnv("car", ncars, track=track)
    x0 = close_starts(env0, ncars, B)
    x0[1, 8 * 1:8 * 1 + 2] += [2.5, 0.0]                  # 2.5 m apart: contact, not coincident
    eng.set_state(x0)
    rec, acts = eng.run_trials(num_steps=steps, laps=2, log_actions=True)
    eng.close()
    crash = 0.0
    for b in range(B):
        env = oracle.OracleEnv("car", ncars, track=track)
        env.state = x0[b]
        pol = oracle.OraclePolicy(kind, env, K, T, lam=10.0, U0=np.zeros(2 * ncars), cov=cov, N=N, lam_ais=20.0, nthreads=8)
        r = pol.run_trial(env, seed + b + 1, num_steps=steps, laps=2, log_actions=True)
        assert r["status"] == 0 and rec[b, 15] == 0
        n = int(r["steps"])
        assert rec[b, 1] == r["steps"]
        assert rec[b, 14] == r["rollouts"]
        assert np.max(np.abs(acts[b][:n] - r["actions"][:n])) < 1e-6
        ref = np.array([r["rew"], r["steps"], r["rew_per_step"]] + r["lap_t"] + [r["mean_v"], r["max_v"], r["mean_beta"], r["max_beta"], r["beta_viol"], r["trk_viol"], r["crash_viol"]])
        assert np.array_equal(rec[b, 11:14], ref[11:14]), (rec[b, 11:14], ref[11:14])
        assert np.max(np.abs(rec[b, :11] - ref[:11]) / np.maximum(1.0, np.abs(ref[:11]))) < 1e-6, (rec[b, :11], ref[:11])
        crash += r["crash_viol"]
    assert crash > 0                                      # the contact branch was taken


def test_env_step_and_query_eight_cars(eng_mod, oracle, track):
    ncars, B = 8, 2
    rng = np.random.default_rng(8)
    eng = eng_mod.Engine("car", ncars, "gmppi", 16, 4, batch=B, lam=10.0, cov=np.tile([0.0625, 0.1], ncars), track=track)
    env0 = oracle.OracleEnv("car", ncars, track=track)
    x0 = close_starts(env0, ncars, B)
    x0[1, 8 * 7] += 40.0                                  # car 7 of slot 1 off the track
    eng.set_state(x0)
    envs = []
    for b in range(B):
        e = oracle.OracleEnv("car", ncars, track=track)
        e.state = x0[b]
        envs.append(e)
    for step in range(6):
        a = np.clip(rng.uniform(-0.5, 0.9, (B, 2 * ncars)), -1, 1)
        rew = eng.env_step(a)
        r_q, within, dist, beta = eng.env_query()
        xs = eng.get_state()[0]
        for b in range(B):
            envs[b].step(a[b])
            ref_rew = envs[b].reward()
            assert abs(rew[b] - ref_rew) <= 1e-9 * max(1.0, abs(ref_rew)), (step, b, rew[b], ref_rew)
            assert abs(r_q[b] - envs[b].reward()) <= 1e-9 * max(1.0, abs(ref_rew))
            assert np.max(np.abs(xs[b] - envs[b].state)) < 1e-9
            s = envs[b].state.reshape(ncars, 8)
            win = [oracle.within_track(track, s[c, :2]) for c in range(ncars)]
            assert bool(within[b]) == all(w[0] for w in win)
            assert np.max(np.abs(dist[b] - [w[1] for w in win])) < 1e-9
            assert np.max(np.abs(beta[b] - np.arctan2(s[:, 4], s[:, 3]))) < 1e-12
    assert not within[1]
    eng.close()


def test_simulate_car_racing_eight_cars():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import examples
    rec, summ = examples.simulate_car_racing(num_trials=2, num_steps=20, num_cars=8, policy_type=":cemppi", num_samples=64, horizon=10,
                                             ais_its=2, seed=5, quiet=True)
    assert rec.shape == (2, 18) and np.all(rec[:, 2] >= 1)
    # the summary table carries C Viol for more than one car: Reward, Steps, Reward/Step, 2 laps, 6 speed / β / violation columns, C Viol, Ex Time
    assert summ["AVE"].shape == (3 + 2 + 6 + 1 + 1,)
