"""Per-slot λ, α, λ_ais, σ and pol.Σ (mpopis_set_slot_hyper / mpopis_set_Sigma_slots): slot b of one handle must behave like a handle
created with that slot's values.  Checked against the CPU oracle (one OraclePolicy per slot) with injected noise and with the device RNG,
under the part-chain schedules, through every entry point that runs a policy, and back to the shared values.  Tolerances are those of
the shared-value tests they mirror (tests/test_gpu_parity.py, tests/test_gpu_nes.py)."""
import os
import types
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-8
LAM = np.array([10.0, 2.5, 40.0])
ALPHA = np.array([1.0, 0.9, 0.5])
LAM_AIS = np.array([20.0, 5.0, 60.0])
SIG = np.array([0.75, 0.4, 1.2])
RHO = np.array([0.0, 0.5, 0.8])
COV0 = [0.0625, 0.1]
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


def sig_err(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(np.diag(b))))


def d_of(b):
    return np.array([0.0625 * (1 + b), 0.1 / (1 + b)])


def sigma_of(b, T, as_=2):
    """Σ_b: d_bj ρ_b^|t-u| between step t and step u of action j, 0 between different actions (slot 0 diagonal, the others dense)"""
    b = b % 3
    cs = as_ * T
    S = np.zeros((cs, cs))
    d = d_of(b)
    for t in range(T):
        for u in range(T):
            for j in range(as_):
                S[t * as_ + j, u * as_ + j] = d[j % 2] * RHO[b] ** abs(t - u)
    return S


def cyc(v, B):
    return np.array([v[b % 3] for b in range(B)])


def slot_states(oracle, track, B):
    """slot 1 starts from the modified state of test_level2_policy_step"""
    out = []
    for b in range(B):
        e = oracle.OracleEnv("car", 1, track=track)
        if b % 3 == 1:
            s = e.state; s[3] = 14.0; s[1] = 3.0; e.state = s
        out.append(e)
    return out


def slot_oracles(oracle, track, kind, K, T, N, B, per_slot_sigma):
    envs = slot_states(oracle, track, B)
    pols = []
    for b in range(B):
        p = oracle.OraclePolicy(kind, envs[b], K, T, lam=LAM[b % 3], alpha=ALPHA[b % 3], U0=np.zeros(2), cov=COV0,
                                N=N, lam_ais=LAM_AIS[b % 3], elite_threshold=0.8, cma_sigma=SIG[b % 3], nthreads=8)
        if per_slot_sigma:
            p.Sigma = sigma_of(b, T)
        pols.append(p)
    return envs, pols


def slot_engine(eng_mod, track, kind, K, T, N, B, per_slot_sigma, seed=0, **kw):
    eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cma_sigma=0.75, cov=COV0,
                         track=track, seed=seed, **kw)
    eng.set_slot_hyper(lam=cyc(LAM, B), alpha=cyc(ALPHA, B), lam_ais=cyc(LAM_AIS, B), cma_sigma=cyc(SIG, B))
    if per_slot_sigma:
        eng.set_Sigma_slots(np.stack([sigma_of(b, T) for b in range(B)]))
    return eng


# ---- 1. parity per slot against the oracle, injected noise -----------------------------------------------------------------------------------

@pytest.mark.parametrize("per_slot_sigma", [False, True], ids=["sharedSigma", "slotSigma"])
@pytest.mark.parametrize("kind", ["gmppi", "imppi", "muaismppi", "musigmaaismppi", "cemppi", "pmcmppi", "cmamppi"])
def test_policy_step_per_slot(eng_mod, oracle, track, kind, per_slot_sigma):
    rng = np.random.default_rng(11)
    B, K, T, N = 3, 192, 10, 4
    cs = 2 * T
    Neff = 1 if kind == "gmppi" else N
    eng = slot_engine(eng_mod, track, kind, K, T, N, B, per_slot_sigma)
    envs, pols = slot_oracles(oracle, track, kind, K, T, N, B, per_slot_sigma)
    eng.set_state(np.stack([e.state for e in envs]))
    sigma_fixed = kind in ("gmppi", "imppi", "muaismppi")
    for step in range(2):
        Z = rng.standard_normal((B, Neff, K, cs))
        di = rng.integers(0, K, (B, max(Neff - 1, 1), K)).astype(np.int32)
        du = rng.random((B, max(Neff - 1, 1), K))
        got = eng.policy_step(Z, di, du, want_E=True)
        U_dev, Sig_dev = eng.get_U(), eng.get_Sigma()
        for b in range(B):
            ref = pols[b](envs[b], Z[b], di[b], du[b])
            assert ref["status"] == 0
            assert got["iters_run"][b] == ref["iters_run"]
            if kind == "pmcmppi":
                assert np.array_equal(got["res_idx0"][b][:Neff - 1], ref["res_idx0"][:Neff - 1])
            errs = dict(cost=rel_err(got["cost"][b], ref["cost"]), w=np.max(np.abs(got["weights"][b] - ref["weights"])),
                        E=np.max(np.abs(got["E"][b].T - ref["E"])), control=np.max(np.abs(got["control"][b] - ref["control"])),
                        U=np.max(np.abs(U_dev[b] - pols[b].U)), Sigma=sig_err(Sig_dev[b], ref["Sigma_last"]))
            print("[slot_hyper] %s slotSigma=%d step %d slot %d: %s" % (kind, per_slot_sigma, step, b, " ".join("%s=%.2e" % kv for kv in errs.items())))
            assert errs["cost"] < RTOL, (kind, step, b)
            assert errs["w"] < 1e-9
            assert errs["E"] < 1e-8
            assert errs["control"] < 1e-8, (got["control"][b], ref["control"])
            assert errs["U"] < 1e-8
            assert errs["Sigma"] < 1e-8
            if sigma_fixed:                                    # each slot's own pol.Σ comes back
                want = sigma_of(b, T) if per_slot_sigma else np.diag(np.tile(COV0, T))
                assert sig_err(Sig_dev[b], want) < 1e-8
        c = got["control"]                                     # the slots really ran different policies
        assert not np.allclose(c[0], c[1]) and not np.allclose(c[0], c[2]) and not np.allclose(c[1], c[2])
    eng.close()


# ---- 2. :mppi and :nesmppi -----------------------------------------------------------------------------------------------------------------

def test_mppi_mountaincar_per_slot(eng_mod, oracle):
    rng = np.random.default_rng(2)
    K, T, B = 20, 15, 2
    lam, cov, x0 = [0.1, 0.3], [1.5, 0.8], [[-0.5, 0.0], [-0.45, 0.0]]
    envs, pols = [], []
    for b in range(B):
        e = oracle.OracleEnv("mountaincar"); e.state = x0[b]
        envs.append(e); pols.append(oracle.OraclePolicy("mppi", e, K, T, lam=lam[b], U0=[0.0], cov=[cov[b]]))
    eng = eng_mod.Engine("mountaincar", 0, "mppi", K, T, batch=B, lam=0.1, cov=[1.5])
    eng.set_slot_hyper(lam=lam)
    eng.set_Sigma_slots(np.array(cov).reshape(B, 1, 1))
    eng.set_state(np.array(x0))
    for step in range(3):
        Z = rng.standard_normal((B, T, K, 1))
        got = eng.policy_step(Z, want_E=True)
        U_dev = eng.get_U()
        rew = eng.env_step(got["control"])
        x, t, done = eng.get_state()
        for b in range(B):
            ref = pols[b](envs[b], Z[b])
            assert rel_err(got["cost"][b], ref["cost"]) < 1e-12
            assert np.max(np.abs(got["E"][b] - ref["E"])) < 1e-13
            assert abs(got["control"][b, 0] - ref["control"][0]) < 1e-12
            assert np.max(np.abs(U_dev[b] - pols[b].U)) < 1e-12
            envs[b].step(ref["control"])
            assert abs(rew[b] - envs[b].reward()) < 1e-12
            assert np.max(np.abs(x[b] - envs[b].state)) < 1e-13 and t[b] == envs[b].e.t and done[b] == envs[b].e.done
    eng.close()


def test_nesmppi_per_slot(eng_mod, oracle, track):
    from tests.helpers.nes_ref import nes_ref
    # the cost comparison, its tolerance and the start states are the shared-value test's own objects, not copies that could drift from them
    # (tests/test_gpu_nes.py takes start_states from tests/test_gpu_baseline_shapes.py the same way)
    from tests.test_gpu_nes import nes_cost_err, TOL
    from tests.test_gpu_baseline_shapes import start_states
    rng = np.random.default_rng(4321)
    B, K, T, N = 2, 256, 10, 4
    cs = 2 * T
    sf, lam = [0.01, 0.03], [10.0, 2.5]
    Sig = [sigma_of(1, T), sigma_of(2, T)]                     # both dense: per-slot A0 = sqrt(Σ_b) and Σ_b^-1
    eng = eng_mod.Engine("car", 1, "nesmppi", K, T, batch=B, lam=10.0, ais_its=N, step_factor=0.01, cov=COV0, track=track)
    eng.set_slot_hyper(lam=lam, step_factor=sf)
    eng.set_Sigma_slots(np.stack(Sig))
    x0 = start_states(oracle, track, 1, B)
    eng.set_state(x0)
    envs, pols = [], []
    for b in range(B):
        e = oracle.OracleEnv("car", 1, track=track); e.state = x0[b]
        p = oracle.OraclePolicy("gmppi", e, K, T, lam=lam[b], alpha=1.0, U0=np.zeros(2), cov=COV0, N=1, nthreads=8)
        p.Sigma = Sig[b]
        envs.append(e); pols.append(p)
    worst = dict(cost=0.0, control=0.0, U=0.0, E=0.0, w=0.0, Sigma=0.0)
    for step in range(2):
        Z = rng.standard_normal((B, N, K, cs))
        got = eng.policy_step(Z, want_E=True)
        U_dev, Sig_dev = eng.get_U(), eng.get_Sigma()
        for b in range(B):
            U_orig = pols[b].U
            ref = nes_ref(pols[b], envs[b], Z[b], N, sf[b], lam[b])
            assert got["iters_run"][b] == ref["iters_run"]
            worst["cost"] = max(worst["cost"], nes_cost_err(pols[b], U_orig, got["cost"][b], got["E"][b].T, ref, 0.0, worst))
            worst["w"] = max(worst["w"], float(np.max(np.abs(got["weights"][b] - ref["weights"]))))
            worst["E"] = max(worst["E"], float(np.max(np.abs(got["E"][b].T - ref["E"]))))
            worst["control"] = max(worst["control"], float(np.max(np.abs(got["control"][b] - ref["control"]))))
            worst["U"] = max(worst["U"], float(np.max(np.abs(U_dev[b] - ref["U"]))))
            worst["Sigma"] = max(worst["Sigma"], sig_err(Sig_dev[b], ref["Sigma_last"]))
    eng.close()
    print("[slot_hyper] nesmppi: %s" % " ".join("%s=%.2e" % kv for kv in worst.items()))
    for key in ("cost", "control", "U", "E", "w"):
        assert worst[key] < TOL, worst
    assert worst["Sigma"] < 1e-8, worst


# ---- 3. device RNG, first draw ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [10, 72], ids=["cs20_fused", "cs144_through_memory"])
def test_first_draw_dense_per_slot(eng_mod, oracle, track, T):
    B, K, seed = 3, 128, 20240000
    cs = 2 * T
    eng = eng_mod.Engine("car", 1, "gmppi", K, T, batch=B, lam=10.0, cov=COV0, track=track, seed=seed)
    Sig = [sigma_of(b + 1, T) for b in range(B)]               # ρ = 0.5, 0.8, 0: two dense slots make the whole handle dense
    eng.set_Sigma_slots(np.stack(Sig))
    got = eng.policy_step(None, want_E=True)
    for b in range(B):
        z = oracle.philox_normals(seed + b + 1, 0, 0, cs * K).reshape(K, cs)
        err = np.max(np.abs(got["E"][b] - z @ np.linalg.cholesky(Sig[b]).T))
        print("[slot_hyper] first draw cs=%d slot %d: %.2e" % (cs, b, err))
        assert err < 1e-12
    eng.close()


def test_first_draw_diagonal_per_slot(eng_mod, oracle, track):
    B, K, T, seed = 3, 128, 10, 20240000
    cs = 2 * T
    eng = eng_mod.Engine("car", 1, "gmppi", K, T, batch=B, lam=10.0, cov=COV0, track=track, seed=seed)
    eng.set_Sigma_slots(np.stack([d_of(b) for b in range(B)]))  # (B, as) vectors: every slot diagonal, each its own sqrt(diag)
    got = eng.policy_step(None, want_E=True)
    for b in range(B):
        z = oracle.philox_normals(seed + b + 1, 0, 0, cs * K).reshape(K, cs)
        assert np.max(np.abs(got["E"][b] - z * np.sqrt(np.tile(d_of(b), T)))) < 1e-13
    eng.close()


# ---- 4. schedules -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["cemppi", "musigmaaismppi"])
def test_part_chain_schedule_bit_identical(eng_mod, oracle, track, kind):
    B, K, T, N = 6, 256, 10, 4
    x0 = np.stack([e.state for e in slot_states(oracle, track, B)])
    outs = []
    for overlap in (1, 3):
        eng = slot_engine(eng_mod, track, kind, K, T, N, B, True, seed=77)
        eng.set_overlap(overlap)
        eng.set_state(x0)
        steps = []
        for step in range(2):
            got = eng.policy_step(None)
            steps.append((got["control"], got["cost"], eng.get_U()))
        outs.append(steps)
        eng.close()
    for step in range(2):
        for b in range(B):
            for i in range(3):
                assert np.array_equal(outs[0][step][i][b], outs[1][step][i][b]), (kind, step, b, i)
    assert not np.allclose(outs[0][0][0][0], outs[0][0][0][1])


# ---- 5. back to shared ------------------------------------------------------------------------------------------------------------------------

def test_back_to_shared_is_a_never_switched_handle(eng_mod, oracle, track):
    B, K, T, N, kind, seed = 3, 256, 10, 4, "musigmaaismppi", 31
    x0 = np.stack([e.state for e in slot_states(oracle, track, B)])
    kw = dict(lam=10.0, ais_its=N, lam_ais=20.0, cov=COV0, track=track, seed=seed)
    eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, **kw)
    eng.set_state(x0)
    first = eng.policy_step(None)
    eng.set_slot_hyper(lam=LAM, alpha=ALPHA, lam_ais=LAM_AIS)
    eng.set_Sigma_slots(np.stack([sigma_of(b, T) for b in range(B)]))
    switched = eng.policy_step(None)
    assert not np.allclose(switched["control"][1], switched["control"][2])
    eng.set_slot_hyper()                                       # four NULLs: the shared scalars
    eng.set_Sigma(COV0)                                        # the shared Σ
    h = eng.get_slot_hyper()
    assert np.array_equal(h["lam"], [10.0] * B) and np.array_equal(h["alpha"], [1.0] * B) and np.array_equal(h["lam_ais"], [20.0] * B)
    eng.seed(seed); eng.set_state(x0); eng.set_U(np.zeros((B, 2 * T)))
    again = eng.policy_step(None)
    U_again = eng.get_U()
    fresh = eng_mod.Engine("car", 1, kind, K, T, batch=B, **kw)
    fresh.set_state(x0)
    ref = fresh.policy_step(None)
    for key in ("control", "cost", "weights", "iters_run"):
        assert np.array_equal(again[key], ref[key]), key
        assert np.array_equal(first[key], ref[key]), key
    assert np.array_equal(U_again, fresh.get_U())
    assert np.array_equal(eng.get_Sigma(), fresh.get_Sigma())
    eng.close(); fresh.close()


# ---- 6. per-slot values equal to the config's -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["musigmaaismppi", "cemppi"])
def test_per_slot_values_that_repeat_the_config(eng_mod, oracle, track, kind):
    rng = np.random.default_rng(5)
    B, K, T, N = 3, 192, 10, 4
    cs = 2 * T
    x0 = np.stack([e.state for e in slot_states(oracle, track, B)])
    Z = rng.standard_normal((B, N, K, cs))
    outs = []
    for per_slot in (False, True):
        eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, lam=10.0, alpha=0.9, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=COV0, track=track)
        if per_slot:
            eng.set_slot_hyper(lam=[10.0] * B, alpha=[0.9] * B, lam_ais=[20.0] * B, cma_sigma=[1.0] * B)
            eng.set_Sigma_slots(np.tile(COV0, (B, 1)))
        eng.set_state(x0)
        got = eng.policy_step(Z, want_E=True)
        outs.append((got, eng.get_U()))
        eng.close()
    (a, Ua), (b, Ub) = outs
    same = all(np.array_equal(a[k], b[k]) for k in ("control", "cost", "weights", "E")) and np.array_equal(Ua, Ub)
    print("[slot_hyper] %s, per-slot values == config: bit-identical to the shared run: %s" % (kind, same))
    assert np.array_equal(a["iters_run"], b["iters_run"])
    assert rel_err(b["cost"], a["cost"]) < RTOL
    assert np.max(np.abs(b["weights"] - a["weights"])) < 1e-9
    assert np.max(np.abs(b["E"] - a["E"])) < 1e-8
    assert np.max(np.abs(b["control"] - a["control"])) < 1e-8
    assert np.max(np.abs(Ub - Ua)) < 1e-8


# ---- 7. closed loop ---------------------------------------------------------------------------------------------------------------------------

def closed_loop_refs(oracle, track, kind, K, T, N, B, steps, seed):
    out = []
    for b in range(B):
        env = oracle.OracleEnv("car", 1, track=track)
        pol = oracle.OraclePolicy(kind, env, K, T, lam=LAM[b], alpha=ALPHA[b], U0=np.zeros(2), cov=d_of(b), N=N, lam_ais=LAM_AIS[b],
                                  elite_threshold=0.8, cma_sigma=0.75, nthreads=8)
        out.append(pol.run_trial(env, seed + b + 1, num_steps=steps, laps=2, log_actions=True))
    return out


@pytest.mark.parametrize("kind,K,T,N", [("cemppi", 150, 20, 4), ("musigmaaismppi", 256, 20, 3)])
def test_run_trials_per_slot(eng_mod, oracle, track, kind, K, T, N):
    B, steps, seed = 3, 12, 20240000
    eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, cov=COV0, track=track, seed=seed)
    eng.set_slot_hyper(lam=LAM, alpha=ALPHA, lam_ais=LAM_AIS)
    eng.set_Sigma_slots(np.stack([d_of(b) for b in range(B)]))
    rec, acts = eng.run_trials(num_steps=steps, laps=2, log_actions=True)
    refs = closed_loop_refs(oracle, track, kind, K, T, N, B, steps, seed)
    for b, r in enumerate(refs):
        assert r["status"] == 0 and rec[b, 15] == 0
        assert rec[b, 1] == r["steps"] and rec[b, 14] == r["rollouts"]
        assert np.max(np.abs(acts[b] - r["actions"])) < 1e-6, np.max(np.abs(acts[b] - r["actions"]))
        ref = [r["rew"], r["steps"], r["rew_per_step"]] + r["lap_t"] + [r["mean_v"], r["max_v"], r["mean_beta"], r["max_beta"],
                                                                     r["beta_viol"], r["trk_viol"], r["crash_viol"]]
        assert rel_err(rec[b, :14], ref) < 1e-6, (rec[b, :14], ref)
    assert not np.allclose(acts[0], acts[1]) and not np.allclose(acts[1], acts[2])
    eng.close()


# ---- 8. Level 1 -------------------------------------------------------------------------------------------------------------------------------

def test_rollout_costs_per_slot_gamma(eng_mod, oracle, track):
    rng = np.random.default_rng(102)
    B, K, T, ncars = 3, 70, 13, 2
    cs = 2 * ncars * T
    cov = np.tile(COV0, ncars)
    eng = eng_mod.Engine("car", ncars, "gmppi", K, T, batch=B, lam=10.0, cov=cov, track=track)
    eng.set_slot_hyper(lam=LAM, alpha=ALPHA)
    env = oracle.OracleEnv("car", ncars, track=track)
    U = rng.uniform(-0.3, 0.3, (B, cs)); U[:, 1::2] += 0.3
    Uo = rng.uniform(-0.3, 0.3, (B, cs))
    A = rng.standard_normal((cs, cs))
    Sinv = A @ A.T / cs + np.eye(cs)
    E = rng.standard_normal((B, K, cs)) * np.tile([0.25, 0.32], ncars * T)
    E[0, :4] *= 8.0
    x0 = np.stack([env.state for _ in range(B)])
    x0[1, 0] += 2.0; x0[1, 3] = 17.0
    got = eng.rollout_costs(U, E, x0=x0, U_orig=Uo, Sigma_inv=Sinv)
    for b in range(B):
        env.state = x0[b]
        pol = oracle.OraclePolicy("gmppi", env, K, T, lam=LAM[b], alpha=ALPHA[b], U0=np.zeros(2 * ncars), cov=cov, N=1, nthreads=8)
        ref = pol.simulate_model(U[b], E[b].T, Sigma_inv=Sinv, U_orig=Uo[b])
        print("[slot_hyper] level 1 slot %d (gamma %g): rel_err %.2e" % (b, LAM[b] * (1 - ALPHA[b]), rel_err(got[b], ref)))
        assert rel_err(got[b], ref) < 1e-12, (b, rel_err(got[b], ref))
    eng.close()


# ---- 9. policy_call and a custom env ----------------------------------------------------------------------------------------------------------

def test_policy_call_honours_the_slots(eng_mod, oracle, track):
    B, K, T, N, kind = 3, 192, 10, 4, "cemppi"
    x0 = np.stack([e.state for e in slot_states(oracle, track, B)])
    a = slot_engine(eng_mod, track, kind, K, T, N, B, True, seed=9)
    b = slot_engine(eng_mod, track, kind, K, T, N, B, True, seed=9)
    a.set_state(x0)
    step = a.policy_step(None)
    U = np.zeros((B, 2 * T))
    call = b.policy_call(x=x0, U=U, want_cost=True)
    assert np.array_equal(step["control"], call["control"]) and np.array_equal(step["cost"], call["cost"])
    assert np.array_equal(a.get_U(), U) and np.array_equal(step["iters_run"], call["iters_run"])
    assert not np.allclose(call["control"][0], call["control"][1])
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["gmppi", "cemppi"])
def test_custom_env_per_slot(eng_mod, kind):
    from mpopis_amd import build
    from tests.helpers import pointmass_ref as PM
    env = types.SimpleNamespace(code_object=build.build_env(os.path.join(ROOT, "tests", "helpers", "envs", "pointmass_sdk.hip")), state_size=PM.SS,
                                action_size=PM.AS, params=np.array(PM.PARAMS, dtype=np.float64), lo=PM.LO, hi=PM.HI, reset_state=None)
    rng = np.random.default_rng(43)
    B, K, T, N = 2, 130, 9, 3
    cs = PM.AS * T
    Neff = 1 if kind == "gmppi" else N
    lam = [1.5, 4.0]
    Sig = [np.diag([0.3, 0.3, 0.1]), np.array([[0.2, 0.05, 0.0], [0.05, 0.4, -0.03], [0.0, -0.03, 0.15]])]
    x0 = np.array([[0.2, -0.3, 0.5, 0.1, 0.0], [-0.6, 0.4, -0.2, 0.3, 0.25]])
    U0 = rng.uniform(-0.3, 0.3, (B, cs))
    Z = rng.standard_normal((B, Neff, K, cs))
    kw = dict(ais_its=N, lam_ais=5.0, elite_threshold=0.8, custom_env=env)
    eng = eng_mod.Engine("custom", 0, kind, K, T, batch=B, lam=lam[0], cov=[0.3, 0.3, 0.1], **kw)
    eng.set_slot_hyper(lam=lam)
    eng.set_Sigma_slots(np.stack(Sig))
    eng.set_state(x0); eng.set_U(U0)
    got = eng.policy_step(Z)
    U_dev = eng.get_U()
    eng.close()
    for b in range(B):
        one = eng_mod.Engine("custom", 0, kind, K, T, batch=1, lam=lam[b], cov=Sig[b], **kw)
        one.set_state(x0[b][None]); one.set_U(U0[b][None])
        ref = one.policy_step(Z[b][None])
        assert got["iters_run"][b] == ref["iters_run"][0]
        assert rel_err(got["cost"][b], ref["cost"][0]) < 1e-8
        assert np.max(np.abs(got["control"][b] - ref["control"][0])) < 1e-8
        assert np.max(np.abs(U_dev[b] - one.get_U()[0])) < 1e-8
        one.close()
    assert not np.allclose(got["control"][0], got["control"][1])


# ---- 10. errors and read-back -----------------------------------------------------------------------------------------------------------------

def test_errors_and_read_back(eng_mod, oracle, track):
    from mpopis_amd._lib import MPOPISError
    rng = np.random.default_rng(8)
    B, K, T, N = 3, 128, 10, 3
    cs = 2 * T
    eng = eng_mod.Engine("car", 1, "cemppi", K, T, batch=B, lam=7.0, alpha=0.95, ais_its=N, lam_ais=11.0, cma_sigma=0.6, cov=COV0, track=track)
    h = eng.get_slot_hyper()
    assert np.array_equal(h["lam"], [7.0] * B) and np.array_equal(h["alpha"], [0.95] * B)
    assert np.array_equal(h["lam_ais"], [11.0] * B) and np.array_equal(h["cma_sigma"], [0.6] * B)
    eng.set_slot_hyper(lam=LAM, lam_ais=LAM_AIS)               # alpha and sigma NULL: the config's values
    h = eng.get_slot_hyper()
    assert np.array_equal(h["lam"], LAM) and np.array_equal(h["lam_ais"], LAM_AIS)
    assert np.array_equal(h["alpha"], [0.95] * B) and np.array_equal(h["cma_sigma"], [0.6] * B)
    good = np.stack([sigma_of(b, T) for b in range(B)])
    eng.set_Sigma_slots(good)
    Z = rng.standard_normal((B, N, K, cs))
    before = eng.policy_step(Z)
    U_before = eng.get_U()
    bad = good.copy()
    bad[2] = -np.eye(cs) + 0.1                                 # dense and not positive definite: found by the device's factorisation
    with pytest.raises(MPOPISError) as ei:
        eng.set_Sigma_slots(bad)
    assert ei.value.code == -2 and "slot 2" in str(ei.value), str(ei.value)
    bad = good.copy()
    bad[1] = np.diag(np.r_[-1.0, np.ones(cs - 1)])             # diagonal and not positive: found on the host
    with pytest.raises(MPOPISError) as ei:
        eng.set_Sigma_slots(bad)
    assert ei.value.code == -2 and "slot 1" in str(ei.value), str(ei.value)
    with pytest.raises(MPOPISError) as ei:
        eng.set_Sigma_slots(np.tile(np.eye(3), (B, 1, 1)))     # "Covariance matrix size problem"
    assert ei.value.code == -1 and "size" in str(ei.value)
    eng.set_U(np.zeros((B, cs)))
    after = eng.policy_step(Z)                                 # the refused calls left the handle as it was
    for key in ("control", "cost", "weights"):
        assert np.array_equal(before[key], after[key]), key
    assert np.array_equal(U_before, eng.get_U())
    eng.close()
    nes = eng_mod.Engine("car", 1, "nesmppi", K, T, batch=B, lam=10.0, ais_its=N, step_factor=0.01, cov=COV0, track=track)
    with pytest.raises(MPOPISError) as ei:
        nes.set_slot_hyper(step_factor=[0.01, np.nan, 0.02])
    assert ei.value.code == -1
    assert np.array_equal(nes.get_slot_hyper()["cma_sigma"], [0.01] * B)
    nes.close()


# ---- 11. Python harness -----------------------------------------------------------------------------------------------------------------------

def test_simulate_car_racing_sweep(eng_mod):
    from mpopis_amd.examples import simulate_car_racing
    B, steps, seed = 3, 6, 4242
    covs = [d_of(b) for b in range(B)]
    allrec, _ = simulate_car_racing(num_trials=B, num_steps=steps, λ=list(LAM), α=list(ALPHA), cov_mat=covs, seed=seed, quiet=True)
    eng = eng_mod.Engine("car", 1, "cemppi", 150, 50, batch=B, lam=LAM[0], alpha=ALPHA[0], ais_its=10, lam_ais=20.0, elite_threshold=0.8,
                         sigma_est="ss", cma_sigma=0.75, seed=seed, U0=np.zeros(2))
    eng.set_slot_hyper(lam=LAM, alpha=ALPHA)
    eng.set_Sigma_slots(np.stack(covs))
    eng.seed_slots([seed + k for k in range(1, B + 1)])
    rec = eng.run_trials(steps, 2)
    eng.close()
    assert np.array_equal(allrec[:, 0], [1, 2, 3])
    assert np.array_equal(allrec[:, 1:1 + rec.shape[1]], rec)
    assert not np.allclose(rec[0, :3], rec[1, :3])
