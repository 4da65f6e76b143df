""":nesmppi on the device against the NumPy restatement of NESMPPI_Policy (tests/helpers/nes_ref.py), whose rollouts are the oracle's
:gmppi simulate_model: one-iteration identity with :gmppi, parity over shapes / envs / α < 1 with injected and device noise, the early
break, a dense pol.Σ (device square root), the benched shape under every overlap schedule, the closed loop, and the Python mirror."""
import numpy as np
import pytest

from tests.helpers.nes_ref import nes_ref, sym_sqrt
from tests.test_gpu_baseline_shapes import start_states, sig_err

pytestmark = pytest.mark.gpu

TOL = 1e-7


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


def nes_cost_err(pol, U_orig, cost_dev, E_dev, ref, gamma, worst):
    """max relative cost deviation from the reference.  The adapted proposal reaches the last iteration through a few FP64 reductions of
    K-term sums whose order differs between the device and NumPy (E agrees to ~1e-9), and a car rollout's cost is discontinuous (lane edge,
    standstill chatter, contact between cars): a rollout whose cost deviates beyond the tolerance is re-run by the oracle on the DEVICE's own
    sample (V = U_orig + E_out_k) and must agree with that to the tolerance; at most 1 % of K may need it (3 cars, K = 1024: 4)."""
    rel = np.abs(cost_dev - ref["cost"]) / (np.abs(ref["cost"]) + 1e-9)
    bad = np.where(rel >= TOL)[0]
    if len(bad) == 0:
        return float(rel.max())
    own = pol.simulate_model(U_orig, np.ascontiguousarray(E_dev), ref["Sinv_last"] if gamma != 0.0 else None, U_orig)[bad]
    rel_own = np.abs(cost_dev[bad] - own) / (np.abs(own) + 1e-9)
    assert np.all(rel_own < TOL), ("cost deviates on the device's own samples", bad[rel_own >= TOL][:10], rel_own[rel_own >= TOL][:10])
    assert len(bad) <= max(2, len(rel) // 100), ("too many rollouts deviate", len(bad))
    worst["reeval"] = worst.get("reeval", 0) + len(bad)
    return float(np.max(np.delete(rel, bad))) if len(bad) < len(rel) else 0.0


def _setup(oracle, track, env_kind, ncars, K, T, B, lam, alpha, cov):
    if env_kind == "car":
        x0 = start_states(oracle, track, ncars, B)
    elif env_kind == "mountaincar":
        x0 = np.array([[-0.5, 0.0], [-0.42, 0.012]] * B)[:B]
    else:
        x0 = np.array([[0.02, 0.0, -0.03, 0.05], [-0.01, 0.1, 0.04, -0.2]] * B)[:B]
    envs, pols = [], []
    for b in range(B):
        e = oracle.OracleEnv(env_kind, ncars, track=track if env_kind == "car" else None)
        e.state = x0[b]
        p = oracle.OraclePolicy("gmppi", e, K, T, lam=lam, alpha=alpha, U0=np.zeros(e.as_), cov=cov, N=1, nthreads=8)
        envs.append(e); pols.append(p)
    return x0, envs, pols


def nes_case(eng_mod, oracle, track, env_kind="car", ncars=1, K=1024, T=50, N=4, B=2, steps=2, device_rng=False, alpha=1.0, lam=10.0,
             sf=0.01, cov=None, seed=20250000, slots=None, overlap=None):
    as_ = 2 * ncars if env_kind == "car" else 1
    cs = as_ * T
    if cov is None:
        cov = np.tile([0.0625, 0.1], ncars) if env_kind == "car" else np.array([0.5])
    eng = eng_mod.Engine(env_kind, ncars, "nesmppi", K, T, batch=B, lam=lam, alpha=alpha, ais_its=N, step_factor=sf, cov=cov,
                         track=track if env_kind == "car" else None, seed=seed)
    if overlap is not None:
        eng.set_overlap(overlap)
    slots = list(range(B)) if slots is None else slots
    x0, envs, pols = _setup(oracle, track, env_kind, ncars, K, T, B, lam, alpha, cov)
    eng.set_state(x0)
    if np.asarray(cov).ndim == 2 and np.asarray(cov).shape[0] == cs:
        for p in pols:
            p.Sigma = cov
    rng = np.random.default_rng(4321 + K + cs)
    worst = dict(cost=0.0, control=0.0, U=0.0, E=0.0, w=0.0, Sigma=0.0)
    outs = []
    for step in range(steps):
        if device_rng:
            Z = {b: np.stack([oracle.philox_normals(seed + b + 1, step, n, cs * K).reshape(K, cs) for n in range(N)]) for b in slots}
            got = eng.policy_step(None, want_E=True)
        else:
            Zall = rng.standard_normal((B, N, K, cs))
            Z = {b: Zall[b] for b in slots}
            got = eng.policy_step(Zall, want_E=True)
        U_dev, Sig_dev = eng.get_U(), eng.get_Sigma()
        outs.append((got, U_dev, Sig_dev))
        for b in slots:
            U_orig = pols[b].U
            ref = nes_ref(pols[b], envs[b], Z[b], N, sf, lam, gamma=lam * (1 - alpha))
            assert got["iters_run"][b] == ref["iters_run"], (step, b, got["iters_run"][b], ref["iters_run"])
            worst["cost"] = max(worst["cost"], nes_cost_err(pols[b], U_orig, got["cost"][b], got["E"][b].T, ref, lam * (1 - alpha), worst))
            worst["w"] = max(worst["w"], float(np.max(np.abs(got["weights"][b] - ref["weights"]))))
            worst["E"] = max(worst["E"], float(np.max(np.abs(got["E"][b].T - ref["E"]))))
            worst["control"] = max(worst["control"], float(np.max(np.abs(got["control"][b] - ref["control"]))))
            worst["U"] = max(worst["U"], float(np.max(np.abs(U_dev[b] - ref["U"]))))
            worst["Sigma"] = max(worst["Sigma"], sig_err(Sig_dev[b], ref["Sigma_last"]))
    eng.close()
    print("\n[nes] %s ncars=%d K=%d T=%d N=%d B=%d alpha=%g rng=%s: %s" % (env_kind, ncars, K, T, N, B, alpha,
          "device" if device_rng else "injected", " ".join("%s=%.2e" % kv for kv in worst.items())))
    for key in ("cost", "control", "U", "E", "w"):
        assert worst[key] < TOL, worst
    assert worst["Sigma"] < 1e-8, worst
    return outs


def test_one_iteration_is_gmppi_bit_for_bit(eng_mod, track):
    K, T, B = 512, 50, 3
    kw = dict(lam=10.0, cov=[0.0625, 0.1], track=track, seed=77)
    for device_rng in (False, True):
        g = eng_mod.Engine("car", 1, "gmppi", K, T, batch=B, **kw)
        n = eng_mod.Engine("car", 1, "nesmppi", K, T, batch=B, ais_its=1, **kw)
        Z = None if device_rng else np.random.default_rng(3).standard_normal((B, 1, K, 2 * T))
        for _ in range(2):
            a, b = g.policy_step(Z), n.policy_step(Z)
            for key in ("control", "cost", "weights"):
                assert np.array_equal(a[key], b[key]), key
            assert np.array_equal(g.get_U(), n.get_U())
        g.close(); n.close()


@pytest.mark.parametrize("device_rng", [False, True])
@pytest.mark.parametrize("case", ["car1", "car3_cs300", "mountaincar", "cartpole", "alpha_lt_1"])
def test_parity_with_reference(eng_mod, oracle, track, case, device_rng):
    if case == "car1":
        nes_case(eng_mod, oracle, track, "car", 1, 1024, 50, 4, device_rng=device_rng)
    elif case == "car3_cs300":
        # (the default step_factor 0.01 against mid-lap 3-car costs of ~4e7 takes Σ′ to cond ~1e10 within two iterations, in the reference as on
        # the device: no two FP64 evaluation orders agree there.  1e-7 keeps every update a modest change of a well-conditioned Σ′.)
        nes_case(eng_mod, oracle, track, "car", 3, 1024, 50, 3, sf=1e-7, device_rng=device_rng)
    elif case == "mountaincar":
        nes_case(eng_mod, oracle, track, "mountaincar", 1, 256, 40, 4, lam=0.1, device_rng=device_rng)
    elif case == "cartpole":
        nes_case(eng_mod, oracle, track, "cartpole", 1, 256, 30, 4, lam=0.1, device_rng=device_rng)
    else:
        nes_case(eng_mod, oracle, track, "car", 1, 512, 30, 3, alpha=0.5, sf=1e-7, device_rng=device_rng)   # (step factor: see the 3-car case)


def test_early_break(eng_mod, oracle, track):
    K, T, N, B = 256, 20, 5, 2
    cs = 2 * T
    eng = eng_mod.Engine("car", 1, "nesmppi", K, T, batch=B, lam=10.0, ais_its=N, cov=np.full(2, 1e-12), track=track, seed=3)
    eng.set_state(start_states(oracle, track, 1, B))
    out = eng.policy_step(None)
    assert list(out["iters_run"]) == [1] * B                      # every sample costs the same to 1e-2: the reference breaks at n = 1
    S = eng.get_Sigma()
    assert np.array_equal(S[0], np.diag(np.full(cs, 1e-12)))      # Σ′ of the last executed iteration = pol.Σ
    eng.close()
    eng = eng_mod.Engine("car", 1, "nesmppi", K, T, batch=B, lam=10.0, ais_its=N, cov=[0.0625, 0.1], track=track, seed=3)
    eng.set_state(start_states(oracle, track, 1, B))
    assert list(eng.policy_step(None)["iters_run"]) == [N] * B
    eng.close()


def test_dense_sigma_device_square_root(eng_mod, oracle, track):
    T, K, N = 10, 256, 2
    cs = 2 * T
    rng = np.random.default_rng(8)
    Q, _ = np.linalg.qr(rng.standard_normal((cs, cs)))
    S = (Q * np.linspace(0.03, 0.2, cs)) @ Q.T
    S = 0.5 * (S + S.T)
    assert np.max(np.abs(S - np.diag(np.diag(S)))) > 1e-3
    for device_rng in (False, True):
        nes_case(eng_mod, oracle, track, "car", 1, K, T, N, B=2, steps=2, cov=S, device_rng=device_rng)
    # the square root itself: A0 = sqrt(Σ) by the device eigen-solve, seen through the first update of a slot
    assert np.max(np.abs(sym_sqrt(S) @ sym_sqrt(S) - S)) < 1e-14


def test_benched_shape_slots_and_overlap_schedules(eng_mod, oracle, track):
    K, T, N, B = 4096, 50, 10, 64
    sf = 1e-7          # all ten iterations run in every slot (with 0.01 the mid-lap slots blow Σ′ up and break after 2-4), see the 3-car case
    outs = nes_case(eng_mod, oracle, track, "car", 1, K, T, N, B=B, steps=1, device_rng=True, sf=sf, slots=[0, 21, 42, 63])
    base = outs[0]
    for ov in (1, 2, 4):
        eng = eng_mod.Engine("car", 1, "nesmppi", K, T, batch=B, lam=10.0, ais_its=N, step_factor=sf, cov=[0.0625, 0.1], track=track, seed=20250000)
        eng.set_overlap(ov)
        eng.set_state(start_states(oracle, track, 1, B))
        got = eng.policy_step(None, want_E=True)
        for key in ("control", "cost", "weights", "iters_run", "E"):
            assert np.array_equal(got[key], base[0][key]), (ov, key)
        assert np.array_equal(eng.get_U(), base[1]) and np.array_equal(eng.get_Sigma(), base[2]), ov
        eng.close()


def test_closed_loop_run_trials_matches_host_loop(eng_mod, track):
    K, T, N, B, steps = 256, 20, 3, 4, 20
    kw = dict(lam=10.0, ais_its=N, cov=[0.0625, 0.1], track=track, seed=41)
    a = eng_mod.Engine("car", 1, "nesmppi", K, T, batch=B, **kw)
    rec, acts = a.run_trials(steps, 2, log_actions=True)
    a.close()
    assert np.all(np.isfinite(rec)) and np.all(rec[:, 15] == 0)
    h = eng_mod.Engine("car", 1, "nesmppi", K, T, batch=B, **kw)
    host = []
    for _ in range(steps + 1):
        out = h.policy_step(None)
        host.append(out["control"].copy())
        h.env_step(out["control"])
    h.close()
    host = np.stack(host, axis=1)                                 # (B, steps + 1, as)
    assert np.array_equal(acts, host)


def test_python_mirror_matches_engine(eng_mod, track):
    import mpopis_amd as M
    K, T, N = 256, 20, 3
    env = M.CarRacingEnv()
    pol = M.NESMPPI_Policy(env, opt_its=N, step_factor=0.02, num_samples=K, horizon=T, λ=10.0, U0=np.zeros(2), cov_mat=np.array([0.0625, 0.1]))
    eng = eng_mod.Engine("car", 1, "nesmppi", K, T, batch=1, lam=10.0, ais_its=N, step_factor=0.02, cov=[0.0625, 0.1], seed=0)
    eng.set_state(env.state[None])
    for _ in range(2):
        ctl = pol(env)
        ref = eng.policy_step(None)["control"][0]
        assert np.array_equal(ctl, ref)
    assert np.array_equal(pol.U, eng.get_U()[0])
    pol.close(); eng.close()
