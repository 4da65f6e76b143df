"""Slot views of the part-chain schedule, for the per-slot buffers the other schedule-identity tests do not reach: the injected-noise staging
(d_Zin, d_resi_in, d_resu_in), the trajectory log, the global alias stacks, the simple envs under a forced split, and the buffers that are
only allocated after a handle has already run split steps (env_query's outputs, the harness accumulators and action log, per-slot Σ and
λ / α / λ_ais / σ).  A part-chain works on "slots [b0, b0 + nb)" through pointers moved by each buffer's per-slot extent; a buffer that is not
moved, or moved by another extent than it was allocated with, makes the later parts work on the first part's slots -- no fault, wrong numbers.
So every case runs one stream (set_overlap(1)) against 2, 3 and 4 parts and demands equal bits.  B = 5 slots split as 3 + 2, 2 + 2 + 1 and
2 + 1 + 1 + 1; every slot has its own start state and seed, so no slot's result can stand in for another's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 5
COV = {"car": [0.0625, 0.1], "mountaincar": [1.5], "cartpole": [1.5]}
LAM = {"car": 10.0, "mountaincar": 0.1, "cartpole": 0.1}


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


def make_engine(eng_mod, track, env, kind, K, T, N, overlap, batch=B, **kw):
    """An engine whose slots all differ: slot b starts from its own state and draws from its own seed."""
    eng = eng_mod.Engine(env, 1 if env == "car" else 0, kind, K, T, batch=batch, lam=LAM[env], ais_its=N, lam_ais=20.0 if env == "car" else 0.1,
                         elite_threshold=0.8, cov=COV[env], track=track if env == "car" else None, **kw)
    eng.set_overlap(overlap)
    x = eng.get_state()[0]
    b = np.arange(batch)
    if env == "car":
        x[:, 0] += 0.3 * b; x[:, 1] += 0.7 * b; x[:, 3] += 0.5 * b
    elif env == "mountaincar":
        x[:, 0] += 0.02 * b; x[:, 1] += 0.004 * b
    else:
        x[:, 0] += 0.01 * b; x[:, 2] += 0.01 * (b + 1)
    eng.set_state(x)
    eng.seed_slots(1000 + 17 * b)
    return eng


def step_outputs(eng, got):
    out = [got[k] for k in ("control", "cost", "weights", "iters_run", "res_idx0")] + [eng.get_U()]
    if "E" in got:
        out.append(got["E"])
    if eng.policy != "mppi":
        out.append(eng.get_Sigma())
    return out


def assert_same(outs, overlaps):
    """outs[i]: the list of arrays the run under overlaps[i] produced; the first is the one-stream run"""
    assert overlaps[0] == 1
    for i in range(1, len(outs)):
        assert len(outs[i]) == len(outs[0])
        for j, (a, c) in enumerate(zip(outs[0], outs[i])):
            assert np.array_equal(a, c), (overlaps[i], j)


def assert_slots_differ(a):
    for b in range(1, len(a)):
        assert not np.array_equal(a[0], a[b])


@pytest.mark.parametrize("kind", ["musigmaaismppi", "pmcmppi", "mppi"])
def test_injected_noise(eng_mod, track, kind):
    """d_Zin moves by N cs K per slot, the resampling draws by (N - 1) K; K = 96 is no multiple of the wave size"""
    K, T, N = 96, 10, 3
    cs = 2 * T
    rng = np.random.default_rng(96)
    Neff = 1 if kind == "mppi" else N
    noise = []
    for step in range(2):
        Z = rng.standard_normal((B, T, K, 2) if kind == "mppi" else (B, N, K, cs))
        di = rng.integers(0, K, (B, max(Neff - 1, 1), K)).astype(np.int32) if kind == "pmcmppi" else None
        du = rng.random((B, max(Neff - 1, 1), K)) if kind == "pmcmppi" else None
        noise.append((Z, di, du))
    overlaps = (1, 2, 3, 4)
    outs = []
    for overlap in overlaps:
        eng = make_engine(eng_mod, track, "car", kind, K, T, N, overlap)
        res = []
        for Z, di, du in noise:
            res += step_outputs(eng, eng.policy_step(Z, di, du, want_E=True))
        eng.close()
        outs.append(res)
    assert_same(outs, overlaps)
    assert_slots_differ(outs[0][0])


@pytest.mark.parametrize("env,kind", [("car", "gmppi"), ("mountaincar", "mppi")])
def test_trajectory_log(eng_mod, track, env, kind):
    K, T = 64, 10
    overlaps = (1, 2, 3, 4)
    outs = []
    for overlap in overlaps:
        eng = make_engine(eng_mod, track, env, kind, K, T, 1, overlap, log_trajectories=True)
        got = eng.policy_step(None)
        outs.append([eng.get_trajectories(), got["control"], got["cost"]])
        eng.close()
    assert_same(outs, overlaps)
    assert_slots_differ(outs[0][0])


def test_global_alias_stacks(eng_mod, track):
    """K = 7169 is the first K whose alias tables are built on the global stacks (two K-int stacks per slot)"""
    K, T, N, nb = 7169, 10, 3, 3
    overlaps = (1, 3)
    outs = []
    for overlap in overlaps:
        eng = make_engine(eng_mod, track, "car", "pmcmppi", K, T, N, overlap, batch=nb)
        res = []
        for step in range(2):
            res += step_outputs(eng, eng.policy_step(None))
        eng.close()
        outs.append(res)
    assert_same(outs, overlaps)
    assert_slots_differ(outs[0][0])


@pytest.mark.parametrize("env", ["mountaincar", "cartpole"])
def test_simple_envs_forced_split(eng_mod, track, env):
    """the default schedule never splits these envs; mpopis_set_overlap may"""
    K, T, N = 128, 20, 3
    overlaps = (1, 2, 3, 4)
    outs = []
    for overlap in overlaps:
        eng = make_engine(eng_mod, track, env, "cemppi", K, T, N, overlap)
        res = []
        for step in range(2):
            res += step_outputs(eng, eng.policy_step(None, want_E=True))
        rec, act = eng.run_trials(6, 2, log_actions=True)
        res += [rec, act, eng.get_state()[0]]
        eng.close()
        outs.append(res)
    assert_same(outs, overlaps)
    assert_slots_differ(outs[0][0])


def test_buffers_allocated_after_the_first_split_step(eng_mod, track):
    """One handle through every call that allocates per-slot buffers late, each after the handle has already run as part-chains"""
    K, T, N = 128, 10, 3
    cs = 2 * T
    rng = np.random.default_rng(128)
    Z = rng.standard_normal((B, N, K, cs))
    b = np.arange(B)
    rho = 0.15 * b                                              # slot 0 diagonal, the others dense
    tu = np.abs(np.subtract.outer(np.arange(T), np.arange(T)))
    covs = np.stack([np.kron(rho[i] ** tu, np.diag([0.0625 * (1 + 0.2 * i), 0.1 / (1 + 0.2 * i)])) for i in range(B)])
    overlaps = (1, 3)
    outs = []
    for overlap in overlaps:
        eng = make_engine(eng_mod, track, "car", "musigmaaismppi", K, T, N, overlap)
        res = step_outputs(eng, eng.policy_step(None, want_E=True))                        # 1. device RNG
        res += step_outputs(eng, eng.policy_step(Z, want_E=True))                           # 2. injected noise
        rec, act = eng.run_trials(4, 2, log_actions=True)                                   # 3. harness accumulators, alive flags, action log
        res += [rec, act, eng.get_state()[0]]
        res += list(eng.env_query())                                                        # 4. query outputs
        eng.set_Sigma_slots(covs)                                                           # 5. per-slot Σ and per-slot λ, α, λ_ais, σ
        eng.set_slot_hyper(lam=10.0 + 2 * b, alpha=1.0 - 0.1 * b, lam_ais=20.0 + 5 * b, cma_sigma=0.75 + 0.05 * b)
        res += step_outputs(eng, eng.policy_step(None, want_E=True))
        eng.set_Sigma(COV["car"])                                                           # 6. back to the shared values
        eng.set_slot_hyper()
        res += step_outputs(eng, eng.policy_step(None, want_E=True))
        eng.close()
        outs.append(res)
    assert_same(outs, overlaps)
    assert_slots_differ(outs[0][0])
