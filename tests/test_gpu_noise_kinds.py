"""The noise kinds through the engine (mpopis_set_noise_kind / mpopis_get_noise_kind / mpopis_draw_normals): a device step under the antithetic
or Latin-hypercube draw must equal, bit for bit, a step with the normals of mpopis_draw_normals injected; the read-out must be the normals the
Philox kind draws; slots are independent; a handle that returns to the Philox kind computes the bits of one that never left it; the schedule
does not matter; the resident closed loop equals the host loop.  Shapes are the smallest that run every path: car env K = 64, H = 5 (cs = 10:
the diagonal first iteration through the row scaling, the adapted iterations through the matrix product), MountainCar K = 20, H = 15 for :mppi."""
import numpy as np
import pytest
from tests.helpers import strat_cases as sc
from tests.helpers.sample_cases import RNG_TOL

pytestmark = pytest.mark.gpu
K, T = 64, 5
CS = 2 * T
COV = [0.0625, 0.1]
SEEDS = [20240001, (1 << 32) + 77, 987654321]
NEW_KINDS = ["antithetic", "lhs"]
POLICIES = [("cemppi", 3), ("musigmaaismppi", 2)]
STEP_KEYS = ("control", "cost", "weights", "E", "iters_run")


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


def car(eng_mod, track, policy, N, seeds=SEEDS, noise=None, overlap=None):
    eng = eng_mod.Engine("car", 1, policy, K, T, batch=len(seeds), lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=COV, track=track, seed=0)
    eng.seed_slots(seeds)
    x, _, _ = eng.get_state()
    x[1::3, 3] = 14.0                                              # every third slot starts faster and off the centre line
    x[1::3, 1] = 3.0
    eng.set_state(x)
    if overlap is not None:
        eng.set_overlap(overlap)
    if noise is not None:
        eng.set_noise_kind(noise)
    return eng


def mountaincar(eng_mod, noise=None):
    eng = eng_mod.Engine("mountaincar", 0, "mppi", 20, 15, batch=3, lam=0.1, cov=[1.5], seed=0)
    eng.seed_slots(SEEDS)
    eng.set_state(np.array([[-0.5, 0.0], [-0.45, 0.0], [-0.55, 0.01]]))
    if noise is not None:
        eng.set_noise_kind(noise)
    return eng


def same_step(a, b, label):
    for key in STEP_KEYS:
        assert np.array_equal(a[key], b[key]), (label, key)


# ---- 1. a device step is the injected step on the normals of the read-out -------------------------------------------------------------------------

@pytest.mark.parametrize("noise", NEW_KINDS)
@pytest.mark.parametrize("policy,N", POLICIES)
def test_device_step_equals_the_injected_step(eng_mod, track, policy, N, noise):
    dev_eng, inj_eng = car(eng_mod, track, policy, N, noise=noise), car(eng_mod, track, policy, N, noise=noise)
    assert dev_eng.noise_kind == noise
    for step in range(2):                                          # (the second step: another MPC step index, a rolled pol.U)
        dev = dev_eng.policy_step(None, want_E=True)
        Z = np.stack([inj_eng.draw_normals(step, n) for n in range(N)], axis=1)
        assert Z.shape == (len(SEEDS), N, K, CS)
        inj = inj_eng.policy_step(Z, want_E=True)
        same_step(dev, inj, (policy, noise, step))
        assert np.array_equal(dev_eng.get_U(), inj_eng.get_U())
    assert np.all(dev["iters_run"] >= 1) and np.all(np.isfinite(dev["cost"]))
    dev_eng.close(); inj_eng.close()


@pytest.mark.parametrize("noise", NEW_KINDS)
def test_device_step_equals_the_injected_step_mppi_mountaincar(eng_mod, noise):
    dev_eng, inj_eng = mountaincar(eng_mod, noise), mountaincar(eng_mod, noise)
    for step in range(2):
        dev = dev_eng.policy_step(None, want_E=True)
        Z = inj_eng.draw_normals(step, 0)
        assert Z.shape == (3, 15, 20, 1)
        inj = inj_eng.policy_step(Z, want_E=True)
        same_step(dev, inj, ("mppi", noise, step))
    dev_eng.close(); inj_eng.close()


def test_pmcmppi_resampling_stays_philox_under_lhs(eng_mod, oracle, track):
    """:pmcmppi, N = 2: under LHS the device step resamples with the Philox draws it always used -- the indices equal those of a step given the
    same Z and the oracle's restatement of those draws"""
    N = 2
    dev_eng, inj_eng = car(eng_mod, track, "pmcmppi", N, noise="lhs"), car(eng_mod, track, "pmcmppi", N, noise="lhs")
    dev = dev_eng.policy_step(None, want_E=True)
    Z = np.stack([inj_eng.draw_normals(0, n) for n in range(N)], axis=1)
    draws = [oracle.philox_resample_draws(s, 0, 0x80000000, K) for s in SEEDS]
    ri = np.stack([d[0] for d in draws])[:, None, :]
    ru = np.stack([d[1] for d in draws])[:, None, :]
    inj = inj_eng.policy_step(Z, ri, ru, want_E=True)
    assert np.array_equal(dev["res_idx0"], inj["res_idx0"])
    same_step(dev, inj, "pmcmppi")
    assert len(np.unique(dev["res_idx0"][0])) < K                  # (a resampling happened: some sample was drawn twice)
    dev_eng.close(); inj_eng.close()


# ---- 2. the read-out ------------------------------------------------------------------------------------------------------------------------------

def test_draw_normals_under_philox_is_the_oracle_stream(eng_mod, oracle, track):
    eng = car(eng_mod, track, "cemppi", 3)
    assert eng.noise_kind == "philox"
    for step, n in ((0, 0), (0, 2), (3, 1)):
        Z = eng.draw_normals(step, n)
        for b, seed in enumerate(SEEDS):
            ref = oracle.philox_normals(seed, step, n, CS * K).reshape(K, CS)
            assert np.max(np.abs(Z[b] - ref)) < RNG_TOL, (step, n, b)
    before = eng.policy_step(None)                                 # the read-out moved nothing: a fresh handle takes the same step
    eng.close()
    eng = car(eng_mod, track, "cemppi", 3)
    assert np.array_equal(eng.policy_step(None)["control"], before["control"])
    eng.close()
    mc = mountaincar(eng_mod)
    Z = mc.draw_normals(2, 0)                                      # :mppi order: element ((t K + k) as + a)
    for b, seed in enumerate(SEEDS):
        assert np.max(np.abs(Z[b].ravel() - oracle.philox_normals(seed, 2, 0, 15 * 20))) < RNG_TOL
    mc.close()


@pytest.mark.parametrize("noise", NEW_KINDS)
def test_draw_normals_is_the_restated_draw(eng_mod, track, noise):
    """the engine's read-out against the definition: antithetic = the Philox read-out's first half and its negation; LHS = strata and jitter of
    the NumPy restatement through the inverse normal CDF, within its bound of the float64 restatement's neighbourhood"""
    eng = car(eng_mod, track, "cemppi", 3)
    P = eng.draw_normals(1, 2)
    eng.set_noise_kind(noise)
    Z = eng.draw_normals(1, 2)
    h = (K + 1) // 2
    if noise == "antithetic":
        assert np.array_equal(Z[:, :h], P[:, :h]) and np.array_equal(Z[:, h:], -Z[:, :K - h])
    else:
        j, x = sc.lhs_inputs(SEEDS, (1, 1, 1), 1, 2, CS, K)        # [B, cs, K]
        want = sc.phi_inv_f64(j, sc.xi_of(x), K).transpose(0, 2, 1)
        assert np.all(np.abs(Z - want) <= 2 * sc.phi_inv_bound(j, sc.xi_of(x), K).transpose(0, 2, 1))
        assert np.array_equal(np.argsort(Z, axis=1), np.argsort(j.transpose(0, 2, 1), axis=1))       # one sample per stratum in every row
    eng.close()


@pytest.mark.parametrize("noise", ["philox"] + NEW_KINDS)
def test_slots_draw_like_one_slot_handles(eng_mod, track, noise):
    eng = car(eng_mod, track, "cemppi", 3, noise=noise)
    Z = eng.draw_normals(4, 1)
    eng.close()
    assert not np.array_equal(Z[0], Z[1]) and not np.array_equal(Z[1], Z[2])
    for b, seed in enumerate(SEEDS):
        one = car(eng_mod, track, "cemppi", 3, seeds=[seed], noise=noise)
        assert np.array_equal(one.draw_normals(4, 1)[0], Z[b]), (noise, b)
        one.close()


# ---- 3. back to Philox, refusals ----------------------------------------------------------------------------------------------------------------

def test_back_to_philox_is_a_never_switched_handle(eng_mod, track):
    policy, N = "musigmaaismppi", 2
    ref_eng = car(eng_mod, track, policy, N)
    x0, _, _ = ref_eng.get_state()
    ref = [ref_eng.policy_step(None, want_E=True) for _ in range(2)]
    ref_U = ref_eng.get_U()
    ref_eng.close()
    eng = car(eng_mod, track, policy, N)
    eng.set_noise_kind("lhs")
    lhs = eng.policy_step(None, want_E=True)
    assert not np.array_equal(lhs["control"], ref[0]["control"])
    eng.set_noise_kind("philox")
    assert eng.noise_kind == "philox"
    eng.seed_slots(SEEDS); eng.set_state(x0); eng.set_U(np.zeros((len(SEEDS), CS)))
    for step in range(2):
        same_step(eng.policy_step(None, want_E=True), ref[step], ("back", step))
    assert np.array_equal(eng.get_U(), ref_U)
    eng.close()


def test_unknown_kind_is_refused_and_changes_nothing(eng_mod, track):
    from mpopis_amd._lib import ERR_ARG
    ref_eng, eng = car(eng_mod, track, "cemppi", 3, noise="antithetic"), car(eng_mod, track, "cemppi", 3, noise="antithetic")
    for bad in (3, -1, 99):
        assert eng.L.mpopis_set_noise_kind(eng._h, bad) == ERR_ARG
        assert b"noise kind" in eng.L.mpopis_last_error(eng._h)
    assert eng.noise_kind == "antithetic"
    with pytest.raises(eng_mod.MPOPISError):
        eng.set_noise_kind("sobol")
    assert eng.L.mpopis_draw_normals(eng._h, 0, -1, None) == ERR_ARG
    same_step(eng.policy_step(None, want_E=True), ref_eng.policy_step(None, want_E=True), "after a refusal")
    ref_eng.close(); eng.close()


# ---- 4. schedules -----------------------------------------------------------------------------------------------------------------------------------

def test_schedule_does_not_matter_under_lhs(eng_mod, track):
    seeds = [500 + 7 * b for b in range(8)]
    outs = []
    for overlap in (1, 3):
        eng = car(eng_mod, track, "cemppi", 3, seeds=seeds, noise="lhs", overlap=overlap)
        steps = []
        for _ in range(2):
            got = eng.policy_step(None, want_E=True)
            steps.append([got[k] for k in STEP_KEYS] + [eng.get_U()])
        outs.append(steps)
        eng.close()
    for step in range(2):
        for a, b in zip(outs[0][step], outs[1][step]):
            assert np.array_equal(a, b), step
    assert not np.array_equal(outs[0][0][0][0], outs[0][0][0][2])


# ---- 5. the resident closed loop ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise", NEW_KINDS)
def test_run_trials_equals_the_host_loop(eng_mod, track, noise):
    policy, N, steps, seeds = "cemppi", 3, 5, SEEDS[:2]
    eng = car(eng_mod, track, policy, N, seeds=seeds, noise=noise)
    rec, acts, tr = eng.run_trials(num_steps=steps, laps=2, log_actions=True, trace=True)
    eng.close()
    eng = car(eng_mod, track, policy, N, seeds=seeds, noise=noise)
    plain_rec, plain_acts = eng.run_trials(num_steps=steps, laps=2, log_actions=True)
    eng.close()
    assert np.array_equal(plain_rec, rec) and np.array_equal(plain_acts, acts)                 # traced or not: the same bits
    host = car(eng_mod, track, policy, N, seeds=seeds, noise=noise)
    S = steps + 1
    h_acts, h_rew, h_iters, h_states = np.zeros((2, S, 2)), np.zeros((2, S)), np.zeros((2, S), dtype=np.int32), np.zeros((2, S + 1, 8))
    for s in range(S):
        h_states[:, s] = host.get_state()[0]
        out = host.policy_call()
        h_acts[:, s], h_iters[:, s] = out["control"], out["iters_run"]
        h_rew[:, s] = host.env_step(out["control"])
    h_states[:, S] = host.get_state()[0]
    host.close()
    assert np.all(rec[:, 15] == 0) and np.all(rec[:, 1] == steps)                              # nobody stops early in six steps
    assert np.array_equal(acts, h_acts)
    assert np.array_equal(tr["states"], h_states) and np.array_equal(tr["rewards"], h_rew) and np.array_equal(tr["iters"], h_iters)
    # the records, from the host loop's terms: reward sum (in step order), steps, reward per step, rollouts executed, status
    assert np.array_equal(rec[:, 0], np.cumsum(h_rew, axis=1)[:, -1])
    assert np.array_equal(rec[:, 2], rec[:, 0] / rec[:, 1])
    assert np.array_equal(rec[:, 14], h_iters.sum(axis=1) * float(K))
    philox = car(eng_mod, track, policy, N, seeds=seeds)
    assert not np.array_equal(philox.run_trials(num_steps=steps, laps=2, log_actions=True)[1], acts)
    philox.close()
