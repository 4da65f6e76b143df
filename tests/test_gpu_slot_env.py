"""Per-slot tracks and env parameters (mpopis_set_tracks / mpopis_set_env_params_slots) against the CPU oracle, one
OracleEnv(params=..., track=...) per slot, and against one-slot handles given the same track and parameters through the shared setters.

Tolerances are those of tests/test_gpu_parity.py: RTOL = 1e-8 relative on Level-1 costs (test_level1_rollout_costs_car) and on logged
trajectories (test_trajectory_logger); 1e-8 absolute on Level-2 controls and pol.U (test_level2_policy_step); 1e-10 / 1e-9 relative on the real
env's state / reward (test_level1_custom_car_params); 1e-12 on within-track distances and the query's reward (test_bundled_reference_tracks);
1e-12 on the simple envs' costs (test_level1_mountaincar, test_level1_cartpole_with_logger); tests/test_gpu_edge_cases.py:158-165 for run_trials.

In this process the Level-1 cases are few rollout waves, i.e. the two-wave body; the one-wave bodies (K <= S + 1: one sample-wave per workgroup,
K = 1024 + S + 1: four) are selected by running the same cases in a fresh child process with MPOPIS_ROLLOUT_DUO=0, which the library reads once per
process (as tests/helpers/duo_case.py does).  The logger cases run the one-wave body in either process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import slot_env_cases as SC

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


def _cov(nc):
    return np.tile(SC.COV, nc)


def _level1(eng_mod, oracle, *args, **kw):
    return SC.level1_check(eng_mod.Engine, oracle, *args, **kw)


# ---- 1. Level 1 against the oracle per slot ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("nc", [1, 3, 8])
def test_level1_per_slot(eng_mod, oracle, track, nc, T):
    tracks, params = SC.tracks3(track), SC.car_params4(oracle)
    S = 64 // nc
    for K in (S - 1, S, S + 1, 1024 + S + 1):
        _level1(eng_mod, oracle, tracks, SC.TRACK_OF_SLOT, params, nc, K, T, seed=1000 * nc + K)


def test_level1_one_wave_bodies_in_a_child_process():
    """every case of test_level1_per_slot and test_mixed_track_sizes once more with MPOPIS_ROLLOUT_DUO=0 (tests/helpers/slot_env_level1_case.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e["MPOPIS_ROLLOUT_DUO"] = "0"
    try:
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "helpers", "slot_env_level1_case.py")], capture_output=True, text=True, timeout=240, env=e)
    except subprocess.TimeoutExpired as t:
        pytest.exit("slot_env_level1_case.py hung: %s" % str(t.stdout)[-2000:], returncode=3)        # a hang: nothing more is started on this GPU either
    if r.returncode < 0 or r.returncode in (134, 139) or "HIP error" in r.stdout + r.stderr:
        pytest.exit("slot_env_level1_case.py died (%s): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]), returncode=3)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["cases"] == 3 * 2 * 4 + 2 * 2 and out["worst"] < RTOL, out
    print("\n[slot env level 1, one-wave bodies] %d cases, worst deviation from the oracle %.2e" % (out["cases"], out["worst"]))


@pytest.mark.parametrize("nc", [1, 3])
def test_logger_of_the_last_slot(eng_mod, oracle, track, nc):
    tracks, params = SC.tracks3(track), SC.car_params4(oracle)
    _level1(eng_mod, oracle, tracks, SC.TRACK_OF_SLOT, params, nc, 64 // nc + 1, 5, seed=77 + nc, log_slot=3)


# ---- 2. mixed sizes across the LDS limit ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("sizes", [(5, 190, 191), (2, 2048)], ids=["ring_only_placement", "raised_lds_limit"])
def test_mixed_track_sizes(eng_mod, oracle, nc, sizes):
    """the handle's largest track decides the table placement and the dynamic LDS of every slot's workgroups; each stages its own P points"""
    tracks = SC.mixed_tracks(sizes)
    params = SC.car_params4(oracle)[:len(sizes)]
    _level1(eng_mod, oracle, tracks, list(range(len(sizes))), params, nc, 64 // nc + 1, 3, seed=5 + nc)


# ---- 3. a slot is a one-slot handle -----------------------------------------------------------------------------------------------------------

def _two_steps(eng, x0, seeds):
    eng.set_state(x0)
    eng.seed_slots(seeds)
    out = []
    for _ in range(2):
        g = eng.policy_step(None)
        out.append((g["cost"].copy(), g["control"].copy(), eng.get_U(), g["iters_run"].copy()))
    return out


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("kind", ["gmppi", "cemppi"])
def test_slot_equals_one_slot_handle(eng_mod, oracle, track, kind, nc):
    tracks, params, tos = SC.tracks3(track), SC.car_params4(oracle), SC.TRACK_OF_SLOT
    B, K, T, N = 4, 150, 8, 3
    kw = dict(lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=_cov(nc))
    x0 = np.stack([SC.start_state(tracks[tos[b]], nc, b) for b in range(B)])
    eng = eng_mod.Engine("car", nc, kind, K, T, batch=B, track=None, **kw)
    eng.set_tracks(tracks, tos)
    eng.set_env_params_slots(params)
    got = _two_steps(eng, x0, [900 + b for b in range(B)])
    eng.close()
    for b in range(B):
        one = eng_mod.Engine("car", nc, kind, K, T, batch=1, track=tracks[tos[b]], env_params=params[b], **kw)
        ref = _two_steps(one, x0[b][None], [900 + b])
        one.close()
        for step in range(2):
            for i, name in enumerate(("cost", "control", "U", "iters_run")):
                assert np.array_equal(got[step][i][b], ref[step][i][0]), (kind, nc, b, step, name)
    assert not np.array_equal(got[1][1][0], got[1][1][2])       # slots 0 and 2 share a track and differ in their parameters


@pytest.mark.parametrize("kind", ["gmppi", "cemppi"])
def test_slot_on_a_small_track_beside_a_large_one(eng_mod, oracle, kind):
    """the 5-point slot runs the ring-only placement here and every table in LDS as a one-slot handle: held to the oracle tolerances, bits reported"""
    tracks = [SC.ring(5, 45.0), SC.ring(191, 191 * 6.0 / (2 * np.pi))]
    params = SC.car_params4(oracle)[:2]
    B, K, T, N = 2, 150, 8, 3
    kw = dict(lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=SC.COV)
    x0 = np.stack([SC.start_state(tracks[b], 1, b) for b in range(B)])
    eng = eng_mod.Engine("car", 1, kind, K, T, batch=B, track=None, **kw)
    eng.set_tracks(tracks)
    eng.set_env_params_slots(params)
    got = _two_steps(eng, x0, [900, 901])
    eng.close()
    for b in range(B):
        one = eng_mod.Engine("car", 1, kind, K, T, batch=1, track=tracks[b], env_params=params[b], **kw)
        ref = _two_steps(one, x0[b][None], [900 + b])
        one.close()
        for step in range(2):
            assert got[step][3][b] == ref[step][3][0]
            assert rel_err(got[step][0][b], ref[step][0][0]) < RTOL
            assert np.max(np.abs(got[step][1][b] - ref[step][1][0])) < 1e-8 and np.max(np.abs(got[step][2][b] - ref[step][2][0])) < 1e-8
        print("[slot env] %s slot %d (P %d beside P 191): bits equal to its one-slot handle: %s"
              % (kind, b, len(tracks[b][0]), all(np.array_equal(got[s][i][b], ref[s][i][0]) for s in range(2) for i in range(4))))


# ---- 4. schedules -----------------------------------------------------------------------------------------------------------------------------

def test_part_chain_schedules_bit_identical(eng_mod, oracle, track):
    tracks, p4 = SC.tracks3(track), SC.car_params4(oracle)
    B, K, T, N = 5, 128, 8, 3
    tos = [2, 0, 2, 1, 0]
    params = p4[[0, 1, 2, 3, 2]]
    x0 = np.stack([SC.start_state(tracks[tos[b]], 1, b) for b in range(B)])
    outs = []
    for parts in (1, 3):
        eng = eng_mod.Engine("car", 1, "musigmaaismppi", K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, cov=SC.COV, track=None)
        eng.set_tracks(tracks, tos)
        eng.set_env_params_slots(params)
        eng.set_overlap(parts)
        outs.append(_two_steps(eng, x0, [300 + b for b in range(B)]))
        eng.close()
    for step in range(2):
        for i in range(4):
            for b in range(B):
                assert np.array_equal(outs[0][step][i][b], outs[1][step][i][b]), (step, i, b)
    assert len({outs[0][1][1][b].tobytes() for b in range(B)}) == B


def test_early_break_leaves_a_slot_alone_in_every_schedule(eng_mod, oracle, track):
    """:cemppi, slot 1's noise so small that its costs tie: it breaks in the first iteration (as tests/test_gpu_parity.py::test_elite_early_break),
    under one stream and under three part-chains, beside slots with other tracks and parameters"""
    tracks, p4 = SC.tracks3(track), SC.car_params4(oracle)
    B, K, T, N = 5, 150, 8, 3
    tos = [2, 0, 2, 1, 0]
    params = p4[[0, 1, 2, 3, 2]]
    x0 = np.stack([SC.start_state(tracks[tos[b]], 1, b) for b in range(B)])
    Z = np.random.default_rng(12).standard_normal((B, N, K, 2 * T))
    Z[1] *= 1e-9
    outs = []
    for parts in (1, 3):
        eng = eng_mod.Engine("car", 1, "cemppi", K, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=SC.COV, track=None)
        eng.set_tracks(tracks, tos)
        eng.set_env_params_slots(params)
        eng.set_overlap(parts)
        eng.set_state(x0)
        g = eng.policy_step(Z)
        outs.append((g["cost"], g["control"], eng.get_U(), g["iters_run"]))
        eng.close()
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
    env = oracle.OracleEnv("car", 1, params=params[1], track=tracks[tos[1]])
    env.state = x0[1]
    pol = oracle.OraclePolicy("cemppi", env, K, T, lam=10.0, U0=np.zeros(2), cov=SC.COV, N=N, lam_ais=20.0, elite_threshold=0.8)
    ref = pol(env, Z[1])
    assert outs[0][3][1] == ref["iters_run"] < N and all(outs[0][3][b] == N for b in (0, 2, 3, 4)), outs[0][3]
    assert rel_err(outs[0][0][1], ref["cost"]) < 1e-7 and np.max(np.abs(outs[0][1][1] - ref["control"])) < 1e-7      # (the tolerances of test_elite_early_break)


# ---- 5. switching -----------------------------------------------------------------------------------------------------------------------------

def test_switching_back_and_refused_calls(eng_mod, oracle, track):
    from mpopis_amd._lib import MPOPISError
    tracks, params, tos = SC.tracks3(track), SC.car_params4(oracle), SC.TRACK_OF_SLOT
    B, K, T, N = 4, 128, 8, 3
    kw = dict(lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=SC.COV)
    Z = np.random.default_rng(3).standard_normal((2, B, N, K, 2 * T))
    x0 = np.stack([SC.start_state(tracks[0], 1, b) for b in range(B)])
    pshared = params[3]

    def step(eng, z):
        eng.set_state(x0); eng.set_U(np.zeros((B, 2 * T)))
        g = eng.policy_step(z)
        return g["cost"], g["control"], eng.get_U(), g["iters_run"]

    eng = eng_mod.Engine("car", 1, "cemppi", K, T, batch=B, track=tracks[1], **kw)
    eng.set_tracks(tracks, tos)
    eng.set_env_params_slots(params)
    first = step(eng, Z[0])
    # refused calls between two steps: the handle stays exactly as it was, and the message names the slot or track
    with pytest.raises(MPOPISError) as ei:
        eng.set_tracks(tracks, [0, 1, 3, 2])
    assert ei.value.code == -1 and "slot 2" in str(ei.value), str(ei.value)
    with pytest.raises(MPOPISError) as ei:
        eng.set_tracks([tracks[0], tuple(v[:1] for v in tracks[1]), tracks[2]], tos)
    assert ei.value.code == -1 and "track 1" in str(ei.value), str(ei.value)
    with pytest.raises(MPOPISError) as ei:
        eng.set_env_params_slots(params[:, :19])
    assert ei.value.code == -1 and "20" in str(ei.value), str(ei.value)
    again = step(eng, Z[0])
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # back to the shared track and parameters: a handle that was never switched
    eng.set_track(*tracks[0])
    eng.set_env_params(pshared)
    second = step(eng, Z[1])
    eng.close()
    fresh = eng_mod.Engine("car", 1, "cemppi", K, T, batch=B, track=tracks[0], env_params=pshared, **kw)
    ref = step(fresh, Z[1])
    fresh.close()
    assert all(np.array_equal(a, b) for a, b in zip(second, ref))
    assert not np.array_equal(first[0], ref[0])


def test_only_one_of_the_two_per_slot(eng_mod, oracle, track):
    """per-slot tracks with shared parameters, and per-slot parameters with the shared track: the other half is the shared value in every slot"""
    tracks, params = SC.tracks3(track), SC.car_params4(oracle)
    nc, K, T, B = 1, 65, 5, 3
    rng = np.random.default_rng(21)
    U, E = SC.level1_inputs(rng, B, nc, K, T)
    for which in ("tracks", "params"):
        eng = eng_mod.Engine("car", nc, "gmppi", K, T, batch=B, lam=10.0, cov=SC.COV, track=tracks[0], env_params=params[3])
        if which == "tracks":
            eng.set_tracks(tracks)
        else:
            eng.set_env_params_slots(params[:B])
        trk = [tracks[b] if which == "tracks" else tracks[0] for b in range(B)]
        par = [params[3] if which == "tracks" else params[b] for b in range(B)]
        x0 = np.stack([SC.start_state(trk[b], nc, b) for b in range(B)])
        got = eng.rollout_costs(U, E, x0=x0)
        eng.close()
        for b in range(B):
            env = oracle.OracleEnv("car", nc, params=par[b], track=trk[b])
            env.state = x0[b]
            pol = oracle.OraclePolicy("gmppi", env, K, T, lam=10.0, U0=np.zeros(2), cov=SC.COV)
            assert rel_err(got[b], pol.simulate_model(U[b], E[b].T)) < RTOL, (which, b)


def test_wrong_handle_kinds(eng_mod, track):
    import os
    import types
    from mpopis_amd import build
    from mpopis_amd._lib import MPOPISError
    from tests.helpers import pointmass_ref as PM
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mc = eng_mod.Engine("mountaincar", 0, "gmppi", 64, 5, batch=2, lam=0.1, cov=[1.5])
    with pytest.raises(MPOPISError) as ei:
        mc.set_tracks([track, track])
    assert ei.value.code == -1 and "car" in str(ei.value)
    mc.close()
    env = types.SimpleNamespace(code_object=build.build_env(os.path.join(root, "tests", "helpers", "envs", "pointmass_sdk.hip")), state_size=PM.SS,
                                action_size=PM.AS, params=np.array(PM.PARAMS, dtype=np.float64), lo=PM.LO, hi=PM.HI, reset_state=None)
    cu = eng_mod.Engine("custom", 0, "gmppi", 64, 5, batch=2, lam=1.0, cov=[0.3, 0.3, 0.1], custom_env=env)
    with pytest.raises(MPOPISError) as ei:
        cu.set_env_params_slots(np.tile(PM.PARAMS, (2, 1)))
    assert ei.value.code == -1 and "mpopis_set_env_table" in str(ei.value) and "per_slot" in str(ei.value)
    cu.close()


# ---- 6. real env and harness ------------------------------------------------------------------------------------------------------------------

def test_env_step_and_query_per_slot(eng_mod, oracle, track):
    tracks, p4 = SC.tracks3(track), SC.car_params4(oracle)
    # slots 0, 1: the same position, off slot 0's polygon (P 5) and on slot 1's ellipse (P 12); slots 2, 3: the same sliding state, beyond slot 2's β_limit
    # (0.785) and within slot 3's (1.7)
    tos = [1, 2, 0, 0]
    params = p4[[0, 0, 0, 1]]
    B = 4
    on_ellipse = np.array([tracks[2][0][1], tracks[2][1][1]])
    assert not oracle.within_track(tracks[1], on_ellipse)[0] and oracle.within_track(tracks[2], on_ellipse)[0]
    x0 = np.stack([SC.start_state(tracks[tos[b]], 1, b) for b in range(B)])
    x0[0, :2] = on_ellipse; x0[1] = x0[0]
    x0[3] = x0[2]
    x0[2:, 3], x0[2:, 4] = 15.0, 18.0                           # |β| = atan(18 / 15) = 0.876
    eng = eng_mod.Engine("car", 1, "gmppi", 64, 5, batch=B, lam=10.0, cov=SC.COV, track=None)
    eng.set_tracks(tracks, tos)
    eng.set_env_params_slots(params)
    eng.set_state(x0)
    envs = []
    for b in range(B):
        env = oracle.OracleEnv("car", 1, params=params[b], track=tracks[tos[b]])
        env.state = x0[b]
        envs.append(env)
    rew, within, dist, beta = eng.env_query()
    for b in range(B):
        w_ref, d_ref = oracle.within_track(tracks[tos[b]], x0[b, :2])
        assert bool(within[b]) == w_ref and abs(dist[b, 0] - d_ref) <= 1e-12 * max(1.0, d_ref)
        assert abs(rew[b] - envs[b].reward()) <= 1e-12 * abs(envs[b].reward()), (b, rew[b], envs[b].reward())
    assert not within[0] and within[1]
    assert abs(rew[2] - rew[3]) > 1000.0                        # the β penalty in slot 2 only
    acts = np.array([[0.5, 0.2], [0.5, 0.2], [-0.3, 0.4], [-0.3, 0.4]])
    for _ in range(4):
        r = eng.env_step(acts)
        x, _, _ = eng.get_state()
        for b in range(B):
            envs[b].step(acts[b])
            assert np.max(np.abs(x[b] - envs[b].state)) < 1e-10 and abs(r[b] - envs[b].reward()) < 1e-9 * abs(envs[b].reward()), b
    eng.close()


def test_run_trials_per_slot(eng_mod, oracle, track):
    tracks, p4 = SC.tracks3(track), SC.car_params4(oracle)
    B, K, T, N, steps, seed = 3, 64, 8, 3, 12, 4100
    tos = [2, 0, 1]
    params = p4[[1, 2, 3]]
    kw = dict(lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=SC.COV, seed=seed)
    x0 = np.stack([SC.start_state(tracks[tos[b]], 1, b) for b in range(B)])
    eng = eng_mod.Engine("car", 1, "cemppi", K, T, batch=B, track=None, **kw)
    eng.set_tracks(tracks, tos)
    eng.set_env_params_slots(params)
    eng.set_state(x0)
    rec, acts = eng.run_trials(num_steps=steps, laps=1, log_actions=True)
    eng.close()
    for b in range(B):
        env = oracle.OracleEnv("car", 1, params=params[b], track=tracks[tos[b]])
        env.state = x0[b]
        pol = oracle.OraclePolicy("cemppi", env, K, T, lam=10.0, U0=np.zeros(2), cov=SC.COV, N=N, lam_ais=20.0, elite_threshold=0.8, nthreads=8)
        r = pol.run_trial(env, seed + b + 1, num_steps=steps, laps=1, log_actions=True)
        assert r["status"] == 0 and rec[b, 15] == 0
        n = int(r["steps"])
        assert rec[b, 1] == r["steps"] and rec[b, 14] == r["rollouts"]
        assert np.max(np.abs(acts[b][:n] - r["actions"][:n])) < 1e-6
        ref = np.array([r["rew"], r["steps"], r["rew_per_step"]] + r["lap_t"] + [r["mean_v"], r["max_v"], r["mean_beta"], r["max_beta"], r["beta_viol"], r["trk_viol"], r["crash_viol"]])
        assert np.array_equal(rec[b, 11:14], ref[11:14]), (rec[b, 11:14], ref[11:14])
        assert np.max(np.abs(rec[b, :11] - ref[:11]) / np.maximum(1.0, np.abs(ref[:11]))) < 1e-6, (rec[b, :11], ref[:11])
        one = eng_mod.Engine("car", 1, "cemppi", K, T, batch=1, track=tracks[tos[b]], env_params=params[b], **kw)
        one.seed_slots([seed + b + 1])
        one.set_state(x0[b][None])
        rec1, acts1 = one.run_trials(num_steps=steps, laps=1, log_actions=True)
        one.close()
        assert np.array_equal(rec1[0], rec[b]) and np.array_equal(acts1[0], acts[b]), b


# ---- 7. simple envs ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 15])
@pytest.mark.parametrize("K", [63, 65])
@pytest.mark.parametrize("kind", ["mountaincar", "cartpole"])
def test_simple_envs_per_slot(eng_mod, oracle, kind, K, T):
    rng = np.random.default_rng(K + T)
    if kind == "mountaincar":
        B = 3
        params = np.stack([oracle.mountaincar_default_params() for _ in range(B)])
        params[1, 5] *= 1.6; params[1, 6] *= 0.8; params[1, 7] = 7        # power, gravity, max_steps (reached inside the longer horizon)
        params[2, 5] *= 0.5; params[2, 6] *= 1.3; params[2, 7] = 150
        x0 = np.array([[-0.5, 0.0], [-0.45, 0.01], [-0.6, -0.01]])
        scale, lam, cov = 1.2, 0.1, [1.5]
    else:
        B = 2
        params = np.stack([oracle.cartpole_default_params() for _ in range(B)])
        params[1, 0] = 7.0; params[1, 6] = 14.0; params[1, 7] = 0.03; params[1, 10] = 9       # gravity, force_mag, dt, max_steps
        x0 = np.array([[0.01, -0.02, 0.03, 0.01], [-0.03, 0.04, -0.02, 0.02]])
        scale, lam, cov = 0.8, 0.1, [1.5]
    eng = eng_mod.Engine(kind, 0, "gmppi", K, T, batch=B, lam=lam, cov=cov)
    eng.set_env_params_slots(params)
    E = rng.standard_normal((B, K, T)) * scale
    U = rng.uniform(-0.2, 0.2, (B, T))
    got = eng.rollout_costs(U, E, x0=x0)
    eng.close()
    for b in range(B):
        env = oracle.OracleEnv(kind, params=params[b])
        env.state = x0[b]
        pol = oracle.OraclePolicy("gmppi", env, K, T, lam=lam, U0=[0.0], cov=cov)
        assert rel_err(got[b], pol.simulate_model(U[b], E[b].T)) < 1e-12, (kind, b)


# ---- 8. Python harness ------------------------------------------------------------------------------------------------------------------------

def test_simulate_car_racing_tracks_and_params(eng_mod, oracle):
    from mpopis_amd.examples import simulate_car_racing
    names = ["curve", "cubic", "curve"]
    params = SC.car_params4(oracle)[[1, 2, 3]]
    kw = dict(num_steps=5, num_samples=64, quiet=True)
    allrec, _ = simulate_car_racing(num_trials=3, track=names, car_params=params, seed=1, **kw)
    assert np.array_equal(allrec[:, 0], [1, 2, 3])
    for k in (1, 2, 3):
        one, _ = simulate_car_racing(num_trials=1, track=names[k - 1], car_params=params[k - 1], seed=1 + k - 1, **kw)
        assert np.array_equal(one[0, 1:-1], allrec[k - 1, 1:-1]), k          # every column but the trial id and the wall time
    assert not np.array_equal(allrec[0, 1:4], allrec[2, 1:4])
