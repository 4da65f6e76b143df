"""No GPU: what tests/test_gpu_loop_harness.py relies on, shown on the CPU (tests/helpers/loop_cases.py).
(a) bookkeeping_ref, restated from the Julia trial loop, reproduces the oracle's own loop: OraclePolicy.run_trial on a rough and a calm closed loop for
    1 and 3 cars, with and without state noise, its logged actions replayed through OracleEnv.step -- counters, steps and lap times exact, sums within
    the bound of (c).
(b) every scripted case reaches the branch it is named for, asserted on the reference's trace.
(c) the derived bound of the accumulated statistics holds for a float64 restatement against np.longdouble; the measured margin is printed.
(d) each checker refuses the corruption it is meant for, on results built on the host and put through the harness's file format."""
import numpy as np
import pytest
from tests.helpers import loop_cases as LC

NS = 54


def _start(oracle, nc, mood):
    """rough: a start that is already in trouble (tests/test_gpu_edge_cases.py) -- near the lane's edge heading outwards, sliding beyond the slip-angle limit"""
    env = oracle.OracleEnv("car", nc)
    env.reset()
    if mood == "rough":
        s = env.state
        for c in range(nc):
            s[8 * c] += 11.0; s[8 * c + 2] -= 0.6; s[8 * c + 3] = 12.0; s[8 * c + 4] = 14.0 + c
        env.state = s
    return env


def _replay(oracle, nc, actions, seed, sig, mood):
    env = _start(oracle, nc, mood)
    xs, rew = [], []
    for s, a in enumerate(actions):
        assert env.step(a) == 0
        xs.append(env.state)
        rew.append(env.reward())
        if sig is not None and nc == 1:
            env.state = LC.noise_ref(env.state, seed, s, sig, np.float64)[0]
    return np.array(xs), np.array(rew)


# ================================================================ (a) ==========================================================================
@pytest.mark.parametrize("sig", [None, (0.05, 0.03, 0.001)], ids=["quiet", "noise"])
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("mood", ["rough", "calm"])
def test_bookkeeping_ref_reproduces_the_oracles_loop(oracle, mood, nc, sig):
    K, T, kw = (16, 8, dict(lam=1e4, cov=np.full(2 * nc, 1.0))) if mood == "rough" else (64, 12, dict(lam=1.0, cov=np.full(2 * nc, 0.3)))
    num_steps, laps, seed = (60, 2, 7) if mood == "rough" else (40, 1, 11)
    env = _start(oracle, nc, mood)
    pol = oracle.OraclePolicy("mppi", env, K, T, **kw)
    rec = pol.run_trial(env, seed, num_steps=num_steps, laps=laps, log_actions=True, state_noise=sig or (0.0, 0.0, 0.0))
    assert rec["status"] == 0
    xs, rew = _replay(oracle, nc, rec["actions"], seed, sig, mood)
    tk, blim = oracle.load_track(), float(LC.car_params()[17])
    ref = LC.bookkeeping_ref(LC.ENV_CAR, nc, xs, rew, np.ones(len(xs), dtype=np.int32), np.zeros(len(xs)), K, num_steps, laps, blim=blim,
                             within_fn=lambda p: oracle.within_track(tk, p)[0], noise=(seed, sig) if sig else None)
    got = LC.record_of(ref[-1]["hs"])
    print("\n[oracle loop %s, %d cars, %s] steps %d laps %s trk %d beta %d crash %d" % (mood, nc, "noise" if sig else "quiet", rec["steps"], rec["lap_t"], rec["trk_viol"],
                                                                                   rec["beta_viol"], rec["crash_viol"]))
    for k in ("steps", "beta_viol", "trk_viol", "crash_viol", "rollouts"):
        assert got[k] == rec[k], (k, got[k], rec[k])
    assert got["lap_t"] == rec["lap_t"]
    assert got["rew"] == rec["rew"]                                          # the same additions in the same order
    n = int(rec["steps"]) + 1
    for k, f in (("mean_v", LC.H_VMEAN), ("mean_beta", LC.H_BMEAN)):
        assert abs(got[k] - rec[k]) * n <= 2 * LC.stat_bound(f, nc, n, rec[k] * n), (k, got[k], rec[k])      # two float64 evaluations, each within the bound
    assert abs(got["max_v"] - rec["max_v"]) <= 2 * LC.ulp_of(rec["max_v"]) and abs(got["max_beta"] - rec["max_beta"]) <= 2 * LC.ulp_of(rec["max_beta"])
    if mood == "rough":
        assert rec["trk_viol"] + rec["beta_viol"] > 0, "the rough loop must violate something"
    else:
        assert rec["trk_viol"] + rec["beta_viol"] + rec["crash_viol"] == 0 and rec["steps"] == num_steps, "the calm loop runs clean to the step limit"


# ================================================================ (b) ==========================================================================
@pytest.mark.parametrize("nc", [1, 3, 8])
def test_every_scripted_case_reaches_its_branch(oracle, nc):
    tk, blim = LC.default_track(), float(LC.car_params()[17])
    ON, OFF = LC.on_off_points(tk)
    assert oracle.within_track(tk, ON)[0] and not oracle.within_track(tk, OFF)[0] and np.hypot(*ON) > 40
    scripts = LC.update_scripts(nc, NS, tk, blim)
    seen = set()
    for sc in scripts:
        ref = LC.bookkeeping_ref(LC.ENV_CAR, nc, sc["xs"], sc["rew"], sc["iters"], np.zeros(NS), 7, NS - 1, 4, blim=blim, within_fn=lambda p: oracle.within_track(tk, p)[0])
        for s, want in sc["notes"].items():
            tr, r = ref[s]["tr"], ref[s]
            assert tr["ran"], (sc["name"], s)
            for k, v in want.items():
                if k == "alive":
                    assert r["alive"] == v, (sc["name"], s, k)
                elif k == "neg_zero":
                    assert tr["curr_y"] == 0.0 and np.signbit(tr["curr_y"]), (sc["name"], s)
                elif k == "neg_zero_prev":
                    assert tr["prev_y"] == 0.0 and np.signbit(tr["prev_y"]), (sc["name"], s)
                elif k == "lap_and_end":
                    assert tr["lapped"] and (tr["trk"] == 11 or tr["beta"] == 51) and tr["lap"] < 4 and r["alive"] == 0 and ref[s - 1]["alive"] == 1, (sc["name"], s, tr)
                elif k in ("curr_y", "prev_y", "d", "temp_rew"):
                    assert tr[k] == v and np.signbit(tr[k]) == np.signbit(v), (sc["name"], s, k, tr[k], v)
                else:
                    assert tr[k] == v, (sc["name"], s, k, tr[k], v)
            seen.add(sc["name"])
        if sc["name"] == "trk_11":
            assert [ref[s]["tr"]["trk"] for s in range(1, 12)] == list(range(1, 12)) and not ref[12]["tr"]["ran"]      # violation 11 at step 11 and not before
        if sc["name"] == "beta_51":
            assert ref[50]["alive"] == 1 and ref[51]["alive"] == 0 and not ref[52]["tr"]["ran"]
        if sc["name"] == "lap_zero":
            assert list(ref[-1]["hs"][LC.H_LAP0:LC.H_LAP0 + 4]) == [3.0, 5.0, 7.0, 10.0]                                # laps 1..4 with their step numbers (cnt = s + 1)
            assert ref[8]["tr"]["curr_y"] == -5e-324 and ref[6]["tr"]["curr_y"] == 5e-324
        if sc["name"] == "plain":
            assert ref[NS - 2]["cnt"] == NS - 1 and ref[NS - 2]["alive"] == 1 and ref[NS - 1]["cnt"] == NS and ref[NS - 1]["alive"] == 0      # alive through cnt == num_steps
        if sc["name"].startswith("crash") or sc["name"] == "rew_4000":
            if nc > 1:                                                        # exactly one car is outside / over the limit
                last = sc["xs"][2].reshape(nc, 8)
                outside = [not oracle.within_track(tk, c[:2])[0] for c in last]
                over = [abs(np.arctan2(c[4], c[3])) > blim for c in last]
                assert sum(outside) <= 1 and sum(over) <= 1 and sum(outside) + sum(over) >= (0 if sc["name"] == "crash_00" else 1)
    assert seen == {sc["name"] for sc in scripts}
    # laps == 0 ends every slot at step 0
    ref = LC.bookkeeping_ref(LC.ENV_CAR, nc, scripts[-1]["xs"][:3], scripts[-1]["rew"][:3], scripts[-1]["iters"][:3], np.zeros(3), 7, 5, 0, blim=blim, within_fn=lambda p: True)
    assert [r["alive"] for r in ref] == [0, 0, 0] and ref[2]["cnt"] == 1


def test_pair_edge_cases_are_what_they_claim(oracle):
    q, st = LC.pair_edge_launches()
    for b, contact in enumerate(q["contact"]):
        dd = LC.pair_terms(q["x"][b], 2)[0]
        assert (dd <= 4.0) == contact, (b, dd)
    assert LC.pair_terms(q["x"][0], 2)[0] == 4.0 and LC.pair_terms(q["x"][1], 2)[0] == np.nextafter(4.0, 5.0) and LC.pair_terms(q["x"][2], 2)[0] == 5.0
    for b, contact in enumerate(st["contact"]):
        x, _, _, rew = LC.step_ref(oracle, st, b)
        dd = LC.pair_terms(x, 2)[0]
        assert (dd <= 4.0) == contact, (b, dd)
        assert 8.0 < x[1] < 16.0 and 8.0 < x[9] < 16.0                       # both cars stay inside the binade the argument needs
    assert LC.pair_terms(LC.step_ref(oracle, st, 0)[0], 2)[0] == 4.0
    assert LC.step_ref(oracle, st, 0)[3] < LC.step_ref(oracle, st, 1)[3] - 10000.0      # the contact term is what separates the two


# ================================================================ (c) ==========================================================================
def test_statistics_bound_holds_for_a_float64_restatement(oracle):
    rng = np.random.default_rng(3)
    worst = {LC.H_VMEAN: 0.0, LC.H_BMEAN: 0.0}
    for nc, n in ((1, 54), (3, 54), (8, 54), (1, 400), (8, 400)):
        xs = rng.normal(size=(n, nc, 8)) * np.array([50, 50, 1, 15, 3, 1, 1, 1])
        xs[:, :, 1] = 100.0                                                   # no laps: the loop runs to the end
        xs = xs.reshape(n, 8 * nc)
        args = (LC.ENV_CAR, nc, xs, np.full(n, -1.0), np.ones(n, dtype=np.int32), np.zeros(n), 1, n, 4)
        a = LC.bookkeeping_ref(*args, blim=0.7, within_fn=lambda p: True)
        b = LC.bookkeeping_ref(*args, blim=0.7, within_fn=lambda p: True, dtype=LC.LD)
        for s in range(n):
            for f in worst:
                bound = LC.stat_bound(f, nc, s + 1, b[s]["hs"][f])
                err = abs(float(LC.LD(a[s]["hs"][f]) - b[s]["hs"][f]))
                assert err <= bound, (nc, s, f, err, bound)
                worst[f] = max(worst[f], err / bound)
            assert LC.ulp_err(a[s]["hs"][LC.H_VMAX], b[s]["hs"][LC.H_VMAX]) <= 2 and LC.ulp_err(a[s]["hs"][LC.H_BMAX], b[s]["hs"][LC.H_BMAX]) <= 2
    print("\n[bound] float64 restatement against long double: vmean error / bound %.3f, bmean error / bound %.3f (margin %.1fx, %.1fx)" %
          (worst[LC.H_VMEAN], worst[LC.H_BMEAN], 1 / worst[LC.H_VMEAN], 1 / worst[LC.H_BMEAN]))
    assert 0 < worst[LC.H_VMEAN] <= 1 and 0 < worst[LC.H_BMEAN] <= 1
    # the noise cases keep sigma RNG_TOL below half an ulp of the coordinate they move
    xs = LC.noise_scripts(6)[0]["xs"]
    assert np.all(LC.NOISE_SIG[0] * LC.RNG_TOL <= 0.5 * LC.ulp_of(xs[:, 0])) and np.all(LC.NOISE_SIG[1] * LC.RNG_TOL <= 0.5 * LC.ulp_of(xs[:, 1]))
    assert np.all(LC.NOISE_SIG[2] * LC.RNG_TOL <= 0.5 * LC.ulp_of(xs[:, 2]))


# ================================================================ (d) ==========================================================================
def _host_loop(oracle, L):
    """what tools/kbench_loop.hip would write for a scripted LOOP launch if the kernels were the reference"""
    env, B, nS, S = L["env"], L["B"], L["nS"], L["num_steps"] + 1
    ss, as_, nc = LC.state_size(env), LC.action_size(env), max(1, env["ncars"])
    car = env["kind"] == LC.ENV_CAR
    R = dict(hs_log=np.zeros((nS, B, 16)), alive_log=np.zeros((nS, B), dtype=np.int32), x_log=L["xs"].copy(), reward_log=L["reward"].copy(),
             q_within=np.ones((nS, B), dtype=np.int32), q_dist=LC.poisoned((nS, B, nc)), q_beta=LC.poisoned((nS, B, nc)), actlog=LC.poisoned((B, S, as_)), status=np.zeros(B, dtype=np.int32),
             t=np.zeros(B, dtype=np.int32), states=LC.poisoned((B, S + 1, ss)), rewards=LC.poisoned((B, S)), iters=LC.poisoned((B, S), 1), tr_within=LC.poisoned((B, S), 1),
             tr_dist=LC.poisoned((B, S, nc)), tr_beta=LC.poisoned((B, S, nc)))
    R["states"][:, 0] = L["x0"]
    cache = {}
    alive0 = np.ones(B, dtype=np.int32) if L["alive0"] is None else L["alive0"]
    for b in range(B):
        ref = list(LC.slot_ref(L, b, oracle, np.float64, cache))
        for s in range(nS):
            if not alive0[b]:                                                 # dead from the start: launch_harness_init's values stay
                ref[s] = dict(hs=LC.init_hs(), alive=0, tr=dict(ran=False))
            R["hs_log"][s, b], R["alive_log"][s, b] = ref[s]["hs"], ref[s]["alive"]
            if car:
                cars = L["xs"][s, b].reshape(nc, 8)
                wd = [oracle.within_track(LC.slot_track(env, b), c[:2]) for c in cars]
                R["q_within"][s, b] = int(all(w for w, _ in wd)); R["q_dist"][s, b] = [d for _, d in wd]; R["q_beta"][s, b] = [np.arctan2(c[4], c[3]) for c in cars]
            if ref[s]["tr"]["ran"]:
                R["actlog"][b, s] = L["control"][s, b]; R["states"][b, s + 1] = L["xs"][s, b]; R["rewards"][b, s] = L["reward"][s, b]; R["iters"][b, s] = L["iters"][s, b]
                R["tr_within"][b, s] = R["q_within"][s, b]
                if car:
                    R["tr_dist"][b, s] = R["q_dist"][s, b]; R["tr_beta"][b, s] = R["q_beta"][s, b]
    R["hs"], R["alive"], R["x"] = R["hs_log"][-1], R["alive_log"][-1], R["x_log"][-1]
    return R


def _through_file(L, R, **kw):
    return LC.unpack_result(LC.pack_result([L], [R], **kw), [L])[0]


def test_loop_checker_refuses_what_it_is_meant_for(oracle):
    nc = 3
    tk, blim = LC.default_track(), float(LC.car_params()[17])
    scripts = LC.update_scripts(nc, NS, tk, blim)
    names = [s["name"] for s in scripts]
    L = LC.loop_launch(LC.car_env(nc), scripts, list(range(len(scripts))), NS, NS - 1, 4)
    assert len(LC.pack([L])) > 0
    R = _host_loop(oracle, L)
    cache = {}
    LC.check_loop(L, _through_file(L, R), oracle, log=lambda *a: None, cache=cache)
    def refused(mutate, **kw):
        M = {k: (None if v is None else np.array(v, copy=True)) for k, v in R.items()}
        mutate(M)
        with pytest.raises(AssertionError):
            LC.check_loop(L, _through_file(L, M, **kw), oracle, log=lambda *a: None, cache=cache)
    b = names.index("trk_11")
    def counter_off(M): M["hs_log"][11:, b, LC.H_TRK] += 1; M["hs"][b, LC.H_TRK] += 1
    refused(counter_off)                                                      # a counter off by one
    b2 = names.index("lap_zero")
    def lap_shift(M): M["hs_log"][2:, b2, LC.H_LAP0] += 1; M["hs"][b2, LC.H_LAP0] += 1
    refused(lap_shift)                                                        # a lap time shifted by a step
    b3 = names.index("rew_4000")
    def within_dropped(M): M["tr_within"][b3, 3] = 1; M["q_within"][3, b3] = 1
    refused(within_dropped)                                                   # `within` of the one car outside dropped from the AND (trace and query alike)
    def trk_not_counted(M): M["hs_log"][3:, b3, LC.H_TRK] -= 1; M["hs"][b3, LC.H_TRK] -= 1
    refused(trk_not_counted)                                                  # ... and from the violation counter
    def alive_late(M): M["alive_log"][11, b] = 1
    refused(alive_late)                                                       # the slot ends one step late
    def dead_row_written(M): M["actlog"][b, 20] = 0.0
    refused(dead_row_written)                                                 # a dead slot's action log row written
    def mean_off(M): M["hs_log"][5:, 0, LC.H_VMEAN] *= 1 + 1e-13; M["hs"][0, LC.H_VMEAN] *= 1 + 1e-13
    refused(mean_off)                                                         # a per-car mean off in the 13th digit (the 1e-6 of the closed-loop tests hides it)
    refused(lambda M: None, guard_hit=(0, "hs", 5))                           # a write past the end


def test_plan_and_reorder_checkers_refuse_what_they_are_meant_for():
    rng = np.random.default_rng(1)
    K, top, cs = 65, 4, 6
    rows = LC.weight_rows(K, rng)
    L = LC.plan_launch(K, top, cs, [rows["ties_across_strides"], rows["random"], rows["equal"]], 5, active=np.array([1, 1, 0], dtype=np.int32))
    idx = np.stack([LC.plan_order(r, top) for r in L["w"]])
    R = dict(idx=idx.copy(), wsel=np.take_along_axis(L["w"], idx, 1), controls=L["Uin"] + L["wn"],
             Eplan=np.concatenate([L["wn"][:, :, None], np.stack([L["E"][b][:, idx[b]] + (L["Ucur"][b] - L["Uin"][b])[:, None] for b in range(3)])], axis=2))
    for k in R:
        R[k][2] = LC.poisoned(R[k][2].shape, 1 if k == "idx" else 0)
    LC.check_plan(L, _through_file(L, R))
    def refused(mutate):
        M = {k: v.copy() for k, v in R.items()}
        mutate(M)
        with pytest.raises(AssertionError):
            LC.check_plan(L, _through_file(L, M))
    assert L["w"][0][idx[0, 0]] == L["w"][0][idx[0, 1]] == 0.75
    def tie_swapped(M): M["idx"][0, [0, 1]] = M["idx"][0, [1, 0]]
    refused(tie_swapped)                                                      # a plan index swapped under a tie (wsel stays right: only the order catches it)
    def poison_left(M): M["Eplan"][1, 3, 2] = LC.poisoned((1,))[0]
    refused(poison_left)                                                      # poison left in an active slot
    def inactive_written(M): M["controls"][2, 0] = 0.0
    refused(inactive_written)
    def duplicate(M): M["idx"][1, 1] = M["idx"][1, 0]
    refused(duplicate)
    Lr = LC.reorder_launches()[-1]
    want = np.ascontiguousarray(np.transpose(Lr["in"], (1, 0, 2)))
    LC.check_reorder(Lr, _through_file(Lr, dict(out=want)))
    bad = want.copy(); bad[0, 1], bad[1, 0] = want[1, 0].copy(), want[0, 1].copy()
    with pytest.raises(AssertionError):
        LC.check_reorder(Lr, _through_file(Lr, dict(out=bad)))
    for K in LC.PLAN_K:                                                       # every weight row is inside the kernel's contract, every unsafe row outside it
        for name, r in LC.weight_rows(K, rng).items():
            assert r.shape == (K,) and np.all(np.isfinite(r)) and not np.any(np.signbit(r)), (K, name)
        for name, r in LC.unsafe_rows(K, rng).items():
            assert np.any(np.isnan(r) | np.isinf(r) | np.signbit(r)), (K, name)
