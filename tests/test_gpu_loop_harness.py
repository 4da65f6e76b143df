"""The closed loop between two policy steps -- k_env_step / k_env_query (kernels_reweight.hip), k_harness_init / k_harness_update (kernels_harness.hip),
k_trace_start / _step / _reorder (kernels_trace.hip), k_plan_select / _assemble (kernels_plan.hip) -- exercised directly, below the API, through the C++
harness tools/kbench_loop.hip: one process per case file, inputs written by the test, raw device outputs read back.  The harness holds no reference
arithmetic, fills every output with 0xA5 and gives it 64 guard entries (checked on every read).  The bookkeeping cases are SCRIPTED: the test decides
the state and the reward of every step, so each branch is reached on purpose and the counters are held exactly after EVERY step.  Cases, references
and checks are those of tests/helpers/loop_cases.py; tests/test_loop_cases_cpu.py shows on the CPU that bookkeeping_ref reproduces the oracle's own
loop, that every case reaches the branch it is named for, that the derived bounds hold, and that each checker refuses the corruption it is meant for.

Held exactly (bits) after every step: the violation counters, cnt, lap, the lap times, prev_y, the reward sum (the same additions in the same order),
rollouts, alive, the action log; a dead slot's hs, x, action log row and trace rows; the trace's dist / beta / within against k_env_query's on the same
state; idx against plan_order, wsel, controls and every column of the plan's noise block; the reorder against NumPy's transpose.  Held to a derived
bound (loop_cases.py's docstring): vmean within gamma(NC + 1 + n) of the sum, bmean within gamma(NC + 3 + n), vmax / bmax within 2 ulp, the noised x, y,
psi within 2 ulp of the long-double result and the rotated velocity within rot_bound; the env step against the oracle at 1e-10 (state) and 1e-9 (reward),
the query at 1e-12 (tests/test_gpu_parity.py's tolerances).

Branch -> case that takes it / case that does not (CPU proof: test_every_scripted_case_reaches_its_branch, test_pair_edge_cases_are_what_they_claim):
  k_harness_update  b >= B                       B = 1, 63, 65, 130 (a last block with idle lanes) / B = 64
                    !alive[b]                    alive0 = 0 slots, every slot after its end / every live slot
                    noise (seeds, car, 1 car)    test_state_noise one car / three cars, MountainCar, seeds == null everywhere else
                    actlog                       every scripted launch / the noise launches (actlog null)
                    kind != CAR                  test_update_simple_envs / every car launch
                    s[1] < curr_y                lap_zero with 3 and 8 cars (the rearmost car is the last) / one car
                    be > blim                    beta_edge step 1, crash_1x, beta_51 / beta_edge step 2
                    !within_track                rew_4000, crash_x1, trk_11 / plain
                    step_rew < -4000             rew_4000 step 3 / rew_4000 step 2 (-4000 exactly)
                    ex_b, !within_t counters     crash_10, crash_01, crash_11 / crash_00
                    temp_rew < -10500            crash_* step 2 / crash_* step 1 (-10500 exactly)
                    prev_y < 0, curr_y >= 0      lap_zero steps 2, 4 (-0.0), 6 / step 8 (-tiny), step 0 (first step), lap_prev_zero steps 3, 5
                    d <= 15                      lap_d15 step 2 (15.0) / step 4 (the next double)
                    lap 1..4 -> lap0..lap3       lap_zero
                    lap >= laps                  lap_zero step 9, test_update_laps_zero / plain
                    trk > 10, beta > 50          trk_11 step 11, beta_51 step 51 / steps 10, 50
                    cnt <= num_steps             plain: alive at cnt == num_steps, dead at num_steps + 1
  k_env_step        alive null / 0 / 1           test_step_* (alive null == all ones; alive 0 untouched)
                    kind != CAR                  MountainCar, CartPole / car
                    action check                 test_step_action_check: lo, hi pass; neighbours, NaN, +-inf raise; several cars: no check
                    status null                  the null-pointer launch / all others
                    reward null                  the null-pointer launch / all others
                    dd <= 4.0                    pair edges: 4.0 exactly, coincident / the next double, 5.0
  k_env_query       kind != CAR, each null ptr   as above
                    !w (one car outside)         parity slot 1 / the others
  k_trace_step      cnt != step + 1              dead slots and ended slots / live ones
                    each null output             test_trace_null_subsets (every subset of the six)
                    kind != CAR                  test_update_simple_envs (within = 1, no dist / beta)
                    slot_tk                      test_update_slot_env / shared track
                    e < ncars                    8 cars (ss = 64 fills the wave) / 1 and 3 cars
                    the copy's `i += 64`         test_update_simple_envs with ss = 65, 130 / ss = 2, 4, 64

Not asserted: an exact pair distance of 4.0 from a 3-4-5 offset does not exist in binary floating point; the exact 4.0 is axis-aligned (through the query and
through a step), the 3-4-5 offset gives 5.0 exactly.  The state of a simple env after an out-of-range action is not compared (the oracle refuses the step).

Found: nothing wrong in the kernels.  Measured on the MI355X (every run prints its own; DESIGN.md section 2 has the same): see MEASURED below."""
import os
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import loop_cases as LC

MEASURED = """vmean error / bound 0.21 (1 car), 0.20 (3), 0.09 (8), 0.28 (per-slot envs), 0.31 (6 steps after the noise); bmean error / bound 0.21, 0.19, 0.19, 0.21, 0.17
(54 steps unless said); vmax <= 0.87 ulp, bmax <= 0.99 ulp; noise: x, y, psi <= 0.50 ulp, rotated velocity 0.15 of rot_bound, bit-identical across B and slot
position; env step against the oracle: state <= 9.5e-16, reward <= 1.4e-15; several cars, step reward against query reward: bitwise equal in every case run
(bound: 2 ulp per pair term)."""

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NS = 54


@pytest.fixture(scope="module")
def harness():
    return HR.build("loop")


def _run(exe, tmp_path, launches):
    return LC.unpack_result(HR.run_case(exe, tmp_path, LC.pack(launches)), launches)      # checks every guard


def _alive0(B):
    a = np.ones(B, dtype=np.int32)
    a[3::7] = 0
    return a if B > 3 else None


# ================================================================ k_harness_update =============================================================
@pytest.mark.parametrize("nc,Bs", [(1, (1, 63, 64, 65, 130)), (3, (1, 65, 130)), (8, (64, 65))], ids=["1car", "3cars", "8cars"])
def test_update_scripted_thresholds_laps_and_termination(harness, tmp_path, oracle, nc, Bs):
    """every scripted slot (update_scripts) at every batch size, some slots dead from the start; after every step against bookkeeping_ref"""
    tk, blim = LC.default_track(), float(LC.car_params()[17])
    scripts = LC.update_scripts(nc, NS, tk, blim)
    env = LC.car_env(nc)
    Ls = [LC.loop_launch(env, scripts, [(5 * b + 1) % len(scripts) for b in range(B)] if B > 1 else [len(scripts) - 4], NS, NS - 1, 4, alive0=_alive0(B)) for B in Bs]
    Ls.append(LC.loop_launch(env, scripts, list(range(len(scripts))), NS, NS - 1, 4))                 # every script once, whatever the cycle above picks
    res = _run(harness, tmp_path, Ls)
    cache = {}
    print()
    for L, R in zip(Ls, res):
        LC.check_loop(L, R, oracle, what="scripted", cache=cache)
    # the slot's result depends on its script alone, not on B or its position: the same script in two launches, bit for bit
    seen = {}
    for L, R in zip(Ls, res):
        S = LC.loop_shapes(L, R)
        a0 = np.ones(L["B"], dtype=np.int32) if L["alive0"] is None else L["alive0"]
        for b in range(L["B"]):
            if a0[b]:
                key = L["slot_script"][b]
                cur = (LC.bits(S["hs_log"][:, b]), S["alive_log"][:, b], LC.bits(S["tr_dist"][b]), LC.bits(S["tr_beta"][b]))
                if key in seen:
                    assert all(np.array_equal(p, q) for p, q in zip(seen[key], cur)), (L["B"], b, key)
                seen[key] = cur
    assert len(seen) == len(scripts)


def test_update_laps_zero_ends_every_slot_at_step_zero(harness, tmp_path, oracle):
    tk, blim = LC.default_track(), float(LC.car_params()[17])
    scripts = LC.update_scripts(3, NS, tk, blim)
    L = LC.loop_launch(LC.car_env(3), scripts, [b % len(scripts) for b in range(65)], 3, 5, 0)
    R = _run(harness, tmp_path, [L])[0]
    LC.check_loop(L, R, oracle, what="laps 0")
    S = LC.loop_shapes(L, R)
    assert not S["alive_log"].any() and np.all(S["hs_log"][:, :, LC.H_CNT] == 1.0)


def test_update_slot_env_uses_the_slots_own_blim_and_track(harness, tmp_path, oracle):
    """per-slot car parameters (blim 0.3 / 0.5 / 0.7) and per-slot tracks of different P: each slot's centre-line point is off every other slot's road"""
    tracks = [LC.default_track(), LC.resampled_track(100, (1000.0, 0.0)), LC.resampled_track(31, (0.0, -2000.0), 9.0)]
    blims = [0.3, 0.5, 0.7]
    scripts, pick = [], []
    for v in range(3):
        sc = LC.update_scripts(1, NS, tracks[v], blims[v])
        for name in ("beta_edge", "rew_4000", "crash_11", "trk_11"):
            pick.append(len(scripts) + [s["name"] for s in sc].index(name))
        scripts += sc
    B = len(pick)
    env = LC.car_env(1, slot_params=np.stack([LC.car_params(blims[b // 4]) for b in range(B)]), slot_tracks=[tracks[b // 4] for b in range(B)])
    L = LC.loop_launch(env, scripts, pick, NS, NS - 1, 4)
    R = _run(harness, tmp_path, [L])[0]
    print()
    LC.check_loop(L, R, oracle, what="slot env")
    S = LC.loop_shapes(L, R)
    assert list(S["hs"][:, LC.H_TRK]) == [0, 1, 2, 11] * 3 and list(S["hs"][:, LC.H_BETA]) == [1, 0, 2, 0] * 3
    for b in (4, 8):                                                          # on its own road, off the shared one
        assert not oracle.within_track(tracks[0], L["xs"][5, b, :2])[0] and oracle.within_track(tracks[b // 4], L["xs"][5, b, :2])[0]


@pytest.mark.parametrize("kind", [LC.ENV_MC, LC.ENV_CP], ids=["mountaincar", "cartpole"])
def test_update_simple_envs(harness, tmp_path, oracle, kind):
    """done_env ends the slot; no car statistics are written; the trace writes within = 1 and no dist / beta; noise given: absent"""
    env = LC.simple_env(kind)
    nS, ss = 11, LC.state_size(env)
    rng = np.random.default_rng(kind + 1)
    scripts = []
    for i, end in enumerate((0, 3, 9, 10, None)):
        dn = np.zeros(nS, dtype=np.int32)
        if end is not None:
            dn[end:] = 1
        scripts.append(dict(name="done_%s" % end, nc=0, xs=rng.normal(size=(nS, ss)), rew=rng.normal(size=nS) - 1, iters=rng.integers(1, 9, nS).astype(np.int32), done=dn, notes={}))
    Ls = [LC.loop_launch(env, scripts, [b % 5 for b in range(B)], nS, nS - 1, 2, alive0=_alive0(B), noise=nz, seeds=None if nz is None else np.arange(B, dtype=np.uint64) + 5)
          for B, nz in ((65, None), (5, LC.NOISE_SIG))]
    # the trace's strided copy (k_trace_start, k_trace_step: `i += 64`) beyond one wave: the same scripts with states of 65 and 130 entries
    for wide in (64, 65, 130):
        ws = [dict(sc, xs=rng.normal(size=(nS, wide))) for sc in scripts]
        Ls.append(LC.loop_launch(LC.simple_env(kind, ss=wide), ws, [b % 5 for b in range(7)], nS, nS - 1, 2, alive0=_alive0(7), query=False))
    print()
    for L, R in zip(Ls, _run(harness, tmp_path, Ls)):
        LC.check_loop(L, R, oracle, what="simple")
        S = LC.loop_shapes(L, R)
        assert [int(S["hs"][b, LC.H_CNT]) for b in (0, 1, 2, 4)] == [1, 4, 10, 11] and S["hs"][3, LC.H_CNT] == 0        # (slot 3 is dead from the start)


def test_state_noise(harness, tmp_path, oracle):
    """one car: x, y, psi within 2 ulp of the long-double result, the rotated velocity within rot_bound, bit-identical across B and slot position (keyed by
    seed and step, not by the launch); three cars and noise sigmas given: absent"""
    nS = 6
    sc = LC.noise_scripts(nS)
    seeds3 = np.array([0x1234567890ABCDEF, 7, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    env = LC.car_env(1)
    def launch(B, off):
        pick = [(b + off) % 3 for b in range(B)]
        return LC.loop_launch(env, sc, pick, nS, nS - 1, 4, noise=LC.NOISE_SIG, seeds=seeds3[pick], actlog=False)
    Ls = [launch(1, 0), launch(65, 0), launch(130, 1)]
    tk, blim = LC.default_track(), float(LC.car_params()[17])
    sc3 = LC.update_scripts(3, NS, tk, blim)
    Ls.append(LC.loop_launch(LC.car_env(3), sc3, [0, 1, 2], nS, nS - 1, 4, noise=LC.NOISE_SIG, seeds=seeds3))
    res = _run(harness, tmp_path, Ls)
    print()
    for L, R in zip(Ls, res):
        LC.check_loop(L, R, oracle, what="noise")
    X = [LC.loop_shapes(L, R)["x_log"] for L, R in zip(Ls[:3], res[:3])]
    for b in range(65):
        assert np.array_equal(LC.bits(X[1][:, b]), LC.bits(X[1][:, b % 3])), b
    for b in range(130):
        assert np.array_equal(LC.bits(X[2][:, b]), LC.bits(X[1][:, (b + 1) % 3])), b
    assert np.array_equal(LC.bits(X[0][:, 0]), LC.bits(X[1][:, 0]))
    w = LC.noise_worst()
    print("[noise] worst position / psi error %.2f ulp (bound 2), rotated velocity %.3f of its bound" % (w["pos_ulp"], w["rot_ratio"]))
    assert w["pos_ulp"] <= 2.0 and w["rot_ratio"] <= 1.0


@pytest.mark.parametrize("nc", [1, 3])
def test_true_sequence_env_step_then_update(harness, tmp_path, oracle, nc):
    """launch_env_step with scripted actions in front of the update, as mpopis_run_trials enqueues them: the states against the oracle's env at 1e-10 per
    step, the bookkeeping on the states and rewards the device produced, the step counter t == cnt"""
    B, nS = 3, 5
    env = LC.car_env(nc)
    x0, _ = LC.parity_states(nc, B, 50 + nc)
    rng = np.random.default_rng(nc)
    L = dict(op=LC.OP_LOOP, B=B, env=env, nS=nS, num_steps=4, laps=4, K=5, noise=None, env_step=True, actlog=True, mask=63, query=True, x0=x0, xs=None, reward=None,
             iters=rng.integers(1, 5, (nS, B)).astype(np.int32), done_env=None, control=rng.uniform(-1, 1, (nS, B, 2 * nc)), seeds=None, alive0=None)
    R = _run(harness, tmp_path, [L])[0]
    S = LC.loop_shapes(L, R)
    worst = 0.0
    for b in range(B):
        x = x0[b]
        for s in range(L["nS"]):
            x = np.concatenate([oracle.car_step(env["params"], x[8 * c:8 * c + 8], L["control"][s, b].reshape(nc, 2)[c]) for c in range(nc)])
            e = LC.rel(S["x_log"][s, b], x)
            assert e <= 1e-10 * (s + 1), (b, s, e)
            worst = max(worst, e)
            x = S["x_log"][s, b]
    assert np.all(S["t"] == L["nS"]) and np.all(S["status"] == 0)
    L.update(xs=S["x_log"], reward=S["reward_log"], done_env=np.zeros((nS, B), dtype=np.int32), scripts=[dict(name="env step %d" % b) for b in range(B)], slot_script=list(range(B)))
    print()
    LC.check_loop(L, R, oracle, what="true sequence (state dev %.1e)" % worst)
    assert not S["alive"].any() and np.all(S["hs"][:, LC.H_CNT] == 5.0)       # dead at cnt == num_steps + 1


def test_trace_null_subsets(harness, tmp_path, oracle):
    """every subset of the six trace outputs given / null: what is given is written as before, nothing else is"""
    tk, blim = LC.default_track(), float(LC.car_params()[17])
    scripts = LC.update_scripts(3, NS, tk, blim)
    Ls = [LC.loop_launch(LC.car_env(3), scripts, [0, 5, 9], 13, 12, 4, mask=m, alive0=np.array([1, 1, 0], dtype=np.int32)) for m in range(64)]
    res = _run(harness, tmp_path, Ls)
    full = LC.loop_shapes(Ls[63], res[63])
    cache = {}
    for m, (L, R) in enumerate(zip(Ls, res)):
        LC.check_loop(L, R, oracle, log=lambda *a: None, cache=cache)
        S = LC.loop_shapes(L, R)
        for bit, name in enumerate(("states", "rewards", "iters", "tr_within", "tr_dist", "tr_beta")):
            if m >> bit & 1:
                assert np.array_equal(S[name].view(np.uint8), full[name].view(np.uint8)), (m, name)
            else:
                assert S[name] is None, (m, name)
        assert np.array_equal(LC.bits(S["hs_log"]), LC.bits(full["hs_log"])), m


# ================================================================ k_env_step / k_env_query ====================================================
def _slot_env(nc, B):
    tracks = [LC.default_track(), LC.resampled_track(100), LC.resampled_track(31, width=9.0), LC.resampled_track(257), LC.default_track()]
    sp = np.stack([LC.car_params(0.3 + 0.1 * b) for b in range(B)])
    sp[:, 0] *= 1 + 0.05 * np.arange(B)                                       # mass
    sp[:, 9:11] *= (1 - 0.04 * np.arange(B))[:, None]                         # friction
    return LC.car_env(nc, slot_params=sp, slot_tracks=[tracks[b % 5] for b in range(B)])


@pytest.mark.parametrize("nc", [1, 2, 3, 8])
def test_step_and_query_against_the_oracle_cars(harness, tmp_path, oracle, nc):
    B = 5
    x, act = LC.parity_states(nc, B, 10 + nc)
    t0 = np.array([0, 5, 199, 200, 1000], dtype=np.int32)
    alive = np.array([1, 1, 0, 1, 1], dtype=np.int32)
    none = dict(reward=False, within=False, dist=False, beta=False, qreward=False)
    base = LC.step_launch(LC.car_env(nc), x, act, t=t0, status=np.zeros(B, dtype=np.int32))
    Ls = [base,
          LC.step_launch(_slot_env(nc, B), x, act, t=t0, status=np.zeros(B, dtype=np.int32)),
          LC.step_launch(LC.car_env(nc), x, act, t=t0, status=np.zeros(B, dtype=np.int32), alive=np.ones(B, dtype=np.int32)),      # == alive null
          LC.step_launch(LC.car_env(nc), x, act, t=t0, status=np.zeros(B, dtype=np.int32), alive=alive),
          LC.step_launch(LC.car_env(nc), x, act, t=t0, want=none),                                                                  # every nullable pointer null
          LC.step_launch(LC.car_env(nc), x[3:4], act[3:4], t=t0[3:4], status=np.zeros(1, dtype=np.int32)),                          # slot 3 alone
          LC.step_launch(LC.car_env(nc), x[::-1], act[::-1], t=t0[::-1], status=np.zeros(B, dtype=np.int32)),                       # the batch reversed
          LC.step_launch(LC.car_env(nc), x, act, t=t0, want=dict(reward=False, within=True, dist=False, beta=True, qreward=False)),  # some null, some given
          LC.step_launch(LC.car_env(nc), x, act, t=t0, status=np.zeros(B, dtype=np.int32), want=dict(reward=True, within=False, dist=True, beta=False, qreward=True))]
    res = _run(harness, tmp_path, Ls)
    print()
    for i, (L, R) in enumerate(zip(Ls, res)):
        LC.check_step(oracle, L, R, what="launch %d" % i)
    S = [LC.step_shapes(L, R) for L, R in zip(Ls, res)]
    for k in ("x", "t", "done", "reward", "status", "qreward", "within", "dist", "beta"):
        assert np.array_equal(S[0][k].view(np.uint8), S[2][k].view(np.uint8)), k                      # alive null == all ones
        assert np.array_equal(S[0][k][3:4].view(np.uint8), S[5][k].view(np.uint8)), k                  # no dependence on B
        assert np.array_equal(np.ascontiguousarray(S[0][k][::-1]).view(np.uint8), S[6][k].view(np.uint8)), k                 # ... or on the position in the batch
        for b in (0, 1, 3, 4):
            if k not in ("reward", "status"):
                assert np.array_equal(S[0][k][b:b + 1].view(np.uint8), S[3][k][b:b + 1].view(np.uint8)), (k, b)
    for k in ("x", "t", "done"):
        assert np.array_equal(S[0][k].view(np.uint8), S[4][k].view(np.uint8)), k                      # null outputs change nothing else
    assert all(S[4][k] is None for k in ("reward", "status", "qreward", "within", "dist", "beta"))
    for i in (7, 8):
        for k in ("x", "t", "done", "reward", "qreward", "within", "dist", "beta"):
            assert S[i][k] is None or np.array_equal(S[0][k].view(np.uint8), S[i][k].view(np.uint8)), (i, k)
    assert S[7]["reward"] is None and S[7]["dist"] is None and S[7]["within"] is not None and S[8]["within"] is None and S[8]["dist"] is not None
    assert S[0]["within"][1] == 0 and (nc > 3 or S[0]["within"][0] == 1)                                         # slot 1 is off the road
    assert not np.array_equal(LC.bits(S[0]["x"]), LC.bits(S[1]["x"]))                                  # the slot parameters are used


@pytest.mark.parametrize("kind", [LC.ENV_MC, LC.ENV_CP], ids=["mountaincar", "cartpole"])
def test_step_and_query_against_the_oracle_simple_envs(harness, tmp_path, oracle, kind):
    env = LC.simple_env(kind)
    B = 6
    rng = np.random.default_rng(kind)
    if kind == LC.ENV_MC:
        x = np.stack([[-0.5, 0.0], [0.44, 0.069], [-1.19, -0.06], [0.5, 0.01], [-0.3, 0.02], [0.0, -0.07]])
    else:
        x = rng.uniform(-0.05, 0.05, (B, 4)); x[1, 0] = 2.39; x[1, 1] = 2.0; x[2, 2] = 0.2; x[2, 3] = 1.0
    t0 = np.array([0, 5, 198, 199, 200, 7], dtype=np.int32)
    act = np.array([[0.3], [1.0], [-1.0], [0.0], [-0.7], [0.9]])
    Ls = [LC.step_launch(env, x, act, t=t0, status=np.zeros(B, dtype=np.int32)),
          LC.step_launch(env, x, act, t=t0, status=np.zeros(B, dtype=np.int32), alive=np.array([1, 0, 1, 1, 0, 1], dtype=np.int32)),
          LC.step_launch(env, x, act, t=t0, want=dict(reward=False, within=False, dist=False, beta=False, qreward=False))]
    res = _run(harness, tmp_path, Ls)
    print()
    for i, (L, R) in enumerate(zip(Ls, res)):
        LC.check_step(oracle, L, R, what="launch %d" % i)
    S = [LC.step_shapes(L, R) for L, R in zip(Ls, res)]
    assert np.array_equal(S[0]["t"], t0 + 1)                                                           # t advances by one for every env kind
    assert S[0]["done"].any() and not S[0]["done"].all()
    assert np.array_equal(LC.bits(S[0]["x"]), LC.bits(S[2]["x"])) and np.array_equal(S[0]["done"], S[2]["done"])


def test_step_pair_term_edges(harness, tmp_path, oracle):
    q, st = LC.pair_edge_launches()
    Rq, Rs = _run(harness, tmp_path, [q, st])
    print()
    LC.check_step(oracle, q, Rq, what="pair edges, query")
    LC.check_step(oracle, st, Rs, what="pair edges, step")
    Sq, Ss = LC.step_shapes(q, Rq), LC.step_shapes(st, Rs)
    assert Sq["qreward"][0] < Sq["qreward"][1] - 10999.0 and Ss["reward"][0] < Ss["reward"][1] - 10999.0      # 4.0 is contact, the next double is not
    for b, contact in enumerate(st["contact"]):
        assert (LC.pair_terms(Ss["x"][b], 2)[0] <= 4.0) == contact, b
    assert LC.pair_terms(Ss["x"][0], 2)[0] == 4.0


@pytest.mark.parametrize("envname", ["car1", "car3", "mountaincar", "cartpole"])
def test_step_action_check_and_status_precedence(harness, tmp_path, oracle, envname):
    """a == lo and a == hi pass; the neighbouring doubles outside, NaN and +-inf raise MPOPIS_ERR_ACTION (one car, simple envs; several cars: no check); a slot
    that enters with NOT_PD or NUMERIC leaves with ACTION, one that enters with HIP keeps it"""
    if envname in ("car1", "car3"):
        nc = int(envname[3:])
        lo, hi = np.tile([-0.5, -0.75], nc), np.tile([0.25, 1.0], nc)
        env = LC.car_env(nc, lo=lo, hi=hi)
    else:
        nc = 0
        env = LC.simple_env(LC.ENV_MC if envname == "mountaincar" else LC.ENV_CP)
        lo, hi = env["lo"], env["hi"]
    na = len(lo)
    acts, names = [], []
    mid = 0.5 * (lo + hi)
    for i in range(min(na, 2)):
        for name, v in (("lo", lo[i]), ("hi", hi[i]), ("below lo", np.nextafter(lo[i], -np.inf)), ("above hi", np.nextafter(hi[i], np.inf)), ("nan", np.nan), ("+inf", np.inf),
                        ("-inf", -np.inf)):
            a = mid.copy(); a[i] = v
            acts.append(a); names.append("a[%d] = %s" % (i, name))
    acts, B0 = np.array(acts), len(acts)
    before = np.array([0, LC.ERR_NOT_PD, LC.ERR_NUMERIC, LC.ERR_HIP], dtype=np.int32)
    act = np.concatenate([acts] * 4)
    status = np.repeat(before, B0)
    B = len(act)
    x = LC.parity_states(max(nc, 1), B, 3)[0] if nc else np.tile(np.array([-0.5, 0.0] if envname == "mountaincar" else [0.01, 0.0, 0.02, 0.0]), (B, 1))
    L = LC.step_launch(env, x, act, status=status)
    R = _run(harness, tmp_path, [L])[0]
    print()
    LC.check_step(oracle, L, R, what=envname)
    S = LC.step_shapes(L, R)
    raised = np.array([not LC.in_bounds(L, b) for b in range(B)])
    assert raised[:B0].sum() == 5 * min(na, 2)
    if nc > 1:
        assert np.array_equal(S["status"], status)
    else:
        assert np.array_equal(S["status"], np.where(raised & (status != LC.ERR_HIP), LC.ERR_ACTION, status))
    assert np.all(S["t"] == 1)


# ================================================================ k_plan_* ====================================================================
def test_plan_select_and_assemble(harness, tmp_path):
    rng = np.random.default_rng(2)
    Ls, unsafe = [], []
    for K in LC.PLAN_K:
        rows = LC.weight_rows(K, rng)
        bad = LC.unsafe_rows(K, rng)
        for top in LC.plan_tops(K):
            act = None if top != 2 else np.array([1, 0] * (len(rows) // 2) + [1] * (len(rows) % 2), dtype=np.int32)
            Ls.append(LC.plan_launch(K, top, 3, list(rows.values()), K * 100 + top, active=act)); unsafe.append(False)
            Ls.append(LC.plan_launch(K, top, 2, list(bad.values()), K * 100 + top + 1)); unsafe.append(True)
    for cs, top in ((127, 1), (128, 1), (129, 1), (255, 1), (256, 1), (257, 1), (3, 64), (4, 64), (7, 64), (8, 64)):      # cs (top + 1) on both sides of 256 and of 512
        Ls.append(LC.plan_launch(65, top, cs, [rng.random(65), np.full(65, 0.5)], cs, active=None if cs % 2 else np.array([1, 0], dtype=np.int32))); unsafe.append(False)
    res = _run(harness, tmp_path, Ls)
    for L, R, u in zip(Ls, res, unsafe):
        LC.check_plan(L, R, safety_only=u)
    sizes = sorted({L["cs"] * (L["top"] + 1) for L in Ls})
    assert any(s < 256 for s in sizes) and any(256 < s < 512 for s in sizes) and any(s > 512 for s in sizes) and 256 in sizes and 512 in sizes


# ================================================================ k_trace_reorder ==============================================================
def test_trace_reorder_is_the_transpose(harness, tmp_path):
    Ls = LC.reorder_launches()
    assert len(Ls) == 5 * 3 * 3 * 2
    for L, R in zip(Ls, _run(harness, tmp_path, Ls)):
        LC.check_reorder(L, R)
