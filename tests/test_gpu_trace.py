"""mpopis_run_trials_traced / Engine.run_trials(trace=...): the resident closed loop that also records each MPC step's
driven state, reward, iteration count, lane / β read-out and, every plan_every steps, the plan of mpopis_get_plan.

What is compared.  The expected trace is a host loop on a SECOND handle with the same seed -- per MPC step policy_step(None), get_plan(top),
get_state, env_step, env_query -- which tests/test_gpu_nes.py::test_closed_loop_run_trials_matches_host_loop shows to drive the same bits as the
device loop (device Philox keyed by the MPC step) and which runs none of the code under test.  Every comparison is np.array_equal: slot b up to
steps_run[b] = records[b][1] + 1, and zeros beyond.  The host loop steps every slot at every step; a slot's entries past its own end are simply
not looked at (the slots are independent).  Only the state-noise case has no host twin (the noise is drawn on the device): there the step fields
are checked against env_step / env_query of fresh handles and the plans against the oracle, to the 1e-8 of tests/test_gpu_parity.py.
Shapes follow tests/test_gpu_persistent_chains.py (K = 128, T = 10, N = 3)."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from tests.test_gpu_baseline_shapes import start_states
from tests.helpers import slot_env_cases as SC
from tests.helpers import pointmass_ref as PM

pytestmark = pytest.mark.gpu

K, T, N = 128, 10, 3
RTOL = 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_FIELDS = ("rewards", "iters", "within", "dist", "beta")
PLAN_FIELDS = ("plan_controls", "plan_traj", "plan_cost", "plan_idx0", "plan_weights")
PLAN_OF = dict(plan_controls="controls", plan_traj="traj", plan_cost="cost", plan_idx0="idx0", plan_weights="weights")


@pytest.fixture(scope="module")
def eng_mod():
    from mpopis_amd import build
    build.build()
    from mpopis_amd import engine
    return engine


def car(eng_mod, track, B, kind="musigmaaismppi", nc=1, Kc=K, cov=(0.0625, 0.1), overlap=4, x0=None, seed=777):
    eng = eng_mod.Engine("car", nc, kind, Kc, T, batch=B, lam=10.0, ais_its=N, lam_ais=20.0, elite_threshold=0.8, cov=list(np.tile(cov, nc)), track=track, seed=seed)
    eng.set_overlap(overlap)
    if x0 is not None:
        eng.set_state(x0)
    return eng


def host_loop(eng, num_steps, top, plan_every=1):
    """The alternative the feature replaces: five host round trips per MPC step.  Returns the trace it yields, every slot stepped S times."""
    B, S = eng.B, num_steps + 1
    nc = max(1, eng.as_ // 2) if eng.env_kind == "car" else 1
    ref = dict(states=np.zeros((B, S + 1, eng.ss)), rewards=np.zeros((B, S)), iters=np.zeros((B, S), dtype=np.int32), within=np.zeros((B, S), dtype=bool),
               dist=np.zeros((B, S, nc)), beta=np.zeros((B, S, nc)), actions=np.zeros((B, S, eng.as_)), plans={})
    for s in range(S):
        g = eng.policy_step(None, minimal=True)
        if plan_every and s % plan_every == 0:
            ref["plans"][s] = eng.get_plan(top)
        ref["states"][:, s] = eng.get_state()[0]
        ref["iters"][:, s], ref["actions"][:, s] = g["iters_run"], g["control"]
        ref["rewards"][:, s] = eng.env_step(g["control"])
        _, ref["within"][:, s], ref["dist"][:, s], ref["beta"][:, s] = eng.env_query()
    ref["states"][:, S] = eng.get_state()[0]
    return ref


def check_steps(tr, ref, label=""):
    n_run = tr["steps_run"]
    for b in range(len(n_run)):
        n = int(n_run[b])
        if "states" in tr:
            assert np.array_equal(tr["states"][b, :n + 1], ref["states"][b, :n + 1]), (label, "states", b)
            assert np.all(tr["states"][b, n + 1:] == 0), (label, "states past the end", b)
        for f in STEP_FIELDS:
            if f in tr:
                assert tr[f].dtype == ref[f].dtype and tr[f].shape == ref[f].shape, (label, f)
                assert np.array_equal(tr[f][b, :n], ref[f][b, :n]), (label, f, b, tr[f][b, :n], ref[f][b, :n])
                assert np.all(tr[f][b, n:] == 0), (label, f, "past the end", b)


def check_plans(tr, ref, top, label=""):
    """entry j of every recorded plan field against get_plan of the host loop at step plan_steps[j] (a reference taken with a larger top holds
    the smaller one's answer in its leading entries: the order is total)"""
    n_run = tr["steps_run"]
    for b in range(len(n_run)):
        for j, s in enumerate(tr["plan_steps"]):
            p = ref["plans"][int(s)]
            for f in PLAN_FIELDS:
                if f not in tr:
                    continue
                got = tr[f][b, j]
                if s >= n_run[b]:
                    assert np.all(got == 0), (label, f, "plan past the end", b, j)
                    continue
                want = p[PLAN_OF[f]][b]
                want = want if f == "plan_controls" else want[:top + 1] if f in ("plan_traj", "plan_cost") else want[:top]
                assert got.shape == want.shape and got.dtype == want.dtype, (label, f, got.shape, want.shape)
                assert np.array_equal(got, want), (label, f, b, j)


# ---- 1. core --------------------------------------------------------------------------------------------------------------------------------------

CORE = dict(B=5, num_steps=14, laps=2, top=3)


@pytest.fixture(scope="module")
def core(eng_mod, oracle, track):
    """B = 5 (parts 2 / 1 / 1 / 1), 15 MPC steps (the host looks at steps 7 and 14): the untraced run and the host loop's trace, shared by the tests below"""
    B, ns = CORE["B"], CORE["num_steps"]
    x0 = start_states(oracle, track, 1, B)
    eng = car(eng_mod, track, B, x0=x0)
    rec, acts = eng.run_trials(num_steps=ns, laps=CORE["laps"], log_actions=True)
    eng.close()
    eng = car(eng_mod, track, B, x0=x0)
    ref = host_loop(eng, ns, CORE["top"])
    eng.close()
    return types.SimpleNamespace(x0=x0, rec=rec, acts=acts, ref=ref)


def traced(eng_mod, track, core, overlap=4, **trace):
    eng = car(eng_mod, track, CORE["B"], overlap=overlap, x0=core.x0)
    out = eng.run_trials(num_steps=CORE["num_steps"], laps=CORE["laps"], log_actions=True, trace=trace or True)
    eng.close()
    return out


def test_core_every_field_equals_the_host_loop(eng_mod, track, core):
    ns, top = CORE["num_steps"], CORE["top"]
    outs = [traced(eng_mod, track, core, overlap=ov, plan_every=1, top=top) for ov in (4, 1)]
    rec, acts, tr = outs[0]
    assert np.array_equal(rec, core.rec) and np.array_equal(acts, core.acts)                # the bits of the untraced call
    assert np.all(rec[:, 15] == 0)
    assert np.array_equal(tr["steps_run"], rec[:, 1].astype(np.int64) + 1) and np.array_equal(tr["plan_steps"], np.arange(ns + 1))
    print("\n[trace] core: steps per slot %s" % tr["steps_run"])
    early = np.where(tr["steps_run"] < ns + 1)[0]
    assert len(early) > 0 and np.max(tr["steps_run"]) == ns + 1                            # a slot ends early, others run to the end
    assert tr["states"].shape == (CORE["B"], ns + 2, 8) and tr["plan_traj"].shape == (CORE["B"], ns + 1, top + 1, T, 8)
    for b in range(CORE["B"]):
        n = int(tr["steps_run"][b])
        assert np.array_equal(acts[b, :n], core.ref["actions"][b, :n])                       # (the premise: the host loop drives the same bits)
    check_steps(tr, core.ref, "core")
    check_plans(tr, core.ref, top, "core")
    assert np.array_equal(rec[:, 0], np.cumsum(tr["rewards"], axis=1)[:, -1])              # records[0] is the sum of these terms, in this order
    assert not np.array_equal(tr["plan_traj"][0, 0], tr["plan_traj"][0, 1]) and not np.array_equal(tr["plan_traj"][0, 0], tr["plan_traj"][1, 0])
    rec1, acts1, tr1 = outs[1]                                                              # one stream: the same bits in every field
    assert np.array_equal(rec1, rec) and np.array_equal(acts1, acts) and sorted(tr1) == sorted(tr)
    for f in tr:
        assert np.array_equal(tr1[f], tr[f]), f


# ---- 2. plan_every, top, single fields ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plan_every,top", [(3, 3), (CORE["num_steps"] + 1, 2), (1, 0), (CORE["num_steps"], 1)])
def test_plan_every_and_top(eng_mod, track, core, plan_every, top):
    from mpopis_amd.engine import trace_plan_steps
    rec, acts, tr = traced(eng_mod, track, core, plan_every=plan_every, top=top)
    assert np.array_equal(rec, core.rec) and np.array_equal(acts, core.acts)
    steps = trace_plan_steps(CORE["num_steps"], plan_every)
    assert np.array_equal(tr["plan_steps"], steps) and tr["plan_cost"].shape == (CORE["B"], len(steps), top + 1)
    assert tr["plan_idx0"].shape == (CORE["B"], len(steps), top) and tr["plan_traj"].shape == (CORE["B"], len(steps), top + 1, T, 8)
    check_steps(tr, core.ref, "every %d top %d" % (plan_every, top))
    check_plans(tr, core.ref, top, "every %d top %d" % (plan_every, top))


def test_step_fields_only(eng_mod, track, core):
    rec, acts, tr = traced(eng_mod, track, core)                                            # trace=True: plan_every = 0
    assert np.array_equal(rec, core.rec) and np.array_equal(acts, core.acts)
    assert sorted(tr) == sorted(("states",) + STEP_FIELDS + ("steps_run", "plan_steps")) and len(tr["plan_steps"]) == 0
    check_steps(tr, core.ref, "steps only")


@pytest.mark.parametrize("field", ["states", "rewards", "within", "beta", "plan_controls", "plan_cost", "plan_idx0", "plan_traj"])
def test_one_pointer_alone(eng_mod, track, core, field):
    plan = field.startswith("plan_")
    rec, acts, tr = traced(eng_mod, track, core, plan_every=2 if plan else 0, top=2 if plan else 0, fields=[field])
    assert np.array_equal(rec, core.rec) and np.array_equal(acts, core.acts)
    assert sorted(tr) == sorted((field, "steps_run", "plan_steps"))
    check_steps(tr, core.ref, field)
    check_plans(tr, core.ref, 2, field)


# ---- 3. other policies ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mppi", "cemppi", "pmcmppi", "nesmppi"])
def test_other_policies(eng_mod, oracle, track, kind):
    B, ns, top = 4, 9, 3
    x0 = start_states(oracle, track, 1, B)
    Kc = 150 if kind == "cemppi" else K

    def make():
        eng = car(eng_mod, track, B, kind=kind, Kc=Kc, x0=x0, seed=31)
        if kind == "cemppi":
            # slot 1 draws from a vanishing proposal: its elite costs agree and it leaves the AIS loop in its first iteration (:458-461)
            eng.set_Sigma_slots(np.array([[0.0625, 0.1], [1e-12, 1e-12], [0.0625, 0.1], [0.0625, 0.1]]))
        return eng

    eng = make()
    rec, acts, tr = eng.run_trials(num_steps=ns, laps=2, log_actions=True, trace=dict(plan_every=2, top=top))
    eng.close()
    eng = make()
    rec0, acts0 = eng.run_trials(num_steps=ns, laps=2, log_actions=True)
    eng.close()
    eng = make()
    ref = host_loop(eng, ns, top, plan_every=2)
    eng.close()
    assert np.all(rec[:, 15] == 0) and np.array_equal(rec, rec0) and np.array_equal(acts, acts0)
    check_steps(tr, ref, kind)
    check_plans(tr, ref, top, kind)
    n1 = int(tr["steps_run"][1])
    if kind == "cemppi":
        assert n1 > 0 and np.all(tr["iters"][1, :n1] == 1) and np.max(tr["iters"][0]) > 1, tr["iters"]
    elif kind == "mppi":
        assert np.all(tr["iters"][1, :n1] == 1)


# ---- 4. other envs --------------------------------------------------------------------------------------------------------------------------------

def run_three(make, ns, laps, top, plan_every, label):
    """the traced run, the untraced run and the host loop on three handles built alike"""
    eng = make()
    rec, acts, tr = eng.run_trials(num_steps=ns, laps=laps, log_actions=True, trace=dict(plan_every=plan_every, top=top))
    eng.close()
    eng = make()
    rec0, acts0 = eng.run_trials(num_steps=ns, laps=laps, log_actions=True)
    eng.close()
    eng = make()
    ref = host_loop(eng, ns, top, plan_every=plan_every)
    eng.close()
    assert np.all(rec[:, 15] == 0) and np.array_equal(rec, rec0) and np.array_equal(acts, acts0), label
    check_steps(tr, ref, label)
    check_plans(tr, ref, top, label)
    return rec, tr, ref


def test_three_cars(eng_mod, oracle, track):
    B = 2
    x0 = start_states(oracle, track, 3, B)
    rec, tr, ref = run_three(lambda: car(eng_mod, track, B, nc=3, x0=x0, seed=41), 9, 2, 2, 3, "3 cars")
    assert tr["dist"].shape == (B, 10, 3) and tr["states"].shape == (B, 11, 24)
    assert len({tr["beta"][1, 0, c] for c in range(3)}) == 3


def test_per_slot_tracks_params_and_lambda(eng_mod, oracle, track):
    B = 4
    tracks, tos, params = SC.tracks3(track), SC.TRACK_OF_SLOT, SC.car_params4(oracle)
    x0 = np.stack([SC.start_state(tracks[tos[b]], 1, b) for b in range(B)])

    def make():
        eng = car(eng_mod, None, B, seed=51)
        eng.set_tracks(tracks, tos)
        eng.set_env_params_slots(params)
        eng.set_slot_hyper(lam=[10.0, 1.0, 50.0, 5.0])
        eng.set_state(x0)
        return eng

    rec, tr, ref = run_three(make, 9, 2, 2, 2, "per slot")
    # the slot's own track decided its distances: slots 0 and 2 (track 2) start beside DIFFERENT points of the same track, slot 1 on another
    n = tr["steps_run"]
    assert np.all(n >= 1) and len({tr["dist"][b, 0, 0] for b in range(B)}) == B


@pytest.mark.parametrize("kind", ["mountaincar", "cartpole"])
def test_simple_envs(eng_mod, kind):
    B = 3
    x0 = np.array([[-0.5, 0.0], [-0.45, 0.01], [-0.55, -0.01]]) if kind == "mountaincar" else \
        np.array([[0.01, -0.02, 0.03, 0.01], [-0.03, 0.04, -0.02, 0.02], [0.02, 0.0, 0.05, 0.1]])

    def make():
        eng = eng_mod.Engine(kind, 0, "musigmaaismppi", K, 15, batch=B, lam=0.1, ais_its=N, lam_ais=0.1, cov=[1.5], seed=61)
        eng.set_state(x0, t=[0, 195, 0])                               # slot 1 runs into max_steps = 200 (t >= 200 / t > 200): env.done ends its trial
        return eng

    rec, tr, ref = run_three(make, 9, 0, 2, 2, kind)
    n = tr["steps_run"]
    assert n[1] == (5 if kind == "mountaincar" else 6) and n[0] > 6, n
    assert np.all(tr["within"][0, :n[0]]) and np.all(tr["dist"] == 0) and np.all(tr["beta"] == 0)
    assert tr["plan_traj"].shape == (B, 5, 3, 15, 2 if kind == "mountaincar" else 4)
    if kind == "cartpole":
        print("\n[trace] cartpole steps per slot %s" % n)


def test_custom_env(eng_mod):
    from mpopis_amd import build
    env = types.SimpleNamespace(code_object=build.build_env(os.path.join(ROOT, "tests", "helpers", "envs", "pointmass_sdk.hip")), state_size=PM.SS,
                                action_size=PM.AS, params=np.array(PM.PARAMS, dtype=np.float64), lo=PM.LO, hi=PM.HI, reset_state=None)
    B = 3
    x0 = np.random.default_rng(8).uniform(-0.5, 0.5, (B, PM.SS))

    def make():
        eng = eng_mod.Engine("custom", 0, "musigmaaismppi", K, 6, batch=B, lam=1.0, ais_its=N, lam_ais=1.0, cov=[0.3, 0.3, 0.1], custom_env=env, seed=71)
        eng.set_state(x0)
        return eng

    rec, tr, ref = run_three(make, 9, 0, 2, 3, "pointmass")
    assert np.all(tr["steps_run"] == 10) and np.all(tr["within"]) and tr["states"].shape == (B, 11, PM.SS)
    # the NumPy restatement of the env, one step from each recorded state (rounding only: tests/helpers/pointmass_ref.py)
    eng = make()
    acts = eng.run_trials(num_steps=9, laps=0, log_actions=True)[1]
    eng.close()
    for s in range(10):
        nxt, _, _ = PM.step(tr["states"][:, s], s, np.clip(acts[:, s], PM.LO, PM.HI))
        assert np.allclose(nxt, tr["states"][:, s + 1], rtol=1e-12, atol=1e-14)
        assert np.allclose(PM.reward(tr["states"][:, s + 1]), tr["rewards"][:, s], rtol=1e-12, atol=1e-14)


# ---- 5. state noise -------------------------------------------------------------------------------------------------------------------------------

def test_state_noise(eng_mod, oracle, track):
    B, ns, top = 2, 5, 2
    x0 = np.stack([SC.start_state(track, 1, b) for b in range(B)])

    def make(noise=True):
        eng = car(eng_mod, track, B, x0=x0, seed=81)
        if noise:
            eng.set_state_noise(0.05, 0.05, 0.01)
        return eng

    eng = make()
    rec, acts, tr = eng.run_trials(num_steps=ns, laps=2, log_actions=True, trace=dict(plan_every=1, top=top))
    eng.close()
    eng = make()
    rec0, acts0 = eng.run_trials(num_steps=ns, laps=2, log_actions=True)
    eng.close()
    assert np.all(rec[:, 15] == 0) and np.array_equal(rec, rec0) and np.array_equal(acts, acts0)
    n_run = tr["steps_run"]
    assert np.all(n_run == ns + 1)
    assert np.array_equal(tr["states"][:, 0], x0)
    fresh = make(noise=False)
    moved = np.zeros(8, dtype=bool)
    for s in range(ns + 1):
        fresh.set_state(tr["states"][:, s])
        rew = fresh.env_step(acts[:, s])
        x_free = fresh.get_state()[0]
        assert np.array_equal(rew, tr["rewards"][:, s])                                      # reward(env) is taken before the noise (car_example.jl:210-236)
        assert np.array_equal(x_free[:, 5:], tr["states"][:, s + 1, 5:])                    # r, δ, pedal: untouched by the noise
        moved |= np.any(x_free != tr["states"][:, s + 1], axis=0)
        fresh.set_state(tr["states"][:, s + 1])
        _, win, dist, beta = fresh.env_query()
        assert np.array_equal(win, tr["within"][:, s]) and np.array_equal(dist, tr["dist"][:, s]) and np.array_equal(beta, tr["beta"][:, s])
    assert np.array_equal(moved, [True] * 5 + [False] * 3), moved
    fresh.close()
    for b in range(B):
        for s in range(ns + 1):
            env = oracle.OracleEnv("car", 1, track=track)
            env.state = tr["states"][b, s]
            pol = oracle.OraclePolicy("gmppi", env, 1, T, lam=1.0, U0=np.zeros(2), cov=np.ones(2))
            cref, tref = pol.simulate_model(np.zeros(2 * T), tr["plan_controls"][b, s][:, None], log=True)
            assert SC.min_logged_vx(tref, 1) > 1.0
            et, ec = SC.rel_err(tr["plan_traj"][b, s, 0], tref[0]), SC.rel_err(tr["plan_cost"][b, s, 0], cref[0])
            print("[trace] noise slot %d step %d: traj %.2e cost %.2e" % (b, s, et, ec))
            assert et < RTOL and ec < RTOL, (b, s, et, ec)
            assert np.array_equal(acts[b, s], np.clip(tr["plan_controls"][b, s, :2], -1.0, 1.0))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_as_it_was(eng_mod, oracle, track):
    from mpopis_amd import _lib
    from mpopis_amd._lib import MPOPISError, ERR_ARG
    B, ns = 2, 3
    x0 = start_states(oracle, track, 1, B)
    eng = car(eng_mod, track, B, x0=x0, seed=91)
    rec = np.zeros((B, _lib.RECORD_LEN))
    buf = np.zeros(B * (ns + 1) * 4 * T * 8)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))

    def refused(word, laps=2, **fields):
        tr = _lib.Trace()
        for k, v in fields.items():
            setattr(tr, k, v)
        assert eng.L.mpopis_run_trials_traced(eng._h, ns, laps, rec.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(tr)) == ERR_ARG
        msg = eng.L.mpopis_last_error(eng._h).decode()
        assert word in msg, msg

    refused("plan_every must be >= 0", plan_every=-1)
    for top in (K + 1, 65, -1):
        refused("top must be 0..64", plan_every=1, top=top)
    refused("top > 0 needs plan_every > 0", plan_every=0, top=1)
    for f in PLAN_FIELDS:
        refused("a plan array needs plan_every > 0", **{f: buf.ctypes.data_as(C.POINTER(C.c_int32)) if f == "plan_idx0" else dp})
    refused("laps", laps=5, states=dp)                                                       # what mpopis_run_trials refuses
    assert eng.L.mpopis_run_trials_traced(eng._h, ns, 2, None, None, None) == ERR_ARG
    assert eng.L.mpopis_run_trials_traced(None, ns, 2, None, None, None) == ERR_ARG
    # Python refuses top and plan_every before the library is reached
    for bad in (dict(plan_every=-1), dict(plan_every=1, top=K + 1), dict(plan_every=1, top=-1), dict(top=1), dict(fields=["plan_cost"]), dict(every=1),
                dict(fields=["speed"])):
        with pytest.raises(MPOPISError) as ei:
            eng.run_trials(num_steps=ns, laps=2, trace=bad)
        assert ei.value.code == ERR_ARG
    assert np.array_equal(eng.get_state()[0], x0)                                            # nothing ran
    # ... and the handle is as it was: its traced run is that of a handle that was never refused; NULL trace is mpopis_run_trials
    rec_a, tr_a = eng.run_trials(num_steps=ns, laps=2, trace=dict(plan_every=1, top=2))
    eng.set_state(x0)
    eng.policy_step(None, minimal=True)
    assert np.all(np.isfinite(eng.get_plan(1)["traj"]))
    eng.run_trials(num_steps=1, laps=2, trace=True)                                          # a traced run ends the source of get_plan, like an untraced one
    with pytest.raises(MPOPISError) as ei:
        eng.get_plan(1)
    assert ei.value.code == ERR_ARG and "mpopis_run_trials_traced" in str(ei.value), str(ei.value)
    eng.close()
    eng = car(eng_mod, track, B, x0=x0, seed=91)
    rec_b, tr_b = eng.run_trials(num_steps=ns, laps=2, trace=dict(plan_every=1, top=2))
    eng.close()
    assert np.array_equal(rec_a, rec_b) and all(np.array_equal(tr_a[f], tr_b[f]) for f in tr_a)
    eng = car(eng_mod, track, B, x0=x0, seed=91)
    rec_c = np.zeros((B, _lib.RECORD_LEN))
    assert eng.L.mpopis_run_trials_traced(eng._h, ns, 2, rec_c.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0
    eng.close()
    assert np.array_equal(rec_c, rec_a)


def test_python_harness_returns_the_trace(eng_mod):
    from mpopis_amd import examples
    kw = dict(num_trials=3, num_steps=5, policy_type=":μΣaismppi", num_samples=K, horizon=T, ais_its=N, seed=5, quiet=True)
    rec, summ, tr = examples.simulate_car_racing(trace=dict(plan_every=5, top=1), **kw)
    rec0, summ0 = examples.simulate_car_racing(**kw)
    assert np.array_equal(rec[:, :17], rec0[:, :17])                                         # (the last column is the wall time)
    assert tr["states"].shape == (3, 7, 8) and tr["plan_traj"].shape == (3, 2, 2, T, 8) and np.array_equal(tr["plan_steps"], [0, 5])
    assert np.array_equal(tr["steps_run"], rec[:, 2].astype(np.int64) + 1)
    for fn, ss in ((examples.simulate_mountaincar, 2), (examples.simulate_cartpole, 4)):
        out = fn(num_trials=2, num_steps=4, num_samples=K, seed=6, quiet=True, trace=True)
        assert len(out) == 3 and out[2]["states"].shape == (2, 6, ss) and np.array_equal(out[2]["steps_run"], out[0][:, 1].astype(np.int64) + 1)
        assert len(fn(num_trials=2, num_steps=4, num_samples=K, seed=6, quiet=True)) == 2
