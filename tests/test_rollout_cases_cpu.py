"""No GPU: shows that the cases of tests/helpers/rollout_cases.py are what tests/test_gpu_rollout_harness.py takes them for -- every case's form
recomputed from the constants read back from the sources, the designed ties exact, the logger cases' cars driving -- and that the checkers check:
a passing "result" is built from the HOST build of mpopis_amd/csrc/car_dynamics.h (tests/shim/host_shim.cpp: shim_car_rollout_log per car, pair terms
and car sums added here in NumPy; shim_simple_step for the two simple envs), put through the harness's file format, and accepted by every checker;
then named corruptions of it, one at a time, must each fail exactly the check meant for it.  The same for the per-slot and fleet cases of
tests/test_gpu_rollout_slots_harness.py (shim_car_rollout_log once per car with that car's vector): cars 1 and 2 with each other's vector, slot 0's
parameters or track in every slot, pair terms from the positions of step t - 1, the last car left out, car 0's bounds for every car, cmin over a lane
past K, the anchor searched on slot 0's track."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from tests.helpers import rollout_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "shim", "host_shim.cpp")
SHIM_SO = os.path.join(HERE, "shim", "libhost_shim.so")
HDR = os.path.join(os.path.dirname(HERE), "mpopis_amd", "csrc", "car_dynamics.h")
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def shim():
    if (not os.path.exists(SHIM_SO)) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(SHIM_SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", SHIM_SO, SHIM_SRC])
    L = C.CDLL(SHIM_SO)
    L.shim_car_rollout_log.argtypes = [dp, C.c_int, dp, dp, dp, C.c_int, dp, dp, C.c_int, dp, dp, ip]
    L.shim_car_rollout_log.restype = None
    L.shim_simple_step.argtypes = [C.c_int, dp, dp, ip, ip, C.c_double]
    L.shim_simple_step.restype = C.c_double
    return L


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(dp)


# ================================================================ a result from the host build =================================================
def host_rollout(shim, L, env=None, corrupt=None):
    """what the harness would return for launch L, computed on the host; corrupt: one of the named corruptions.  A per-slot launch: slot b under its own
    parameters on its own track; a fleet: shim_car_rollout_log once per car with that car's vector"""
    B, K, T, nc = L["B"], L["K"], L["T"], L["ncars"]
    car = L["kind"] == RC.ENV_CAR
    ss = RC.state_size(L)
    R = dict(form=RC.expected_form(L, *RC.env_form_args(env or {"MPOPIS_ROLLOUT_DUO": "0"})), cost=RC.poisoned((B, K)), traj=RC.poisoned((B, K, ss, T)) if L["traj"] else None,
             cmin=None if L["cmin"] is None else L["cmin"].copy(), status=None if L["status"] is None else L["status"].copy(),
             iters=RC.poisoned((B,), 1) if L["iters"] else None, xext=RC.poisoned((B, nc, 13)) if car else None)
    for b in RC.active_slots(L):
        if R["iters"] is not None:
            R["iters"][b] = L["iter_n"]
        Lc = L
        if corrupt == "stale_noise":                                          # step t + 1 uses step t's noise
            a = len(L["lo"])
            E = L["E"].copy(); E[:, a:] = L["E"][:, :-a]
            Lc = dict(L, E=E)
        lo, hi = (np.tile(L["lo"][:2], nc), np.tile(L["hi"][:2], nc)) if corrupt == "car0_bounds" else (L["lo"], L["hi"])
        bp = 0 if corrupt == "slot0_params" else b                            # the slot whose parameters / track this slot runs with
        bt = 0 if corrupt == "slot0_track" else b
        V, A = RC.controls(Lc, b, lo, hi)
        cc = np.zeros(K) if L["gvec"] is None else (L["gvec"][b][:, None] * (V - L["Uo"][b][:, None]))
        if car:
            ctrl = np.ascontiguousarray(A.reshape(T, nc, 2, K).transpose(3, 1, 0, 2))               # [K][nc][T][2]
            s8 = np.ascontiguousarray(np.broadcast_to(L["x0"][b].reshape(1, nc, 8), (K, nc, 8)))
            X, rew, near = np.zeros((K, nc, T, 8)), np.zeros((K, nc, T)), np.zeros((K, nc), dtype=np.int32)
            tr = RC.slot_track(L, bt)
            if RC.is_fleet(L):
                for c in range(nc):
                    cv = {1: 2, 2: 1}.get(c, c) if corrupt == "swap_car_params" else c       # cars 1 and 2 integrate with each other's vector
                    Xc, rc, nr = np.zeros((K, T, 8)), np.zeros((K, T)), np.zeros(K, dtype=np.int32)
                    shim.shim_car_rollout_log(_p(np.ascontiguousarray(RC.car_params(L, bp, cv))), len(tr[0]), _p(tr[0]), _p(tr[1]), _p(tr[2]), K, _p(np.ascontiguousarray(s8[:, c])),
                                              _p(np.ascontiguousarray(ctrl[:, c])), T, _p(Xc), _p(rc), nr.ctypes.data_as(ip))
                    X[:, c], rew[:, c], near[:, c] = Xc, rc, nr
            else:
                shim.shim_car_rollout_log(_p(np.ascontiguousarray(RC.slot_params(L, bp))), len(tr[0]), _p(tr[0]), _p(tr[1]), _p(tr[2]), K * nc, _p(s8), _p(ctrl), T, _p(X), _p(rew), near.ctypes.data_as(ip))
            Xpair = X
            if corrupt == "stale_exchange":                                   # the pair terms read the positions of step t - 1: the other buffer of the exchange
                Xpair = np.concatenate([np.broadcast_to(L["x0"][b].reshape(1, nc, 1, 8), (K, nc, 1, 8)), X[:, :, :-1]], axis=2)
            for c in range(nc):                                               # multi-car_racing.jl:145-158, in the kernel's order
                for q in range(c + 1, nc):
                    if corrupt == "drop_pair" and (c, q) == (0, 1):
                        continue
                    dx, dy = Xpair[:, q, :, 0] - X[:, c, :, 0], Xpair[:, q, :, 1] - X[:, c, :, 1]
                    dd = np.sqrt(dx * dx + dy * dy)
                    rew[:, c] += -dd
                    rew[:, c] += np.where(dd <= 4.0, -11000.0, 0.0)
            cost = np.zeros((K, nc))
            for t in range(T):
                cost -= rew[:, :, t]
            if L["gvec"] is not None:
                cost += cc.reshape(T, nc, 2, K).sum(axis=(0, 2)).T
            total = np.zeros(K)
            for c in range(nc - 1 if corrupt == "skip_last_car" else nc):
                total = total + cost[:, c]
            R["cost"][b] = np.where(np.isnan(total), np.nan, total)           # (the sign of a NaN the host arithmetic makes is the compiler's choice)
            if L["traj"]:
                R["traj"][b] = (X.transpose(0, 2, 1, 3).reshape(K, T, ss).reshape(K, ss, T) if corrupt == "traj_T_ss" else X.transpose(0, 1, 3, 2).reshape(K, ss, T))
            x = L["x0"][b].reshape(nc, 8)
            R["xext"][b] = np.column_stack([x, np.sin(x[:, 2]), np.cos(x[:, 2]), np.sin(x[:, 6]), np.cos(x[:, 6]), near[0].astype(np.float64)])
        else:
            prm = np.ascontiguousarray(RC.slot_params(L, bp))
            for k in range(K):
                s = np.ascontiguousarray(L["x0"][b].copy())
                t, done = C.c_int(int(L["t0"][b]) if L["t0"] is not None else 0), C.c_int(int(L["done0"][b]) if L["done0"] is not None else 0)
                cost = 0.0
                for i in range(T):
                    if A[i, k] != A[i, k]:
                        cost = A[i, k]
                    cost -= shim.shim_simple_step(L["kind"], _p(prm), _p(s), C.byref(t), C.byref(done), A[i, k])
                    if L["traj"]:
                        R["traj"][b, k, :, i] = s
                R["cost"][b, k] = cost
        if corrupt == "swap_costs":
            R["cost"][b, [0, 1]] = R["cost"][b, [1, 0]]
        if R["cmin"] is not None:
            keys = RC.cost_key(R["cost"][b][:K - 1] if corrupt == "cmin_short" else R["cost"][b])
            if corrupt == "cmin_past_K":                                      # a lane past K takes part in the minimum with a cost of its own
                keys = np.append(keys, RC.cost_key(np.array([R["cost"][b].min() - 1.0])))
            R["cmin"][b] = min(int(L["cmin"][b]), int(keys.min()))
            if R["status"] is not None and not np.all(np.isfinite(R["cost"][b])):
                R["status"][b] = RC.ERR_ACTION
    if corrupt == "write_past_K":
        R["guard"] = ("cost", 0, 1.0)
    return R


def host_begin(L, corrupt=None):
    B, nc = L["B"], L["ncars"]
    R = dict(form=(0, 0, 0, 0), status=None if L["status"] is None else np.zeros(B, dtype=np.int32), active=L["alive"].copy() if L["alive"] is not None else np.ones(B, dtype=np.int32),
             iters=np.zeros(B, dtype=np.int32), iters_acc=None if L["iters_acc"] is None else L["iters_acc"] + L["iters"].astype(np.uint64),
             Uin=L["U"].copy(), Ucur=L["U"].copy(), cmin=None if L["cmin"] is None else np.full(B, RC.ALL_ONES), xext=RC.poisoned((B, nc, 13)) if nc else None, xref=None)
    if L["x"] is not None:
        x = L["x"]
        ext = np.concatenate([x, np.sin(x[:, :, 2:3]), np.cos(x[:, :, 2:3]), np.sin(x[:, :, 6:7]), np.cos(x[:, :, 6:7]), np.zeros((B, nc, 1))], axis=2)
        R["xref"] = ext.copy()
        for b in range(B):
            for c in range(nc):
                first, allmin = RC.exact_argmin(RC.slot_track(L, 0 if corrupt == "slot0_track" else b), x[b, c, 0], x[b, c, 1])
                R["xref"][b, c, 12] = first
                ext[b, c, 12] = allmin[-1] if corrupt == "tie_high" else first
        R["xext"] = ext
    return R


def through_the_file(launches, results):
    return RC.unpack_result(RC.pack_result(launches, results), launches)


# ================================================================ the cases are what they claim ================================================
def test_constants_are_read_from_the_sources_and_the_lds_limit_is_where_the_cases_put_it():
    c = RC.source_constants()
    assert c["kCarExt"] == 13 and c["spb4_K"] == 1024 and c["kDuoCarWaves"] >= 1 and c["kDuoCarsWaves"] >= 1
    pmax = RC.max_tlds_points(c)
    assert RC.track_lds_bytes(pmax, min(c["kTrackNbrW"], pmax), True, c) <= c["kRolloutDynLdsDefault"] < RC.track_lds_bytes(pmax + 1, min(c["kTrackNbrW"], pmax + 1), True, c)
    assert pmax < RC.BIG_P and len(RC.default_track()[0]) <= pmax


def test_every_form_case_recomputes_to_the_form_it_was_written_for():
    seen = set()
    for name, L, env, body in RC.form_cases():
        f = RC.expected_form(L, *RC.env_form_args(env))
        assert f[0] == body, (name, RC.BODY_NAME[f[0]], RC.BODY_NAME[body])
        seen.add((f[0], f[1], f[2]))
    for nc in range(1, 9):
        for body in (RC.TWO_WAVE, RC.SPB1, RC.SPB4):
            for L in RC.parity_launches(nc, body):
                f = RC.expected_form(L, RC.duo_of(body))
                assert f[0] == body and not f[1], (nc, body, f)
                seen.add((f[0], f[1], f[2]))
        A, two, _ = RC.invariant_launches(nc)
        assert RC.expected_form(A["base"], 0)[0] == RC.SPB1 and RC.expected_form(A["big"], 0)[0] == RC.SPB4 and RC.expected_form(A["logged"], 0)[:2] == (RC.SPB1, True)
        assert all(RC.expected_form(A[n], RC.DUO_ALWAYS)[0] == RC.TWO_WAVE for n in two)
    for nc in (1, 3, 6):
        for L in RC.logger_launches(nc):
            f = RC.expected_form(L, 0)
            assert f[1], (nc, f)
            seen.add((f[0], f[1], f[2]))
    want = {(b, False, t) for b in (RC.TWO_WAVE, RC.SPB1, RC.SPB4) for t in (True, False)} | {(b, True, t) for b in (RC.SPB1, RC.SPB4) for t in (True, False)}
    assert want <= seen, want - seen                                          # body x logger x table placement, all of it


def test_edges_of_the_sample_wave_and_the_start_states(oracle):
    for nc in range(1, 9):
        S = 64 // nc
        assert set(RC.k_edges(nc)) >= {1, S, S + 1, 2 * S + 3} and RC.spb4_K(nc) % (4 * S) != 0 and RC.spb4_K(nc) >= 1024
        assert np.array_equal(RC.reset_state(nc), oracle.OracleEnv("car", nc).state)
        x0 = RC.start_states(nc, 3)
        assert np.all(x0[:, 3::8] >= 10.0)
        if nc >= 3:
            assert np.array_equal(x0[1, 8:10], x0[1, 0:2]) and x0[1, 16] - x0[1, 0] == 3.0
        lo, hi = RC.car_bounds(nc)
        assert np.all(lo >= -1.0) and np.all(hi <= 1.0) and np.all(lo < hi) and np.all(lo != -hi)
        assert nc == 1 or (len(set(lo[0::2])) == nc and len(set(hi[1::2])) == nc)


def test_designed_ties_are_exact_ties_of_the_intended_threads():
    classes = set()
    for L in RC.begin_launches():
        if L["tie"] is None:
            continue
        classes.add(L["name"])
        for b in range(L["B"]):
            for c in range(L["ncars"]):
                first, allmin = RC.exact_argmin(L["track"], L["x"][b, c, 0], L["x"][b, c, 1])
                assert np.array_equal(allmin, np.sort(L["tie"])) and first == min(L["tie"])
        i = L["tie"]
        if L["name"] == "thread":
            assert i[0] % 256 == i[1] % 256
        if L["name"] == "waves":
            assert (i[0] % 256) // 64 != (i[1] % 256) // 64 and i[0] % 64 == i[1] % 64
        if L["name"] == "lanes":
            assert i[1] == i[0] + 1
        if L["name"] == "wrap":
            assert i == (0, L["P"] - 1)
    assert classes == {"thread", "three", "waves", "lanes", "wrap", "single"}
    assert {L["P"] for L in RC.begin_launches() if L["x"] is not None} == set(RC.BEGIN_P) and {L["cs"] for L in RC.begin_launches() if L["x"] is None} == set(RC.BEGIN_CS)


def test_the_oracle_alone_sets_no_logged_state_aside(oracle):
    """the logger cases' cars keep driving: along the oracle's own trajectories Vx stays far from the zero where the sign rules of the model switch"""
    for nc in (1, 3, 6):
        for L in RC.logger_launches(nc):
            for b, (cost, traj) in RC.oracle_costs(oracle, L, log=True).items():
                assert np.isfinite(cost).all() and traj[:, :, 3::8].min() > 1.0, (nc, L["K"], b, float(traj[:, :, 3::8].min()))


def test_the_set_aside_rule_holds_on_a_logger_case_itself(shim, oracle):
    """check_logger, with its set-aside rule (none allowed) and both bounds, on the host build's result for logger cases as the GPU test runs them (T = 9):
    the SPB 1 cases of 1 and 6 cars on both tracks, and the SPB 4 case (K = 1024 + S + 1) of 6 cars"""
    for L in RC.logger_launches(1)[:2] + RC.logger_launches(6)[:3]:
        R, = through_the_file([L], [host_rollout(shim, L)])
        dev, ratio = RC.check_logger(oracle, L, R)
        assert dev < 1e-11 and ratio <= 1.0


# ================================================================ the checkers check ===========================================================
def _checks(oracle, L, R):
    """every checker on one result -> the names of those that fail"""
    failed = set()
    try:
        R, = through_the_file([L], [R])
    except AssertionError:
        return {"guards"}
    for name, fn in (("form", lambda: RC.check_form(L, R, 0)), ("slots", lambda: RC.check_slots(L, R)), ("parity", lambda: RC.check_parity(oracle, L, R)),
                     ("cmin", lambda: RC.check_cmin(L, R)), ("logger", lambda: RC.check_logger(oracle, L, R) if L["traj"] else None)):
        try:
            fn()
        except AssertionError:
            failed.add(name)
    return failed


def _cpu_launch(nc, traj, track=None):
    S = 64 // nc
    L = RC.car_launch(nc, 2, S + 1, 5, 600 + nc, track=track, traj=traj, iters=True, cmin=np.array([RC.ALL_ONES] * 2, dtype=np.uint64), status=np.zeros(2, dtype=np.int32))
    return L


@pytest.mark.parametrize("nc", [1, 3, 6])
def test_checkers_accept_the_host_build_and_each_corruption_fails_its_check(shim, oracle, nc):
    plain, logged = _cpu_launch(nc, False), _cpu_launch(nc, True, track=RC.big_track(RC.BIG_P) if nc == 3 else None)
    assert _checks(oracle, plain, host_rollout(shim, plain)) == set()
    assert _checks(oracle, logged, host_rollout(shim, logged)) == set()
    # cmin over K - 1 samples: the case whose minimum is the last sample
    R = host_rollout(shim, plain)
    k = [int(np.argmin(R["cost"][b])) for b in range(2)]
    E = plain["E"].copy()
    for b in range(2):
        E[b][:, [k[b], -1]] = E[b][:, [-1, k[b]]]
    last = dict(plain, E=E)
    assert all(int(np.argmin(host_rollout(shim, last)["cost"][b])) == last["K"] - 1 for b in range(2))
    want = [("swap_costs", plain, "parity"), ("stale_noise", plain, "parity"), ("car0_bounds", plain, "parity"), ("drop_pair", plain, "parity"), ("skip_last_car", plain, "parity"),
            ("traj_T_ss", logged, "logger"), ("cmin_short", last, "cmin"), ("write_past_K", plain, "guards")]
    for corrupt, L, check in want:
        if nc == 1 and corrupt in ("car0_bounds", "drop_pair", "skip_last_car"):
            continue                                                          # one car: nothing to corrupt
        failed = _checks(oracle, L, host_rollout(shim, L, corrupt=corrupt))
        if corrupt == "traj_T_ss":
            failed.discard("parity")                                          # (the oracle's trajectory sees the layout too: both are meant for it)
        assert failed == {check}, (corrupt, failed)


def test_invariant_checks_accept_the_host_build(shim, oracle):
    for nc in (1, 4):
        A, two, notes = RC.invariant_launches(nc)
        RA = dict(zip(A, through_the_file(list(A.values()), [host_rollout(shim, L) for L in A.values()])))
        RB = {n: through_the_file([A[n]], [host_rollout(shim, A[n], env={"MPOPIS_ROLLOUT_DUO": str(RC.DUO_ALWAYS)})])[0] for n in two}
        RC.check_invariants(nc, A, RA, RB, two, notes)
        bad = dict(RA, perm=dict(RA["perm"], cost=RA["base"]["cost"]))
        with pytest.raises(AssertionError):
            RC.check_invariants(nc, A, bad, RB, two, notes)


def test_gamma_check_accepts_the_host_build(shim, oracle):
    for nc in (1, 4):
        L1, L0 = RC.gamma_launches(nc)
        q = RC.check_gamma(oracle, L1, host_rollout(shim, L1), host_rollout(shim, L0))
        assert q <= 1.0, q
        R1 = host_rollout(shim, L1)
        assert RC.check_gamma(oracle, L1, dict(R1, cost=np.nextafter(R1["cost"], 0.0) - 1e-9), host_rollout(shim, L0)) > 1.0


@pytest.mark.parametrize("kind", [RC.ENV_MC, RC.ENV_CP])
def test_simple_env_cases_terminate_where_they_claim_and_the_host_build_passes(shim, oracle, kind):
    Ls = RC.simple_launches(kind)
    Rs = through_the_file(Ls, [host_rollout(shim, L) for L in Ls])
    for L, R in zip(Ls[:-1], Rs[:-1]):
        RC.check_slots(L, R)
        assert RC.check_parity(oracle, L, R) < 1e-12
    n = len(RC.SIMPLE_K) * len(RC.SIMPLE_T)
    started_done, ends_inside = RC.oracle_costs(oracle, Ls[n], log=True), RC.oracle_costs(oracle, Ls[n + 1], log=True)
    if kind == RC.ENV_MC:                                                     # a done MountainCar earns |v| without the -1 of a running one: costs below / above 0
        assert np.all(started_done[0][0] <= 0.0) and np.all(started_done[1][0] > 0.0)
        assert np.all(ends_inside[0][0] < 15.0 - 4.0) and np.all(ends_inside[0][0] > 0.0)
    else:                                                                     # CartPole: 1 per step until done
        assert np.all(started_done[0][0] == 0.0) and np.all(ends_inside[0][0] == -5.0) and np.all(ends_inside[1][0] == -1.0)
        fell = RC.oracle_costs(oracle, Ls[n + 2])
        assert np.all(fell[0] > -15.0) and np.all(fell[1] > -15.0)
    nan = np.isnan(Ls[-1]["E"]).any(axis=1)                                   # [B][K]: the samples that hold a NaN action
    assert nan.sum() == 2 and np.array_equal(np.isnan(Rs[-1]["cost"]), nan)
    assert np.array_equal(RC.bits(Rs[-1]["cost"][~nan]), RC.bits(Rs[-2]["cost"][~nan]))


def test_begin_checks_accept_the_definition_and_refuse_the_higher_index():
    Ls = RC.begin_launches()
    for L, R in zip(Ls, through_the_file(Ls, [host_begin(L) for L in Ls])):
        RC.check_begin(L, R)
    refused = 0
    for L in Ls:
        if L["tie"] is not None and len(L["tie"]) > 1:
            R, = through_the_file([L], [host_begin(L, corrupt="tie_high")])
            with pytest.raises(AssertionError, match="anchor"):
                RC.check_begin(L, R)
            refused += 1
    assert refused >= 60
    L = RC.copy_launch(257, 1)
    R = host_begin(L)
    R["Ucur"][1, 256] = np.nextafter(R["Ucur"][1, 256], 9.0)
    with pytest.raises(AssertionError, match="U copies"):
        RC.check_begin(L, through_the_file([L], [R])[0])


def test_case_files_round_trip():
    L = RC.car_launch(2, 2, 5, 3, 1, traj=True, iters=True, cmin=np.array([1, 2], dtype=np.uint64))
    buf = RC.pack([L, RC.copy_launch(7, 2)])
    assert buf[:8] == RC.MAGIC_IN and len(buf) % 8 == 0
    R = dict(form=(4, 1, 1, 100), cost=np.zeros((2, 5)), traj=np.ones((2, 5, 16, 3)), cmin=np.array([3, 4], dtype=np.uint64), iters=np.array([3, 3], dtype=np.int32), xext=np.zeros((2, 2, 13)))
    back, = through_the_file([L], [R])
    assert back["form"] == (4, True, True, 100) and back["status"] is None and back["traj"].shape == (2, 5, 16, 3) and back["cmin"][1] == 4
    with pytest.raises(AssertionError, match="guard"):
        through_the_file([L], [dict(R, guard=("traj", 63, 0.0))])


# ================================================================ per-slot envs and fleets =====================================================
def test_fleet_constants_and_the_fleet_lds_limit():
    c = RC.source_constants()
    assert RC.fleet_static_lds(8, c) == 16640 and c["kFleetLdsDefault"] == 64 * 1024
    for nc in (2, 8):
        pf = RC.max_tlds_points_fleet(nc, c)
        W = lambda P: min(c["kTrackNbrW"], P)
        assert RC.track_lds_bytes(pf, W(pf), True, c) + RC.fleet_static_lds(nc, c) <= 64 * 1024 < RC.track_lds_bytes(pf + 1, W(pf + 1), True, c) + RC.fleet_static_lds(nc, c)
        assert pf < RC.BIG_P
    assert RC.track_lds_bytes(2048, c["kTrackNbrW"], False, c) == 131360                       # the ring table of the largest track: the raised limit


def test_every_per_slot_case_recomputes_to_the_form_it_was_written_for():
    seen = set()
    for name, L, env, body in RC.slot_form_cases():
        f = RC.expected_form(L, *RC.env_form_args(env))
        assert f[0] == body, (name, RC.BODY_NAME[f[0]], RC.BODY_NAME[body])
        big = max(len(RC.slot_track(L, b)[0]) for b in range(L["B"]))         # the largest-track rule: the form of the same launch with that track in every slot
        assert f == RC.expected_form(dict(L, tracks=[RC.big_track(big)], tos=[0] * L["B"]), *RC.env_form_args(env)), name
        assert min(len(RC.slot_track(L, b)[0]) for b in range(L["B"])) < big
        seen.add(f[:3])
    assert {(RC.FLEET, l, t) for l in (True, False) for t in (True, False)} | {(b, False, t) for b in (RC.TWO_WAVE, RC.SPB1, RC.SPB4) for t in (True, False)} <= seen
    for nc in range(1, 9):
        for body in (RC.TWO_WAVE, RC.SPB1, RC.SPB4):
            Ls = RC.twin_parity_launches(nc, body)
            assert all(RC.expected_form(L, RC.duo_of(body))[:2] == (body, False) for L in Ls) and {RC.expected_form(L, 0)[2] for L in Ls} == {True, False}
            assert all(L["tos"] == RC.SLOT_TOS and [len(t[0]) for t in L["tracks"]][1:] == [3, 12] for L in Ls)
        if nc >= 2:
            Ls = RC.fleet_parity_launches(nc)
            assert all(RC.expected_form(L, 0)[0] == RC.FLEET and RC.expected_form(L, RC.DUO_ALWAYS)[0] == RC.FLEET for L in Ls) and {RC.expected_form(L, 0)[2] for L in Ls} == {True, False}
            assert {L["K"] for L in Ls} == set(RC.FLEET_K) and {L["T"] for L in Ls} == set(RC.T_FULL if nc in (2, 3, 8) else (1, 2, 5))
            assert sum(len(L["tracks"]) > 1 for L in Ls) >= len(Ls) // 2 and np.all(Ls[0]["params"][1, :, 19] == 0.02) and np.array_equal(Ls[0]["params"][1, :, 0], Ls[0]["params"][0, ::-1, 0])
    for fleet, nc in ((False, 1), (False, 3), (True, 2), (True, 3), (True, 8)):
        assert [RC.expected_form(L, 0)[:3] for L in RC.slot_logger_launches(nc, fleet)] == [(RC.FLEET if fleet else RC.SPB1, True, True), (RC.FLEET if fleet else RC.SPB1, True, False)]
    for nc in (1, 3, 8):
        A, two, _ = RC.twin_invariant_launches(nc)
        assert RC.expected_form(A["base"], 0)[0] == RC.SPB1 and RC.expected_form(A["big"], 0)[0] == RC.SPB4 and all(RC.expected_form(A[n], RC.DUO_ALWAYS)[0] == RC.TWO_WAVE for n in two)
        assert A["slot_perm"]["tos"] == A["base"]["tos"][::-1] and np.array_equal(A["slot_perm"]["params"][0], A["base"]["params"][2])
    for nc in (2, 3, 5, 8):
        A, two, notes = RC.fleet_invariant_launches(nc)
        assert not two and all(RC.expected_form(L, 0)[0] == RC.FLEET for L in A.values()) and not np.any(notes["car_perm"] == np.arange(nc))
        assert len(notes["nan_names"]) == 3 * len({0, nc // 2, nc - 1})


def test_the_reference_alone_sets_no_logged_state_aside_in_the_per_slot_logger_cases(oracle):
    """the premise of (k)'s "none set aside": along the reference's own trajectories every car keeps Vx > 1, far from the zero where the model's sign rules switch"""
    for fleet, nc in ((False, 1), (False, 3), (True, 2), (True, 3), (True, 8)):
        for L in RC.slot_logger_launches(nc, fleet):
            for b, (cost, traj) in RC.oracle_costs(oracle, L, log=True).items():
                assert np.isfinite(cost).all() and traj[:, :, 3::8].min() > 1.0, (fleet, nc, b, float(traj[:, :, 3::8].min()))


def _slot_cpu_launch(nc, fleet, traj):
    make = RC.fleet_launch if fleet else RC.twin_launch
    kw = dict(tracks=RC.small_tracks(), tos=[2, 0, 1]) if fleet else {}
    return make(nc, 3, 64 + 3 if fleet else 64 // nc + 1, 5, 650 + nc, traj=traj, iters=True, cmin=np.array([RC.ALL_ONES] * 3, dtype=np.uint64), status=np.zeros(3, dtype=np.int32), **kw)


@pytest.mark.parametrize("fleet,nc", [(False, 1), (False, 3), (True, 3), (True, 8)], ids=["twin1", "twin3", "fleet3", "fleet8"])
def test_per_slot_checkers_accept_the_host_build_and_each_corruption_fails_its_check(shim, oracle, fleet, nc):
    plain, logged = _slot_cpu_launch(nc, fleet, False), _slot_cpu_launch(nc, fleet, True)
    assert _checks(oracle, plain, host_rollout(shim, plain)) == set()
    assert _checks(oracle, logged, host_rollout(shim, logged)) == set()
    want = [("slot0_params", plain, {"parity"}), ("slot0_track", plain, {"parity"}), ("cmin_past_K", plain, {"cmin"}), ("slot0_params", logged, {"parity", "logger"})]
    if nc > 1:
        want += [("car0_bounds", plain, {"parity"}), ("skip_last_car", plain, {"parity"}), ("stale_exchange", plain, {"parity"}), ("stale_exchange", logged, {"parity", "logger"})]
    if fleet:
        want += [("swap_car_params", logged, {"parity", "logger"})]
    for corrupt, L, checks in want:
        assert _checks(oracle, L, host_rollout(shim, L, corrupt=corrupt)) == checks, (corrupt, bool(L["traj"]))
    if fleet:                                                                 # cars 1 and 2 with each other's vector: whatever the costs say, the trajectory and the logger checks fail
        R, = through_the_file([logged], [host_rollout(shim, logged, corrupt="swap_car_params")])
        ref = RC.oracle_costs(oracle, logged, log=True)
        with pytest.raises(AssertionError, match="trajectory deviates"):
            RC.check_parity(oracle, logged, dict(R, cost=np.stack([ref[b][0] for b in range(3)])), ref=ref)
        with pytest.raises(AssertionError, match="state"):
            RC.check_logger(oracle, logged, R)


def test_car_permutation_check_accepts_the_host_build_and_sees_a_car_with_anothers_vector(shim, oracle):
    A, _, notes = RC.fleet_invariant_launches(3)
    L, Lp, perm = dict(A["logged"], active=None), dict(A["car_perm"], active=None), notes["car_perm"]
    R, Rp = through_the_file([L, Lp], [host_rollout(shim, L), host_rollout(shim, Lp)])
    assert RC.check_car_permutation(oracle, L, R, Lp, Rp, perm) <= 1.0
    bad, = through_the_file([Lp], [host_rollout(shim, Lp, corrupt="swap_car_params")])
    with pytest.raises(AssertionError, match="logs another trajectory"):
        RC.check_car_permutation(oracle, L, R, Lp, bad, perm)


def test_per_slot_invariant_and_gamma_checks_accept_the_host_build(shim, oracle):
    A, two, notes = RC.twin_invariant_launches(3)
    RA = dict(zip(A, through_the_file(list(A.values()), [host_rollout(shim, L) for L in A.values()])))
    RB = {n: through_the_file([A[n]], [host_rollout(shim, A[n], env={"MPOPIS_ROLLOUT_DUO": str(RC.DUO_ALWAYS)})])[0] for n in two}
    RC.check_invariants(3, A, RA, RB, two, notes)
    with pytest.raises(AssertionError, match="permuting the slots"):
        RC.check_invariants(3, A, dict(RA, slot_perm=through_the_file([A["slot_perm"]], [host_rollout(shim, A["slot_perm"], corrupt="slot0_params")])[0]), RB, two, notes)
    A, two, notes = RC.fleet_invariant_launches(3)
    RA = dict(zip(A, through_the_file(list(A.values()), [host_rollout(shim, L) for L in A.values()])))
    RC.check_invariants(3, A, RA, {}, two, notes)
    for make, nc, S in ((RC.fleet_launch, 4, 64), (lambda *a, **kw: RC.slot_launch(*a, params=RC.slot_params3((2,)), **kw), 1, None)):
        L1, L0 = RC.gamma_launches(nc, make=make, S=S)
        assert RC.check_gamma(oracle, L1, host_rollout(shim, L1), host_rollout(shim, L0)) <= 1.0


@pytest.mark.parametrize("kind", [RC.ENV_MC, RC.ENV_CP])
def test_simple_per_slot_cases_end_where_they_claim_and_the_host_build_passes(shim, oracle, kind):
    Ls = RC.simple_slot_launches(kind)
    Rs = through_the_file(Ls, [host_rollout(shim, L) for L in Ls])
    for L, R in zip(Ls[:-1], Rs[:-1]):
        RC.check_slots(L, R)
        assert RC.check_parity(oracle, L, R) < 1e-12
    assert not np.array_equal(Ls[0]["params"][0], Ls[0]["params"][1]) and not np.array_equal(Ls[0]["params"][1], Ls[0]["params"][2])
    ends = Ls[len(RC.SIMPLE_K) * len(RC.SIMPLE_T)]                              # slot 1's own step limit ends its episode 5 steps in; its neighbours run on
    ref = RC.oracle_costs(oracle, ends, log=True)
    same_limit = RC.oracle_costs(oracle, dict(ends, params=Ls[0]["params"]))
    assert not np.array_equal(ref[1][0], same_limit[1]) and np.array_equal(ref[0][0], same_limit[0]) and np.array_equal(ref[2][0], same_limit[2])
    if kind == RC.ENV_CP:
        assert np.all(ref[1][0] == -5.0) and np.all(ref[0][0] < -5.0)
    with pytest.raises(AssertionError):                                       # slot 0's parameters in every slot
        RC.check_parity(oracle, Ls[1], through_the_file([Ls[1]], [host_rollout(shim, Ls[1], corrupt="slot0_params")])[0])
    nan = np.isnan(Ls[-1]["E"]).any(axis=1)
    assert nan.sum() == 2 and np.array_equal(np.isnan(Rs[-1]["cost"]), nan)


def test_begin_with_slot_tracks_accepts_the_definition_and_refuses_slot_0s_track():
    Ls = RC.begin_slots_launches()
    assert {len(t[0]) for L in Ls for t in L["tracks"]} == set(RC.BEGIN_SLOT_P) and {L["ncars"] for L in Ls} == {1, 3, 8} and all(L["B"] == 3 and len({len(t[0]) for t in L["tracks"]}) == 3 for L in Ls)
    assert all(L["tos"] != [0, 1, 2] for L in Ls)
    for L, R in zip(Ls, through_the_file(Ls, [host_begin(L) for L in Ls])):
        RC.check_begin(L, R)
        bad, = through_the_file([L], [host_begin(L, corrupt="slot0_track")])
        with pytest.raises(AssertionError, match="anchor"):
            RC.check_begin(L, bad)


def test_per_slot_case_files_round_trip():
    from tests.helpers import harness_io as IO
    F = RC.fleet_launch(3, 2, 5, 3, 1, tracks=[RC.default_track(), RC.ring_track(12)], tos=[1, 0], traj=True)
    S = RC.simple_slot_launches(RC.ENV_MC)[0]
    Bg = RC.begin_slots_launches()[0]
    buf = RC.pack([F, S, Bg, RC.car_launch(1, 1, 3, 2, 1)])
    assert buf[:8] == RC.MAGIC_IN
    off, recs = 16, []
    for _ in range(4):
        rec, off = IO.unpack_launch(buf, off)
        recs.append(rec)
    assert off == len(buf) and [r[0] for r in recs] == [RC.OP_ROLLOUT_SLOTS, RC.OP_ROLLOUT_SLOTS, RC.OP_BEGIN_SLOTS, RC.OP_ROLLOUT]
    op, B, ipar, _, arrays = recs[0]
    assert ipar == [RC.ENV_CAR, 3, 5, 3, 2, 3, 1, 1, 0, 0, 1] and len(arrays) == 18 and arrays[1][1].size == 2 * 3 * 20 and list(arrays[16][1]) == [48, 12] and list(arrays[17][1]) == [1, 0]
    assert arrays[2][1].size == 60 and np.array_equal(arrays[2][1][48:], RC.ring_track(12)[0])
    assert recs[1][2][4] == 0 and recs[1][4][1][1].size == 3 * 8 and recs[1][4][16][1].size == 0
    assert len(recs[3][4]) == 16                                              # the shared ops pack as before
    assert len(recs[2][4]) == 12 and list(recs[2][4][11][1]) == Bg["tos"]
    R = dict(form=(6, 1, 1, 100), cost=np.zeros((2, 5)), traj=np.ones((2, 5, 24, 3)), cmin=None, status=None, iters=None, xext=np.zeros((2, 3, 13)))
    back, = through_the_file([F], [R])
    assert back["form"] == (6, True, True, 100) and back["traj"].shape == (2, 5, 24, 3)
