"""No GPU: shows that the cases of tests/helpers/rollout_cases.py are what tests/test_gpu_rollout_harness.py takes them for -- every case's form
recomputed from the constants read back from the sources, the designed ties exact, the logger cases' cars driving -- and that the checkers check:
a passing "result" is built from the HOST build of mpopis_amd/csrc/car_dynamics.h (tests/shim/host_shim.cpp: shim_car_rollout_log per car, pair terms
and car sums added here in NumPy; shim_simple_step for the two simple envs), put through the harness's file format, and accepted by every checker;
then named corruptions of it, one at a time, must each fail exactly the check meant for it."""
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
    """what the harness would return for launch L, computed on the host; corrupt: one of the named corruptions"""
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
        V, A = RC.controls(Lc, b, lo, hi)
        cc = np.zeros(K) if L["gvec"] is None else (L["gvec"][b][:, None] * (V - L["Uo"][b][:, None]))
        if car:
            ctrl = np.ascontiguousarray(A.reshape(T, nc, 2, K).transpose(3, 1, 0, 2))               # [K][nc][T][2]
            s8 = np.ascontiguousarray(np.broadcast_to(L["x0"][b].reshape(1, nc, 8), (K, nc, 8)))
            X, rew, near = np.zeros((K, nc, T, 8)), np.zeros((K, nc, T)), np.zeros((K, nc), dtype=np.int32)
            tr = L["track"]
            shim.shim_car_rollout_log(_p(np.ascontiguousarray(L["params"])), len(tr[0]), _p(tr[0]), _p(tr[1]), _p(tr[2]), K * nc, _p(s8), _p(ctrl), T, _p(X), _p(rew), near.ctypes.data_as(ip))
            for c in range(nc):                                               # multi-car_racing.jl:145-158, in the kernel's order
                for q in range(c + 1, nc):
                    if corrupt == "drop_pair" and (c, q) == (0, 1):
                        continue
                    dx, dy = X[:, q, :, 0] - X[:, c, :, 0], X[:, q, :, 1] - X[:, c, :, 1]
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
            prm = np.ascontiguousarray(L["params"])
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
                first, allmin = RC.exact_argmin(L["track"], x[b, c, 0], x[b, c, 1])
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
