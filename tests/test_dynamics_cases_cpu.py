"""CPU side of the direct tests of the car model (tests/helpers/dynamics_cases.py, tools/kbench_dynamics.hip): shows without a GPU that the cases are
what they claim -- the files round-trip, every regime starts with Vx > 0 and with Vx <= 0, every anchor arrangement reaches its intended tier, the
exact ties are exact in double -- and holds the HOST build of mpopis_amd/csrc/car_dynamics.h (tests/shim/host_shim.cpp: shim_dyn_prims, shim_dyn_step,
shim_dyn_reward, the harness's lane programs with one lane per "wave") to every bound tests/test_gpu_dynamics_harness.py holds the device build to, on
the same cases and through the same check functions.  That is also the first state-level check of car_action_step<false> and of renorm = false on any
platform.  The host takes the #else side of every device-only form (IEEE division and sqrt, fmin / fmax, one-bit masks), so this proves the cases and
the references, not the device arithmetic."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from tests.helpers import dynamics_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "shim", "host_shim.cpp")
SHIM_SO = os.path.join(HERE, "shim", "libhost_shim.so")
HDR = os.path.join(os.path.dirname(HERE), "mpopis_amd", "csrc", "car_dynamics.h")
dp = C.POINTER(C.c_double)
TRACKS = {n: t for n, t in D.tracks() if n in ("curve", "ring3", "ring5")}


@pytest.fixture(scope="module")
def shim():
    if (not os.path.exists(SHIM_SO)) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(SHIM_SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", SHIM_SO, SHIM_SRC])
    L = C.CDLL(SHIM_SO)
    L.shim_dyn_prims.argtypes = [C.c_int, dp, dp, C.c_double, C.c_double]
    L.shim_dyn_step.argtypes = [dp, C.c_int, C.c_int, dp, C.c_int, dp, dp]
    L.shim_dyn_reward.argtypes = [dp, C.c_int, dp, dp, dp, C.c_int, dp, dp]
    for f in (L.shim_dyn_prims, L.shim_dyn_step, L.shim_dyn_reward):
        f.restype = None
    return L


def _ptr(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(dp)


def _poisoned(n, w):
    return np.frombuffer(b"\xa5" * (8 * n * w), dtype=np.float64).copy().reshape(n, w)


def host_prims(shim, inp, lo, hi):
    inp = np.ascontiguousarray(inp); out = _poisoned(len(inp), D.PRIM_OUT)
    shim.shim_dyn_prims(len(inp), _ptr(inp), _ptr(out), lo, hi)
    return out


def host_step(shim, p, psi, renorm, inp):
    inp, p, bnd = np.ascontiguousarray(inp), np.ascontiguousarray(p), np.ascontiguousarray(D.ACTION_BOUNDS)
    out = _poisoned(len(inp), D.STEP_OUT)
    shim.shim_dyn_step(_ptr(p), int(psi), int(renorm), _ptr(bnd), len(inp), _ptr(inp), _ptr(out))
    return out


def host_reward(shim, p, track, inp):
    inp, p = np.ascontiguousarray(inp), np.ascontiguousarray(p)
    out = _poisoned(len(inp), D.REW_OUT)
    shim.shim_dyn_reward(_ptr(p), len(track[0]), _ptr(track[0]), _ptr(track[1]), _ptr(track[2]), len(inp), _ptr(inp), _ptr(out))
    return out


# ================================================================ files ========================================================================
def test_case_and_result_files_round_trip(oracle):
    rng = np.random.default_rng(0)
    inp = D.prim_inputs(n=1501)
    c = D.unpack_case(D.pack_prims(inp, -1.0, 0.5))
    assert (c["op"], c["n"], c["lo"], c["hi"]) == (D.OP_PRIMS, 1501, -1.0, 0.5) and np.array_equal(D.bits(c["inp"]), D.bits(inp))     # NaNs included
    groups = [dict(psi=g % 2, renorm=g // 2, p20=rng.standard_normal(20), bnd=D.ACTION_BOUNDS, inp=rng.standard_normal((30 + g, D.STEP_IN))) for g in range(4)]
    c = D.unpack_case(D.pack_steps(groups))
    assert c["op"] == D.OP_STEP and c["G"] == 4
    for g, h in zip(groups, c["groups"]):
        assert (h["psi"], h["renorm"]) == (bool(g["psi"]), bool(g["renorm"])) and all(np.array_equal(g[k], h[k]) for k in ("p20", "bnd", "inp"))
    track = TRACKS["ring5"]
    rin = rng.standard_normal((70, D.REW_IN))
    c = D.unpack_case(D.pack_reward(oracle.car_default_params(), track, rin))
    assert (c["op"], c["n"], c["P"]) == (D.OP_REWARD, 70, 5) and np.array_equal(c["inp"], rin) and all(np.array_equal(a, b) for a, b in zip(c["track"], track))
    outs = [rng.standard_normal((n, D.STEP_OUT)) for n in (30, 7500)]
    back = D.unpack_result(D.pack_result(D.OP_STEP, outs), D.OP_STEP, [30, 7500])
    assert all(np.array_equal(a, b) for a, b in zip(outs, back))
    spoiled = bytearray(D.pack_result(D.OP_STEP, outs)); spoiled[32 + 8 * 30 * D.STEP_OUT + 3] = 0          # a byte of the first launch's guard
    with pytest.raises(AssertionError):
        D.unpack_result(bytes(spoiled), D.OP_STEP, [30, 7500])


# ================================================================ 1. primitives ================================================================
def test_primitive_inputs_cover_their_ranges_and_the_host_meets_the_bounds(shim):
    inp = D.prim_inputs()
    n = len(inp)
    assert n % 64 != 0 and 2 ** 16 <= n < 2 ** 16 + 64
    x, q, v = inp[:, D.X], inp[:, D.Q], inp[:, D.ANG]
    assert np.nanmin(np.abs(x)) <= 1e-12 and np.nanmax(np.abs(x)) >= 2e3 and np.any(x < 0)
    assert np.any(q == 0.0) and np.any(q == 1e-8) and np.nanmax(q) >= 1e10 and np.any((q > 0) & (q < 1e-8))
    for col, k in ((x, 3), (q, 20), (v, -9)):                              # a power of two, its two neighbours; the lower one is the mantissa of all ones
        for val in (2.0 ** k, np.nextafter(2.0 ** k, 0.0), np.nextafter(2.0 ** k, np.inf)):
            assert np.any(col == val), (k, val)
    assert np.frexp(np.nextafter(8.0, 0.0))[0] == 1.0 - 2.0 ** -53
    assert np.any(v == D.TINY_ANGLE) and np.any(v == -D.TINY_ANGLE) and np.any(v == 0.0)
    for col in (x, q, v, inp[:, D.CV]):
        assert np.isnan(col).any()
    fig = D.check_prims(inp, host_prims(shim, inp, -1.0, 1.0), -1.0, 1.0, device=False)
    assert fig["fast_rcp"] <= 0.5 and fig["fast_sqrt"] <= 0.5                # IEEE division and square root: the reference and its ulp measure agree with them
    small = D.prim_inputs(n=1501, lo=0.25, hi=0.25, seed=12)                 # clampd_u with lo == hi
    D.check_prims(small, host_prims(shim, small, 0.25, 0.25), 0.25, 0.25, device=False)


def test_the_exact_fma_reference_is_a_fused_multiply_add():
    a = 1.0 + 2.0 ** -30
    assert D.fma_exact(a, a, -(a * a)) == 2.0 ** -60 and a * a - a * a == 0.0           # the product's rounding error: invisible to an unfused evaluation
    assert D.fma_exact(3.0, 5.0, 7.0) == 22.0 and D.fma_exact(0.1, 10.0, -1.0) == 2.0 ** -54
    assert float(D.ulps(np.array([1.0 + 2.0 ** -52]), np.array([1.0], dtype=D.LD))[0]) == 1.0
    assert float(D.ulps(np.array([np.nextafter(2.0, 0.0)]), np.array([2.0], dtype=D.LD))[0]) == 0.5       # the last place of the REFERENCE


# ================================================================ 2. one model step ============================================================
def test_which_force_rules_each_regime_runs(oracle):
    """Which force rules the cases of each regime run: the hot rules need Vx > 0 at the start of a sub-step, the general rules take Vx <= 0.  The generator
    of tests/test_dynamics_shim.py draws both signs in "spinning" only; "crawling" cars brake through Vx = 0 inside the step and "stopped" / "backwards"
    cars are driven forwards inside it, so these three switch rule sets between sub-steps; "driving" (never below 2 m/s) stays on the hot rules.  Counted
    from the start states and the oracle's end states."""
    p, S, A, R, ref = D.default_step_cases(oracle)
    assert S.shape == (7500, 8) and np.array_equal(R, np.repeat(np.arange(5), 1500))
    start = {regime: (int(np.sum(S[R == r, 3] > 0)), int(np.sum(S[R == r, 3] <= 0))) for r, regime in enumerate(D.REGIMES)}
    end = {regime: (int(np.sum(ref[R == r, 3] > 0)), int(np.sum(ref[R == r, 3] <= 0))) for r, regime in enumerate(D.REGIMES)}
    print("\n[dynamics cases] starts with Vx > 0 / Vx <= 0 per regime: %s; ends: %s" % (start, end))
    assert start["spinning"][0] > 100 and start["spinning"][1] > 100
    assert start["driving"][1] == 0 and start["stopped"][0] == 0 and start["backwards"][0] == 0 and start["crawling"][1] == 0          # what the generator draws
    # crawling brakes through Vx = 0, stopped and backwards cars are driven forwards: both signs occur within the step
    assert end["crawling"][1] > 10 and end["stopped"][0] > 100 and end["backwards"][0] > 10
    order = D.interleave_order(R)
    assert sorted(order.tolist()) == list(range(7500))
    for at in range(0, 7500, 64):                                          # every wave of the interleaved run holds every regime
        assert len(set(R[order[at:at + 64]].tolist())) == 5
    e = np.array(D.EPS)[np.arange(7500) % 5]
    for r in range(5):
        assert set(e[R == r].tolist()) == set(D.EPS)


@pytest.mark.parametrize("psi,renorm", D.VARIANTS)
def test_host_model_step_in_the_four_forms(shim, oracle, psi, renorm):
    p, S, A, R, ref = D.default_step_cases(oracle)
    inp = D.step_inp(S, A)
    out = host_step(shim, p, psi, renorm, inp)
    worst, aside = D.check_step(oracle, p, inp, out, ref, R, psi, renorm, 1e-11, "default parameters (host)")
    assert aside.size == 0                                                 # the host build sets none of the 7500 aside
    order = D.interleave_order(R)
    assert np.array_equal(D.bits(host_step(shim, p, psi, renorm, inp[order])), D.bits(out[order]))
    D.check_pair_drift(inp, out, renorm)                                   # renorm = false carries the pairs' drift on, renorm = true removes it


def test_host_model_step_with_random_parameters(shim, oracle):
    groups = D.random_param_groups(oracle)
    assert len(groups) == 40 and all(len(g[1]) == 30 for g in groups)
    nsubs = [int(round(g[0][18] / g[0][19])) for g in groups]
    assert all(nsubs.count(k) == 5 for k in D.NSUBS)
    dd = np.concatenate([np.abs(D.steer_increment(p, S, A)) for p, S, A, R, ref in groups])
    assert np.sum(dd > D.TINY_ANGLE) >= 20 and np.sum(dd <= D.TINY_ANGLE) >= 20, (np.sum(dd > D.TINY_ANGLE), len(dd))      # both steering-rate classes run
    for psi, renorm in D.VARIANTS:
        worst = 0.0
        for g, (p, S, A, R, ref) in enumerate(groups):
            inp = D.step_inp(S, A)
            w, _ = D.check_step(oracle, p, inp, host_step(shim, p, psi, renorm, inp), ref, R, psi, renorm, 1e-10, "random parameters, group %d (host)" % g, log=lambda s: None)
            worst = max(worst, max(w.values()))
        print("\n[dynamics step] random parameters (host) PSI=%d renorm=%d: worst relative state deviation %.2e" % (psi, renorm, worst))


@pytest.mark.parametrize("psi,renorm", D.VARIANTS)
def test_host_nan_action_poisons_the_state(shim, oracle, psi, renorm):
    S, A, must = D.nan_action_cases(oracle)
    out = host_step(shim, oracle.car_default_params(), psi, renorm, D.step_inp(S, A, eps=0.0))
    assert np.array_equal(np.isnan(out[:, [0, 1, 3, 4, 5]]).any(axis=1), must), out


def test_the_substep_trace_of_the_oracle_ends_at_its_step(oracle):
    """oracle_vx_trace (what shows that a case set aside passes Vx = 0): cutting dt to k sub-steps with the steering command rescaled reproduces the full step
    at k = nsub, and a full brake from a crawl is seen passing zero"""
    p, S, A, R, ref = D.default_step_cases(oracle)
    for i in (0, 1600, 3100, 4700, 6200):
        q = p.copy(); nsub = int(round(p[18] / p[19]))
        tgt = A[i, 0] * p[11] - S[i, 6]
        full = oracle.car_step(q, S[i], [(S[i, 6] + tgt * nsub / nsub) / p[11], A[i, 1]])
        assert np.max(np.abs(full - ref[i]) / np.maximum(1.0, np.abs(ref[i]))) < 1e-13
        assert len(D.oracle_vx_trace(oracle, p, S[i], A[i])) == nsub
    s = np.array([0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.0])
    vx = D.oracle_vx_trace(oracle, p, s, np.array([0.0, -1.0]))
    assert vx[0] > 0 and vx.min() < 0.0


# ================================================================ 3. reward and nearest-point paths ===========================================
@pytest.mark.parametrize("name", list(TRACKS))
def test_anchor_arrangements_reach_their_tiers_and_the_host_meets_the_bounds(shim, oracle, name):
    track = TRACKS[name]
    L = D.reward_lanes(name, track)
    n = len(L["case"])
    assert n % 64 != 0 and L["good"] > 3 * L["poor"]
    nw = (n + 63) // 64
    assert all(len(L["intent"][arr]) == nw for arr in D.ARRANGEMENTS)
    pure = nw if L["poor"] == 0 else -(-L["good"] // 63)                   # the waves made of positions with a certified anchor only: their tier is asserted
    assert pure >= 1 and L["intent"]["a"].count(1) == pure and L["intent"]["c"] == [3] * nw
    if name == "curve":
        assert pure >= 10 and L["intent"]["b"].count(2) == pure and len({s[0] for s in L["seeds"]}) >= 4
    P = len(track[0])
    for arr in D.ARRANGEMENTS:
        a = L["inp"][arr][:, 4]
        assert np.all((a >= -1) & (a < P) & (a == np.floor(a)))
        special = a[::64]
        near = np.array([L["cases"][k]["ex"]["i"] for k in L["case"][::64]])
        if arr == "b" and P >= 5:
            assert np.all(np.minimum((special - near) % P, (near - special) % P) == 2)          # lane 0 of every wave: two ring steps from its nearest point
        if arr == "c":
            assert np.all(special == -1)
    p = oracle.car_default_params()
    outs = {arr: host_reward(shim, p, track, L["inp"][arr]) for arr in D.ARRANGEMENTS}
    D.check_reward_positions(name, track, L, outs, device=False)
    # one lane per wave on the host: the tier of every LANE is its arrangement's
    for arr in D.ARRANGEMENTS:
        o = outs[arr]
        for w, want in enumerate(L["intent"][arr]):
            lanes = o[64 * w:64 * w + 64]
            if want == 1:
                assert np.all(lanes[:, 2] == 1.0)
            elif want == 2:
                assert lanes[0, 2] == 0.0 and np.all(lanes[:, 4] == 1.0)
            elif want == 3:
                assert lanes[0, 2] == 0.0 and lanes[0, 4] == 0.0


def test_exact_ties_are_exact_and_go_to_the_lower_index(shim, oracle):
    track, inp, low = D.tie_cases()
    tx, ty, _ = track
    P = len(tx)
    assert len(inp) % 64 != 0 and len(inp) > 64 and np.all(inp[:, :2] == np.floor(inp[:, :2])) and set(low.tolist()) == set(range(P - 1))     # the pair (P-1, 0) -> 0
    tables = D.ring_tables(track)
    pairs = set()
    for (px, py, _, _, a), lo in zip(inp, low):
        d2 = (tx - px) ** 2 + (ty - py) ** 2                              # integers below 2^53: exact
        tied = np.flatnonzero(d2 == d2.min())
        assert len(tied) == 2 and tied.min() == lo and (tied[1] - tied[0]) in (1, P - 1), (px, py, tied)
        key = [D.fma_exact(ty[i], -2.0 * py, D.fma_exact(tx[i], -2.0 * px, tables[0][i])) for i in tied]
        assert key[0] == key[1] and key[0] == d2.min() - (px * px + py * py)
        m3, _, m5, _, _, _ = D.ring_masks_np(track, tables, int(a), px, py)
        assert not m3 and not m5
        pairs.add(tuple(tied.tolist()))
    assert (0, P - 1) in pairs and len(pairs) == P
    out = host_reward(shim, oracle.car_default_params(), track, inp)
    D.check_ties(inp, out, low)


def test_certificate_boundaries_are_exact_and_strict(shim, oracle):
    track, inp, want = D.boundary_cases()
    tables = D.ring_tables(track)
    assert want.tolist() == [[False, True], [True, True], [False, False], [False, True]]
    for lane, c in ((0, tables[1][0]), (2, tables[2][0])):                # exactly the certificate, and a few ulp below it
        at = 4.0 * D.fma_exact(inp[lane, 0], inp[lane, 0], inp[lane, 1] * inp[lane, 1])
        below = 4.0 * D.fma_exact(inp[lane + 1, 0], inp[lane + 1, 0], inp[lane + 1, 1] * inp[lane + 1, 1])
        assert at == c and below < c and c - below < 1e-13, (at, below, c)
    assert tables[1][0] == 64.0 * (1.0 - 1e-9) and tables[2][0] == 80.0 * (1.0 - 1e-9)
    D.check_boundary(inp, host_reward(shim, oracle.car_default_params(), track, inp), want)


def test_host_slip_and_speed_terms(shim, oracle):
    track = TRACKS["curve"]
    inp, ref = D.slip_cases(oracle, track)
    assert len(inp) % 64 != 0 and np.any(inp[:, 4] == -1) and np.any(inp[:, 4] >= 0)
    D.check_slip(inp, host_reward(shim, oracle.car_default_params(), track, inp), ref)
