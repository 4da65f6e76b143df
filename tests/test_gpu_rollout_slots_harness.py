"""The other half of the rollout code, through the same harness as tests/test_gpu_rollout_harness.py (tools/kbench_rollout.hip, ops ROLLOUT_SLOTS and
BEGIN_SLOTS): the SENV = true twins of mpopis_amd/csrc/kernels_rollout_slots.hip and k_rollout_simple<2 | 4, true>, which take per-slot CarParams / Track
through a SlotEnv, the k_rollout_fleet<NC, LOG, TLDS> kernels of kernels_rollout_fleet.hip (one wave per car, the double-buffered LDS position exchange),
and launch_extend_state / launch_step_begin with slot_tk.  The SlotEnv is the one a handle forms: its LDS sizes come from slot_tracks_lds (engine.h), which
mpopis_set_tracks calls too.  Cases, references and checks are those of tests/helpers/rollout_cases.py, generalised to per-slot and per-car parameters;
tests/test_rollout_cases_cpu.py shows on the CPU that the cases are what they claim and that each checker refuses the corruption it is meant for.  Every
launch asserts the form rollout_form reported against the form restated from the constants in the sources (the largest-track rule, the fleet's TLDS rule).

(h) form: a twin takes the body a shared launch of its shape takes; placement by the LARGEST track of the launch (3 points beside pmax / pmax + 1); the fleet
    always body 6, on both sides of max_tlds_points_fleet(nc) for 2 and 8 cars, with and without traj; a 2048-point track in the launch (the raised limit).
(i) twin parity with simulate_model of slot b's own env at RTOL = 1e-8 (floor 1e-9): 1..8 cars x three bodies, B = 3 with track_of_slot = [2, 0, 1] on
    48, 3 and 12 points, three parameter vectors (one with dt / 5), K over k_edges(nc) (SPB 4: spb4_K), T in {1, 5} (1 and 3 cars: T_FULL), both start-state
    launchers, and a launch with the 240-point track among the three.
(j) fleet parity with car_fleet_ref.fleet_rollout: 2..8 cars, two fleets (graded; reversed at dt / 5), K in {1, 63, 64, 65, 131}, T in {1, 2, 3, 4, 5, 8, 9}
    for 2, 3, 8 cars and {1, 2, 5} otherwise, per-slot tracks in every other launch, one ring-only launch; costs, and in a traj twin of every launch the logged
    trajectories.
(k) the logger step by step (check_logger) for twins of 1 and 3 cars and fleets of 2, 3, 8 in both placements at T = 9, K = 65: every logged state against
    oracle.car_step under THAT car's parameters at 1e-11, none set aside; the cost against the long-double sum of the rewards at the logged states.
(l) exact invariants, bit for bit: twins of 1, 3, 8 cars (two-wave = one-wave, SPB 4 head = SPB 1, slot alone, the slots permuted with their tracks and
    parameters, an inactive middle slot with a valid but different SlotEnv entry, ...), fleets of 2, 3, 5, 8 (column permutation, slot alone, inactive slot,
    iters, (U + d, E - d), zero gvec, cmin, +-inf, NaN containment in car 0 / a middle car / the last car at t = 0, 2, T - 1, the all-NaN key) and the car
    permutation: every car's logged 8 x T block is that of the unpermuted run, the costs within the summation bound.
(m) gamma != 0 (check_gamma) for a 4-car fleet and a 1-car twin.
(n) k_rollout_simple<2 | 4, true> with three parameter vectors per launch against the oracle at 1e-12, a slot whose own step limit ends the episode, NaN.
(o) launch_step_begin / launch_extend_state with slot_tk: the first minimum on the slot's OWN track under designed exact ties, P in {1, 2, 5, 64, 65, 257,
    2048}, 1, 3, 8 cars; the case builder asserts that slot 0's track would give another anchor.
(x) three cross-body comparisons: a twin whose SlotEnv holds copies of the shared env against the shared launch; an equal fleet against the lane-packed
    body; a fleet car's logged trajectory against a one-car logger launch.  Both sides are held to the project bounds against the same oracle reference;
    every test prints whether they are equal bit for bit.  The first run on the MI355X showed identity in all three, which the tests assert since.

Found: no defect.  Measured on the MI355X (every run prints its own; DESIGN.md, "Launch-level tests of the per-slot and fleet rollout kernels", has the same):
(i) worst deviation from the oracle, two-wave = SPB 1 / SPB 4: 1 car 2.3e-15 / 2.7e-15, 2 cars 2.4e-15 / 2.5e-15, 3 cars 3.5e-15 / 4.5e-15, 4 cars 4.0e-15 /
5.4e-15, 5 cars 1.4e-13 / 3.5e-13, 6 cars 6.3e-15 / 9.0e-15, 7 cars 2.2e-15 / 3.3e-15, 8 cars 1.2e-15 / 1.9e-15; (j) costs and logged trajectories, 2..8 cars:
7.4e-11, 3.2e-10, 2.5e-11, 1.9e-10, 2.0e-10, 2.9e-11, 1.9e-10; (k) RATIO LOGGER <= 0.0003, states <= 2.0e-15 per step; (l) RATIO CAR PERMUTATION <= 0.060;
(m) RATIO GAMMA 0.016 (fleet of 4), 0.085 (one-car twin); (n) MountainCar 1.1e-16, CartPole 6.7e-16."""
import os
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import rollout_cases as RC

pytestmark = pytest.mark.gpu
BODIES = (RC.TWO_WAVE, RC.SPB1, RC.SPB4)
same = lambda x, y: np.array_equal(RC.bits(x), RC.bits(y))


@pytest.fixture(scope="module")
def harness():
    return HR.build("rollout")


def _run(exe, tmp_path, launches, env):
    e = dict(os.environ)
    for k in ("MPOPIS_ROLLOUT_DUO", "MPOPIS_COOP_MAX_WG"):
        e.pop(k, None)
    e.update(env)
    res = RC.unpack_result(HR.run_case(exe, tmp_path, RC.pack(launches), env=e), launches)      # checks every guard
    for L, R in zip(launches, res):
        if RC.is_rollout(L):
            RC.check_form(L, R, *RC.env_form_args(env))
    return res


def _duo(body):
    return {"MPOPIS_ROLLOUT_DUO": str(RC.duo_of(body))}


# ================================================================ (h) form ====================================================================
def test_form_of_twins_and_fleets(harness, tmp_path, oracle):
    cases = RC.slot_form_cases()
    c = RC.source_constants()
    seen = set()
    for env in sorted({tuple(sorted(x[2].items())) for x in cases}):
        group = [x for x in cases if tuple(sorted(x[2].items())) == env]
        res = _run(harness, tmp_path, [x[1] for x in group], dict(env))
        for (name, L, _, body), R in zip(group, res):
            RC.check_form(L, R, *RC.env_form_args(dict(env)), want_body=body)
            RC.check_slots(L, R)
            RC.check_parity(oracle, L, R, what=name)
            seen.add(R["form"][:3])
            if "2048" in name:                                               # the raised dynamic-LDS limit: more than the default beside the static part
                assert R["form"][3] == RC.track_lds_bytes(2048, c["kTrackNbrW"], False, c) and R["form"][3] + (RC.fleet_static_lds(8, c) if body == RC.FLEET else 0) > 64 * 1024
    want = {(RC.FLEET, l, t) for l in (True, False) for t in (True, False)} | {(b, False, t) for b in BODIES for t in (True, False)}
    assert want <= seen, want - seen


# ================================================================ (i) twin parity =============================================================
@pytest.mark.parametrize("body", BODIES, ids=["two_wave", "spb1", "spb4"])
@pytest.mark.parametrize("nc", range(1, 9))
def test_twin_parity_with_each_slots_own_oracle_env(harness, tmp_path, oracle, nc, body):
    Ls = RC.twin_parity_launches(nc, body)
    res = _run(harness, tmp_path, Ls, _duo(body))
    worst = 0.0
    for L, R in zip(Ls, res):
        assert R["form"][0] == body, (RC.BODY_NAME[R["form"][0]], RC.BODY_NAME[body])
        RC.check_slots(L, R)
        worst = max(worst, RC.check_parity(oracle, L, R, what="K %d T %d" % (L["K"], L["T"])))
    assert {R["form"][2] for R in res} == {True, False}                  # both table placements
    print("\n[twin parity] %d cars, %s: worst deviation from the oracle %.2e over %d launches (bound %.0e)" % (nc, RC.BODY_NAME[body], worst, len(Ls), RC.RTOL))


# ================================================================ (j) fleet parity ============================================================
@pytest.mark.parametrize("nc", range(2, 9))
def test_fleet_parity_costs_and_logged_trajectories(harness, tmp_path, oracle, nc):
    Ls = RC.fleet_parity_launches(nc)
    both = [M for L in Ls for M in (L, dict(L, traj=True))]
    res = _run(harness, tmp_path, both, {})
    worst, equal = 0.0, True
    for i, L in enumerate(Ls):
        R, Rt = res[2 * i], res[2 * i + 1]
        assert R["form"][:2] == (RC.FLEET, False) and Rt["form"][:2] == (RC.FLEET, True)
        ref = RC.oracle_costs(oracle, L, log=True)                           # once for the pair
        what = "K %d T %d" % (L["K"], L["T"])
        RC.check_slots(L, R); RC.check_slots(both[2 * i + 1], Rt)
        worst = max(worst, RC.check_parity(oracle, L, R, what=what, ref={b: r[0] for b, r in ref.items()}), RC.check_parity(oracle, both[2 * i + 1], Rt, what=what + " logged", ref=ref))
        equal = equal and same(R["cost"], Rt["cost"])
    assert {R["form"][2] for R in res} == {True, False}
    print("\n[fleet parity] %d cars: worst deviation from fleet_rollout %.2e over %d launches x {costs, logged} (bound %.0e); logged costs == unlogged bit for bit: %s" %
          (nc, worst, len(Ls), RC.RTOL, equal))


# ================================================================ (k) the logger, step by step ================================================
@pytest.mark.parametrize("fleet,nc", [(False, 1), (False, 3), (True, 2), (True, 3), (True, 8)], ids=["twin1", "twin3", "fleet2", "fleet3", "fleet8"])
def test_logger_step_by_step_under_each_cars_parameters(harness, tmp_path, oracle, fleet, nc):
    Ls = RC.slot_logger_launches(nc, fleet)
    res = _run(harness, tmp_path, Ls, _duo(RC.SPB1))
    assert [R["form"][:3] for R in res] == [(RC.FLEET if fleet else RC.SPB1, True, True), (RC.FLEET if fleet else RC.SPB1, True, False)]
    print()
    for L, R in zip(Ls, res):
        RC.check_slots(L, R)
        dev, ratio = RC.check_logger(oracle, L, R, what="%d cars" % nc)
        print("RATIO LOGGER %.4f  (%s of %d cars, tables %s: worst state deviation per step %.2e, bound 1e-11)" %
              (ratio, "fleet" if fleet else "twin", nc, "in LDS" if R["form"][2] else "in global memory", dev))


# ================================================================ (l) exact invariants ========================================================
@pytest.mark.parametrize("nc", [1, 3, 8])
def test_twin_invariants_bit_for_bit(harness, tmp_path, nc):
    A, two, notes = RC.twin_invariant_launches(nc)
    RA = dict(zip(A, _run(harness, tmp_path, list(A.values()), _duo(RC.SPB1))))
    RB = dict(zip(two, _run(harness, tmp_path, [A[n] for n in two], _duo(RC.TWO_WAVE))))
    assert RA["base"]["form"][0] == RC.SPB1 and RA["big"]["form"][0] == RC.SPB4 and RA["logged"]["form"][:2] == (RC.SPB1, True)
    assert all(R["form"][0] == RC.TWO_WAVE for R in RB.values())
    assert RC.slot_track(A["base"], 1) is RC.ring_track(3) and A["base"]["active"][1] == 0      # the inactive slot's entry: valid, different (check_slots: nothing of it shows)
    RC.check_invariants(nc, A, RA, RB, two, notes)


@pytest.mark.parametrize("nc", [2, 3, 5, 8])
def test_fleet_invariants_and_the_car_permutation(harness, tmp_path, oracle, nc):
    A, two, notes = RC.fleet_invariant_launches(nc)
    RA = dict(zip(A, _run(harness, tmp_path, list(A.values()), {})))
    assert all(R["form"][0] == RC.FLEET for R in RA.values()) and RA["logged"]["form"][1] and not two
    RC.check_invariants(nc, A, RA, {}, two, notes)
    q = RC.check_car_permutation(oracle, A["logged"], RA["logged"], A["car_perm"], RA["car_perm"], notes["car_perm"])
    print("\nRATIO CAR PERMUTATION %.4f  (%d cars in the order %s: every car's logged block bit for bit, costs within the summation bound)" % (q, nc, list(notes["car_perm"])))


# ================================================================ (m) gamma != 0 ==============================================================
@pytest.mark.parametrize("fleet,nc,body", [(True, 4, RC.FLEET), (False, 1, RC.TWO_WAVE), (False, 1, RC.SPB1)], ids=["fleet4", "twin1_two_wave", "twin1_spb1"])
def test_control_cost_against_long_double(harness, tmp_path, oracle, fleet, nc, body):
    make = (lambda *a, **kw: RC.fleet_launch(*a, **kw)) if fleet else (lambda *a, **kw: RC.slot_launch(*a, params=RC.slot_params3((2,)), **kw))
    L1, L0 = RC.gamma_launches(nc, make=make, S=64 if fleet else None)
    R1, R0 = _run(harness, tmp_path, [L1, L0], _duo(body))
    assert R1["form"][0] == body
    assert RC.check_parity(oracle, L0, R0) < RC.RTOL
    q = RC.check_gamma(oracle, L1, R1, R0)
    print("\nRATIO GAMMA %.4f  (%s of %d cars, %s)" % (q, "fleet" if fleet else "twin", nc, RC.BODY_NAME[body]))
    assert q <= 1.0, q


# ================================================================ (n) the simple envs per slot ================================================
@pytest.mark.parametrize("kind", [RC.ENV_MC, RC.ENV_CP], ids=["mountaincar", "cartpole"])
def test_simple_envs_with_per_slot_parameters(harness, tmp_path, oracle, kind):
    Ls = RC.simple_slot_launches(kind)
    res = _run(harness, tmp_path, Ls, {})
    worst = 0.0
    for L, R in zip(Ls[:-1], res[:-1]):
        assert R["form"][0] == (RC.SIMPLE4 if kind == RC.ENV_CP else RC.SIMPLE2)
        RC.check_slots(L, R)
        e = RC.check_parity(oracle, L, R, what="K %d T %d" % (L["K"], L["T"]))
        assert e < 1e-12, (L["K"], L["T"], e)
        worst = max(worst, e)
    nan = np.isnan(Ls[-1]["E"]).any(axis=1)
    assert np.array_equal(np.isnan(res[-1]["cost"]), nan), "a NaN action must poison its sample's cost and no other"
    assert same(res[-1]["cost"][~nan], res[-2]["cost"][~nan])
    print("\n[rollout simple, per slot] %s: worst deviation from the oracle %.2e over %d launches (bound 1e-12)" % ("cartpole" if kind == RC.ENV_CP else "mountaincar", worst, len(Ls) - 1))


# ================================================================ (o) step begin with slot_tk =================================================
def test_step_begin_anchor_on_the_slots_own_track(harness, tmp_path):
    Ls = RC.begin_slots_launches()
    res = _run(harness, tmp_path, Ls, {})
    for L, R in zip(Ls, res):
        RC.check_begin(L, R)


# ================================================================ (x) three cross-body comparisons ===========================================
def _state_dev(a, b):
    """two logs of the same states: the deviation relative to max(1, |state|), check_logger's metric"""
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def _both_bounds(oracle, L, R, ref=None):
    """One side of a comparison against the oracle, by the project's bounds: the costs at RTOL (check_parity), the logged states step by step at 1e-11
    (check_logger).  The logged states are not taken by check_parity's relative error here: these launches keep car_launch's far-out samples, whose steering
    angle returns through zero, and an angle of 1e-16 carries the rounding of its O(0.1) history (host build and oracle differ by 5.6e-17 there, 5.6e-8 of
    the 1e-9 floor) -- the reason check_logger and dynamics_cases.check_step take a state relative to max(1, |ref|)."""
    dev = RC.check_parity(oracle, dict(L, traj=False), dict(R, traj=None), ref=ref)
    if L["traj"]:
        RC.check_logger(oracle, L, R)
    return dev


@pytest.mark.parametrize("body", [RC.TWO_WAVE, RC.SPB1], ids=["two_wave", "spb1"])
@pytest.mark.parametrize("nc", [1, 3, 8])
def test_twin_with_copies_of_the_shared_env_against_the_shared_launch(harness, tmp_path, oracle, nc, body):
    """Outcome on the MI355X: equal bit for bit (costs, and the logged trajectories of the SPB 1 form), for 1, 3, 8 cars in both bodies -- asserted."""
    S = RC.samples_per_wave(nc)
    Ls = [RC.car_launch(nc, 2, 2 * S + 3, 5, 8000 + nc), RC.car_launch(nc, 2, 2 * S + 3, 5, 8000 + nc, traj=True)]
    Ls += [RC.shared_as_slots(L) for L in Ls]
    res = _run(harness, tmp_path, Ls, _duo(body))
    assert [R["form"][0] for R in res] == [body, RC.SPB1, body, RC.SPB1]
    dev = [_both_bounds(oracle, L, R) for L, R in zip(Ls, res)]                # each side within the project bounds of the same reference
    eq = (same(res[0]["cost"], res[2]["cost"]), same(res[1]["cost"], res[3]["cost"]) and same(res[1]["traj"], res[3]["traj"]))
    print("\n[cross-body 1] %d cars, %s: twin == shared bit for bit: costs %s, logged %s (deviations from the oracle %s)" % (nc, RC.BODY_NAME[body], eq[0], eq[1], ["%.1e" % d for d in dev]))
    assert all(eq), eq


@pytest.mark.parametrize("nc", [2, 3, 8])
def test_equal_fleet_against_the_lane_packed_body(harness, tmp_path, oracle, nc):
    """Outcome on the MI355X: the fleet body with equal vectors gives the lane-packed SPB 1 body's costs, logged costs and logged trajectories bit for bit at
    2, 3 and 8 cars -- asserted since."""
    S = RC.samples_per_wave(nc)
    Ls = [RC.car_launch(nc, 2, 2 * S + 3, 5, 8100 + nc), RC.car_launch(nc, 2, 2 * S + 3, 5, 8100 + nc, traj=True)]
    Ls += [RC.shared_as_slots(L, fleet=True) for L in Ls]
    res = _run(harness, tmp_path, Ls, _duo(RC.SPB1))
    assert [R["form"][0] for R in res] == [RC.SPB1, RC.SPB1, RC.FLEET, RC.FLEET]
    ref = RC.oracle_costs(oracle, Ls[0])                                       # the SAME reference for both sides: simulate_model of the shared env
    dev = [_both_bounds(oracle, L, R, ref=ref) for L, R in zip(Ls, res)]
    eq = (same(res[0]["cost"], res[2]["cost"]), same(res[1]["cost"], res[3]["cost"]), same(res[1]["traj"], res[3]["traj"]))
    worst = (RC.rel_err(res[2]["cost"], res[0]["cost"]), _state_dev(res[3]["traj"], res[1]["traj"]))
    print("\n[cross-body 2] %d cars: equal fleet == lane-packed bit for bit: costs %s, logged costs %s, trajectories %s; worst deviation between the two: costs %.2e, states %.2e (deviations from the oracle %s)" %
          (nc, eq[0], eq[1], eq[2], worst[0], worst[1], ["%.1e" % d for d in dev]))
    assert worst[0] < 2 * RC.RTOL and worst[1] < 2e-11                        # each side within RTOL / 1e-11 of the same reference: the condition written before the first run
    assert all(eq), eq                                                          # the first run showed identity: held from here on


@pytest.mark.parametrize("nc", [2, 3, 8])
def test_fleet_cars_logged_trajectory_against_a_one_car_logger_launch(harness, tmp_path, oracle, nc):
    """Outcome on the MI355X: every car of a graded fleet of 2, 3 and 8 logs, in both slots, bit for bit what a one-car SPB 1 logger launch with that car's
    parameters, bounds, start state and control rows logs -- asserted since."""
    F = RC.fleet_launch(nc, 2, 65, 9, 8200 + nc, traj=True)
    ones = [M for c in range(nc) for M in RC.one_car_of(F, c)]                  # [car][slot]
    res = _run(harness, tmp_path, [F] + ones, _duo(RC.SPB1))
    assert res[0]["form"][:2] == (RC.FLEET, True) and all(R["form"][:2] == (RC.SPB1, True) for R in res[1:])
    _both_bounds(oracle, F, res[0])                                             # the fleet's costs against fleet_rollout, its logged states step by step
    X = res[0]["traj"].reshape(2, 65, nc, 8, 9)
    equal, worst = True, 0.0
    for c in range(nc):
        for b in range(2):
            L1, R1 = ones[2 * c + b], res[1 + 2 * c + b]
            _both_bounds(oracle, L1, R1)                                       # the same per-step reference as the fleet's car: oracle.car_step under that car's parameters
            equal = equal and same(X[b, :, c], R1["traj"][0])
            worst = max(worst, _state_dev(X[b, :, c], R1["traj"][0]))
    print("\n[cross-body 3] %d cars: every fleet car's logged trajectory == the one-car logger launch bit for bit: %s (worst deviation %.2e)" % (nc, equal, worst))
    assert worst < 2e-11                                                        # each side within 1e-11 per state of the same reference: the condition written before the first run
    assert equal                                                                # the first run showed identity: held from here on
