"""The car model of mpopis_amd/csrc/car_dynamics.h AS THE DEVICE COMPILES IT -- the v_rcp_f64 / v_rsq_f64 seeds with their Newton steps, the inline v_min /
v_max / v_fma forms with their hand-written NaN rule, the wave masks of the ring tiers (__builtin_amdgcn_fcmp / sicmp by predicate code) and the compare
against exec -- exercised directly, one lane per case, through the C++ harness tools/kbench_dynamics.hip: one process per case file, inputs written by
the test, raw device outputs read back; the harness holds no reference arithmetic, poisons every output buffer and gives it guard entries (checked on
every read).  Every launch has 64-lane workgroups and a lane count that is no multiple of 64.  Cases, references and checks are those of
tests/helpers/dynamics_cases.py; tests/test_dynamics_cases_cpu.py shows on the CPU that the cases are what they claim and holds the header's host
build to the same bounds.

1. Primitives against long double / exact rationals, errors in units of the last place of the reference, about 2^16 lanes (log-uniform over the model's
   own ranges + powers of two with both neighbours, mantissas of all ones, 0, NaN): fast_rcp1 <= 19 ulp, fast_rcp <= 1 ulp, fast_sqrt <= 1 ulp (an exact
   0 gives exactly 1e-150, NaN stays NaN), fast_sqrt_rsq: the root has fast_sqrt's bits and the reciprocal is within 1 ulp of 1 / s for the returned s,
   sincos_tiny within 1 ulp on |v| <= 1/32, tire_consts within 2 / 5 / 8 / 14 u relative (operation counts: dynamics_cases.TIRE_BOUND_U), clampd_u /
   clampd_v equal to clampd (NaN comes back NaN), clamp_sym equal to fmax(fmin(v, thr), -thr), fma_v the bits of the correctly rounded fma.
2. One model step against oracle.car_step in the four forms PSI x renorm, on the 5 x 1500 cases of tests/test_dynamics_shim.py at its bounds (1e-11;
   1e-10 under random parameters; cases whose sign(Vx) is decided within rounding of zero set aside, counted, capped, and each shown to pass Vx = 0 in
   the oracle), with (sin, cos) pairs fed 1 + eps off the unit circle; lanes do not influence each other (interleaved = sorted, bit for bit); NaN actions
   poison hot and general lanes.
3. Reward and nearest-point paths against the long-double projection and the oracle's reward under three anchor arrangements that send whole waves
   through the three-point tier, the five-point tier and the general search; mask bits against their definition; exact ties; slip and speed terms.

Not asserted: the sign of a zero result (clamps: -0.0 against a bound of +0.0 and the like compare equal as numbers; the device's v_min / v_max and the
reference's comparisons may pick either zero).

Measured on the MI355X (every run prints its own): fast_rcp1 10.23 ulp, fast_rcp 0.500, fast_sqrt 0.500, fast_sqrt_rsq's 1 / s 0.500, sincos_tiny 0.52 (sin) /
0.70 (cos) ulp; tire_consts 0.99 / 3.29 / 3.62 / 5.74 u; model step 1.4e-15 driving, 2.1e-14 crawling, 2.1e-12 stopped, 1.6e-15 backwards, 2.1e-15 spinning in
all four forms, none set aside, 1.9e-13 under random parameters; distance 1.60 (default track) / 1.52 (3-point ring) / 1.98 (5-point ring) u |p - p1|; reward
1.4e-14 from the oracle's."""
import os
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import dynamics_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TRACKS = {n: t for n, t in D.tracks() if n in ("curve", "ring3", "ring5")}


@pytest.fixture(scope="module")
def harness():
    return HR.build("dynamics", library=False)      # header-only: nothing of the library


def _run(exe, tmp_path, case, op, ns):
    return D.unpack_result(HR.run_case(exe, tmp_path, case), op, ns)     # checks the header (which operation ran, how many launches) and every guard


# ================================================================ 1. primitives ================================================================
@pytest.mark.parametrize("n,lo,hi,seed", [(65536 + 37, -1.0, 1.0, 11), (1501, 0.25, 0.25, 12), (1501, -3.5, 7.0, 13)], ids=["full", "lo_eq_hi", "wide"])
def test_primitives_against_long_double(harness, tmp_path, n, lo, hi, seed):
    """the full input set with the action bounds of the rollout; two short ones for clampd_u's other bounds (lo == hi; bounds that are not symmetric)"""
    inp = D.prim_inputs(n=n, lo=lo, hi=hi, seed=seed)
    out, = _run(harness, tmp_path, D.pack_prims(inp, lo, hi), D.OP_PRIMS, [n])
    print()
    D.check_prims(inp, out, lo, hi, device=True)


# ================================================================ 2. one model step ============================================================
def _step_groups(p, inp):
    return [dict(psi=psi, renorm=renorm, p20=p, bnd=D.ACTION_BOUNDS, inp=inp) for psi, renorm in D.VARIANTS]


def test_model_step_in_the_four_forms_and_lane_independence(harness, tmp_path, oracle):
    """7500 cases x (PSI, renorm) sorted by regime -- whole waves skip the general region -- and interleaved round robin -- every wave holds hot and general
    lanes: each against the oracle's step, and both runs bit for bit the same per case"""
    p, S, A, R, ref = D.default_step_cases(oracle)
    inp = D.step_inp(S, A)
    order = D.interleave_order(R)
    n = len(S)
    assert n % 64 != 0
    outs = _run(harness, tmp_path, D.pack_steps(_step_groups(p, inp) + _step_groups(p, inp[order])), D.OP_STEP, [n] * 8)
    print()
    for v, (psi, renorm) in enumerate(D.VARIANTS):
        worst, aside = D.check_step(oracle, p, inp, outs[v], ref, R, psi, renorm, 1e-11, "default parameters")
        D.check_pair_drift(inp, outs[v], renorm)                           # renorm = false carries the pairs' drift on, renorm = true removes it
        mixed = outs[4 + v]
        bad = np.flatnonzero((D.bits(mixed) != D.bits(outs[v][order])).any(axis=1))
        assert bad.size == 0, ("a lane's result depends on its wave", psi, renorm, order[bad[:5]])


def test_model_step_with_random_parameters(harness, tmp_path, oracle):
    """40 random parameter sets x 30 lanes (6 per regime) x the four forms, one launch each in one process: every sub-step count of 1, 2, 3, 5, 7, 10, 13,
    20 (odd counts end the two-per-trip loop half way), steering increments on both sides of 1/32 rad per sub-step (the library path)"""
    groups = D.random_param_groups(oracle)
    case, ns = [], []
    for p, S, A, R, ref in groups:
        case += _step_groups(p, D.step_inp(S, A)); ns += [len(S)] * 4
    outs = _run(harness, tmp_path, D.pack_steps(case), D.OP_STEP, ns)
    worst = {v: 0.0 for v in D.VARIANTS}
    for g, (p, S, A, R, ref) in enumerate(groups):
        for v, (psi, renorm) in enumerate(D.VARIANTS):
            w, _ = D.check_step(oracle, p, D.step_inp(S, A), outs[4 * g + v], ref, R, psi, renorm, 1e-10, "random parameters, group %d" % g, log=lambda s: None)
            worst[(psi, renorm)] = max(worst[(psi, renorm)], max(w.values()))
    print()
    for (psi, renorm), w in worst.items():
        print("[dynamics step] random parameters PSI=%d renorm=%d: worst relative state deviation %.2e over %d groups" % (psi, renorm, w, len(groups)))


def test_nan_action_poisons_hot_and_general_lanes(harness, tmp_path, oracle):
    S, A, must = D.nan_action_cases(oracle)
    outs = _run(harness, tmp_path, D.pack_steps(_step_groups(oracle.car_default_params(), D.step_inp(S, A, eps=0.0))), D.OP_STEP, [len(S)] * 4)
    for o, (psi, renorm) in zip(outs, D.VARIANTS):
        assert np.array_equal(np.isnan(o[:, [0, 1, 3, 4, 5]]).any(axis=1), must), (psi, renorm, o)


# ================================================================ 3. reward and nearest-point paths ===========================================
@pytest.mark.parametrize("name", list(TRACKS))
def test_reward_paths_under_three_anchor_arrangements(harness, tmp_path, oracle, name):
    """(a) every lane anchored at its nearest point or a ring neighbour, (b) lane 0 of every wave anchored two ring steps away, inside the five-point
    certificate, (c) lane 0 of every wave without an anchor: the waves whose tier the case generator intends (three-point / five-point / general search)
    must report it through their lanes' mask bits; results do not depend on the tier"""
    track = TRACKS[name]
    L = D.reward_lanes(name, track)
    p = oracle.car_default_params()
    outs = {arr: _run(harness, tmp_path, D.pack_reward(p, track, L["inp"][arr]), D.OP_REWARD, [len(L["case"])])[0] for arr in D.ARRANGEMENTS}
    print()
    D.check_reward_positions(name, track, L, outs, device=True)


def test_exact_ties_take_the_general_search_to_the_lower_index(harness, tmp_path, oracle):
    track, inp, low = D.tie_cases()
    out, = _run(harness, tmp_path, D.pack_reward(oracle.car_default_params(), track, inp), D.OP_REWARD, [len(inp)])
    D.check_ties(inp, out, low)
    D.check_wave_masks(out)
    assert D.wave_tiers(out) == [3] * ((len(inp) + 63) // 64)


def test_certificates_are_compared_strictly(harness, tmp_path, oracle):
    """4 |p - q_a|^2 exactly equal to the three-point / five-point certificate: not applicable; a few ulp below it: applicable (a partial wave of 4)"""
    track, inp, want = D.boundary_cases()
    out, = _run(harness, tmp_path, D.pack_reward(oracle.car_default_params(), track, inp), D.OP_REWARD, [len(inp)])
    D.check_boundary(inp, out, want)
    D.check_wave_masks(out)


def test_slip_and_speed_terms_against_the_oracle_reward(harness, tmp_path, oracle):
    track = TRACKS["curve"]
    inp, ref = D.slip_cases(oracle, track)
    out, = _run(harness, tmp_path, D.pack_reward(oracle.car_default_params(), track, inp), D.OP_REWARD, [len(inp)])
    print()
    D.check_slip(inp, out, ref)
    D.check_wave_masks(out)
