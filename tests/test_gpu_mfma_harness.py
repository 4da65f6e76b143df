"""The matrix-core kernels of the AIS loop -- the sampler E = L Z (generic form with 1..7 row groups, the two fused Philox forms), the covariance scatter
(pair list with 64- and 16-column chunks, row form, tall form, the fourth-moment variant; weights from w, from the costs or none; gathered or contiguous
columns; ones-row or external mean) with its finish kernel, the shrinkage kernels, both CE updates and the gather / mean helpers -- exercised directly,
below the policy level, through the C++ harness tools/kbench_mfma.hip: one process per launch, inputs written by the test, raw device outputs read back.
Shapes sit on both sides of every threshold and every scatter case asserts the form wcov_form reported, so a threshold that moves fails a test instead
of dropping a form from coverage.  References are np.longdouble and the oracle (tests/helpers/mfma_cases.py, where the error bounds are derived;
tests/test_mfma_cases_cpu.py shows on the CPU that inputs and references are what they claim), never the engine.  The harness poisons every output:
inactive slots and guard entries must stay untouched and no active entry may keep the poison.

Every check prints `RATIO <op> <worst error / bound>`; DESIGN.md ("kernel-level tests") records the worst per op.
A second run of the same case must give the same bits; that is asserted for every op of the harness and every form of the sampler and the scatter on
chosen cases, not on all of them, to keep the run time of the file down."""
import os
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import mfma_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LD = M.LD


@pytest.fixture(scope="module")
def harness():
    return HR.build("mfma")


def _run(exe, tmp_path, data, env=None):
    e = dict(os.environ)
    e.pop("MPOPIS_WCOV_ROWS", None)
    e.update(env or {})
    return M.unpack_result(HR.run_case(exe, tmp_path, data, env=e))


def _same(r1, r2):
    return r1[0] == r2[0] and len(r1[1]) == len(r2[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(r1[1], r2[1]))


def _body(a, shape, active, name, written=True):
    """guard untouched, inactive slots untouched, and -- when the launch writes this buffer -- no poison and no NaN left in an active slot"""
    body, guard = M.split_guard(a, shape)
    assert np.all(M.is_poison(guard)), name + ": guard entries written"
    for b in range(shape[0]):
        if not active[b] or not written:
            assert np.all(M.is_poison(body[b])), "%s: slot %d written" % (name, b)
        else:
            assert not np.any(M.is_poison(body[b])), "%s: slot %d keeps %d untouched entries" % (name, b, int(np.sum(M.is_poison(body[b]))))
            assert not np.any(np.isnan(body[b])), "%s: slot %d has NaN" % (name, b)
    return body


def _ratio(op, got, ref, bound, what):
    err = np.abs(np.asarray(got).astype(LD) - ref)
    bound = np.asarray(bound, dtype=LD)
    zero = bound == 0
    assert np.all(err[zero] == 0), (what, "nonzero error where the bound is zero")
    r = float(np.max(np.where(zero, 0, err / np.where(zero, 1, bound)))) if err.size else 0.0
    print("RATIO %s %.4f  (%s)" % (op, r, what))
    assert r <= 1.0, (what, r, float(err.max()))
    return r


# ================================================================ sampler ======================================================================
@pytest.mark.parametrize("n,K,shared,osc", M.TRMM_CASES)
def test_sampler_generic_form(harness, tmp_path, n, K, shared, osc):
    """k_trmm_LZ_mfma<false>: 1 .. 7 row groups with balanced tile counts, ragged last tile, K on both sides of the 16-sample wave and the 64-sample workgroup"""
    c = M.trmm_case(n, K, shared=shared, osc=osc)
    r = _run(harness, tmp_path, c["data"])
    E = _body(r[1][0], (c["B"], n, K), c["active"], "E")
    for b in np.flatnonzero(c["active"]):
        ref, bound = M.sampler_reference(c["L"][0 if shared else b], c["Z"][b], c["osc"][b] if osc else None)
        _ratio("TRMM", E[b], ref, bound, "n %d K %d slot %d" % (n, K, b))
    if n in (17, 300, 800):
        assert _same(r, _run(harness, tmp_path, c["data"]))


@pytest.mark.parametrize("n,K", [(17, 65), (129, 65), (300, 17)])
def test_sampler_ignores_the_strict_upper_triangle(harness, tmp_path, n, K):
    """the kernel predicates the entries above the diagonal instead of relying on stored zeros: 1e300 there changes no bit of E"""
    clean = _run(harness, tmp_path, M.trmm_case(n, K)["data"])
    dirty = _run(harness, tmp_path, M.trmm_case(n, K, upper=1e300)["data"])
    assert _same(clean, dirty)


def _fused_outputs(c, r):
    n, K, B = c["n"], c["K"], c["B"]
    nb = 1 if c["shared"] else B
    lact = np.ones(1, dtype=np.int32) if c["shared"] else c["active"]                # the shared factor is made without the slots' flags
    Lc = _body(r[1][0], (nb, n, n), lact, "L")
    L = np.swapaxes(Lc, 1, 2)
    second = r[1][1]
    E = r[1][2]
    for b in np.flatnonzero(lact):
        assert np.all(L[b][np.triu_indices(n, 1)] == 0.0) and np.all(np.diag(L[b]) > 0)
    return L, lact, second, E


@pytest.mark.parametrize("n,K,shared,osc", M.FUSED_CASES)
def test_sampler_fused_form(harness, tmp_path, oracle, n, K, shared, osc):
    """launch_potrf's panel copy + k_trmm_LZ_mfma<true, 112 | 144>: the panel is the factor in the documented layout and zero elsewhere; E = L Z with L the
    factor the device returned and Z the oracle's Philox normals of the slot's stream (sample k draws numbers k n .. k n + n - 1; K beside a multiple
    of 16 draws the clamped sample's counters for the padding lanes, which must not reach E)"""
    c = M.fused_case(M.OP_FUSED, n, K, shared=shared, osc=osc)
    r = _run(harness, tmp_path, c["data"])
    assert r[0] == 1
    L, lact, panel, E = _fused_outputs(c, r)
    pd = M.panel_doubles(n)
    P = _body(panel, (len(lact), pd), lact, "panel")
    for b in np.flatnonzero(lact):
        assert np.array_equal(M.bits(P[b]), M.bits(M.panel_of(L[b]))), "panel differs from the factor"
    E = _body(E, (c["B"], n, K), c["active"], "E")
    for b in np.flatnonzero(c["active"]):
        Z = oracle.philox_normals(int(c["seeds"][b]), c["slo"], c["shi"], n * K).reshape(K, n).T
        ref, bound = M.sampler_reference(L[0 if shared else b], Z, c["osc"][b] if osc else None, fused=True)
        _ratio("FUSED", E[b], ref, bound, "n %d K %d slot %d" % (n, K, b))
    if n in (12, 124):
        assert _same(r, _run(harness, tmp_path, c["data"]))


@pytest.mark.parametrize("n", [102, 132])
def test_sampler_not_fusable_leaves_E_alone(harness, tmp_path, n):
    """4 does not divide 102 (a lane's four rows are one Philox call); 132 rows are nine tiles: the launcher returns false and launches nothing"""
    c = M.fused_case(M.OP_FUSED, n, 64)
    assert not M.fusable(n)
    r = _run(harness, tmp_path, c["data"])
    assert r[0] == 0
    _body(r[1][2], (c["B"], n, 64), c["active"], "E", written=False)


@pytest.mark.parametrize("n,K,shared,osc", [(12, 17, False, False), (100, 100, False, True), (112, 257, True, False), (116, 64, False, False), (128, 100, True, True)])
def test_sampler_fused_equals_the_two_kernel_path(harness, tmp_path, oracle, n, K, shared, osc):
    """launch_sample_normal (the quad kernel: the same counters) + the generic form on the same factor: MFMA slot (q, lk) carries the same column of L and
    the same normal in both paths and the accumulation order is the same, so E agrees bit for bit"""
    cf, ct = M.fused_case(M.OP_FUSED, n, K, shared=shared, osc=osc), M.fused_case(M.OP_TWOKERNEL, n, K, shared=shared, osc=osc)
    rf, rt = _run(harness, tmp_path, cf["data"]), _run(harness, tmp_path, ct["data"])
    if n == 100:
        assert _same(rt, _run(harness, tmp_path, ct["data"]))
    assert rf[0] == 1
    assert rf[1][0].tobytes() == rt[1][0].tobytes()                                   # the same factor
    Z = _body(rt[1][1], (cf["B"], n, K), cf["active"], "Z")
    for b in np.flatnonzero(cf["active"]):
        zo = oracle.philox_normals(int(cf["seeds"][b]), cf["slo"], cf["shi"], n * K).reshape(K, n).T
        assert np.max(np.abs(Z[b] - zo)) <= M.RNG_TOL
    Ef, Et = _body(rf[1][2], (cf["B"], n, K), cf["active"], "E fused"), _body(rt[1][2], (cf["B"], n, K), cf["active"], "E two-kernel")
    assert np.array_equal(M.bits(Ef), M.bits(Et)), int(np.sum(M.bits(Ef) != M.bits(Et)))


# ================================================================ scatter ======================================================================
def _check_wcov(exe, tmp_path, c, env_rows=None, again=False, expect_partial=None):
    env = {"MPOPIS_WCOV_ROWS": str(env_rows)} if env_rows is not None else None
    r = _run(exe, tmp_path, c["data"], env=env)
    partial, sq, aug, from_cost = M.case_form(c, 1 if env_rows is None else env_rows)
    assert r[0] == M.form_code(partial, sq, aug, from_cost), (r[0], partial, sq, aug, from_cost)
    if expect_partial is not None:
        assert partial == expect_partial, (partial, expect_partial)
    B, cs, act = c["B"], c["cs"], c["active"]
    S = _body(r[1][0], (B, cs, cs), act, "S")
    mu = _body(r[1][1], (B, cs), act, "mu_out", written=aug)
    u_all, u_guard = M.split_guard(r[1][2], (B, cs))
    assert np.all(M.is_poison(u_guard))
    cmin = r[1][3]
    tag = "cs %d K %d m %d ksplit %d %s" % (cs, c["K"], c["m"], c["ksplit"], c["variant"])
    for b in range(B):
        key0 = min(M.cost_key(v) for v in c["cost"][b]) if c["cost"] is not None else 0xFFFFFFFFFFFFFFFF
        assert int(cmin[b]) == (0xFFFFFFFFFFFFFFFF if (from_cost and act[b]) else key0), (b, hex(int(cmin[b])))
        if c["u0"] is None:
            assert np.all(M.is_poison(u_all[b]))
        elif not (aug and act[b]):
            assert np.array_equal(M.bits(u_all[b]), M.bits(c["u0"][b])), "u_add changed in slot %d" % b
        if not act[b]:
            continue
        assert np.array_equal(M.bits(S[b]), M.bits(S[b].T)), "S not bitwise symmetric"
        ref = M.wcov_reference(c, b)
        _ratio("WCOV_SQ" if sq else "WCOV", S[b], ref["S"], ref["S_bound"], tag + " S slot %d" % b)
        if aug:
            _ratio("WCOV_MU", mu[b], ref["mu"], ref["mu_bound"], tag + " mu slot %d" % b)
            if c["u0"] is not None:
                assert np.array_equal(M.bits(u_all[b]), M.bits(c["u0"][b] + mu[b])), "u_add != u0 + mu_out"
    if again:
        assert _same(r, _run(exe, tmp_path, c["data"], env=env))
    return r


def _expected_partial(cs):
    return M.WCOV_TALL if cs > 512 else M.WCOV_PAIR64 if cs <= 112 else M.WCOV_PAIR16




@pytest.mark.parametrize("cs", M.WCOV_CS)
def test_scatter_every_row_count(harness, tmp_path, cs):
    """weighted moments as :musigmaaismppi takes them (w with its sum, den = sum w, the mean from the ones row where cs leaves a padding row for it --
    cs & 15 = 0 takes the external mean and must leave mu_out / u_add alone) at K = 257, six splits; cs on both sides of 16, 96 / 97 (seven tiles),
    112 / 113 (64- -> 16-column chunks, the ones row lost at 112), 128 / 129 and 512 / 513 (tall form), and the last rows the staging of each form reaches"""
    c = M.wcov_case(cs, 257, 6, "w_wsum", **M.slots(cs))
    _check_wcov(harness, tmp_path, c, expect_partial=_expected_partial(cs), again=cs in (100, 129, 600))


@pytest.mark.parametrize("cs", range(33, 48))
def test_scatter_ones_row_decode(harness, tmp_path, cs):
    """the finish kernel reads the mean from tile pair (cs >> 4, .) at element (((il & 3) 16 + jl) << 2) + (il >> 2), il = cs & 15: every il = 1 .. 15,
    three row tiles (the mean's tiles are the pairs (2, 0), (2, 1), (2, 2))"""
    _check_wcov(harness, tmp_path, M.wcov_case(cs, 65, 2, "w"), expect_partial=M.WCOV_PAIR64)




@pytest.mark.parametrize("cs", [97, 129, 513])
@pytest.mark.parametrize("K,ksplit", M.WCOV_KSPLITS)
def test_scatter_every_split_count(harness, tmp_path, cs, K, ksplit):
    """K = 64 .. 1000 against 1 .. 32 splits: ranges of one chunk and of many, a ragged last chunk, splits left empty (they must write zero partials) and
    the finish kernel's groups of eight with a clamped tail (ksplit = 1, 5, 8, 9, 32); unweighted, the mean from the ones row, den = K - 1"""
    c = M.wcov_case(cs, K, ksplit, "plain", **M.slots(cs))
    _check_wcov(harness, tmp_path, c, expect_partial=_expected_partial(cs), again=(K, ksplit) in ((257, 32), (1000, 9)))


@pytest.mark.parametrize("cs", [100, 300, 600])
@pytest.mark.parametrize("variant", ["w", "cost"])
def test_scatter_empty_splits(harness, tmp_path, cs, variant):
    """K = 64 in 32 splits: at most four splits hold columns, the rest must contribute exact zeros (the partial workspace starts as NaN)"""
    c = M.wcov_case(cs, 64, 32, variant, **M.slots(cs))
    assert len(M.empty_splits(cs, 64, 32)) >= 28
    _check_wcov(harness, tmp_path, c, expect_partial=_expected_partial(cs), again=True)




@pytest.mark.parametrize("cs", M.VARIANT_CS)
@pytest.mark.parametrize("variant,K,ksplit", M.WEIGHT_SOURCES)
def test_scatter_weight_sources(harness, tmp_path, cs, variant, K, ksplit):
    """pmc: resampled columns made contiguous and shifted by their first one (launch_gather_cols), den = K - 1, the shift added back to mu_out;
    w with / without its sum (the finish kernel adds the weights up itself); weights from the costs with +inf among them (den = 0: sum w from the
    ones row, cmin reset to ~0), once with a single dominant weight.  cs = 112 has no ones row: external mean, no weights from costs, cmin untouched"""
    c = M.wcov_case(cs, K, ksplit, variant, **M.slots(cs))
    _check_wcov(harness, tmp_path, c, expect_partial=_expected_partial(cs), again=variant in ("cost", "pmc") and cs in (100, 513))


def _gathered_mean(exe, tmp_path, c):
    """the external mean as the engine makes it: launch_gather_mean over the case's columns, in a process of its own"""
    g = dict(c, sub=2, X=c["X"])
    data = M.pack_case(M.OP_GATHER, c["B"], [c["cs"], c["K"], c["m"], 2, 1], [], [(M.I32, c["active"]), (M.F64, c["X"]), (M.I32, c["idx"]), (M.F64, None),
                                                                               (M.F64, None), (M.F64, None)])
    r = _run(exe, tmp_path, data)
    mu = _body(r[1][2], (c["B"], c["cs"]), c["active"], "gather_mean")
    for b in np.flatnonzero(c["active"]):
        ref, bound = M.gather_mean_reference(g, b)
        _ratio("GATHER_MEAN", mu[b], ref, bound, "cs %d m %d" % (c["cs"], c["m"]))
    return np.where(c["active"][:, None] == 1, mu, c["mu"])


def _with_mu(c, mu):
    """the case with the device's mean in place of the rounded exact one"""
    op, B, ipar, dpar, arrays = M.unpack_case(c["data"])
    arrays[5] = (M.F64, mu)
    return dict(c, mu=mu, data=M.pack_case(op, B, ipar, dpar, [(t, a if a.size else None) for t, a in arrays]))


@pytest.mark.parametrize("cs", M.VARIANT_CS)
@pytest.mark.parametrize("m,den_is_m,ridge", M.GATHERED)
def test_scatter_gathered_columns(harness, tmp_path, cs, m, den_is_m, ridge):
    """the elite columns of :cemppi: m of K = 257 columns through idx (repeats; at least half of the columns never appear), the external mean from
    launch_gather_mean, den = m or 1, ridge 0 or 10e-9; m = 51 = floor(0.2 K)"""
    c = M.wcov_case(cs, 257, 4, "idx", m=m, den=float(m) if den_is_m else 1.0, ridge=ridge, **M.slots(cs))
    c = _with_mu(c, _gathered_mean(harness, tmp_path, c))
    _check_wcov(harness, tmp_path, c, expect_partial=_expected_partial(cs))


@pytest.mark.parametrize("cs", M.VARIANT_CS)
@pytest.mark.parametrize("variant,m", M.FOURTH)
def test_scatter_fourth_moments(harness, tmp_path, cs, variant, m):
    """SQ: Q_ab = sum_k z_a^2 z_b^2 over the gathered columns, z = (x - mu) rscale with rscale = 1 / sd (:ss) or 1 (:lw); pair list at both chunk widths
    and the tall form"""
    c = M.wcov_case(cs, 257, 6 if cs > 512 else 3, variant, m=m, **M.slots(cs))
    _check_wcov(harness, tmp_path, c, expect_partial=_expected_partial(cs), again=cs == 513)


@pytest.mark.parametrize("cs,ksplit,m,variant", M.ROW_CASES)
def test_scatter_row_form_against_the_reference(harness, tmp_path, cs, ksplit, m, variant):
    """MPOPIS_WCOV_ROWS=2 forces the 8-wave row form at small batches: cs = 97 (the ones row is the first guarded row), 111 (it is the last staged row),
    112 (no ones row: external mean); m not a multiple of 64 leaves the second half of the last workgroup an all-padding half chunk; every weight
    source.  Compared with the longdouble reference, not with the pair-list form."""
    c = M.wcov_case(cs, m, ksplit, variant, B=2, inactive=0)
    _check_wcov(harness, tmp_path, c, env_rows=2, expect_partial=M.WCOV_ROWS, again=m == 65)


@pytest.mark.parametrize("cs,ksplit,variant", M.ROW_GATHERED)
def test_scatter_row_form_gathered(harness, tmp_path, cs, ksplit, variant):
    """819 of 1000 columns through idx (the elite set of K = 4096 scaled down; 319 of the entries repeat a column), external mean, at every (cs, ksplit)
    of the row form's grid; every other point also weighted (w[idx] with their sum given)"""
    c = M.wcov_case(cs, 1000, ksplit, variant, m=819, B=2, inactive=0)
    _check_wcov(harness, tmp_path, c, env_rows=2, expect_partial=M.WCOV_ROWS, again=(cs, ksplit) == (100, 2))


@pytest.mark.parametrize("cs,ksplit,sel_batch,rscale,partial", M.RULE_CASES)
def test_scatter_default_rule_flips_at_its_thresholds(harness, tmp_path, cs, ksplit, sel_batch, rscale, partial):
    """one slot, the batch the choice goes by given as sel_batch: the row form from sel_batch (ksplit / 2) = 192 on, never for an odd split count, the
    compact form (-1), other than seven row tiles or the fourth-moment scatter"""
    c = M.wcov_case(cs, 130, ksplit, "ss" if rscale else "w", m=40 if rscale else None, sel_batch=sel_batch, B=1, inactive=[])
    _check_wcov(harness, tmp_path, c, expect_partial=partial)


@pytest.mark.parametrize("cs,K,ksplit,idx,on", [(100, 1024, 1, False, True), (100, 1025, 1, False, False), (100, 2049, 2, False, False), (100, 2048, 2, False, True),
                                                (129, 1040, 1, False, False), (112, 257, 2, False, False), (100, 257, 2, True, False)])
def test_scatter_from_cost_rule(harness, tmp_path, cs, K, ksplit, idx, on):
    """weights from the costs need a split's weights in LDS (per <= 1024), contiguous columns and the ones row; otherwise the launcher drops the costs,
    takes the weights the caller passed beside them (the engine always does) and leaves cmin alone.  The moments are the same either way."""
    c = M.wcov_case(cs, K, ksplit, "cost_w", B=1, inactive=[])
    if idx:                                                               # idx given: the identity, so that the columns stay what they are
        op, B, ipar, dpar, arrays = M.unpack_case(c["data"])
        arrays[4] = (M.I32, np.arange(K, dtype=np.int32))
        c = dict(c, idx=np.arange(K, dtype=np.int32)[None, :], data=M.pack_case(op, B, ipar, dpar, [(t, a if a.size else None) for t, a in arrays]))
    assert M.case_form(c)[3] == on
    r = _run(harness, tmp_path, c["data"])
    assert r[0] == M.form_code(*M.case_form(c))
    key0 = min(M.cost_key(v) for v in c["cost"][0])
    assert int(r[1][3][0]) == (0xFFFFFFFFFFFFFFFF if on else key0)
    S = _body(r[1][0], (1, cs, cs), c["active"], "S")
    ref = M.wcov_reference(dict(c, w=None) if on else dict(c, cost=None), 0)
    _ratio("WCOV", S[0], ref["S"], ref["S_bound"], "from-cost rule cs %d K %d" % (cs, K))


def test_scatter_without_ones_row_leaves_mean_outputs_alone(harness, tmp_path):
    """cs = 112 with mu_out / u_add asked for: no padding row for the ones, so the launcher hands neither pointer to the finish kernel"""
    c = M.wcov_case(112, 150, 2, "w_wsum", want_mu=True)
    assert c["u0"] is not None and M.case_form(c)[2] is False
    _check_wcov(harness, tmp_path, c)


# ================================================================ shrinkage ====================================================================
def _shrink_run(exe, tmp_path, cs, m, est, S, Q, again=False):
    c = M.shrink_case(cs, m, est, S, Q)
    r = _run(exe, tmp_path, c["data"])
    if again:
        assert _same(r, _run(exe, tmp_path, c["data"]))
    So = np.swapaxes(_body(r[1][0], (3, cs, cs), np.ones(3, dtype=np.int32), "S"), 1, 2)      # (S is uploaded, not poisoned: every slot holds numbers)
    rs, rs_guard = M.split_guard(r[1][1], (3, cs))
    assert np.all(M.is_poison(rs_guard))
    assert np.array_equal(M.bits(So[1]), M.bits(S[1])), "inactive slot's S changed"
    return c, So, rs


@pytest.mark.parametrize("est", ["ss", "lw", "rblw", "oas"])
@pytest.mark.parametrize("cs,m", M.SHRINK_SHAPES)
def test_shrinkage_kernels(harness, tmp_path, oracle, est, cs, m):
    """k_common_shrink / k_inv_sd + k_ss_shrink / k_fill_f64 + k_ss_shrink on the moments of data whose lambda* lies inside (0.05, 0.95) against the oracle's
    cov_*_cols on the data; the intensity's tolerance is the measured float64-vs-longdouble error of the formula (mfma_cases.lam_tolerance)"""
    rng = np.random.default_rng([cs, m, M.EST[est]])
    Xs = [M.elite_data(cs, m, rng) for _ in range(3)]
    mom = [M.moments_for_shrink(X, est) for X in Xs]
    c, So, rs = _shrink_run(harness, tmp_path, cs, m, est, [s for s, _, _ in mom], [q for _, q, _ in mom] if est in ("ss", "lw") else None,
                            again=(cs, m) == (100, 30))
    for b in (0, 2):
        tol_lam, hi = M.lam_tolerance(Xs[b], est)
        assert tol_lam < 1e-10
        ref = oracle.cov_estimate(Xs[b], est)[1].astype(LD) + LD(M.RIDGE) * np.eye(cs)
        assert np.array_equal(M.bits(So[b]), M.bits(So[b].T))
        _ratio("SHRINK", So[b], ref, M.shrunk_tolerance(Xs[b], est, tol_lam, hi), "%s cs %d m %d slot %d" % (est, cs, m, b))
        if est == "ss":
            assert np.all(np.abs(rs[b] * np.sqrt(np.diag(mom[b][0])) - 1.0) <= 4 * 2.0 ** -52)
    if est == "lw":
        assert np.all(rs == 1.0)                                          # launch_fill_f64 takes no active flags: workspace
    elif est == "ss":
        assert np.all(M.is_poison(rs[1]))
    else:
        assert np.all(M.is_poison(rs))


@pytest.mark.parametrize("kind", ["ss_zero", "ss_one", "ss_no_offdiag", "lw_zero", "rblw_one", "oas_one", "rblw_no_spread"])
def test_shrinkage_clamps(harness, tmp_path, kind):
    """lambda* clamped at 0 (fourth moments too small: the raw quotient is negative) and at 1, and the guarded quotients: no off-diagonal mass (:ss) and
    tr(S^2) = tr(S)^2 / p (:rblw) give lambda = 1.  The results are exact: (1 - 0) S, 0 S, and the target"""
    cs, m = 20, 30
    S, Q, est = M.clamp_case(kind, cs, m)
    c, So, rs = _shrink_run(harness, tmp_path, cs, m, est, [S] * 3, None if Q is None else [Q] * 3)
    want = M.clamp_expected(kind, S, M.RIDGE)
    for b in (0, 2):
        assert np.array_equal(So[b], want), (kind, np.max(np.abs(So[b] - want)))


# ================================================================ CE updates ===================================================================
def _check_ce(exe, tmp_path, oracle, op, est, cs, m, K=150):
    c = M.ce_case(op, cs, K, m, est)
    r = _run(exe, tmp_path, c["data"])
    B, act = c["B"], c["active"]
    mu = _body(r[1][0], (B, cs), act, "mu")
    S = _body(r[1][1], (B, cs, cs), act, "S")
    Uo, ug = M.split_guard(r[1][2], (B, cs))
    assert np.all(M.is_poison(ug)) and np.array_equal(M.bits(Uo[1]), M.bits(c["U0"][1]))
    name = "CE_SMALL" if op == M.OP_CE_SMALL else "CE_GENERAL"
    for b in np.flatnonzero(act):
        X = c["E"][b][:, c["order"][b, :m]]
        mean, Sref = oracle.cov_estimate(X, est)
        tol_lam, hi = c["lam"][b]                                         # stored in the case
        Xl = X.astype(LD)
        _ratio(name + "_MU", mu[b], mean.astype(LD), 2 * 4 * (m + 64) * M.U * np.sqrt((Xl * Xl).sum(axis=1) / m), "%s cs %d m %d" % (est, cs, m))
        assert np.array_equal(M.bits(S[b]), M.bits(S[b].T))
        _ratio(name, S[b], Sref.astype(LD) + LD(M.RIDGE) * np.eye(cs), M.shrunk_tolerance(X, est, tol_lam, hi), "%s cs %d m %d slot %d" % (est, cs, m, b))
        assert np.array_equal(M.bits(Uo[b]), M.bits(c["U0"][b] + mu[b])), "U != U0 + mu"
    if (cs, m) in ((100, 30), (128, 64), (129, 30)):                      # a second run: the in-kernel reductions and the split sums are ordered
        assert _same(r, _run(exe, tmp_path, c["data"]))
    return mu, S


@pytest.mark.parametrize("est,cs,m", M.CE_CASES)
def test_ce_small_and_general_against_the_oracle(harness, tmp_path, oracle, est, cs, m):
    """k_ce_cov_small (one launch) and launch_ce_cov_general (gather-mean, scatter -- twice for :ss / :lw --, shrinkage, mean add) on the same elite set,
    each against the oracle's cov_*_cols on the elite columns; pol.U += mu' bit for bit"""
    assert M.ce_small_ok(cs, m)
    _check_ce(harness, tmp_path, oracle, M.OP_CE_SMALL, est, cs, m)
    _check_ce(harness, tmp_path, oracle, M.OP_CE_GENERAL, est, cs, m)


@pytest.mark.parametrize("est", M.ESTS)
@pytest.mark.parametrize("cs,m", M.CE_BEYOND)
def test_ce_general_beyond_the_small_kernel(harness, tmp_path, oracle, est, cs, m):
    assert not M.ce_small_ok(cs, m)
    _check_ce(harness, tmp_path, oracle, M.OP_CE_GENERAL, est, cs, m)


# ================================================================ gather / weighted mean ========================================================
GATHER_KS = (1, 255, 256, 257, 2049)


@pytest.mark.parametrize("K", GATHER_KS)
@pytest.mark.parametrize("shift", [0, 1])
def test_gather_cols(harness, tmp_path, K, shift):
    """Xout = X[:, idx] (minus the first gathered column, stored in shift): copies and one subtraction, so bit for bit"""
    c = M.gather_case(shift, 17, K)
    r = _run(harness, tmp_path, c["data"])
    Xo = _body(r[1][0], (3, 17, K), c["active"], "Xout")
    sh = _body(r[1][1], (3, 17), c["active"], "shift", written=bool(shift))
    _body(r[1][2], (3, 17), c["active"], "mu", written=False)
    for b in (0, 2):
        G = c["X"][b][:, c["idx"][b]]
        first = G[:, :1] if shift else 0.0
        assert np.array_equal(M.bits(Xo[b]), M.bits(G - first))
        if shift:
            assert np.array_equal(M.bits(sh[b]), M.bits(G[:, 0]))
    if K == 2049:
        assert _same(r, _run(harness, tmp_path, c["data"]))


@pytest.mark.parametrize("K,m", [(1, 1), (255, 255), (256, 256), (257, 257), (2049, 2049), (2049, 2048), (257, 30), (2049, 2)])
def test_gather_mean(harness, tmp_path, K, m):
    """eight index -> value round trips in flight per thread: m on both sides of one pass (256 x 8 = 2048) and of the workgroup"""
    c = M.gather_case(2, 17, K, m=m)
    r = _run(harness, tmp_path, c["data"])
    mu = _body(r[1][2], (3, 17), c["active"], "mu")
    _body(r[1][0], (3, 17, K), c["active"], "Xout", written=False)
    for b in (0, 2):
        ref, bound = M.gather_mean_reference(c, b)
        _ratio("GATHER_MEAN", mu[b], ref, bound, "K %d m %d slot %d" % (K, m, b))
    if K == 2049:
        assert _same(r, _run(harness, tmp_path, c["data"]))


@pytest.mark.parametrize("K", [1, 2, 255, 256, 257, 2049, 2050])
@pytest.mark.parametrize("normalize,shift_pair", M.WMEAN_MODES)
def test_wmean(harness, tmp_path, K, normalize, shift_pair):
    """k_wmean: 16-byte loads for even K, scalar ones for odd K; normalised or not; with and without the shift pair"""
    c = M.gather_case(3, 17, K, normalize=normalize, shift_pair=shift_pair)
    r = _run(harness, tmp_path, c["data"])
    mu = _body(r[1][2], (3, 17), c["active"], "mu")
    for b in (0, 2):
        ref, bound = M.wmean_reference(c, b)
        _ratio("WMEAN", mu[b], ref, bound, "K %d normalize %d shift %d slot %d" % (K, normalize, shift_pair, b))
    if K in (257, 2050):
        assert _same(r, _run(harness, tmp_path, c["data"]))
