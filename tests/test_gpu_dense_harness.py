"""The dense linear algebra -- kernels_linalg.hip (the four Cholesky kernels behind launch_potrf with the panel copy, launch_chol_solve_gvec,
launch_gvec_from_inv) and kernels_invsqrt.hip (the paired-block triangular-inverse trace with the Lanczos preparation, the one-workgroup and the
cooperative Lanczos inverse square root, the Jacobi fall-back, launch_sym_sqrt) -- exercised directly, below the policy level, through the C++ harness
tools/kbench_dense.hip: one process per launch, inputs written by the test, raw device outputs read back.  tools/kbench_linalg.hip and
tests/test_gpu_linalg_harness.py stay the timing tool and the bit-identity test of the register Cholesky.
The shapes sit on the thresholds of potrf_form (which the harness reports and every Cholesky case asserts), of the LDS kernel's triangle copy and last
diagonal block, of the 256-thread stride of the solves, of the triangular inverse's block pairing and of the cooperative Lanczos (n = 160, column counts
that 8 does not divide).  What the older tool leaves open is covered here: scale per slot, shared and per-slot A and L, inactive slots, nullptr active,
every non-positive-definite placement in all four kernels, the panel copy, y = A^-1/2 b against a reference, and guards behind every output.
References are np.longdouble (tests/helpers/dense_cases.py, where the bounds are derived; tests/test_dense_cases_cpu.py shows on the CPU that inputs and
references are what they claim), never the engine; every stage of a chain is checked against the bits the stage before it left on the device.
MPOPIS_COOP_MAX_WG=64 pins the form selection (never above the device's CU count).

Every check prints `RATIO <op> <output> <worst error / bound>`; DESIGN.md ("kernel-level tests") records the worst per op and output."""
import os
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import dense_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LD = D.LD
KNOBS = ("MPOPIS_POTRF_REG", "MPOPIS_POTRF_G", "MPOPIS_POTRF_S", "MPOPIS_LANCZOS_G", "MPOPIS_COOP_MAX_WG", "MPOPIS_COOP_TEST_DROP", "MPOPIS_COOP_WAIT_US")


@pytest.fixture(scope="module")
def harness():
    return HR.build("dense")


def _run(exe, tmp_path, data, env=None):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e["MPOPIS_COOP_MAX_WG"] = str(D.MAX_WG)
    e.update(env or {})
    return D.unpack_result(HR.run_case(exe, tmp_path, data, env=e))


def _body(a, shape, computed, name, keep=None):
    """guard untouched, slots that are not computed untouched (keep: their values before the launch), no poison left in a computed slot"""
    body, guard = D.split_guard(a, shape)
    assert np.all(D.is_poison(guard)), name + ": guard entries written"
    for b in range(shape[0]):
        if not computed[b]:
            if keep is None:
                assert np.all(D.is_poison(body[b])), "%s: slot %d written" % (name, b)
            else:
                assert np.array_equal(body[b], keep[b]), "%s: slot %d written" % (name, b)
        else:
            assert not np.any(D.is_poison(body[b])), "%s: slot %d keeps %d untouched entries" % (name, b, int(np.sum(D.is_poison(body[b]))))
    return body


def _ratio(op, got, ref, bound, what):
    got = np.atleast_1d(np.asarray(got))
    assert not np.any(np.isnan(got.astype(np.float64))), (what, "NaN")
    err = np.atleast_1d(np.abs(got.astype(LD) - ref))
    bound = np.asarray(bound, dtype=LD) + np.zeros_like(err)
    zero = bound == 0
    assert np.all(err[zero] == 0), (what, "nonzero error where the bound is zero")
    r = float(np.max(np.where(zero, 0, err / np.where(zero, 1, bound)))) if err.size else 0.0
    print("RATIO %s %.4f  (%s)" % (op, r, what))
    assert r <= 1.0, (what, r, float(err.max()))
    return r


def _same_bits(r1, r2, what):
    assert r1[0] == r2[0], what + ": another form"
    for k, (a, b) in enumerate(zip(r1[1], r2[1])):
        assert a.tobytes() == b.tobytes(), "%s: output %d differs" % (what, k)


# ================================================================ POTRF =========================================================================
def _check_factor(c, b, Lflat, what):
    n = c["n"]
    L = D.cm(Lflat, n)
    assert not np.any(D.bits(L[np.triu_indices(n, 1)])), what + ": the strict upper triangle of L is not +0.0"
    err, bound = D.potrf_residual(c["A"][b], c["scale"][b], L)
    _ratio("POTRF L", err, 0, bound, what + " s A - L L'")
    return L


def _check_potrf(c, res, what):
    """every computed slot that should factor: residual, zeros, panel; slots that fail (c['notpd']: slot 0): status, active, guards only"""
    (kernel, G, _), r = res
    n, B = c["n"], c["B"]
    assert (kernel, G) == D.expected_form(c) and kernel == c["expect"], (what, "form", kernel, G, D.expected_form(c))
    fails = np.zeros(B, dtype=bool)
    if c["notpd"]:
        fails[0] = True
    Lb, Lg = D.split_guard(r[0], (B, n * n))
    assert np.all(D.is_poison(Lg)), what + ": guard behind L written"
    pd = D.panel_doubles(n) if c["panel"] else 0
    Pb, Pg = D.split_guard(r[1], (B, pd))
    assert np.all(D.is_poison(Pg)), what + ": guard behind the panel written"
    st, sg = D.split_guard(r[2], (B,))
    act, ag = D.split_guard(r[3], (B,))
    assert np.all(D.is_poison(sg)) and np.all(D.is_poison(ag))
    Ls = {}
    for b in range(B):
        w = "%s slot %d" % (what, b)
        if not c["computed"][b]:
            assert np.all(D.is_poison(Lb[b])) and np.all(D.is_poison(Pb[b])), w + ": inactive slot written"
            assert st[b] == c["status"][b] and act[b] == c["active"][b], w + ": inactive slot's status / active written"
        elif fails[b]:
            assert st[b] == D.status_after(c["status"][b], D.ERR_NOT_PD), (w, "status", st[b], c["status"][b])
            assert act[b] == 0, w + ": active stays set"
        else:
            assert st[b] == c["status"][b] and act[b] == c["active"][b], (w, "status / active changed", st[b], act[b])
            assert not np.any(D.is_poison(Lb[b])), w + ": L keeps untouched entries"
            Ls[b] = _check_factor(c, b, Lb[b], w)
            if pd:
                assert Pb[b].tobytes() == D.panel_of(Ls[b]).tobytes(), w + ": the panel copy is not the factor in the sampler's layout"
    return Ls


@pytest.mark.parametrize("name", [i for i, _ in D.potrf_cases()])
def test_potrf_factor_zeros_and_panel(harness, tmp_path, name):
    """|s A - L L'| componentwise in longdouble on every computed slot, +0.0 above the diagonal bit for bit, the panel copy bit for bit, shared and
    per-slot A, scale absent and 0.25 / 1 / 9, active given (middle slot inactive) and nullptr; the form is the one the shape was written for"""
    c = D.potrf_case(**dict(D.potrf_cases())[name])
    _check_potrf(c, _run(harness, tmp_path, c["data"], c["env"]), name)


@pytest.mark.parametrize("where", D.NOTPD)
@pytest.mark.parametrize("form", sorted(D.FORM_CASES))
def test_potrf_not_positive_definite(harness, tmp_path, form, where):
    """slot 0 fails at a zero first pivot / a negative interior pivot / a negative pivot in the last, partly padded block / a NaN on the diagonal / a NaN
    off the diagonal that reaches a later pivot: MPOPIS_ERR_NOT_PD by the ranks of status_raise, active 0, the other slots factored"""
    c = D.potrf_case(notpd=where, scaled=True, **D.FORM_CASES[form])
    _check_potrf(c, _run(harness, tmp_path, c["data"], c["env"]), "%s %s" % (form, where))


@pytest.mark.parametrize("form", sorted(D.FORM_CASES))
def test_potrf_reads_the_lower_triangle_only(harness, tmp_path, form):
    """1e300 in the strict upper triangle of A changes no bit of L or the panel"""
    c = D.potrf_case(scaled=True, **D.FORM_CASES[form])
    cu = D.potrf_case(scaled=True, upper=True, **D.FORM_CASES[form])
    r = _run(harness, tmp_path, c["data"], c["env"])
    _check_potrf(c, r, form)
    _same_bits(r, _run(harness, tmp_path, cu["data"], cu["env"]), form + " with 1e300 above the diagonal")


@pytest.mark.parametrize("form", sorted(D.FORM_CASES))
def test_potrf_slot_alone_and_again(harness, tmp_path, form):
    """slot 2 of B = 3 and the same slot alone give the same bits; so does a second run"""
    c = D.potrf_case(scaled=True, **D.FORM_CASES[form])
    c1 = D.potrf_case(scaled=True, single=True, **D.FORM_CASES[form])
    r = _run(harness, tmp_path, c["data"], c["env"])
    _same_bits(r, _run(harness, tmp_path, c["data"], c["env"]), form + " second run")
    r1 = _run(harness, tmp_path, c1["data"], c1["env"])
    L3, L1 = _check_potrf(c, r, form), _check_potrf(c1, r1, form + " alone")
    assert L3[2].tobytes() == L1[0].tobytes()
    pd = D.panel_doubles(c["n"]) if c["panel"] else 0
    assert D.split_guard(r[1][1], (3, pd))[0][2].tobytes() == D.split_guard(r1[1][1], (1, pd))[0][0].tobytes()


# ================================================================ SOLVE / GVEC ==================================================================
def _check_solve(c, res):
    n, B = c["n"], c["B"]
    g = _body(res[1][0], (B, n), c["computed"], "g")
    for b in np.flatnonzero(c["computed"]):
        L = c["L"][0 if c["shared"] else b]
        err, bound = D.solve_residual(L, c["gamma"][b], c["U"][b], g[b], c["isc"][b])
        _ratio("SOLVE g", err, 0, bound, "n %d slot %d" % (n, b))
        if c["gamma"][b] == 0:                                        # zeros of either sign: 0 * U is -0.0 where U is negative, as IEEE has it
            assert not np.any(g[b]), "gamma_b = 0 must give exact zeros"
    return g


@pytest.mark.parametrize("n,kind,shared,gps,isc,use_active", D.SOLVE_CASES)
def test_chol_solve_gvec(harness, tmp_path, n, kind, shared, gps, isc, use_active):
    """launch_chol_solve_gvec with the test's factor (random / graded over 8 decades): componentwise residual of the two substitutions; gamma scalar and
    per slot (gamma_b = 0: exact zeros), inv_scale2 absent and given, Lstride 0 and n^2, active given and nullptr"""
    c = D.solve_case(n, kind, shared, gps, isc, use_active)
    g = _check_solve(c, _run(harness, tmp_path, c["data"]))
    if n in (2, 257):
        c1 = D.solve_case(n, kind, shared, gps, isc, use_active, single=True)
        r1 = _run(harness, tmp_path, c1["data"])
        assert _check_solve(c1, r1)[0].tobytes() == g[2].tobytes()
        _same_bits(r1, _run(harness, tmp_path, c1["data"]), "second run")


@pytest.mark.parametrize("n,gps", D.GVEC_CASES)
def test_gvec_from_inv(harness, tmp_path, n, gps):
    """g[j] = sum_i gamma U[i] Sinv[i][j] against longdouble; gamma scalar and per slot (0.35 / 0 / 2: the zero gives zeros); slot 2 alone and a second
    run give the same bits"""
    c = D.gvec_case(n, gps)
    r = _run(harness, tmp_path, c["data"])
    g = _body(r[1][0], (c["B"], n), c["active"], "g")
    for b in range(c["B"]):
        ref, terms = D.gvec_reference(c["S"], c["U"][b], c["gamma"][b])
        _ratio("GVEC g", g[b], ref, D.sum_bound(n, terms), "n %d slot %d" % (n, b))
        if c["gamma"][b] == 0:
            assert not np.any(g[b]), "gamma_b = 0 must give exact zeros"
    if n in (256, 257):
        _same_bits(r, _run(harness, tmp_path, c["data"]), "second run")
        c1 = D.gvec_case(n, gps, single=True)
        g1 = _body(_run(harness, tmp_path, c1["data"])[1][0], (1, n), [1], "g")
        assert g1[0].tobytes() == g[2].tobytes(), "slot 2 of B = 3 and the same slot alone differ"


# ================================================================ TRTRI + prep ==================================================================
def _check_prep(p, part_dev, scale, A, tol, what):
    """one slot's prep[132] against the device's own part bits and A"""
    n = A.shape[0]
    nb = len(part_dev)
    tr = LD(scale) * np.sum(part_dev.astype(LD))
    _ratio("TRTRI prep[0]", p[0], tr, D.sum_bound(nb, abs(LD(scale)) * np.sum(np.abs(part_dev.astype(LD)))), what + " fro")
    cs = np.sum(np.abs(A.astype(LD)), axis=0)
    _ratio("TRTRI prep[1]", p[1], np.max(cs), D.sum_bound(n, np.max(cs)), what + " M")
    mlo = min(1 / LD(p[0]), LD(p[1]) / 2)
    _ratio("TRTRI prep[2]", p[2], mlo, 2 * LD(D.U) * mlo, what + " m")
    assert p[3] == 1.0, what + ": nodes not usable"
    xs = D.quad_xs(p[2], p[1])
    _ratio("TRTRI nodes", D.quad_eval(p[4:68], p[68:132], xs), 0, tol, what + " sum w / (x + s) sqrt(x) - 1")


def _check_trtri(c, res):
    n, B = c["n"], c["B"]
    nb = D.trtri_blocks(n)[0]
    r = res[1]
    part = _body(r[0], (B, nb), c["computed"], "part")
    npp = D.LAN_PREP if c["prep"] else 0
    prep = _body(r[1], (B, npp), c["computed"] if c["prep"] else np.zeros(B, dtype=int), "prep")
    for b in np.flatnonzero(c["computed"]):
        what = "n %d slot %d" % (n, b)
        ref, bound = c["ref"][b]
        _ratio("TRTRI part", part[b], ref, bound, what)
        if c["prep"]:
            _check_prep(prep[b], part[b], c["scale"][b], c["A"][b], c["quad_tol"][b][0], what)
    sy, sg = D.split_guard(r[4], (2 * B,))
    assert np.all(D.is_poison(sg)) and not np.any(sy), "sync2 is not zero again after the launch"
    if c["launches"] == 2:
        assert r[2].tobytes() == r[0].tobytes() and r[3].tobytes() == r[1].tobytes(), "the second launch on the same sync2 gives other bits"
    return part, prep


@pytest.mark.parametrize("n,kind,shared,hiprio,prep,use_active", D.TRTRI_CASES)
def test_trtri_fro_and_prep(harness, tmp_path, n, kind, shared, hiprio, prep, use_active):
    """part[J] against the longdouble sum of squares of block column J of L^-1; with prep: fro, M, m against the device's own part bits and A, the 64
    nodes by what they are for; two launches on one sync2 give the same bits and leave it zero"""
    c = D.trtri_case(n, kind, shared, hiprio, prep, use_active)
    r = _run(harness, tmp_path, c["data"])
    part, pr = _check_trtri(c, r)
    if n in (33, 300) and prep:
        _same_bits(r, _run(harness, tmp_path, c["data"]), "second run")
        c1 = D.trtri_case(n, kind, shared, hiprio, prep, use_active, single=True)
        p1, pr1 = _check_trtri(c1, _run(harness, tmp_path, c1["data"]))
        assert p1[0].tobytes() == part[2].tobytes() and pr1[0].tobytes() == pr[2].tobytes()


# ================================================================ INVSQRT chain =================================================================
def _check_chain(c, res, what, dense=False):
    """L and part as above; prep from part and A; fro = prep[0] bit for bit; -> (y, msteps, status, prep) of the computed slots"""
    (kernel, G, lanG), r = res
    n, B = c["n"], c["B"]
    nb = D.trtri_blocks(n)[0]
    assert (kernel, G) == D.expected_form(c), (what, kernel, G)
    assert lanG == D.lanczos_groups(B, n, c["coop"], c["regions"]), (what, "Lanczos workgroups per matrix", lanG)
    comp = c["computed"]
    Lb = _body(r[0], (B, n * n), comp, "L")
    part = _body(r[1], (B, nb), comp, "part")
    prep = _body(r[2], (B, D.LAN_PREP), comp, "prep")
    y = _body(r[3], (B, n), comp, "y")
    fro = _body(r[4], (B,), comp, "fro")
    ms = _body(r[5], (B,), comp, "msteps")
    st, sg = D.split_guard(r[6], (B,))
    act, ag = D.split_guard(r[7], (B,))
    assert np.all(D.is_poison(sg)) and np.all(D.is_poison(ag)) and np.array_equal(act, c["active"])
    Ls = {}
    for b in np.flatnonzero(comp):
        w = "%s slot %d" % (what, b)
        Ls[b] = _check_factor(c, b, Lb[b], w)
        ref, bound = D.trtri_reference(Ls[b])
        _ratio("INVSQRT part", part[b], ref, bound, w)
        if not dense:
            _check_prep(prep[b], part[b], c["scale"][b], c["A"][b], D.quad_tolerance(prep[b][2], prep[b][1])[0], w)
            assert D.bits(fro[b:b + 1])[0] == D.bits(prep[b][:1])[0], w + ": fro is not prep[0]"
    return dict(L=Ls, part=part, prep=prep, y=y, fro=fro, msteps=ms, status=st)


def _check_y(c, o, b, what):
    ref = D.invsqrt_reference(c, b)
    tol, (t1, t2) = D.invsqrt_tolerance(ref, o["prep"][b][1])
    d = o["y"][b].astype(LD) - ref["y"]
    err = np.sqrt(d @ d)
    print("TERMS %s: 8 x eigh64 %.3e, stopping rule %.3e, ||y|| %.3e, msteps %d" % (what, t1, t2, ref["ny"], o["msteps"][b]))
    _ratio("INVSQRT y", err, 0, tol, what + " ||y - A^-1/2 b||")
    assert 1 <= o["msteps"][b] <= c["n"], (what, "msteps", o["msteps"][b])
    assert o["status"][b] == c["status"][b], (what, "status", o["status"][b])
    return tol


@pytest.mark.parametrize("n,spectra,coop,regions,in_vec,scaled", D.INVSQRT_CASES)
def test_invsqrt_chain(harness, tmp_path, n, spectra, coop, regions, in_vec, scaled):
    """launch_potrf -> launch_trtri_fro (with prep) -> launch_lanczos_invsqrt in one process, every stage against the stage before; y against the
    longdouble A^-1/2 b of a matrix built with a known spectrum; b contiguous and inside CMA's vec (stride 3 n, offset 2 n, poison around it)"""
    c = D.invsqrt_case(n, spectra, coop, regions, in_vec, scaled)
    o = _check_chain(c, _run(harness, tmp_path, c["data"]), "n %d %s" % (n, "/".join(spectra)))
    for b in np.flatnonzero(c["computed"]):
        _check_y(c, o, b, "n %d %s slot %d" % (n, c["spectra"][b], b))


@pytest.mark.parametrize("n,spectra,in_vec,scaled", D.INVSQRT_NOACTIVE)
def test_invsqrt_chain_without_active(harness, tmp_path, n, spectra, in_vec, scaled):
    """active = nullptr in all three launches of the chain (cluster kernels at n = 160 and 300, one workgroup at n = 100): every slot is computed and
    checked, the middle one included"""
    c = D.invsqrt_case(n, spectra, True, True, in_vec, scaled, use_active=False)
    o = _check_chain(c, _run(harness, tmp_path, c["data"]), "n %d without active" % n)
    for b in range(c["B"]):
        _check_y(c, o, b, "n %d %s slot %d without active" % (n, c["spectra"][b], b))


@pytest.mark.parametrize("n,spectra,coop,regions", D.INVSQRT_SOLO)
def test_invsqrt_cooperative_and_one_workgroup_agree(harness, tmp_path, n, spectra, coop, regions):
    """the same case through the cluster kernel and through the one-workgroup kernel (no CoopCtx, or one region per slot): each within the tolerance of
    the reference, the two within twice the tolerance of each other; slot 2 alone and a second run give the same bits"""
    cc, cs = D.invsqrt_case(n, spectra, True, True), D.invsqrt_case(n, spectra, coop, regions)
    rc = _run(harness, tmp_path, cc["data"])
    oc, os_ = _check_chain(cc, rc, "n %d cluster" % n), _check_chain(cs, _run(harness, tmp_path, cs["data"]), "n %d one workgroup" % n)
    for b in np.flatnonzero(cc["computed"]):
        tol = _check_y(cc, oc, b, "n %d cluster slot %d" % (n, b))
        _check_y(cs, os_, b, "n %d one workgroup slot %d" % (n, b))
        d = oc["y"][b].astype(LD) - os_["y"][b].astype(LD)
        _ratio("INVSQRT coop-solo", np.sqrt(d @ d), 0, 2 * tol, "n %d slot %d cluster against one workgroup" % (n, b))
    if n in (160, 300):
        _same_bits(rc, _run(harness, tmp_path, cc["data"]), "second run")
        c1 = D.invsqrt_case(n, spectra, True, True, single=True)
        o1 = _check_chain(c1, _run(harness, tmp_path, c1["data"]), "n %d alone" % n)
        assert o1["y"][0].tobytes() == oc["y"][2].tobytes() and o1["msteps"][0] == oc["msteps"][2]


@pytest.mark.parametrize("n", (17, 100))
def test_invsqrt_one_workgroup_slot_alone_and_again(harness, tmp_path, n):
    c, c1 = D.invsqrt_case(n, ("cluster", "dec4"), scaled=True), D.invsqrt_case(n, ("cluster", "dec4"), scaled=True, single=True)
    r = _run(harness, tmp_path, c["data"])
    _same_bits(r, _run(harness, tmp_path, c["data"]), "second run")
    o, o1 = _check_chain(c, r, "n %d" % n), _check_chain(c1, _run(harness, tmp_path, c1["data"]), "n %d alone" % n)
    assert o1["y"][0].tobytes() == o["y"][2].tobytes() and o1["L"][0].tobytes() == o["L"][2].tobytes()


@pytest.mark.parametrize("n,coop", [(17, False), (300, True)])
def test_invsqrt_zero_b(harness, tmp_path, n, coop):
    """b = 0: y = +0.0 exactly, msteps 0, status untouched; the other slot unaffected"""
    c = D.invsqrt_case(n, ("cluster", "dec4"), coop, True, special="zero_b", status=[D.ERR_NUMERIC, D.OK, D.OK])
    o = _check_chain(c, _run(harness, tmp_path, c["data"]), "n %d b = 0" % n)
    assert not np.any(D.bits(o["y"][0])) and o["msteps"][0] == 0 and o["status"][0] == D.ERR_NUMERIC
    _check_y(c, o, 2, "n %d slot 2 beside b = 0" % n)


@pytest.mark.parametrize("n,coop,before", [(17, False, D.OK), (300, True, D.OK), (17, True, D.ERR_NOT_PD), (300, True, D.ERR_HIP)])
def test_invsqrt_nan_b(harness, tmp_path, n, coop, before):
    """a NaN in b: MPOPIS_ERR_NUMERIC unless a higher-ranked status was there, y = 0, msteps 0"""
    c = D.invsqrt_case(n, ("cluster", "dec4"), coop, True, special="nan_b", status=[before, D.OK, D.OK])
    o = _check_chain(c, _run(harness, tmp_path, c["data"]), "n %d NaN in b" % n)
    assert not np.any(D.bits(o["y"][0])) and o["msteps"][0] == 0 and o["status"][0] == D.status_after(before, D.ERR_NUMERIC)
    _check_y(c, o, 2, "n %d slot 2 beside the NaN" % n)


@pytest.mark.parametrize("n,decades", [(20, 16), (20, 18), (300, 16), (300, 18)])
def test_invsqrt_dense_fallback(harness, tmp_path, n, decades):
    """beyond the quadrature's range: msteps = -1, status 0, and the three identities of test_dense_fallback_beyond_the_quadrature in longdouble from
    the raw outputs, at that test's 1e-9"""
    c = D.dense_case(n, decades)
    o = _check_chain(c, _run(harness, tmp_path, c["data"]), "n %d, %d decades" % (n, decades), dense=True)
    for b in np.flatnonzero(c["computed"]):
        assert o["msteps"][b] == -1 and o["status"][b] == 0 and o["prep"][b][3] == 0.0
        e = D.dense_identities(c["A"][b], o["L"][b], c["b"][b], o["y"][b], o["fro"][b], o["part"][b])
        print("RATIO DENSE %.4f  (n %d %d decades slot %d: y'y %.2e, y'Ay %.2e, trace %.2e against 1e-9)" % (max(e) / 1e-9, n, decades, b, *e))
        assert max(e) < 1e-9, e


# ================================================================ SYM_SQRT ======================================================================
@pytest.mark.parametrize("n,spec", D.SYM_SQRT_CASES)
def test_sym_sqrt(harness, tmp_path, n, spec):
    """launch_sym_sqrt against the longdouble square root of a matrix with a known spectrum: bit-symmetric, Frobenius error within 8 x what the float64
    eigh route misses (floor 2 (n + 8) u ||S||_F)"""
    c = D.sym_sqrt_case(n, spec)
    r = _run(harness, tmp_path, c["data"])
    out = D.cm(_body(r[1][0], (1, n * n), [1], "out")[0], n)
    st, sg = D.split_guard(r[1][1], (1,))
    assert st[0] == 0 and np.all(D.is_poison(sg))
    assert np.array_equal(D.bits(out), D.bits(out.T)), "sqrt(A) is not bit-symmetric"
    S, tol, (t1, t2) = D.sym_sqrt_reference(c)
    d = out.astype(LD) - S
    print("TERMS n %d %s: 8 x eigh64 %.3e, floor %.3e" % (n, spec, t1, t2))
    _ratio("SYM_SQRT out", np.sqrt(np.sum(d * d)), 0, tol, "n %d %s ||out - sqrt(A)||_F" % (n, spec))
    if n == 17:
        _same_bits(r, _run(harness, tmp_path, c["data"]), "second run")


@pytest.mark.parametrize("bad", ("indefinite", "singular"))
@pytest.mark.parametrize("n,before", [(17, D.OK), (100, D.ERR_NUMERIC), (16, D.ERR_HIP)])
def test_sym_sqrt_rejects(harness, tmp_path, n, before, bad):
    """one eigenvalue -1e-3 or exactly 0 (a zero row and column): MPOPIS_ERR_NOT_PD (by rank) and `out` keeps its poison"""
    c = D.sym_sqrt_case(n, "cluster", bad=bad, status=before)
    r = _run(harness, tmp_path, c["data"])
    _body(r[1][0], (1, n * n), [0], "out")
    st, sg = D.split_guard(r[1][1], (1,))
    assert st[0] == D.status_after(before, D.ERR_NOT_PD) and np.all(D.is_poison(sg))
