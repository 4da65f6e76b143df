"""Inputs, file format, host-side rules, references and bounds for the direct tests of the dense linear algebra (tools/kbench_dense.hip:
kernels_linalg.hip and kernels_invsqrt.hip): shared by tests/test_dense_cases_cpu.py (which proves on the CPU that inputs, references and intended
edges are what they claim) and tests/test_gpu_dense_harness.py.  Nothing here touches the engine.  References are np.longdouble evaluations of the
exact float64 inputs.  The bounds are derived, not measured (u = 2^-53):

  Cholesky          |s A - L L'| <= 2 (n + 8) u |L||L'| + u |s A| componentwise on the lower triangle.  gamma_{n+1} |L||L'| is Higham's bound (Accuracy
                    and Stability, thm 10.3) for any order of the sums, with or without FMA; the + 8 covers the diagonal block's rsqrt + Newton step
                    (<= 2 ulp, rescales a column consistently) and the 4x4 inverses of the blocked substitution, the factor 2 the second-order terms and
                    the reference's own rounding.  u |s A| is the rounding of sc * a at copy-in.
  triangular solves |L L' x - gamma U| <= 2 (2 n + 8) u |L||L'||x| + 4 u |gamma U| with x = g s2: forward and backward substitution are each backward
                    stable with n u |L| per factor; gamma U, the division by s2 (a reciprocal and a product) are the four roundings of the second term.
  sums of products  2 (n + 8) u sum|terms| (tests/helpers/adapt_cases.py).
  trace of L^-1     X = L^-1 by longdouble forward substitution; the device's X' satisfies |X' - X| <= dX = 2 (n + 2) u |X||L||X| (the residual bound
                    |L X' - I| <= 2 (n + 2) u |L||X'| of adapt_cases.py, multiplied by |X| = |L^-1|); a block column's sum of squares then moves by at most
                    sum 2 |X| dX, plus 2 (c + 8) u sum X^2 for the c-term sum itself.
  quadrature nodes  sum_j w_j / (x + s_j) against x^-1/2, relative, at 200 log-spaced x of [m, M]: 8 x the largest difference between a float64 and a
                    longdouble evaluation of the formulas of invsqrt_quad.h at the same (m, M), floor 64 u (the quadrature's own truncation error is
                    below 1e-15 up to M / m = 1e12 and the device uses its own sin / asin).
  A^-1/2 b          normwise: max(8 ||y_eigh64 - y_ref||, 2 kLanTol ||b|| / sqrt(M)): what the reference's eigen-based Sigma^-0.5 itself misses in
                    float64, and the kernel's own stopping rule (error bound <= kLanTol / sqrt(M) per unit ||b||) doubled.
  sqrt(A)           Frobenius: max(8 ||S_eigh64 - S_ref||_F, 2 (n + 8) u ||S||_F).

Matrices with a known function (spd_with_function): A = fl64(Q diag(lam) Q'), Q a product of six Householder reflectors in longdouble.  With
dA = A - Q diag(lam) Q' (longdouble), f(A) = Q f(lam) Q' + Q (F o (Q' dA Q)) Q' to first order, F the divided differences of f -- for x^-1/2:
F_ij = -1 / (sqrt(l_i) sqrt(l_j) (sqrt(l_i) + sqrt(l_j))), for x^1/2: 1 / (sqrt(l_i) + sqrt(l_j)), neither with a cancellation; the remainder is
second order, (kappa u)^2.  NumPy has no longdouble eigen-solver; this needs none.  The CPU file certifies each reference: Y symmetric positive
definite with Y A Y = I to 1 / 100 of the case's tolerance (the SPD solution of Y A Y = I is unique)."""
import functools
import numpy as np
from tests.helpers import harness_io as IO
from tests.helpers.harness_io import U64, is_poison                   # (re-exported)
from tests.helpers.adapt_cases import (LD, U, F64, I32, GUARD, POISON_I32, POISON_F64, POISON_F64_BITS, OK, ERR_ARG, ERR_NOT_PD, ERR_ACTION, ERR_HIP,
                                       ERR_NUMERIC, bits, split_guard, cm, to_cm, sum_bound, status_rank, actives, potri_factor, potri_reference)

MAGIC_IN, MAGIC_OUT = b"DNSCASE1", b"DNSRES01"
OP_POTRF, OP_SOLVE, OP_GVEC, OP_TRTRI, OP_INVSQRT, OP_SYM_SQRT = range(6)
POTRF_LDS, POTRF_REG, POTRF_COOP, POTRF_GLOBAL = range(4)
FORM_NAMES = ("lds", "reg", "coop", "global")
# kernels_linalg.hip / linalg_diag.h / engine.h / kernels_invsqrt.hip (tests/test_dense_cases_cpu.py reads them back from the sources)
NB, PANEL_ROWS, REG_MIN_PAN, REG_MAX_PAN, COOP_MAX_OWN, COOP_PS, LDS_LIMIT, POTRF_G = 16, 128, 16, 19, 16, 17, 150 * 1024, 6
LAN_TOL, LAN_G, LAN_MIN_N, LAN_RED, LAN_PIV_LDS, LAN_PREP, TRI_B = 1e-13, 8, 160, 36, 16, 132, 16
MAX_WG = 64                                                # MPOPIS_COOP_MAX_WG of every harness run (never above the device's CU count)
SCALES = np.array([0.25, 1.0, 9.0])


# ---- the harness's files ---------------------------------------------------------------------------------------------------------------------
def pack_case(op, B, ipar, dpar, arrays):
    return IO.pack_case(MAGIC_IN, op, B, ipar, dpar, arrays)


def unpack_case(buf):
    return IO.unpack_case(MAGIC_IN, buf)


def pack_result(form, arrays):
    return IO.pack_result(MAGIC_OUT, form, arrays)


def unpack_result(buf):
    """-> (form = (Cholesky kernel, its G, Lanczos workgroups per matrix), [arrays as written, guard entries included])"""
    form, arrays = IO.unpack_result(MAGIC_OUT, buf)
    return (form & 255, (form >> 8) & 255, (form >> 16) & 255), arrays


# ---- host rules (restated from the launchers) ---------------------------------------------------------------------------------------------------
def coop_ld(rows):
    return rows if rows & 31 else rows + 16


def potrf_form(B, n, coop=True, reg=True, G=POTRF_G, max_wg=MAX_WG):
    """potrf_form of kernels_linalg.hip -> (kernel, G); reg: MPOPIS_POTRF_REG, G: MPOPIS_POTRF_G, max_wg: MPOPIS_COOP_MAX_WG"""
    npad = (n + NB - 1) // NB * NB
    npan = npad // NB
    if npad * npad * 8 <= LDS_LIMIT:
        return POTRF_LDS, 0
    if reg and REG_MIN_PAN <= npan <= REG_MAX_PAN:
        return POTRF_REG, 0
    G = min(G, npan)
    if G >= 2 and coop:
        own = [coop_ld(npad - c * NB) * NB for c in range(0, npan, G)]
        lds = (sum(own) + npad * COOP_PS) * 8
        if lds <= LDS_LIMIT and len(own) <= COOP_MAX_OWN and B * G <= max_wg:
            return POTRF_COOP, G
    return POTRF_GLOBAL, 0


def lds_edges(n):
    """k_potrf_lds at order n -> (npad, 64-entry chunks of a column pair's triangle copy, sub-block rounds of the last diagonal block)"""
    npad = (n + NB - 1) // NB * NB
    return npad, (npad + 1 + 63) // 64, min(4, (n - (npad - NB) + 3) // 4)


def lanczos_groups(B, n, coop=True, regions=True, max_wg=MAX_WG):
    """workgroups per matrix launch_lanczos_invsqrt uses (invsqrt_coop_groups, capped by the regions the caller allocated)"""
    G = LAN_G
    if not coop or not regions or n < LAN_MIN_N or n > 1000 or B * G > max_wg:
        return 1
    fixed = 6 * n + 1 + LAN_RED + 2 * LAN_PIV_LDS * 64 + (n + G - 1) // G * n
    return G if (fixed + 4 * n) * 8 <= LDS_LIMIT else 1


def trtri_blocks(n):
    """-> (block columns nb, workgroups per slot, whether the middle block column pairs with itself, rows of the last block)"""
    nb = (n + TRI_B - 1) // TRI_B
    return nb, (nb + 1) // 2, nb % 2 == 1, n - (nb - 1) * TRI_B


# ================================================================ matrices ======================================================================
def cma_like(n, seed):
    """tools/kbench_linalg.hip's family: two-eigenvalue diagonal + six rank-one terms + a constant on every entry (entries O(0.1), cond ~ 2)"""
    rng = np.random.default_rng([seed, n, 1])
    a = np.diag(np.where(np.arange(n) % 2 == 1, 0.1, 0.0625))
    for _ in range(6):
        p = 0.05 * rng.standard_normal(n)
        a = 0.99 * a + 1e-3 * np.outer(p, p) + 2e-5
    return 0.5 * (a + a.T)


def graded(n, seed, decades=8.0):
    """D H D with H the CMA-like matrix and variances graded over `decades` decades (scaled diagonally dominant: numerically SPD)"""
    d = 10.0 ** (-0.5 * decades * np.arange(n) / max(n - 1.0, 1.0))
    a = cma_like(n, seed) * d[:, None] * d[None, :]
    return 0.5 * (a + a.T)


def spd(n, kind, seed):
    return cma_like(n, seed) if kind == "cma" else graded(n, seed, 8.0)


# ================================================================ POTRF =========================================================================
NOTPD = ("first", "interior", "last", "nan_diag", "nan_off")
# the status the failing slot holds before the launch, per placement: NOT_PD replaces OK and NUMERIC, never HIP / ACTION / ARG (status_raise)
NOTPD_STATUS = dict(first=OK, interior=ERR_NUMERIC, last=ERR_HIP, nan_diag=ERR_ACTION, nan_off=OK)


def notpd_position(n, where):
    """-> (row of the first pivot that fails, (i, j) of the entry that is changed)"""
    npan = (n + NB - 1) // NB
    if where == "first":
        return 0, (0, 0)                                               # an exactly zero first pivot: the edge of !(piv > 0)
    if where == "last":
        return n - 1, (n - 1, n - 1)
    p = NB * (npan // 2) + 7 if npan > 2 else min(n - 1, NB + 3 if npan == 2 else 7)
    p = min(p, n - 1)
    if where == "nan_off":
        return p, (p, max(0, p - NB - 2) if p > NB + 2 else 0)         # an earlier block column's entry of row p
    return p, (p, p)


def make_notpd(A, where):
    n = A.shape[0]
    A = A.copy()
    p, (i, j) = notpd_position(n, where)
    if where == "first":
        A[0, 0] = 0.0
    elif where in ("interior", "last"):
        A[i, i] = -1e-3 * A[i, i]
    elif where == "nan_diag":
        A[i, i] = np.nan
    else:
        if i == j:                                                      # n = 1 has no off-diagonal entry
            A[i, i] = np.nan
        else:
            A[i, j] = A[j, i] = np.nan
    return A


def potrf_case(n, kind="cma", shared=False, scaled=False, use_active=True, coop=True, panel=None, B=3, single=False, notpd=None, upper=False,
               env=None, expect=None):
    """launch_potrf.  B = 3 with the middle slot inactive (use_active False: nullptr, every slot is factored); single: slot 2 alone.  scaled: scale[b] =
    0.25 / 1 / 9.  notpd: slot 0's matrix fails at that placement (per-slot A only).  upper: 1e300 in the strict upper triangle of every input.
    env: the knobs of the harness process beyond MPOPIS_COOP_MAX_WG; expect: the form the case was written for"""
    ids = [2] if single else list(range(B))
    Bc = len(ids)
    panel = (n <= PANEL_ROWS) if panel is None else (panel and n <= PANEL_ROWS)
    mats = [spd(n, kind, 40 + (0 if shared else i)) for i in ids]
    if notpd:
        assert not shared and not single and use_active
        mats[0] = make_notpd(mats[0], notpd)
    A_in = [np.tril(m) + np.triu(np.full((n, n), 1e300), 1) for m in mats] if upper else mats
    scale = SCALES[ids] if scaled else None
    active = actives(Bc, None if single or not use_active or Bc < 3 else 1)
    status = np.array([(OK, ERR_NUMERIC, ERR_NUMERIC)[i] for i in ids], dtype=np.int32)
    if notpd:
        status[0] = NOTPD_STATUS[notpd]
    computed = active.copy() if use_active else np.ones(Bc, dtype=np.int32)
    arrA = np.array([to_cm(a) for a in (A_in[:1] if shared else A_in)])
    return dict(n=n, kind=kind, B=Bc, A=mats, scale=scale if scaled else np.ones(Bc), shared=shared, scaled=scaled, use_active=use_active, coop=coop, panel=panel,
                active=active, status=status, computed=computed, notpd=notpd, upper=upper, env=dict(env or {}), expect=expect,
                data=pack_case(OP_POTRF, Bc, [n, 0 if shared else n * n, int(use_active), int(coop), int(panel)], [],
                               [(I32, active), (F64, arrA), (F64, scale), (I32, status)]))


def potrf_residual(A, s, L):
    """|s A - L L'| and its bound on the lower triangle, longdouble"""
    n = A.shape[0]
    Ll, sA = L.astype(LD), LD(s) * A.astype(LD)
    err = np.abs(sA - Ll @ Ll.T)
    bound = 2 * (n + 8) * LD(U) * (np.abs(Ll) @ np.abs(Ll).T) + LD(U) * np.abs(sA)
    il = np.tril_indices(n)
    return err[il], bound[il]


def panel_doubles(n):
    return (n + 15) // 16 * 16 * PANEL_ROWS if n <= PANEL_ROWS else 0


def panel_of(L):
    """the factor in the fused sampler's staging layout, as the comment on k_potrf_lds states it: [j / 16][(j & 3) 4 + ((j & 15) >> 2)][i < 128],
    +0.0 above the diagonal and beyond n"""
    n = L.shape[0]
    P = np.zeros(((n + 15) // 16, 16, PANEL_ROWS))
    for j in range(n):
        P[j // 16, (j & 3) * 4 + ((j & 15) >> 2), j:n] = L[j:, j]
    return P.reshape(-1)


def status_after(before, code):
    return code if status_rank(code) > status_rank(before) else before


# the shapes by the thresholds of potrf_form (the CPU file recomputes the form each reaches)
POTRF_LDS_NS = (1, 3, 4, 5, 12, 13, 16, 17, 48, 64, 65, 100, 113, 127, 128)
POTRF_COOP_NS = (129, 144, 145, 240, 305, 320, 400)                      # no knob: whatever potrf_form says beyond the register band (400: LDS rules clusters out)
POTRF_REG_NS = (241, 256, 257, 288, 289, 300, 304)
POTRF_GLOBAL_NS = (129, 145, 300, 305, 400)
GLOBAL_WAYS = {"noctx": dict(coop=False, env={"MPOPIS_POTRF_REG": "0"}, B=3),
               "g0": dict(coop=True, env={"MPOPIS_POTRF_REG": "0", "MPOPIS_POTRF_G": "0"}, B=3),
               "cap8": dict(coop=True, env={"MPOPIS_POTRF_REG": "0", "MPOPIS_COOP_MAX_WG": "8"}, B=2)}
REG_BAND_COOP_NS = (241, 300, 304)                                       # the cluster kernel inside the register band (MPOPIS_POTRF_REG=0)


def expected_form(c):
    """the form the harness process of POTRF / INVSQRT case c must report, from its knobs"""
    e = c["env"]
    return potrf_form(c["B"], c["n"], coop=c["coop"], reg=e.get("MPOPIS_POTRF_REG", "1") != "0", G=int(e.get("MPOPIS_POTRF_G", POTRF_G)),
                      max_wg=int(e.get("MPOPIS_COOP_MAX_WG", MAX_WG)))


def _variant(i, n):
    """rotates kind / stride / scale / active over a shape list so that every option meets every form"""
    return dict(kind=("cma", "graded")[i % 2], shared=i % 3 == 1, scaled=i % 2 == 0 or n in (100, 300), use_active=i % 4 != 3)


def potrf_cases():
    """-> list of (id, kwargs of potrf_case)"""
    out = []
    for i, n in enumerate(POTRF_LDS_NS):
        out.append(("lds-%d" % n, dict(n=n, expect=POTRF_LDS, panel=i % 5 != 4, **_variant(i, n))))
    for i, n in enumerate(POTRF_COOP_NS):
        out.append(("coop-%d" % n, dict(n=n, expect=potrf_form(3, n)[0], **_variant(i, n))))
    for i, n in enumerate(REG_BAND_COOP_NS):
        out.append(("coop-regoff-%d" % n, dict(n=n, expect=POTRF_COOP, env={"MPOPIS_POTRF_REG": "0"}, **_variant(i + 1, n))))
    for i, n in enumerate(POTRF_REG_NS):
        out.append(("reg-%d" % n, dict(n=n, expect=POTRF_REG, **_variant(i, n))))
    for i, n in enumerate(POTRF_GLOBAL_NS):
        for k, (way, w) in enumerate(GLOBAL_WAYS.items()):
            out.append(("global-%s-%d" % (way, n), dict(n=n, expect=POTRF_GLOBAL, coop=w["coop"], env=w["env"], B=w["B"], **_variant(i + k, n))))
    return out


# one n per form for the not-PD placements, the 1e300 upper triangle, slot 2 alone and the second run
FORM_CASES = {"lds": dict(n=100, expect=POTRF_LDS), "coop": dict(n=145, expect=POTRF_COOP), "reg": dict(n=300, expect=POTRF_REG),
              "global": dict(n=145, expect=POTRF_GLOBAL, coop=False)}


# ================================================================ SOLVE / GVEC ==================================================================
SOLVE_NS = (1, 2, 255, 256, 257, 300)
# (n, factor kind, shared factor, per-slot gamma, inv_scale2 given, active given)
SOLVE_CASES = [(1, "random", False, False, False, True), (1, "graded", True, True, True, False), (2, "graded", False, True, False, True),
               (2, "random", True, False, True, True), (255, "random", False, True, True, True), (255, "graded", True, False, False, False),
               (256, "graded", False, False, True, True), (256, "random", True, True, False, True), (257, "random", True, False, True, True),
               (257, "graded", False, True, False, False), (300, "graded", False, True, True, True), (300, "random", True, False, False, True)]
GVEC_CASES = [(n, i % 2 == 0) for i, n in enumerate(SOLVE_NS)] + [(257, False), (300, True)]
GVEC_GAMMAS = np.array([0.35, 0.0, 2.0])                                  # no slot is inactive there: the zero sits in the middle, slot 2 is compared with itself alone
GAMMAS = np.array([0.35, 2.0, 0.0])                                       # per-slot: the last slot's gamma_b = 0 must give exact zeros
INV_SCALE2 = np.array([0.49, 1.0, 3.61])


def solve_case(n, kind, shared, gamma_per_slot, with_isc, use_active, single=False):
    """launch_chol_solve_gvec with the test's factor.  B = 3 with the middle slot inactive; per-slot gamma = 0.35 / 2 / 0"""
    ids = [2] if single else [0, 1, 2]
    B = len(ids)
    L = np.array([potri_factor(n, kind, 21 + i) for i in ([0] if shared else ids)])
    Uo = np.array([np.random.default_rng([77, n, i]).standard_normal(n) for i in ids])
    gam = GAMMAS[ids] if gamma_per_slot else np.full(B, 0.8)
    isc = INV_SCALE2[ids] if with_isc else np.ones(B)
    active = actives(B, None if single else 1)
    computed = active if use_active else np.ones(B, dtype=np.int32)
    return dict(n=n, B=B, L=L, U=Uo, gamma=gam, isc=isc, shared=shared, active=active, computed=computed, with_isc=with_isc,
                data=pack_case(OP_SOLVE, B, [n, 0 if shared else n * n, int(use_active)], [0.8],
                               [(I32, active), (F64, np.array([to_cm(x) for x in L])), (F64, Uo), (F64, gam if gamma_per_slot else None),
                                (F64, isc if with_isc else None)]))


def solve_residual(L, gU_gamma, Uo, g, s2):
    """|L L' (g s2) - gamma U| and its bound, longdouble"""
    n = L.shape[0]
    Ll, x = L.astype(LD), g.astype(LD) * LD(s2)
    rhs = LD(gU_gamma) * Uo.astype(LD)
    err = np.abs(Ll @ (Ll.T @ x) - rhs)
    bound = 2 * (2 * n + 8) * LD(U) * (np.abs(Ll) @ (np.abs(Ll).T @ np.abs(x))) + 4 * LD(U) * np.abs(rhs)
    return err, bound


def gvec_case(n, gamma_per_slot, single=False):
    """launch_gvec_from_inv: one Sigma^-1 for the call (a general matrix serves: the kernel reads S[i][j] as stored), B = 3, no `active`;
    per-slot gamma = 0.35 / 0 / 2; single: slot 2 alone"""
    ids = [2] if single else [0, 1, 2]
    B = len(ids)
    rng = np.random.default_rng([55, n])
    S = rng.standard_normal((n, n)) * (0.5 + rng.random((n, 1)))
    Uo = rng.standard_normal((3, n))[ids]
    gam = GVEC_GAMMAS[ids] if gamma_per_slot else np.full(B, 0.8)
    return dict(n=n, B=B, S=S, U=Uo, gamma=gam, active=actives(B, None),
                data=pack_case(OP_GVEC, B, [n], [0.8], [(I32, actives(B, None)), (F64, to_cm(S)), (F64, Uo), (F64, gam if gamma_per_slot else None)]))


def gvec_reference(S, Uo, gamma):
    Sl, ul = S.astype(LD), LD(gamma) * Uo.astype(LD)
    return ul @ Sl, np.abs(ul) @ np.abs(Sl)


# ================================================================ quadrature ====================================================================
def quad_nodes(m, M, dtype, N=64):
    """the N nodes of invsqrt_quad.h for [m, M], every operation in `dtype` (np.float64: what the header does on the host; LD: the same formulas)"""
    T = dtype
    m, M = T(m), T(M)
    k2 = m / M
    assert 1e-14 < k2 <= 0.75
    a, c = [T(1)], [np.sqrt(T(1) - k2)]
    b = np.sqrt(k2)
    n = 0
    while abs(c[n]) > T(1e-17) * a[n] and n < 16:
        an, cn = T(0.5) * (a[n] + b), T(0.5) * (a[n] - b)
        b = np.sqrt(a[n] * b)
        n += 1; a.append(an); c.append(cn)
    half_pi = T(np.pi) / 2 if T is np.float64 else np.arctan(LD(1)) * 2
    Kp = half_pi / a[n]
    u = (np.arange(N).astype(T) + T(0.5)) * Kp / N
    phi = a[n] * u * T(2.0) ** n
    for i in range(n, 0, -1):
        phi = T(0.5) * (phi + np.arcsin(c[i] * np.sin(phi) / a[i]))
    sn, cn = np.sin(phi), np.cos(phi)
    dn = np.sqrt(cn * cn + k2 * sn * sn)
    icn2 = T(1) / (cn * cn)
    return m * (sn * sn) * icn2, (T(2) * Kp * np.sqrt(m) / (2 * half_pi * N)) * dn * icn2


def quad_xs(m, M, count=200):
    return np.exp(np.linspace(np.log(LD(m)), np.log(LD(M)), count))


def quad_eval(shift, weight, xs):
    """sum_j w_j / (x + s_j) sqrt(x) - 1: the relative error of the nodes as an approximation of x^-1/2, longdouble sums of the given node values"""
    s, w = np.asarray(shift).astype(LD), np.asarray(weight).astype(LD)
    q = np.array([np.sum(w / (x + s)) for x in xs])
    return q * np.sqrt(xs) - 1


def quad_tolerance(m, M):
    """8 x the largest relative difference between the float64 and the longdouble evaluation of the header's formulas over the 200 points, floor 64 u
    -> (tolerance, measured float64 error)"""
    xs = quad_xs(m, M)
    e64 = quad_eval(*quad_nodes(m, M, np.float64), xs)
    eld = quad_eval(*quad_nodes(m, M, LD), xs)
    meas = float(np.max(np.abs(e64 - eld)))
    return max(8 * meas, 64 * U), meas


# ================================================================ TRTRI =========================================================================
TRTRI_NS = (1, 15, 16, 17, 31, 32, 33, 48, 100, 300, 301, 400)
# (n, factor kind, shared factor, hiprio, with A / scale / prep / sync2 (0 none, 1 prep, 2 prep + per-slot scale), active given)
TRTRI_CASES = [(n, ("random", "graded")[i % 2], i % 3 == 1, i % 2 == 1, (1, 2, 0)[i % 3], i % 4 != 2) for i, n in enumerate(TRTRI_NS)] + \
              [(n, ("graded", "random")[i % 2], i % 3 == 0, i % 2 == 0, (2, 0, 1)[i % 3], i % 4 != 1) for i, n in enumerate(TRTRI_NS)]


def trtri_case(n, kind, shared, hiprio, prep, use_active, single=False, launches=2):
    """launch_trtri_fro with the test's factor; A = L L' in float64 of each slot's factor (prep reads only its column sums).  B = 3, middle slot inactive"""
    ids = [2] if single else [0, 1, 2]
    B = len(ids)
    seeds = [31 + (0 if shared else i) for i in ids]
    L = [potri_factor(n, kind, sd) for sd in seeds]
    Am = [l @ l.T for l in L]
    Am = [0.5 * (a + a.T) for a in Am]
    scale = SCALES[ids] if prep == 2 else np.ones(B)
    active = actives(B, None if single else 1)
    computed = active if use_active else np.ones(B, dtype=np.int32)
    c = dict(n=n, B=B, L=L, A=Am, scale=scale, shared=shared, prep=prep, active=active, computed=computed, launches=launches,
             ref={b: trtri_reference_of(n, kind, seeds[b]) for b in range(B) if computed[b]})
    if prep:                                                              # the nodes' tolerance, from the reference's own (m, M)
        c["quad_tol"] = {}
        for b in c["ref"]:
            fro = LD(scale[b]) * np.sum(c["ref"][b][0])
            M = np.max(np.sum(np.abs(Am[b].astype(LD)), axis=0))
            c["quad_tol"][b] = quad_tolerance(float(min(1 / fro, M / 2)), float(M))
    c["data"] = pack_case(OP_TRTRI, B, [n, 0 if shared else n * n, int(use_active), int(hiprio), launches], [],
                          [(I32, active), (F64, np.array([to_cm(x) for x in (L[:1] if shared else L)])),
                           (F64, np.array([to_cm(x) for x in Am]) if prep else None), (F64, scale if prep == 2 else None)])
    return c


def trtri_reference(L):
    """-> (part[J] = sum of squares of block column J of X = L^-1, its bound), longdouble"""
    n = L.shape[0]
    X, _ = potri_reference(L)
    aX, Ll = np.abs(X), np.abs(L.astype(LD))
    dX = 2 * (n + 2) * LD(U) * (aX @ (Ll @ aX))
    nb = (n + TRI_B - 1) // TRI_B
    part, bound = np.zeros(nb, dtype=LD), np.zeros(nb, dtype=LD)
    for J in range(nb):
        c0, c1 = TRI_B * J, min(n, TRI_B * J + TRI_B)
        blk = X[c0:, c0:c1]
        terms = (n - c0) * (c1 - c0)
        part[J] = np.sum(blk * blk)
        bound[J] = np.sum(2 * aX[c0:, c0:c1] * dX[c0:, c0:c1]) + 2 * (terms + 8) * LD(U) * part[J]
    return part, bound


@functools.lru_cache(maxsize=None)
def trtri_reference_of(n, kind, seed):
    return trtri_reference(potri_factor(n, kind, seed))


# ================================================================ matrices with a known function ===============================================
def householder_apply(vs, Mx, side):
    """(H_1 ... H_k) Mx (side "l"), Mx (H_1 ... H_k)' (side "r"), or the transposed products ("lt", "rt"); H = I - 2 v v' (unit v), longdouble"""
    Mx = Mx.copy()
    order = vs if side in ("lt", "rt") else vs[::-1]                     # Q = H_1 ... H_k: Q M applies H_k first, M Q' = M H_k ... H_1 too
    for v in order:
        if side in ("l", "lt"):
            Mx -= 2 * np.outer(v, v @ Mx)
        else:
            Mx -= 2 * np.outer(Mx @ v, v)
    return Mx


def spectrum(n, kind, seed):
    """"cluster": the two CMA-like eigenvalues 0.0625 / 0.1 with a few outliers; "dec4" / "dec8" / "dec12": graded over that many decades"""
    rng = np.random.default_rng([seed, n, 9])
    if kind == "cluster":
        lam = np.where(np.arange(n) % 2 == 1, 0.1, 0.0625) * (1 + 1e-3 * rng.standard_normal(n))
        k = min(n // 3, 4)
        lam[:k] = np.array([0.9, 0.31, 0.02, 2.5])[:k]
        return lam
    dec = float(kind[3:])
    return 10.0 ** (-dec * (np.arange(n) + rng.random(n) * 0.5) / max(n - 0.5, 1.0))


def spd_with_function(lam, seed):
    """-> A (float64, symmetric), and a function f_of(fun, F) -> f(A) in longdouble (see the module docstring)"""
    n = len(lam)
    rng = np.random.default_rng([seed, n, 13])
    vs = []
    for _ in range(6):
        v = rng.standard_normal(n).astype(LD)
        vs.append(v / np.sqrt(v @ v))
    laml = lam.astype(LD)

    def conj(D):                                                          # Q D Q'
        return householder_apply(vs, householder_apply(vs, D, "l"), "r")

    def conj_t(Mx):                                                       # Q' M Q
        return householder_apply(vs, householder_apply(vs, Mx, "lt"), "rt")
    Ae = conj(np.diag(laml))
    Ae = 0.5 * (Ae + Ae.T)
    A = Ae.astype(np.float64)
    A = 0.5 * (A + A.T)
    dA = A.astype(LD) - Ae

    def f_of(fun, F):
        Y = conj(np.diag(fun(laml)) + F(laml) * conj_t(dA))
        return 0.5 * (Y + Y.T)
    return A, f_of


def _invsqrt_fun(l):
    return 1 / np.sqrt(l)


def _invsqrt_F(l):
    r = np.sqrt(l)
    return -1 / (r[:, None] * r[None, :] * (r[:, None] + r[None, :]))


def _sqrt_F(l):
    r = np.sqrt(l)
    return 1 / (r[:, None] + r[None, :])


def eigh64_function(A, fun):
    w, V = np.linalg.eigh(A)
    return (V * fun(w)) @ V.T


# ================================================================ INVSQRT =======================================================================
INVSQRT_NS = (1, 2, 17, 64, 100, 159, 160, 161, 300, 304, 400)
# (n, (spectrum of slot 0, of slot 2), coop, regions = invsqrt_coop_groups, b inside CMA's vec (bstride 3 n, offset 2 n), per-slot scale)
INVSQRT_CASES = []
for _i, _n in enumerate(INVSQRT_NS):
    INVSQRT_CASES.append((_n, ("cluster", "dec4"), True, True, _i % 2 == 0, _i % 2 == 1))
    INVSQRT_CASES.append((_n, ("dec8", "cluster"), _i % 2 == 0 or _n >= LAN_MIN_N, _i % 3 != 0 or _n >= LAN_MIN_N, _i % 2 == 1, _i % 2 == 0))
INVSQRT_CASES += [(160, ("dec12", "dec12"), True, True, False, False), (160, ("dec12", "cluster"), False, True, True, True)]
# the cooperative cases again through the one-workgroup kernel: without a CoopCtx and with one region per slot
INVSQRT_SOLO = [(160, ("cluster", "dec4"), False, True), (161, ("dec8", "cluster"), True, False), (300, ("cluster", "dec4"), True, False),
                (304, ("dec8", "cluster"), False, True)]
# active = nullptr through the whole chain (all three slots are computed): (n, spectra, b inside vec, per-slot scale), the cluster and the one-workgroup kernel
INVSQRT_NOACTIVE = [(300, ("cluster", "dec4"), True, True), (100, ("dec8", "cluster"), False, True), (160, ("cluster", "dec4"), False, False)]


def invsqrt_case(n, spectra, coop=True, regions=True, in_vec=False, scaled=False, use_active=True, single=False, special=None, status=None):
    """the chain launch_potrf -> launch_trtri_fro (with prep) -> launch_lanczos_invsqrt.  B = 3, middle slot inactive; slot 0 / 2 carry the two spectra
    (the inactive slot holds slot 0's matrix).  L = chol(scale A): the trace comes back as scale ||L^-1||_F^2 = tr(A^-1).
    special: "zero_b" (b = 0 in slot 0), "nan_b" (a NaN in slot 0's b)"""
    ids = [2] if single else [0, 1, 2]
    B = len(ids)
    spec = {0: spectra[0], 1: spectra[0], 2: spectra[1]}
    lam, Am, Yref = [], [], []
    for i in ids:
        l = spectrum(n, spec[i], 60 + (0 if i == 1 else i))
        A, f_of = spd_with_function(l, 60 + (0 if i == 1 else i))
        lam.append(l); Am.append(A); Yref.append(f_of)
    bv = np.array([np.random.default_rng([88, n, i]).standard_normal(n) for i in ids])
    if special == "zero_b":
        bv[0] = 0.0
    if special == "nan_b":
        bv[0, n // 2] = np.nan
    scale = SCALES[ids] if scaled else np.ones(B)
    bstride, boff = (3 * n, 2 * n) if in_vec else (n, 0)
    bbuf = np.full((B, bstride), POISON_F64)
    bbuf[:, boff:boff + n] = bv
    active = actives(B, None if single or not use_active else 1)
    st = np.zeros(B, dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32)[ids]
    computed = active if use_active else np.ones(B, dtype=np.int32)
    c = dict(n=n, B=B, spectra=[spec[i] for i in ids], lam=lam, A=Am, f_of=Yref, b=bv, scale=scale, coop=coop, regions=regions, active=active, computed=computed,
             status=st, env={}, special=special,
             data=pack_case(OP_INVSQRT, B, [n, int(use_active), int(coop), int(regions), bstride, boff], [],
                            [(I32, active), (F64, np.array([to_cm(a) for a in Am])), (F64, scale if scaled else None), (F64, bbuf), (I32, st)]))
    return c


def invsqrt_reference(c, b):
    """slot b -> dict(y, tol_eigh = 8 ||y_eigh64 - y_ref||, nb = ||b||, Minf = ||A||_inf): the tolerance's first term and what its second needs"""
    Y = c["f_of"][b](_invsqrt_fun, _invsqrt_F)
    bl = c["b"][b].astype(LD)
    y = Y @ bl
    y64 = eigh64_function(c["A"][b], lambda w: 1 / np.sqrt(w)) @ c["b"][b]
    d = y64.astype(LD) - y
    return dict(Y=Y, y=y, eigh_err=float(np.sqrt(d @ d)), nb=float(np.sqrt(bl @ bl)), ny=float(np.sqrt(y @ y)),
                Minf=float(np.max(np.sum(np.abs(c["A"][b]), axis=0))))


def invsqrt_tolerance(ref, M):
    """max(8 ||y_eigh64 - y_ref||, 2 kLanTol ||b|| / sqrt(M)) -> (tolerance, the two terms)"""
    t1, t2 = 8 * ref["eigh_err"], 2 * LAN_TOL * ref["nb"] / np.sqrt(M)
    return max(t1, t2), (t1, t2)


def dense_case(n, decades, B=3):
    """beyond the quadrature (cond > 1e14): the D H D family of tests/test_gpu_linalg_harness.py::test_dense_fallback_beyond_the_quadrature"""
    Am = [graded(n, 70 + i, float(decades)) for i in range(B)]
    bv = np.array([np.random.default_rng([89, n, i]).standard_normal(n) for i in range(B)])
    active = actives(B, 1)
    st = np.zeros(B, dtype=np.int32)
    return dict(n=n, B=B, A=Am, b=bv, scale=np.ones(B), active=active, computed=active, status=st, coop=True, regions=True, env={}, decades=decades,
                data=pack_case(OP_INVSQRT, B, [n, 1, 1, 1, n, 0], [], [(I32, active), (F64, np.array([to_cm(a) for a in Am])), (F64, None), (F64, bv), (I32, st)]))


def dense_identities(A, L, bv, y, fro, part):
    """the three identities of test_dense_fallback_beyond_the_quadrature in longdouble from the raw outputs: y'y = ||L^-1 b||^2, y'A y = b'b,
    fro = sum of the triangular inverse's partial traces -> relative errors"""
    n = A.shape[0]
    Ll, bl, yl, Al = L.astype(LD), bv.astype(LD), y.astype(LD), A.astype(LD)
    x = np.zeros(n, dtype=LD)
    for i in range(n):
        x[i] = (bl[i] - Ll[i, :i] @ x[:i]) / Ll[i, i]
    xx, yy, yAy, bb = x @ x, yl @ yl, yl @ (Al @ yl), bl @ bl
    tr = np.sum(part.astype(LD))
    return float(abs(yy - xx) / xx), float(abs(yAy - bb) / bb), float(abs(LD(fro) - tr) / tr)


# ================================================================ SYM_SQRT ======================================================================
SYM_SQRT_NS = (1, 2, 3, 16, 17, 100, 300)
SYM_SQRT_CASES = [(n, ("cluster", "dec4", "dec8")[i % 3]) for i, n in enumerate(SYM_SQRT_NS)] + [(17, "cluster"), (100, "dec8")]


def sym_sqrt_case(n, spec, bad=None, status=OK):
    """launch_sym_sqrt (one matrix).  bad: "indefinite" (one eigenvalue -1e-3) | "singular" (one eigenvalue exactly 0: the construction at order n - 1
    with a zero row and column put in the middle -- the float64 rounding of Q diag(lam) Q' with a zero in lam is NOT singular, its smallest
    eigenvalue is +-1e-17 with whatever sign the rounding gives, and a tiny positive one is rightly accepted)"""
    lam = spectrum(n, spec, 90)
    if bad == "indefinite":
        lam[n // 2] = -1e-3
    if bad == "singular":
        k = n // 2
        A1, f_of = spd_with_function(np.delete(lam, k), 90)
        A = np.zeros((n, n))
        keep = np.arange(n) != k
        A[np.ix_(keep, keep)] = A1
        lam[k] = 0.0
    else:
        A, f_of = spd_with_function(lam, 90)
    st = np.array([status], dtype=np.int32)
    return dict(n=n, B=1, lam=lam, A=A, f_of=f_of, bad=bad, status=st,
                data=pack_case(OP_SYM_SQRT, 1, [n], [], [(I32, actives(1, None)), (F64, to_cm(A)), (I32, st)]))


def sym_sqrt_reference(c):
    """-> (S = sqrt(A) in longdouble, tolerance on ||.||_F, (8 x the float64 eigh error, the floor))"""
    n = c["n"]
    S = c["f_of"](np.sqrt, _sqrt_F)
    d = eigh64_function(c["A"], lambda w: np.sqrt(np.maximum(w, 0))).astype(LD) - S
    t1 = 8 * float(np.sqrt(np.sum(d * d)))
    t2 = float(2 * (n + 8) * LD(U) * np.sqrt(np.sum(S * S)))
    return S, max(t1, t2), (t1, t2)
