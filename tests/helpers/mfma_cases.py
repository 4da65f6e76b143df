"""Inputs, file format, host-side rules and references for the direct tests of the matrix-core kernels (tools/kbench_mfma.hip): shared by
tests/test_mfma_cases_cpu.py (which proves on the CPU that the inputs and the references are what they claim) and tests/test_gpu_mfma_harness.py.
Nothing here touches the engine.  References are np.longdouble evaluations of the exact float64 inputs; the error bounds are derived (u = 2^-53):

  sampler  |E_ik - ref| <= (n + 8) u sum_j |L_ij| |Z_jk|      (x sqrt(oscale2), + 4 u |ref| with oscale2; the fused form adds 1e-13 sqrt(oscale2)
           sum_j |L_ij|, the project's per-normal tolerance of the device Box-Muller against the oracle)
  scatter  |S_ab - ref| <= 4 (m + 64) u T_ab,  T_ab = sqrt(sum_k w_k x_ak^2) sqrt(sum_k w_k x_bk^2) / den -- by Cauchy-Schwarz T dominates every
           product term of the one-pass form, the mu mu' correction included; |mu_a - ref| <= 4 (m + 64) u sqrt(sum_k w_k x_ak^2 / sum_k w_k).
           Weights from costs: + 4 u in the constant (relative error of exp).  A mean that had a shift added back carries one more rounding of
           the sum, u |ref| (half an ulp of the float64 result, which no kernel can avoid).
  A structural error -- a dropped column, a wrong row, a stale partial -- moves an entry by >= T / m; the bound is <= 2e-12 T at m = 4096."""
import numpy as np
from tests.helpers import harness_io as IO
from tests.helpers.harness_io import F64, I32, U64, GUARD, LD, U, bits, is_poison, split_guard           # (re-exported: the tests read them as M.<name>)

OP_TRMM, OP_FUSED, OP_TWOKERNEL, OP_WCOV, OP_SHRINK, OP_CE_SMALL, OP_CE_GENERAL, OP_GATHER = range(8)
MAGIC_IN, MAGIC_OUT = b"MFMCASE1", b"MFMRES01"
POISON_I32 = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]
POISON_F64_BITS = np.frombuffer(b"\xa5" * 8, dtype=np.uint64)[0]
RNG_TOL = 1e-13                                            # tests/test_gpu_parity.py::test_device_rng_normals_full_size
# enums of mpopis_amd/csrc/engine.h / include/mpopis.h
WCOV_PAIR64, WCOV_PAIR16, WCOV_ROWS, WCOV_TALL = 0, 1, 2, 3
EST = {"mle": 0, "ss": 1, "lw": 2, "rblw": 3, "oas": 4}
PANEL_ROWS = 128
RIDGE = 10e-9                                              # the reference writes it this way


# ---- the case lists of tests/test_gpu_mfma_harness.py (the CPU file proves what they reach) ------------------------------------------------
TRMM_NS = (1, 3, 16, 17, 100, 127, 128, 129, 144, 300, 304, 800)
TRMM_KS = (1, 15, 16, 17, 63, 64, 65, 200)
# (n, K, shared factor, oscale2): every n at K = 65, every K at n = 17 and 129; the factor's stride and the output scale alternate
TRMM_CASES = [(n, 65, i % 2 == 1, i % 3 == 1) for i, n in enumerate(TRMM_NS)] + [(n, K, i % 2 == 0, i % 3 == 2) for n in (17, 129) for i, K in enumerate(TRMM_KS) if K != 65] + \
             [(100, 65, False, True), (300, 65, True, False), (800, 17, True, True), (304, 64, False, False)]
FUSED_NS = (4, 12, 16, 20, 100, 108, 112, 116, 124, 128)
FUSED_KS = (1, 17, 64, 100, 257)
# every n at K = 100 (n = 4 .. 112: the 112-stride instantiation, 116 .. 128: the 144-stride one), every K at n = 12, 112 and 124
FUSED_CASES = [(n, 100, i % 2 == 1, i % 3 == 1) for i, n in enumerate(FUSED_NS)] + [(n, K, i % 2 == 0, i % 3 == 2) for n in (12, 112, 124) for i, K in enumerate(FUSED_KS) if K != 100] + \
              [(100, 257, True, True), (128, 64, True, False), (116, 17, False, True)]
WCOV_CS = (1, 15, 16, 17, 96, 97, 100, 111, 112, 113, 128, 129, 300, 511, 512, 513, 600, 799, 800)
WCOV_KSPLITS = [(64, 1), (64, 2), (65, 5), (65, 8), (150, 6), (150, 9), (257, 32), (257, 1), (1000, 2), (1000, 5), (1000, 9), (1000, 32), (150, 8), (64, 6)]
VARIANT_CS = (17, 97, 100, 112, 129, 513)
WEIGHT_SOURCES = [("pmc", 257, 6), ("w_wsum", 150, 5), ("w", 257, 8), ("cost", 1000, 6), ("cost_dominant", 257, 2), ("cost", 65, 1)]
GATHERED = [(2, True, 0.0), (30, False, RIDGE), (63, True, RIDGE), (64, False, 0.0), (65, True, 0.0), (51, True, RIDGE)]      # m, den = m (else 1), ridge
FOURTH = [("ss", 30), ("lw", 65), ("ss", 51)]
# row form: cs x ksplit x contiguous m, every weight source at every (cs, ksplit) and at every (cs, m); plus 819 of 1000 gathered at every (cs, ksplit)
ROW_CS, ROW_KSPLITS, ROW_MS = (97, 100, 111, 112), (2, 6), (64, 65, 257)
ROW_SOURCES = ("plain", "w", "cost")
ROW_CASES = [(cs, ks, m, ROW_SOURCES[(i + j + k) % 3]) for i, cs in enumerate(ROW_CS) for j, ks in enumerate(ROW_KSPLITS) for k, m in enumerate(ROW_MS)]
# (the third source of every (cs, m), at alternating split counts)
ROW_CASES += [(cs, ROW_KSPLITS[(i + k) % 2], m, ROW_SOURCES[(i + k + 2) % 3]) for i, cs in enumerate(ROW_CS) for k, m in enumerate(ROW_MS)]
ROW_GATHERED = [(cs, ks, "idx_w" if (i + j) % 2 else "idx") for i, cs in enumerate(ROW_CS) for j, ks in enumerate(ROW_KSPLITS)]
RULE_CASES = [  # cs, ksplit, sel_batch, rscale, partial
    (100, 4, 95, False, 0), (100, 4, 96, False, 2), (100, 6, 63, False, 0), (100, 6, 64, False, 2), (100, 4, -1, False, 0), (100, 5, 400, False, 0),
    (96, 4, 400, False, 0), (97, 4, 400, False, 2), (112, 4, 400, False, 2), (113, 4, 400, False, 1), (100, 4, 400, True, 0), (100, 2, 192, False, 2),
    (100, 2, 191, False, 0)]
SHRINK_SHAPES = [(4, 30), (20, 12), (100, 30), (129, 65)]
CE_CS, CE_MS, ESTS = (4, 20, 100, 128), (2, 3, 30, 63, 64), ("mle", "ss", "lw", "rblw", "oas")
CE_CASES = [(e, cs, m) for e in ESTS for cs in CE_CS for m in CE_MS]                   # the full cross: the small kernel takes all of it
CE_BEYOND = [(129, 30), (100, 65)]                                                   # the general path alone
WMEAN_MODES = [(1, False), (0, False), (0, True), (1, True)]                         # normalize, shift pair


def slots(cs):
    return dict(B=2, inactive=0) if cs > 512 else dict(B=3, inactive=1)            # the tall form's cases: two slots, the first inactive


def scatter_cases():
    """every case of the GPU file's scatter tests that goes against the reference, as (case, MPOPIS_WCOV_ROWS)"""
    out = [(wcov_case(cs, 257, 6, "w_wsum", **slots(cs)), 1) for cs in WCOV_CS]
    out += [(wcov_case(cs, 65, 2, "w"), 1) for cs in range(33, 48)]
    out += [(wcov_case(cs, K, ks, "plain", **slots(cs)), 1) for cs in (97, 129, 513) for K, ks in WCOV_KSPLITS]
    out += [(wcov_case(cs, 64, 32, v, **slots(cs)), 1) for cs in (100, 300, 600) for v in ("w", "cost")]
    out += [(wcov_case(cs, K, ks, v, **slots(cs)), 1) for cs in VARIANT_CS for v, K, ks in WEIGHT_SOURCES]
    out += [(wcov_case(cs, 257, 4, "idx", m=m, den=float(m) if dm else 1.0, ridge=rg, **slots(cs)), 1) for cs in VARIANT_CS for m, dm, rg in GATHERED]
    out += [(wcov_case(cs, 257, 6 if cs > 512 else 3, v, m=m, **slots(cs)), 1) for cs in VARIANT_CS for v, m in FOURTH]
    out += [(wcov_case(cs, m, ks, v, B=2, inactive=0), 2) for cs, ks, m, v in ROW_CASES]
    out += [(wcov_case(cs, 1000, ks, v, m=819, B=2, inactive=0), 2) for cs, ks, v in ROW_GATHERED]
    return out


# ---- the harness's files ---------------------------------------------------------------------------------------------------------------
def pack_case(op, B, ipar, dpar, arrays):
    """arrays: list of (type, array or None) in the op's fixed order (None = not given)"""
    return IO.pack_case(MAGIC_IN, op, B, ipar, dpar, arrays)


def unpack_case(buf):
    return IO.unpack_case(MAGIC_IN, buf)


def pack_result(form, arrays):
    """what the harness writes (used by the CPU round-trip test); arrays: list of (type, array with its guard entries)"""
    return IO.pack_result(MAGIC_OUT, form, arrays)


def unpack_result(buf):
    """-> (form, [arrays as written, guard entries included])"""
    return IO.unpack_result(MAGIC_OUT, buf)


def actives(B, inactive):
    a = np.ones(B, dtype=np.int32)
    a[inactive] = 0
    return a


# ---- host rules ---------------------------------------------------------------------------------------------------------------------------
def cost_key(v):
    """engine.h cost_key: order-preserving double -> uint64"""
    u = int(np.float64(v).view(np.uint64))
    return (~u) & 0xFFFFFFFFFFFFFFFF if u >> 63 else u | 0x8000000000000000


def wcov_kc(cs):
    return 64 if cs <= 112 else 16


def wcov_per(cs, m, ksplit):
    kc = wcov_kc(cs)
    return ((m + ksplit - 1) // ksplit + kc - 1) // kc * kc


def wcov_form(cs, K, m, ksplit, batch, has_rscale, has_idx, wants_mean, has_cost, env_rows=1):
    """transcription of wcov_form (kernels_mfma.hip) -> (partial, sq, aug, from_cost)"""
    aug = wants_mean and not has_rscale and cs % 16 != 0
    from_cost = has_cost and aug and not has_idx and cs % 16 != 0 and wcov_per(cs, K, ksplit) <= 1024
    nt = (cs + 15) // 16
    rows = bool(env_rows) and nt == 7 and not has_rscale and ksplit % 2 == 0 and batch >= 0 and batch * (ksplit // 2) >= (1 if env_rows > 1 else 192)
    partial = WCOV_TALL if nt * 16 > 512 else WCOV_ROWS if rows else WCOV_PAIR64 if wcov_kc(cs) == 64 else WCOV_PAIR16
    return partial, bool(has_rscale), bool(aug), bool(from_cost)


def form_code(partial, sq, aug, from_cost):
    return partial | (sq << 8) | (aug << 9) | (from_cost << 10)


def empty_splits(cs, m, ksplit, rows=False):
    """the K splits whose range is empty (kbeg >= kend); row form: a workgroup's two halves share one range, the second half of the last chunk may be all padding"""
    per = wcov_per(cs, m, ksplit)
    return [s for s in range(ksplit) if (s // 2 * 2 * per if rows else s * per) >= m]


def sampler_groups(n):
    """(row groups, tiles per group) of launch_trmm_LZ_mfma"""
    nt = (n + 15) // 16
    ng = (nt + 7) // 8
    return ng, (nt + ng - 1) // ng


def fusable(n):
    return n % 4 == 0 and (n + 15) // 16 <= 8


# ---- sampler ------------------------------------------------------------------------------------------------------------------------------
def sampler_L(n, nb, rng):
    """lower factors: entries O(0.1), diagonal 0.25 .. 1"""
    L = np.tril(rng.uniform(-0.1, 0.1, (nb, n, n)), -1)
    for b in range(nb):
        L[b][np.diag_indices(n)] = rng.uniform(0.25, 1.0, n)
    return L


def colmajor(M):
    """(nb, n, n) matrices -> the device's column-major storage"""
    return np.ascontiguousarray(np.swapaxes(M, -1, -2))


def trmm_case(n, K, shared=False, osc=False, upper=None, B=3, inactive=1, seed=0):
    rng = np.random.default_rng([seed, n, K])
    L = sampler_L(n, 1 if shared else B, rng)
    Z = rng.standard_normal((B, n, K))
    o = rng.uniform(0.3, 3.0, B) if osc else None
    Lup = L.copy()
    if upper is not None:
        Lup[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = upper
    act = actives(B, inactive)
    data = pack_case(OP_TRMM, B, [n, K, 0 if shared else n * n], [], [(I32, act), (F64, colmajor(Lup)), (F64, Z), (F64, o)])
    return dict(data=data, n=n, K=K, B=B, active=act, L=L, Z=Z, osc=o, shared=shared)


def sampler_reference(L, Z, osc=None, fused=False):
    """L (n, n) lower, Z (n, K) -> (ref, bound) in longdouble"""
    n = L.shape[0]
    Ll, Zl = np.tril(L).astype(LD), Z.astype(LD)
    ref, mag = Ll @ Zl, np.abs(Ll) @ np.abs(Zl)
    s = np.sqrt(LD(osc)) if osc is not None else LD(1)
    bound = (n + 8) * U * s * mag
    ref = s * ref
    if osc is not None:
        bound = bound + 4 * U * np.abs(ref)
    if fused:
        bound = bound + RNG_TOL * s * np.abs(Ll).sum(axis=1)[:, None]
    return ref, bound


def sampler_emulation(L, Z, osc=None):
    """plain float64: chunks of 16 columns of L accumulated in order, as an MFMA chain does"""
    n = L.shape[0]
    Ll = np.tril(L)
    acc = np.zeros((n, Z.shape[1]))
    for j0 in range(0, n, 16):
        acc = acc + Ll[:, j0:j0 + 16] @ Z[j0:j0 + 16]
    return acc * np.sqrt(osc) if osc is not None else acc


def fused_case(op, n, K, shared=False, osc=False, B=3, inactive=1, slo=3, shi=1, seed=0):
    rng = np.random.default_rng([seed, n, K, 7])
    nb = 1 if shared else B
    L0 = sampler_L(n, nb, rng)
    A = np.stack([np.tril(l @ l.T) + np.tril(l @ l.T, -1).T for l in L0])                  # SPD, bitwise symmetric
    seeds = rng.integers(1, 2 ** 63, B, dtype=np.uint64)
    o = rng.uniform(0.3, 3.0, B) if osc else None
    act = actives(B, inactive)
    data = pack_case(op, B, [n, K, 1 if shared else 0, slo, shi], [], [(I32, act), (F64, A), (U64, seeds), (F64, o)])
    return dict(data=data, n=n, K=K, B=B, active=act, A=A, L0=L0, seeds=seeds, osc=o, shared=shared, slo=slo, shi=shi)


def panel_doubles(n):
    return (n + 15) // 16 * 16 * PANEL_ROWS if n <= PANEL_ROWS else 0


def panel_of(L):
    """the factor in the staging layout of the fused sampler (k_potrf_lds): chunk c of 16 columns, LDS row p = (jc & 3) 4 + (jc >> 2) of the chunk's
    column jc, PANEL_ROWS matrix rows each; zero above the diagonal and beyond n"""
    n = L.shape[0]
    nch = (n + 15) // 16
    P = np.zeros((nch, 16, PANEL_ROWS))
    for j in range(n):
        c, jc = divmod(j, 16)
        P[c, (jc & 3) * 4 + (jc >> 2), j:n] = L[j:n, j]
    return P.reshape(-1)


# ---- scatter ------------------------------------------------------------------------------------------------------------------------------
def scatter_X(B, cs, K, rng, offsets=(0.0, 1.0)):
    """entries O(0.3) plus a per-row offset"""
    off = np.array([offsets[r % len(offsets)] for r in range(cs)])
    return 0.3 * rng.standard_normal((B, cs, K)) + off[None, :, None]


def softmax_weights(cost, lam):
    c = cost.astype(LD)
    w = np.exp(-(c - c.min()) / lam)
    return (w / w.sum()).astype(np.float64)


def wcov_case(cs, K, ksplit, variant, m=None, den=None, ridge=RIDGE, sel_batch=0, B=3, inactive=1, seed=0, u_add=True, want_mu=None):
    """variant: 'w_wsum' / 'w' (weights given, with / without their sum; den = 0), 'cost' / 'cost_dominant' (weights from costs with +inf among them),
    'cost_w' (costs and the normalised weights of the same costs, which take over when the launcher drops the costs),
    'pmc' (resampled columns made contiguous and shifted by their first one, den = K - 1), 'plain' (unweighted contiguous, den = K - 1),
    'idx' (m gathered columns, external mean), 'idx_w' (the same with weights w[idx] and their sum), 'ss' / 'lw' (the fourth-moment scatter of the gathered columns, den = 1)"""
    rng = np.random.default_rng([seed, cs, K, ksplit, sum(map(ord, variant)), m or 0])
    act = actives(B, inactive)
    c = dict(cs=cs, K=K, ksplit=ksplit, variant=variant, B=B, active=act, sel_batch=sel_batch, ridge=ridge, w=None, wsum=None, idx=None, mu=None, rscale=None,
             cost=None, shift=None, u0=None, nil=0.0)
    c["m"] = m = K if m is None else m
    X = scatter_X(B, cs, K, rng, (0.0, 1.0, 1e3) if variant == "pmc" else (0.0, 1.0))
    can_mean = cs % 16 != 0
    if variant in ("w_wsum", "w"):
        c["w"] = np.stack([softmax_weights(20.0 * rng.standard_normal(K) + 100.0, 20.0) for _ in range(B)])
        if variant == "w_wsum":
            c["wsum"] = c["w"].sum(axis=1)
        den = 0.0 if den is None else den
    elif variant in ("cost", "cost_dominant", "cost_w"):
        lam = 20.0
        cost = 20.0 * rng.standard_normal((B, K)) + 100.0
        if variant == "cost_dominant":                                    # one column carries the slot: every other weight is < 1e-300 of it or exactly 0
            cost = 100.0 + lam * rng.uniform(700.0, 740.0, (B, K))
            cost[np.arange(B), rng.integers(0, K, B)] = 100.0
        cost[:, rng.choice(K, max(1, K // 16), replace=False)] = np.inf   # a rollout that left the track for good: weight 0
        if variant == "cost_dominant":
            assert np.all(np.isfinite(cost).sum(axis=1) >= 1)
            cost[np.arange(B), np.argmin(np.where(np.isfinite(cost), cost, np.inf), axis=1)] = 100.0
        c["cost"], c["nil"] = cost, -1.0 / lam
        if variant == "cost_w" or cs % 16 == 0:                                           # as the engine calls it: the normalised weights of the same costs ride along (cs & 15 = 0 has no ones row: they are what runs)
            c["w"] = np.stack([softmax_weights(cost[b], lam) for b in range(B)])
        den = 0.0 if den is None else den
    elif variant == "pmc":
        idx = rng.integers(0, K, (B, K)).astype(np.int32)                 # Categorical draws: repeats
        c["shift"] = np.stack([X[b][:, idx[b, 0]] for b in range(B)])
        X = np.stack([X[b][:, idx[b]] - c["shift"][b][:, None] for b in range(B)])       # what launch_gather_cols hands over (one float64 subtraction)
        den = float(K - 1) if den is None else den
    elif variant == "plain":
        den = float(K - 1) if den is None else den
    else:
        assert variant in ("idx", "idx_w", "ss", "lw") and m <= K
        # the elite / resampled columns: at most half of the columns appear and, from m = 4 on, a quarter of the entries repeat an earlier one
        nrep = max(m // 4, m - K // 2) if m >= 4 else 0
        assert 2 * (m - nrep) <= K
        idx = np.zeros((B, K), dtype=np.int32)
        for b in range(B):
            distinct = rng.choice(K, m - nrep, replace=False)
            idx[b, :m] = rng.permutation(np.concatenate([distinct, rng.choice(distinct, nrep)]))
            idx[b, m:] = rng.integers(0, K, K - m)
        c["idx"] = idx
        if variant == "idx_w":                                            # gathered AND weighted (no policy does it; the launcher takes it): w[idx], their sum given
            c["w"] = rng.uniform(0.1, 1.0, (B, K))
            c["wsum"] = np.stack([c["w"][b][idx[b, :m]].sum() for b in range(B)])
        den = {"idx": float(m), "idx_w": 0.0}.get(variant, 1.0) if den is None else den
    c["X"], c["den"] = X, den
    has_rs = variant in ("ss", "lw")
    want = (can_mean and variant not in ("idx", "idx_w", "ss", "lw")) if want_mu is None else want_mu
    c["want_mu"] = want
    aug = want and not has_rs and can_mean
    if not aug:                                                           # external mean: the rounded exact one (launch_wmean / launch_gather_mean give it to ~m u)
        c["mu"] = np.stack([_wcov_inputs(c, b)[2].astype(np.float64) for b in range(B)])
    if has_rs:
        sd = np.stack([np.sqrt(((_wcov_inputs(c, b)[0] - c["mu"][b].astype(LD)[:, None]) ** 2).mean(axis=1)).astype(np.float64) for b in range(B)])
        c["rscale"] = 1.0 / sd if variant == "ss" else np.ones((B, cs))
    if want and u_add:
        c["u0"] = rng.standard_normal((B, cs))
    c["data"] = pack_case(OP_WCOV, B, [cs, K, m, ksplit, sel_batch, 1 if want else 0], [den, ridge, c["nil"]],
                          [(I32, act), (F64, X), (F64, c["w"]), (F64, c["wsum"]), (I32, c["idx"]), (F64, c["mu"]), (F64, c["rscale"]), (F64, c["cost"]),
                           (F64, c["shift"]), (F64, c["u0"])])
    return c


def case_form(c, env_rows=1):
    batch = c["B"] if c["sel_batch"] == 0 else c["sel_batch"]
    return wcov_form(c["cs"], c["K"], c["m"], c["ksplit"], batch, c["rscale"] is not None, c["idx"] is not None, bool(c["want_mu"]), c["cost"] is not None, env_rows)


def _wcov_inputs(c, b):
    """-> (Xg (cs, m) longdouble, w (m) longdouble, exact weighted mean, sum of the weights, weighted?)"""
    cols = c["idx"][b, :c["m"]] if c["idx"] is not None else np.arange(c["K"])
    Xg = c["X"][b][:, cols].astype(LD)
    if c["w"] is not None:
        w = c["w"][b][cols].astype(LD)
    elif c["cost"] is not None:
        cost = c["cost"][b].astype(LD)
        with np.errstate(over="ignore"):
            w = np.exp(LD(c["nil"]) * (cost - cost.min()))
    else:
        w = np.ones(len(cols), dtype=LD)
    wtot = w.sum()
    return Xg, w, (Xg @ w) / wtot, wtot, c["w"] is not None or c["cost"] is not None


def scatter_const(c):
    return 4 * (c["m"] + 64) + (4 if c["cost"] is not None else 0)


def wcov_reference(c, b):
    """-> dict(S, S_bound, mu, mu_bound) for slot b: the centred weighted covariance (centring before squaring, as mean_and_cov does) or, with rscale, the
    fourth-moment scatter; the bounds of the module docstring"""
    Xg, w, mean, wtot, weighted = _wcov_inputs(c, b)
    cs = c["cs"]
    den = LD(c["den"]) if c["den"] != 0 else wtot
    k = scatter_const(c) * U
    if c["rscale"] is not None:
        Zs = ((Xg - c["mu"][b].astype(LD)[:, None]) * c["rscale"][b].astype(LD)[:, None]) ** 2
        t = np.sqrt((Zs * Zs).sum(axis=1))
        return dict(S=np.einsum("ik,jk->ij", Zs, Zs) / den + LD(c["ridge"]) * np.eye(cs, dtype=LD), S_bound=k * np.outer(t, t) / abs(den), mu=None, mu_bound=None)
    Xc = Xg - mean[:, None]
    S = np.einsum("ik,jk->ij", Xc * w[None, :], Xc) / den + LD(c["ridge"]) * np.eye(cs, dtype=LD)
    t2 = (Xg * Xg) @ w
    t = np.sqrt(t2)
    mu, mu_bound = mean, k * np.sqrt(t2 / wtot)
    mean_bound = mu_bound
    if c["shift"] is not None:
        mu = mean + c["shift"][b].astype(LD)
        mu_bound = mu_bound + U * np.abs(mu)
    return dict(S=S, S_bound=k * np.outer(t, t) / abs(den), mu=mu, mu_bound=mu_bound, mean=mean, mean_bound=mean_bound)


def wcov_emulation(c, b):
    """plain float64, the kernel's plan: rows staged as sqrt(w) x, the one-pass uncentred scatter in 8 interleaved partials, the mean from the ones row
    (or the external one), the mu mu' correction, / den, + ridge"""
    cols = c["idx"][b, :c["m"]] if c["idx"] is not None else np.arange(c["K"])
    Xg = c["X"][b][:, cols]
    cs = c["cs"]
    if c["w"] is not None:
        w = c["w"][b][cols]
    elif c["cost"] is not None:
        with np.errstate(over="ignore"):
            w = np.exp(0.5 * c["nil"] * (c["cost"][b] - c["cost"][b].min())) ** 2
    else:
        w = np.ones(len(cols))
    sw = np.sqrt(w)
    if c["rscale"] is not None:
        Zs = ((Xg - c["mu"][b][:, None]) * c["rscale"][b][:, None]) ** 2
        S = sum(Zs[:, p::8] @ Zs[:, p::8].T for p in range(8))
        return S / c["den"] + c["ridge"] * np.eye(cs), None
    Xw = Xg * sw[None, :]
    S = sum(Xw[:, p::8] @ Xw[:, p::8].T for p in range(8))
    wtot = float(sum(np.sum(w[p::8]) for p in range(8))) if (c["w"] is not None or c["cost"] is not None) else float(len(cols))
    mu = c["mu"][b] if c["mu"] is not None else sum(Xw[:, p::8] @ sw[p::8] for p in range(8)) / wtot
    den = c["den"] if c["den"] != 0 else wtot
    S = (S - np.outer(mu * wtot, mu)) / den + c["ridge"] * np.eye(cs)
    return S, mu                                                          # (the mean of the data as given: a shift is not added back here)


# ---- shrinkage ----------------------------------------------------------------------------------------------------------------------------
def shrink_transcription(X, est, dt):
    """the oracle's cov_*_cols formulas (oracle/mpopis_oracle.c) on the columns of X (cs, m) in arithmetic dt
    -> dict(mean, S (MLE), F (target), lam_raw, lam, cond (sum of the magnitudes the intensity cancels, over its denominator: one rounding of it is u cond))"""
    X = np.asarray(X).astype(dt)
    cs, m = X.shape
    mean = X.sum(axis=1) / dt(m)
    Xc = X - mean[:, None]
    S = np.einsum("ik,jk->ij", Xc, Xc) / dt(m)
    off = ~np.eye(cs, dtype=bool)
    if est == "mle":
        return dict(mean=mean, S=S, F=S, lam_raw=dt(0), lam=dt(0), cond=dt(0))
    if est in ("ss", "lw"):
        sd = np.sqrt(np.diag(S)) if est == "ss" else np.ones(cs, dtype=dt)
        Zs = Xc / sd[:, None]
        R = S / np.outer(sd, sd)
        V, A = np.zeros((cs, cs), dtype=dt), np.zeros((cs, cs), dtype=dt)
        for j in range(m):
            W = np.outer(Zs[:, j], Zs[:, j]) - R
            V += W * W
            A += np.outer(Zs[:, j], Zs[:, j]) ** 2
        f = dt(m) / (dt(m - 1) ** 3)
        num, den = V[off].sum() * f, (R[off] ** 2).sum()
        lam_raw = num / den if den > 0 else dt(1)
        cond = (A[off].sum() + m * den) * f / den if den > 0 else dt(0)      # the device forms Q_ab - m r_ab^2
        F = np.diag(np.diag(S))
    else:
        tr, tr2 = np.trace(S), (S * S).sum()
        p, n = dt(cs), dt(m)
        dd = tr2 - tr * tr / p
        lam_raw = (((1 - 2 / p) * tr2 + tr * tr) / ((n + 1 - 2 / p) * dd) if est == "oas" else ((n - 2) / n * tr2 + tr * tr) / ((n + 2) * dd)) if dd > 0 else dt(1)
        cond = lam_raw * (tr2 + tr * tr / p) / dd + lam_raw if dd > 0 else dt(0)
        F = (tr / p) * np.eye(cs, dtype=dt)
    lam = min(max(lam_raw, dt(0)), dt(1))
    return dict(mean=mean, S=S, F=F, lam_raw=lam_raw, lam=lam, cond=cond)


def lam_tolerance(X, est):
    """GPU tolerance on lambda*: 8 x the error of the float64 transcription against its longdouble evaluation (the margin covers another summation
    order across 256 threads).  The measured error can be zero by luck (a clamped or an exactly representable quotient), so it is floored by one
    rounding of the terms the intensity cancels, u cond -- the least any evaluation order can promise.  -> (tolerance, longdouble transcription)"""
    hi, lo = shrink_transcription(X, est, LD), shrink_transcription(X, est, np.float64)
    err = abs(LD(lo["lam_raw"]) - hi["lam_raw"])
    return float(8 * max(err, U * hi["cond"])), hi


def elite_data(cs, m, rng, noise=1.0):
    """columns with a strong common factor and unequal variances: lambda* lands well inside (0, 1)"""
    g = rng.standard_normal(m)
    load = rng.uniform(0.7, 1.3, cs) * rng.choice([-1.0, 1.0], cs)
    scale = rng.uniform(0.2, 0.5, cs)
    return scale[:, None] * (np.outer(load, g) + noise * rng.standard_normal((cs, m))) + rng.uniform(-0.5, 0.5, cs)[:, None]


def moments_for_shrink(X, est):
    """(S, Q) as the scatter kernels hand them to the shrinkage kernels: S = MLE covariance, Q_ab = sum_k z_a^2 z_b^2 (z standardised for :ss), in
    longdouble, rounded"""
    h = shrink_transcription(X, "mle", LD)
    Xc = np.asarray(X).astype(LD) - h["mean"][:, None]
    S = h["S"].astype(np.float64)
    if est in ("ss", "lw"):
        rs = 1.0 / np.sqrt(np.diag(S)) if est == "ss" else np.ones(X.shape[0])
        Z2 = (Xc * rs.astype(LD)[:, None]) ** 2
        return S, np.einsum("ik,jk->ij", Z2, Z2).astype(np.float64), rs
    return S, None, None


def shrink_case(cs, m, est, S, Q, B=3, inactive=1, ridge=RIDGE):
    """S, Q: per-slot lists (B entries; the inactive slot's are used as filler)"""
    act = actives(B, inactive)
    kind = {"rblw": 0, "oas": 1, "ss": 2, "lw": 3}[est]
    data = pack_case(OP_SHRINK, B, [cs, m, kind], [ridge], [(I32, act), (F64, colmajor(np.stack(S))), (F64, None if Q is None else colmajor(np.stack(Q)))])
    return dict(data=data, cs=cs, m=m, est=est, B=B, active=act, ridge=ridge)


def shrunk_tolerance(X, est, tol_lam, hi):
    """|S'_ab - oracle| allowed: the intensity's tolerance times the distance it moves the entry, plus twice the scatter bound (the oracle's own float64
    moments and the device's).  The common-variance target tr(S) / p is a sum over all p diagonal entries, so a diagonal entry of :rblw / :oas also
    carries lambda x (the mean of the diagonal's scatter bounds + (p + 2) u tr / p for the summation and the division), again once per side."""
    Xl = np.asarray(X).astype(LD)
    cs, m = X.shape
    t = np.sqrt((Xl * Xl).sum(axis=1))
    bound = 4 * (m + 64) * U * np.outer(t, t) / m
    tol = tol_lam * np.abs(hi["S"] - hi["F"]) + 2 * bound
    if est in ("rblw", "oas"):
        tol = tol + 2 * hi["lam"] * (np.diag(bound).mean() + (cs + 2) * U * abs(hi["F"][0, 0])) * np.eye(cs, dtype=LD)
    return tol


def clamp_case(kind, cs, m, seed=5):
    """hand-made moments for the clamps and guarded quotients of the shrinkage kernels -> (S, Q or None, est)"""
    rng = np.random.default_rng([seed, cs, m])
    S, _, _ = moments_for_shrink(elite_data(cs, m, rng), "mle")
    est = kind.split("_")[0]
    if kind in ("ss_zero", "lw_zero"):
        # Q_ab = r_ab^2 (resp. s_ab^2): Q_ab - m r_ab^2 < 0 everywhere, raw lambda = -m / (m - 1)^2 (-0.036 at m = 30: 1e14 roundings below 0)
        rs = 1.0 / np.sqrt(np.diag(S)) if est == "ss" else np.ones(cs)
        R = S * np.outer(rs, rs)
        return S, R * R, est
    if kind == "ss_one":
        rs = 1.0 / np.sqrt(np.diag(S))
        R = S * np.outer(rs, rs)
        return S, (m + 2.0 * (m - 1) ** 3 / m) * R * R, est               # raw lambda = 2
    if kind == "ss_no_offdiag":
        return np.diag(np.diag(S)), np.ones((cs, cs)), est                # sum r_ab^2 = 0: lambda = 1
    if kind in ("rblw_one", "oas_one"):
        return 0.5 * np.eye(cs) + 1e-3 * (1 - np.eye(cs)), None, est      # nearly spherical: the raw intensity is ~1e3
    assert kind == "rblw_no_spread"
    return 0.5 * np.eye(cs), None, est                                    # tr(S^2) - tr(S)^2 / p = 0 exactly: lambda = 1


def ss_lambda_f64(S, Q, rs, m):
    """k_ss_shrink's intensity in float64 -> (raw, clamped)"""
    off = ~np.eye(S.shape[0], dtype=bool)
    R = S * np.outer(rs, rs)
    num = (Q - m * R * R)[off].sum() * (m / float((m - 1) ** 3))
    den = (R * R)[off].sum()
    raw = num / den if den > 0 else 1.0
    return raw, min(max(raw, 0.0), 1.0)


def common_lambda_f64(S, m, oas):
    p, n, tr, tr2 = float(S.shape[0]), float(m), np.trace(S), (S * S).sum()
    dd = tr2 - tr * tr / p
    if not dd > 0:
        return np.inf, 1.0
    raw = ((1 - 2 / p) * tr2 + tr * tr) / ((n + 1 - 2 / p) * dd) if oas else ((n - 2) / n * tr2 + tr * tr) / ((n + 2) * dd)
    return raw, min(max(raw, 0.0), 1.0)


def clamp_expected(kind, S, ridge):
    """lambda exactly 0: the off-diagonals as they were; exactly 1: the target alone"""
    d = np.diag(np.diag(S))
    if kind in ("ss_zero", "lw_zero"):
        return S + ridge * np.eye(S.shape[0])
    if kind in ("ss_one", "ss_no_offdiag"):
        return d + ridge * np.eye(S.shape[0])
    return (0.5 + ridge) * np.eye(S.shape[0])                             # (1 - 1) S + (1 x tr / p + ridge) on the diagonal, tr / p = 0.5 exactly


# ---- CE -----------------------------------------------------------------------------------------------------------------------------------
def ce_case(op, cs, K, m, est, ksplit=4, B=3, inactive=1, seed=0):
    rng = np.random.default_rng([seed, cs, K, m, EST[est]])
    act = actives(B, inactive)
    E = np.zeros((B, cs, K))
    order = np.stack([rng.permutation(K) for _ in range(B)]).astype(np.int32)
    for b in range(B):
        E[b] = 0.3 * rng.standard_normal((cs, K))
        E[b][:, order[b, :m]] = elite_data(cs, m, rng)
    U0 = rng.standard_normal((B, cs))
    data = pack_case(op, B, [cs, K, m, EST[est], ksplit], [RIDGE], [(I32, act), (F64, E), (I32, order), (F64, U0)])
    c = dict(data=data, cs=cs, K=K, m=m, est=est, B=B, active=act, E=E, order=order, U0=U0, ksplit=ksplit)
    c["lam"] = [case_lam_tolerance(E[b][:, order[b, :m]], est) for b in range(B)]      # (tolerance on lambda*, longdouble transcription) per slot
    return c


def case_lam_tolerance(X, est):
    """lam_tolerance, except at m = 2 with :ss / :lw: there every w_j equals r exactly, lambda* = 0 / den, and what either side computes is rounding
    noise over den -- the measured difference of two noises says nothing, so the tolerance is the floor 8 u cond alone"""
    if X.shape[1] >= 3 or est not in ("ss", "lw"):
        return lam_tolerance(X, est)
    hi = shrink_transcription(X, est, LD)
    return float(8 * U * hi["cond"]), hi


def ce_small_ok(cs, m):
    rows, ld = (cs + 15) // 16 * 16, ((m + 3) & ~3) + 1
    return cs <= 128 and 2 <= m <= 64 and (rows * ld + rows) * 8 <= 150 * 1024


# ---- gather / weighted mean ---------------------------------------------------------------------------------------------------------------
def gather_case(sub, cs, K, m=None, normalize=1, shift_pair=False, B=3, inactive=1, seed=0):
    """sub: 0 gather_cols, 1 gather_cols + shift, 2 gather_mean over idx[:m], 3 wmean"""
    rng = np.random.default_rng([seed, sub, cs, K, m or 0])
    act = actives(B, inactive)
    X = scatter_X(B, cs, K, rng)
    m = K if m is None else m
    idx = w = sa = sb = None
    if sub != 3:
        idx = rng.integers(0, max(1, K // 2), (B, K)).astype(np.int32)                  # repeats; the upper half of the columns never appears
    else:
        w = np.stack([softmax_weights(20.0 * rng.standard_normal(K) + 100.0, 20.0) for _ in range(B)])
        if shift_pair:
            sa, sb = rng.standard_normal((B, cs)), rng.standard_normal((B, cs))
    data = pack_case(OP_GATHER, B, [cs, K, m, sub, normalize], [], [(I32, act), (F64, X), (I32, idx), (F64, w), (F64, sa), (F64, sb)])
    return dict(data=data, sub=sub, cs=cs, K=K, m=m, B=B, active=act, X=X, idx=idx, w=w, sa=sa, sb=sb, normalize=normalize)


def gather_mean_reference(c, b):
    Xg = c["X"][b][:, c["idx"][b, :c["m"]]].astype(LD)
    m = c["m"]
    return Xg.sum(axis=1) / m, 4 * (m + 64) * U * np.sqrt((Xg * Xg).sum(axis=1) / m)


def wmean_reference(c, b):
    """sum_k w_k (e_k + sft) / (sum_k w_k or 1), sft = shiftA - shiftB as one float64 subtraction; |sum w y| <= sqrt(sum w y^2) sqrt(sum w)"""
    sft = (c["sa"][b] - c["sb"][b]) if c["sa"] is not None else np.zeros(c["cs"])
    Y = c["X"][b].astype(LD) + sft.astype(LD)[:, None]
    w = c["w"][b].astype(LD)
    wt = w.sum()
    k = 4 * (c["K"] + 64) * U
    t2 = (Y * Y) @ w
    if c["normalize"]:
        return (Y @ w) / wt, k * np.sqrt(t2 / wt)
    return Y @ w, k * np.sqrt(t2 * wt)
