"""The two ends of the policy step -- the noise source (the Philox rounds, the table-based Box-Muller of philox.h, k_rng_tab_init, the three
k_sample_normal* forms, k_sample_resample_draws) and the read-out tail (k_finalize, k_transpose_in, k_transpose_out) -- exercised directly, below
the policy level, through the C++ harness tools/kbench_sample.hip: one process per launch, inputs written by the test, raw device outputs read back.
Every NORMALS case asserts the form sample_normal_form reported, so a moved condition fails a test instead of dropping a kernel from coverage.
References are NumPy (np.longdouble where arithmetic is involved) and the oracle (tests/helpers/sample_cases.py; tests/test_sample_cases_cpu.py
proves them and the derived Box-Muller bound on the CPU), never the engine.  The harness poisons every output first: inactive slots and the
entries past the end must stay untouched, and no active entry may keep the poison."""
import os
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import sample_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
B = 3
NMAX = 8256                                                           # normals per (seed, stream) the placement reference holds: >= 32 x 257


@pytest.fixture(scope="module")
def harness():
    return HR.build("sample")


def _run(exe, tmp_path, case, op, **shape):
    return S.unpack_result(HR.run_case(exe, tmp_path, case), op, **shape)


def _clean(r, name):
    """the guard untouched, no entry left at the poison"""
    assert np.all(S.is_poison(r[name + "_guard"])), name
    assert not np.any(S.is_poison(r[name])), (name, int(np.sum(S.is_poison(r[name]))))
    return r[name]


def _box_muller(exe, tmp_path, wr, wa, from_global=False):
    r = _run(exe, tmp_path, S.case_box_muller(wr, wa, from_global), S.OP_BOXMULLER, n=len(wr))
    assert r["form"] == -1
    z = _clean(r, "z").reshape(-1, 2)
    return z[:, 0].copy(), z[:, 1].copy()


@pytest.fixture(scope="module")
def stream_bits(harness, tmp_path_factory):
    """[slot][NMAX]: the first normals of the NORMALS cases' three streams as the BOXMULLER probe makes them from the NumPy Philox words (one launch);
    test_box_muller_* hold the probe to the long double definition, test_words the device's Philox to the NumPy one"""
    words = [S.stream_words(seed, *S.NORMALS_STREAM, NMAX) for seed in S.NORMALS_SEEDS]
    z0, z1 = _box_muller(harness, tmp_path_factory.mktemp("stream"), np.concatenate([w[0] for w in words]), np.concatenate([w[1] for w in words]))
    return np.stack([z0, z1], axis=1).reshape(len(S.NORMALS_SEEDS), NMAX)


@pytest.fixture(scope="module")
def oracle_normals(oracle):
    return np.stack([oracle.philox_normals(seed, *S.NORMALS_STREAM, NMAX) for seed in S.NORMALS_SEEDS])


# ================================================================ the noise source =============================================================
def test_table_entries_within_one_ulp(harness, tmp_path):
    r = _run(harness, tmp_path, S.pack_case(S.OP_TAB), S.OP_TAB)
    tab, ref = _clean(r, "tab"), S.table_ref()
    assert tab[2 * S.TAB_LOG - 2] == 1.0 and tab[2 * S.TAB_LOG - 1] == 0.0 and not np.signbit(tab[2 * S.TAB_LOG - 1])      # the top interval: exactly (1, 0)
    rounded = ref.astype(np.float64)
    err_ulp = (np.abs(tab.astype(np.longdouble) - ref) / np.maximum(S.ulp_of(rounded), 2.0 ** -1074)).astype(np.float64)
    off = tab != rounded
    kinds = np.tile(["1/c", "log c"], S.TAB_LOG).tolist() + np.tile(["sin", "cos"], S.TAB_SC).tolist()
    print("TAB not correctly rounded: %d of %d entries (%s), worst %.3f ulp" % (int(off.sum()), tab.size,
          ", ".join("%s %d" % (k, sum(1 for i in np.flatnonzero(off) if kinds[i] == k)) for k in ("1/c", "log c", "sin", "cos")), err_ulp.max()))
    assert np.all(err_ulp <= 1.0), (int(np.argmax(err_ulp)), err_ulp.max())


def test_words_are_random123_and_the_oracle(harness, tmp_path, oracle):
    sets = S.directed_philox_sets(np.random.default_rng(5))
    r = _run(harness, tmp_path, S.case_words(sets), S.OP_WORDS, n=len(sets))
    assert np.all(S.is_poison(r["out_guard"]))
    out = r["out"].reshape(-1, 4)
    for (c, k, want), got in zip(S.KAT, out[:3].tolist()):
        assert got == want
    assert np.array_equal(out, S.philox_np(sets))
    for s, got in zip(sets.tolist(), out.tolist()):
        assert got == oracle.philox4x32_10(s[:4], s[4:]), s


def test_box_muller_on_directed_and_random_words(harness, tmp_path):
    """Every directed pair (both ends of every log-table interval at six exponents, the extreme radius words, five words per sector of the angle) and
    2^18 random pairs, one launch: error / derived bound <= 1 on every pair, and the outer contract RNG_TOL; the table read from global memory
    (second launch) gives the same bits as the table staged in LDS."""
    dr, da = S.directed_pairs()
    rr, ra = S.random_pairs()
    wr, wa = np.concatenate([dr, rr]), np.concatenate([da, ra])
    z0, z1 = _box_muller(harness, tmp_path, wr, wa)
    ratio, ulps = S.bm_ratio(z0, z1, wr, wa)
    w = int(np.argmax(ratio))
    print("RATIO BOXMULLER %.4f (directed %.4f, random %.4f) at wr %d wa %d; worst error %.2f ulp of a unit normal (directed %.2f, random %.2f)" %
          (ratio.max(), ratio[:dr.size].max(), ratio[dr.size:].max(), wr[w], wa[w], ulps.max(), ulps[:dr.size].max(), ulps[dr.size:].max()))
    assert np.all(ratio <= 1.0), (int((ratio > 1).sum()), wr[w], wa[w], ratio.max())
    assert ulps.max() * 2.0 ** -52 <= S.RNG_TOL
    g0, g1 = _box_muller(harness, tmp_path, wr, wa, from_global=True)
    assert np.array_equal(S.bits(g0), S.bits(z0)) and np.array_equal(S.bits(g1), S.bits(z1))


NORMALQ_ENTRIES = [(seed, slo, shi, q) for seed in S.NORMALS_SEEDS for slo, shi in ((0, 0), (7, 3), (0xFFFFFFFF, 0x80000002), (5, 0x40000000))
                   for q in (0, 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 3)]


def test_normal_quad_and_pair_with_64_bit_counters(harness, tmp_path):
    """philox_normal_quad(q) and philox_normal_pair(2q), (2q + 1) with the key's and the counter's high words set: the pair calls are the halves of the
    quad call, and both are box_muller_u32 of the Philox words of that call -- all bit for bit"""
    n = len(NORMALQ_ENTRIES)
    r = _run(harness, tmp_path, S.case_normalq(NORMALQ_ENTRIES), S.OP_NORMALQ, n=n)
    z = _clean(r, "z").reshape(n, 8)
    assert np.array_equal(S.bits(z[:, 0:4]), S.bits(z[:, 4:8]))
    sets = np.concatenate([S.stream_call_sets(seed, slo, shi, [q]) for seed, slo, shi, q in NORMALQ_ENTRIES])
    assert len({tuple(s) for s in sets.tolist()}) == n
    w = S.philox_np(sets).reshape(-1, 2)
    z0, z1 = _box_muller(harness, tmp_path, w[:, 0], w[:, 1])
    assert np.array_equal(S.bits(np.stack([z0, z1], axis=1).reshape(n, 4)), S.bits(z[:, 0:4]))


def _check_normals(exe, tmp_path, stream_bits, oracle_normals, mppi, cs, K, as_, T, with_dscale, no_active=False):
    rng = np.random.default_rng(cs * 1000 + K)
    dscale = S.normals_dscale(B, cs, rng) if with_dscale else None
    case = S.case_normals(B, cs, K, as_, T, mppi, S.NORMALS_SEEDS, *S.NORMALS_STREAM, S.NORMALS_ACTIVE, dscale=dscale, no_active=no_active)
    r = _run(exe, tmp_path, case, S.OP_NORMALS, B=B, cs=cs, K=K)
    assert r["form"] == S.predicted_form(cs, as_, mppi), (r["form"], S.predicted_form(cs, as_, mppi))
    assert np.all(S.is_poison(r["Z_guard"]))
    Z = r["Z"].reshape(B, cs, K)
    lin = S.lin_map(cs, K, as_, mppi)
    assert lin.max() < NMAX
    for b in range(B):
        if not S.NORMALS_ACTIVE[b] and not no_active:
            assert np.all(S.is_poison(Z[b])), b
            continue
        assert not np.any(S.is_poison(Z[b])), b
        d = dscale[b][:, None] if with_dscale else 1.0
        want = stream_bits[b][lin] * d                                 # one product, as the kernel forms it
        bad = np.argwhere(S.bits(Z[b]) != S.bits(want))
        assert bad.size == 0, (b, len(bad), bad[:4].tolist())
        assert np.all(np.abs(Z[b] - oracle_normals[b][lin] * d) <= S.RNG_TOL * np.abs(d)), b
    return Z


@pytest.mark.parametrize("with_dscale", [False, True])
@pytest.mark.parametrize("mppi,cs,K,as_,T", S.normals_shapes())
def test_normals_sit_where_the_draw_order_puts_them(harness, tmp_path, stream_bits, oracle_normals, mppi, cs, K, as_, T, with_dscale):
    """Entry (r, k) of an active slot is normal number lin(r, k) of the slot's stream (times dscale[r]) bit for bit, in the form the shape was
    written for; the middle slot is inactive and keeps the poison"""
    _check_normals(harness, tmp_path, stream_bits, oracle_normals, mppi, cs, K, as_, T, with_dscale)


ONE_PER_FORM = [(0, 8, 257, 2, 4, S.QUAD), (0, 6, 257, 2, 3, S.PAIR), (1, 9, 257, 3, 3, S.SINGLE)]


@pytest.mark.parametrize("mppi,cs,K,as_,T,form", ONE_PER_FORM)
def test_normals_without_an_active_mask_and_twice(harness, tmp_path, stream_bits, oracle_normals, mppi, cs, K, as_, T, form):
    """active = nullptr: every slot is drawn; a second run of the same case gives the same bits"""
    assert S.predicted_form(cs, as_, mppi) == form
    z1 = _check_normals(harness, tmp_path, stream_bits, oracle_normals, mppi, cs, K, as_, T, True, no_active=True)
    z2 = _check_normals(harness, tmp_path, stream_bits, oracle_normals, mppi, cs, K, as_, T, True, no_active=True)
    assert np.array_equal(S.bits(z1), S.bits(z2))


@pytest.mark.parametrize("mppi,cs,K,as_,T", S.CROSS_FORM_SHAPES)
def test_normals_are_one_sequence_in_every_form(harness, tmp_path, stream_bits, oracle_normals, mppi, cs, K, as_, T):
    """The first 3084 normals of one (seed, stream) drawn through all three kernels and both orders: flattened by lin, every case is the same
    bit-identical sequence (the probe's, which every case is compared with)"""
    Z = _check_normals(harness, tmp_path, stream_bits, oracle_normals, mppi, cs, K, as_, T, False)
    flat = np.empty(S.CROSS_FORM_N)
    flat[S.lin_map(cs, K, as_, mppi).reshape(-1)] = Z[0].reshape(-1)
    assert np.array_equal(S.bits(flat), S.bits(stream_bits[0][:S.CROSS_FORM_N]))


@pytest.mark.parametrize("K", [1, 2, 3, 255, 256, 257, 1000, 16384])
def test_resample_draws(harness, tmp_path, oracle, K):
    slo, shi = 41, 3 | 0x80000000                                       # the engine's stream pattern: (mpc step, AIS iteration | 0x80000000)
    r = _run(harness, tmp_path, S.case_draws(B, K, S.NORMALS_SEEDS, slo, shi, S.NORMALS_ACTIVE), S.OP_DRAWS, B=B, K=K)
    assert np.all(S.is_poison(r["di_guard"])) and np.all(S.is_poison(r["du_guard"]))
    di, du = r["di"].reshape(B, K), r["du"].reshape(B, K)
    for b in range(B):
        if not S.NORMALS_ACTIVE[b]:
            assert np.all(S.is_poison(di[b])) and np.all(S.is_poison(du[b]))
            continue
        i0, u = oracle.philox_resample_draws(S.NORMALS_SEEDS[b], slo, shi, K)
        assert np.array_equal(di[b], i0) and np.array_equal(S.bits(du[b]), S.bits(u)), b
        assert di[b].min() >= 0 and di[b].max() < K and du[b].min() >= 0.0 and du[b].max() < 1.0
        w = S.philox_np(S.stream_call_sets(S.NORMALS_SEEDS[b], slo, shi, np.arange(K))).astype(np.uint64)   # and from the words themselves
        a53, b53 = ((w[:, 1] << np.uint64(32)) | w[:, 0]) >> np.uint64(11), ((w[:, 3] << np.uint64(32)) | w[:, 2]) >> np.uint64(11)
        assert np.array_equal(du[b], b53.astype(np.float64) * 2.0 ** -53)
        assert np.array_equal(di[b], np.minimum((a53.astype(np.float64) * 2.0 ** -53 * K).astype(np.int64), K - 1))


# ================================================================ the tail =====================================================================
@pytest.mark.parametrize("as_,T", S.FINALIZE_SHAPES)
def test_finalize_is_bit_exact(harness, tmp_path, as_, T):
    """control = clamp(U + wn) on its first `as` entries (below, at, between, above the bounds, +-inf -> the bound, NaN -> NaN, -0.0 kept), U rolled by
    `as` with its last `as` entries unchanged, U' = U + wn when T == 1; cs on either side of the kernel's 256-thread stride"""
    cs = as_ * T
    lo, hi, Uin, wn, _ = S.finalize_inputs(as_, T, B, np.random.default_rng(as_ * 1000 + T))
    r = _run(harness, tmp_path, S.case_finalize(B, as_, T, lo, hi, Uin, wn), S.OP_FINALIZE, B=B, cs=cs, as_=as_)
    for name in ("U", "control", "wn"):
        assert np.all(S.is_poison(r[name + "_guard"])), name
    Uo, control = S.finalize_ref(as_, T, lo, hi, Uin, wn)
    assert np.array_equal(S.bits(r["wn"]), S.bits(wn.reshape(-1)))
    assert np.array_equal(S.bits(r["control"]), S.bits(control.reshape(-1))), (r["control"], control)
    bad = np.flatnonzero(S.bits(r["U"]) != S.bits(Uo.reshape(-1)))
    assert bad.size == 0, (bad[:5], r["U"][bad[:5]], Uo.reshape(-1)[bad[:5]])


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("K", S.TRANSPOSE_K)
@pytest.mark.parametrize("cs", S.TRANSPOSE_CS)
def test_transpose_in(harness, tmp_path, cs, K, strided):
    """cs x K column-major -> [cs][K] on both sides of the 32-wide tiles; strided: each slot's matrix is the middle one of three, the other two hold
    a sentinel that must not appear"""
    x = S.transpose_values(B, cs, K, np.random.default_rng(cs * 1000 + K))
    if strided:
        src = np.full((B, 3, K, cs), S.SENTINEL)
        src[:, 1] = x
        case = S.case_transpose_in(B, cs, K, src, src_stride=3 * cs * K, src_off=cs * K)
    else:
        case = S.case_transpose_in(B, cs, K, x)
    r = _run(harness, tmp_path, case, S.OP_T_IN, B=B, cs=cs, K=K)
    dst = _clean(r, "dst")
    assert not np.any(dst == S.SENTINEL)
    assert np.array_equal(S.bits(dst), S.bits(S.transpose_in_ref(x).reshape(-1)))


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("K", S.TRANSPOSE_K)
@pytest.mark.parametrize("cs", S.TRANSPOSE_CS)
def test_transpose_out(harness, tmp_path, cs, K, shift):
    """[cs][K] -> cs x K column-major; with the shift pair dst = src + (A - B) in that order (float64, bit-exact); without it, fed with the device's
    own k_transpose_in result: T_OUT(T_IN(x)) = x"""
    rng = np.random.default_rng(cs * 1000 + K + 1)
    x = S.transpose_values(B, cs, K, rng)
    if shift:
        y = S.transpose_in_ref(x)
        A, Bv = rng.standard_normal((B, cs)) * 1e3, rng.standard_normal((B, cs))
        A[0, 0], Bv[0, 0] = 1e-9, 1.0                                   # (src + A) - B would differ from src + (A - B)
        r = _run(harness, tmp_path, S.case_transpose_out(B, cs, K, y, A, Bv), S.OP_T_OUT, B=B, cs=cs, K=K)
        assert np.array_equal(S.bits(_clean(r, "dst")), S.bits(S.transpose_out_ref(y, A, Bv).reshape(-1)))
        return
    y = _clean(_run(harness, tmp_path, S.case_transpose_in(B, cs, K, x), S.OP_T_IN, B=B, cs=cs, K=K), "dst")
    r = _run(harness, tmp_path, S.case_transpose_out(B, cs, K, y), S.OP_T_OUT, B=B, cs=cs, K=K)
    assert np.array_equal(S.bits(_clean(r, "dst")), S.bits(x.reshape(-1)))


@pytest.mark.parametrize("as_", [1, 2, 3])
def test_transposes_in_the_mppi_wrappers_shape(harness, tmp_path, as_):
    """launch_mppi_Z_in / launch_mppi_E_out call the transposes with B T batches of as x K"""
    T, K = 5, 257
    x = S.transpose_values(B * T, as_, K, np.random.default_rng(as_))
    y = _clean(_run(harness, tmp_path, S.case_transpose_in(B * T, as_, K, x), S.OP_T_IN, B=B * T, cs=as_, K=K), "dst")
    assert np.array_equal(S.bits(y), S.bits(S.transpose_in_ref(x).reshape(-1)))
    r = _run(harness, tmp_path, S.case_transpose_out(B * T, as_, K, y), S.OP_T_OUT, B=B * T, cs=as_, K=K)
    assert np.array_equal(S.bits(_clean(r, "dst")), S.bits(x.reshape(-1)))
