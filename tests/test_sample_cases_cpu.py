"""The helpers, references and bounds of tests/test_gpu_sample_harness.py are what they claim -- shown on the CPU with the oracle and NumPy alone
(tests/helpers/sample_cases.py holds what both files share): the NumPy Philox is the oracle's and Random123's; the `lin` maps of both draw orders are
permutations and the predicted forms reach every kernel; the directed Box-Muller words hold both ends of every log-table interval and every sector
of the tables philox.h declares; a float64 restatement of the device arithmetic stays within the derived bound on all of them while three subtly
wrong restatements do not; the long double references agree with the oracle's stream; the harness's files round-trip."""
from fractions import Fraction
import numpy as np
import pytest
from tests.helpers import sample_cases as S


def test_tables_are_the_size_philox_h_declares_and_long_double_is_wider():
    assert S.table_sizes() == (S.TAB_LOG, S.TAB_SC, S.TAB_DOUBLES)
    assert np.finfo(np.longdouble).nmant >= 63
    t = S.table_ref()
    assert t.shape == (S.TAB_DOUBLES,) and t[2 * S.TAB_LOG - 2] == 1 and t[2 * S.TAB_LOG - 1] == 0
    i = np.arange(S.TAB_LOG - 1)
    assert np.allclose((1 / t[0:2 * S.TAB_LOG - 2:2]).astype(float), 0.5 * (1 + (i + 0.5) / S.TAB_LOG), rtol=1e-15)
    th = 2 * np.pi * (np.arange(S.TAB_SC) + 0.5) / S.TAB_SC
    assert np.allclose(t[2 * S.TAB_LOG::2].astype(float), np.sin(th), atol=1e-15) and np.allclose(t[2 * S.TAB_LOG + 1::2].astype(float), np.cos(th), atol=1e-15)
    s2 = t[2 * S.TAB_LOG::2] ** 2 + t[2 * S.TAB_LOG + 1::2] ** 2
    assert np.max(np.abs(s2 - 1)) < 2.0 ** -60                                          # sin^2 + cos^2 in long double


def test_the_tables_log_restated_in_float64_is_within_one_ulp():
    """rng_tab_log (kernels_sample.hip: 2 atanh((c - 1)/(c + 1)) with the quotient carried in two doubles) on the 256 nodes"""
    i = np.arange(S.TAB_LOG)
    c = 0.5 * (1 + (i + 0.5) / S.TAB_LOG)
    c[-1] = 1.0
    got, ref = S.tab_log_device_f64(c), S.table_ref()[1:2 * S.TAB_LOG:2]
    assert got[-1] == 0.0 and not np.signbit(got[-1])
    err = (np.abs(got.astype(np.longdouble) - ref)[:-1] / S.ulp_of(ref.astype(np.float64))[:-1]).astype(np.float64)
    print("table log restated: %d of %d not correctly rounded, worst %.3f ulp" % (int((got != ref.astype(np.float64)).sum()), got.size, err.max()))
    assert err.max() <= 0.6


def test_numpy_philox_is_the_oracle_and_random123(oracle):
    for c, k, out in S.KAT:
        assert S.philox_np([c + k])[0].tolist() == out == oracle.philox4x32_10(c, k)
    sets = S.directed_philox_sets(np.random.default_rng(5))
    assert sets.shape == (3 + 6 * 4 * 9, 6) and sets.dtype == np.uint32
    for pos in range(6):                                                               # each word at each corner value
        assert {0, 1, 1 << 31, 0xffffffff} <= set(sets[:, pos].tolist())
    got = S.philox_np(sets)
    for s, g in zip(sets.tolist(), got.tolist()):
        assert g == oracle.philox4x32_10(s[:4], s[4:]), s
    q = np.array([0, 1, 0xffffffff, 1 << 32, (1 << 40) + 3], dtype=np.uint64)
    cs = S.stream_call_sets((1 << 32) + 77, 7, 3, q)
    assert cs[4].tolist() == [3, 256, 7, 3, 77, 1]


def test_stream_words_and_the_long_double_definition_give_the_oracles_normals(oracle):
    for seed, (slo, shi), n in ((S.NORMALS_SEEDS[0], S.NORMALS_STREAM, 1001), (S.NORMALS_SEEDS[1], (0, 0), 64), (S.NORMALS_SEEDS[2], (5, 0x40000000), 4000)):
        wr, wa = S.stream_words(seed, slo, shi, n)
        z0, z1 = S.bm_ref(wr, wa)
        z = np.stack([z0, z1], axis=1).reshape(-1).astype(np.float64)[:n]
        assert np.max(np.abs(z - oracle.philox_normals(seed, slo, shi, n))) <= S.RNG_TOL / 10


@pytest.mark.parametrize("mppi,cs,K,as_,T", S.normals_shapes() + S.CROSS_FORM_SHAPES)
def test_lin_maps_are_permutations(mppi, cs, K, as_, T):
    assert cs == as_ * T
    lin = S.lin_map(cs, K, as_, mppi)
    assert lin.shape == (cs, K) and sorted(lin.reshape(-1).tolist()) == list(range(cs * K))
    if mppi:                                                                           # rand(rng, as, K, T) column-major: a fastest, then k, then t
        assert np.array_equal(lin.reshape(T, as_, K).transpose(0, 2, 1).reshape(-1), np.arange(cs * K))
    else:                                                                              # randn!(cs x K) column-major
        assert np.array_equal(lin.T.reshape(-1), np.arange(cs * K))
    form = S.predicted_form(cs, as_, mppi)
    if form != S.SINGLE:                                                               # a draw pair (2p, 2p + 1) sits in adjacent rows of one sample
        assert np.all(lin[0::2] % 2 == 0) and np.array_equal(lin[1::2], lin[0::2] + 1)
    if form == S.QUAD:
        assert np.all(lin[0::4] % 4 == 0) and np.array_equal(lin[3::4], lin[0::4] + 3)


def test_the_listed_shapes_reach_every_form():
    shapes = S.normals_shapes()
    assert len(shapes) == 11 * 2 + 3 * 4 + 8 * 3
    g = {S.predicted_form(cs, a, m) for m, cs, K, a, T in shapes if not m}
    p = {S.predicted_form(cs, a, m) for m, cs, K, a, T in shapes if m}
    assert g == {S.SINGLE, S.PAIR, S.QUAD} and p == {S.SINGLE, S.PAIR}
    assert {S.predicted_form(cs, a, m) for m, cs, K, a, T in S.CROSS_FORM_SHAPES} == {S.SINGLE, S.PAIR, S.QUAD}
    assert all(cs * K == S.CROSS_FORM_N for m, cs, K, a, T in S.CROSS_FORM_SHAPES)
    assert [S.predicted_form(4, 2, 1), S.predicted_form(4, 1, 1), S.predicted_form(6, 2, 0), S.predicted_form(8, 1, 0), S.predicted_form(21, 1, 0)] == \
        [S.PAIR, S.SINGLE, S.PAIR, S.QUAD, S.SINGLE]
    assert len(set(S.NORMALS_SEEDS)) == 3 and max(S.NORMALS_SEEDS) >= 1 << 32
    d = S.normals_dscale(3, 1, np.random.default_rng(0))
    assert d.min() < 0 and np.any(d == 0)


def test_directed_words_hold_both_ends_of_every_interval_and_every_sector():
    n_log, n_sc, _ = S.table_sizes()
    wr = S.directed_wr().astype(np.int64)
    assert {0, 1, 0xfffffffe, 0xffffffff} <= set(wr.tolist())
    assert all(x in wr for e in range(33) for x in ((1 << e) - 1, 1 << e) if x <= 0xffffffff)
    k, i = S.log_interval(wr)
    have = set(wr.tolist())
    for kk in S.BM_EXPONENTS:
        at = k == kk
        assert at.any(), kk
        if kk >= -16:                                                                  # 2^(23 + k) words per interval: all n_log intervals, both ends
            assert set(i[at].tolist()) == set(range(n_log)), kk
        for ii in set(i[at].tolist()):
            lo, hi = wr[at & (i == ii)].min(), wr[at & (i == ii)].max()
            for w, nb in ((lo, lo - 1), (hi, hi + 1)):                                 # an end: the neighbouring word lies in another interval
                if 0 <= nb <= 0xffffffff:
                    kn, inn = S.log_interval(np.array([nb]))
                    assert (kn[0], inn[0]) != (kk, ii), (kk, ii, w)
    assert S.log_interval(np.array([0]))[0][0] == -32 and S.log_interval(np.array([0xffffffff]))[1][0] == n_log - 1
    wa = S.directed_wa().astype(np.int64)
    assert wa.size == 5 * n_sc and set((wa >> 25).tolist()) == set(range(n_sc))
    width = (1 << 32) // n_sc
    for j in range(n_sc):
        assert {j * width, j * width + 1, j * width + width // 2 - 1, j * width + width // 2, (j + 1) * width - 1} <= set(wa.tolist())
    for quarter in (1 << 30, 1 << 31, 3 << 30):                                        # the words either side of u = 1/4, 1/2, 3/4
        assert quarter - 1 in wa and quarter in wa
    dr, da = S.directed_pairs()
    assert 2e4 < dr.size < 1e5
    assert set(S.reduced_wr().tolist()) <= have and set(S.reduced_wa().tolist()) <= set(wa.tolist())


def test_fma_restatement_rounds_once():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(400), rng.standard_normal(400)
    c = -a * b * (1 + rng.standard_normal(400) * 2.0 ** -30)                             # heavy cancellation
    got = S.fma(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        assert abs(Fraction(float(g)) - exact) <= Fraction(float(np.spacing(abs(g)))) * Fraction(513, 1024)


def test_float64_restatement_stays_within_the_derived_bound_and_three_mutations_do_not():
    wr, wa = S.directed_pairs()
    tab = S.table_f64()
    z0, z1 = S.bm_device_f64(wr, wa, tab)
    ratio, ulps = S.bm_ratio(z0, z1, wr, wa)
    print("RATIO BOXMULLER restatement, directed: %.4f  worst error %.2f ulp of a unit normal" % (ratio.max(), ulps.max()))
    assert np.all(ratio <= 1.0), (wr[np.argmax(ratio)], wa[np.argmax(ratio)], ratio.max())
    assert ratio.max() > 0.1                                                           # the bound is not slack by an order of magnitude
    r0, r1 = S.bm_ref(wr, wa)
    assert max(np.max(np.abs(z0 - r0.astype(float))), np.max(np.abs(z1 - r1.astype(float)))) <= S.RNG_TOL
    for mut in S.MUTATIONS:
        m0, m1 = S.bm_device_f64(wr, wa, tab, mutate=mut)
        mr, _ = S.bm_ratio(m0, m1, wr, wa)
        print("RATIO BOXMULLER %s: %.3g, %d of %d pairs beyond the bound" % (mut, mr.max(), int((mr > 1).sum()), mr.size))
        assert mr.max() > 1.0, mut
    # r^5 / 5 dropped stays far inside the outer contract at ordinary radii: RNG_TOL alone cannot see it
    m0, m1 = S.bm_device_f64(wr, wa, tab, mutate="r5_dropped")
    bulk = np.sqrt(-2 * np.log((wr.astype(float) + 0.5) * 2.0 ** -32)) > 0.5
    assert np.max(np.abs(m0 - r0.astype(float))[bulk]) < S.RNG_TOL


def test_float64_restatement_on_random_words():
    wr, wa = S.random_pairs(1 << 16, seed=7)
    z0, z1 = S.bm_device_f64(wr, wa, S.table_f64())
    ratio, ulps = S.bm_ratio(z0, z1, wr, wa)
    print("RATIO BOXMULLER restatement, random: %.4f  worst error %.2f ulp" % (ratio.max(), ulps.max()))
    assert np.all(ratio <= 1.0)


def test_the_bound_blows_up_nowhere():
    """It scales with R: at u1 -> 1 (top interval: table entry (1, 0), the sum exact) it stays a few ulp of R, at the 6.76 sigma end a few ulp of R
    too; at the far end of the top interval the r^6 / 6 remainder is about 20 ulp of log u1 (philox.h says so): 10.7 x 2^-52 more, relative to R"""
    wa = S.directed_wa()
    for w, ulps in ((0xffffffff, 12), (0xfffffffe, 12), (S.interval_ends(0)[S.TAB_LOG - 1][0], 12 + 11), (0, 12), (1, 12)):
        wr = np.full(wa.size, w, dtype=np.uint32)
        b0, b1 = S.bm_bound(wr, wa)
        R = np.sqrt(-2 * np.log((w + 0.5) * 2.0 ** -32))
        assert np.all(np.isfinite(b0)) and np.all(np.isfinite(b1))
        assert max(b0.max(), b1.max()) <= ulps * 2.0 ** -52 * R, (w, max(b0.max(), b1.max()) / (2.0 ** -52 * R))
    wr, wa = S.directed_pairs()
    b0, b1 = S.bm_bound(wr, wa)
    assert max(b0.max(), b1.max()) < S.RNG_TOL / 5 and min(b0.min(), b1.min()) > 0


def test_finalize_inputs_and_reference(oracle):
    seen = set()
    for as_, T in S.FINALIZE_SHAPES:
        lo, hi, Uin, wn, want = S.finalize_inputs(as_, T, 3, np.random.default_rng(as_ * 1000 + T))
        cs = as_ * T
        Uo, control = S.finalize_ref(as_, T, lo, hi, Uin, wn)
        wc = Uin + wn
        for (b, a), kind in want.items():
            seen.add(kind)
            c = control[b, a]
            exp = {"below": lo[a], "lo": lo[a], "hi": hi[a], "above": hi[a], "+inf": hi[a], "-inf": lo[a]}.get(kind)
            if exp is not None:
                assert c == exp and (kind not in ("lo", "hi") or wc[b, a] == exp), (kind, c)
            elif kind == "nan":
                assert np.isnan(c)
            elif kind == "-0":
                assert c == 0 and np.signbit(c)
            else:
                assert lo[a] < c < hi[a] and c == wc[b, a]
        if 3 * as_ >= len(S.FINALIZE_KINDS):
            assert set(want.values()) == set(S.FINALIZE_KINDS)
        if T > 1:
            assert np.array_equal(S.bits(Uo[:, cs - as_:]), S.bits(Uin[:, cs - as_:]))          # the alias quirk
            assert np.array_equal(S.bits(Uo[:, :cs - as_]), S.bits(wc[:, as_:]))
        else:
            assert np.array_equal(S.bits(Uo), S.bits(wc))
    assert seen == set(S.FINALIZE_KINDS)
    assert sorted(a * t for a, t in S.FINALIZE_SHAPES) == sorted([1, 2, 4, 100, 300, 256, 16, 272])
    # the oracle's own roll (tests/test_oracle_kat.py::test_roll_U_alias_quirk) through the reference
    Uo, c = S.finalize_ref(2, 3, np.full(16, -1.0), np.full(16, 1.0), np.array([[0.1, 0.2, 0.3, 0.4, 0.5, 0.6]]), np.zeros((1, 6)))
    assert Uo.tolist() == [[0.3, 0.4, 0.5, 0.6, 0.5, 0.6]] and c.tolist() == [[0.1, 0.2]]


def test_transpose_references():
    rng = np.random.default_rng(1)
    x = S.transpose_values(3, 33, 31, rng)
    assert np.unique(x).size == x.size and not np.any(x == S.SENTINEL)
    y = S.transpose_in_ref(x)
    assert y.shape == (3, 33, 31) and y[1, 5, 7] == x[1, 7, 5]
    assert np.array_equal(S.transpose_out_ref(y), x)
    A, Bv = rng.standard_normal((3, 33)), rng.standard_normal((3, 33))
    assert S.transpose_out_ref(y, A, Bv)[2, 9, 4] == y[2, 4, 9] + (A[2, 4] - Bv[2, 4])


def test_harness_files_round_trip():
    rng = np.random.default_rng(2)
    buf = S.case_normals(3, 6, 5, 2, 3, 1, S.NORMALS_SEEDS, 11, 0x80000002, S.NORMALS_ACTIVE, dscale=rng.random((3, 6)), no_active=True)
    h, payload = S.unpack_case_header(buf)
    assert (h["op"], h["B"], h["cs"], h["K"], h["as"], h["T"], h["mppi"], h["flags"], h["slo"], h["shi"]) == (S.OP_NORMALS, 3, 6, 5, 2, 3, 1, 3, 11, 0x80000002)
    assert len(payload) == 3 * 8 + 3 * 4 + 18 * 8 and np.frombuffer(payload, dtype=np.uint64, count=3).tolist() == list(S.NORMALS_SEEDS)
    h, payload = S.unpack_case_header(S.case_normalq([((1 << 32) + 5, 0xFFFFFFFF, 0x80000002, (1 << 40) + 3)]))
    assert h["n"] == 1 and np.frombuffer(payload, dtype=np.uint64).tolist() == [(1 << 32) + 5, 0x80000002FFFFFFFF, (1 << 40) + 3]
    h, payload = S.unpack_case_header(S.case_transpose_in(2, 3, 4, np.zeros(100), src_stride=36, src_off=12))
    assert (h["n"], h["src_stride"], h["src_off"], len(payload)) == (100, 36, 12, 800)
    shapes = {S.OP_TAB: {}, S.OP_WORDS: dict(n=7), S.OP_BOXMULLER: dict(n=9), S.OP_NORMALQ: dict(n=3), S.OP_NORMALS: dict(B=3, cs=5, K=7),
              S.OP_DRAWS: dict(B=3, K=11), S.OP_FINALIZE: dict(B=3, cs=6, as_=2), S.OP_T_IN: dict(B=2, cs=3, K=5), S.OP_T_OUT: dict(B=2, cs=3, K=5)}
    for op, shape in shapes.items():
        arrays = []
        for name, dt, cnt in S.result_layout(op, **shape):
            a = np.frombuffer(b"\xa5" * ((cnt + S.GUARD) * np.dtype(dt).itemsize), dtype=dt).copy()
            a[:cnt] = np.arange(cnt)
            arrays.append(a)
        r = S.unpack_result(S.pack_result(S.PAIR, arrays), op, **shape)
        assert r["form"] == S.PAIR
        for (name, dt, cnt), a in zip(S.result_layout(op, **shape), arrays):
            assert np.array_equal(r[name], a[:cnt]) and np.all(S.is_poison(r[name + "_guard"])) and r[name + "_guard"].size == S.GUARD
            assert not np.any(S.is_poison(r[name]))
