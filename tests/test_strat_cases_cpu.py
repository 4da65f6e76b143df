"""CPU proofs for the antithetic / Latin-hypercube draws (tests/helpers/strat_cases.py): the NumPy restatement of the keyed permutation is a
bijection, differs between rows / seeds / steps / iterations and is uniform; the restated inverse normal CDF stays inside its derived bound
against mpmath and is exactly antisymmetric; the harness's case files have the layout tools/kbench_strat.hip reads; the Python front end
refuses an unknown noise kind before the library is reached.  No GPU."""
import os
import re
import numpy as np
import pytest

from tests.helpers import strat_cases as sc
from tests.helpers import harness_io as hio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_constants_match_the_sources():
    strat, hdr, eng = _src("mpopis_amd", "csrc", "strat.h"), _src("include", "mpopis.h"), _src("mpopis_amd", "csrc", "engine.h")
    assert re.search(r"kStratTagKeys = 0x%08xu" % sc.TAG_KEYS, strat) and re.search(r"kStratTagJitter = 0x%08xu" % sc.TAG_JITTER, strat)
    assert "MPOPIS_NOISE_PHILOX = %d, MPOPIS_NOISE_ANTITHETIC = %d, MPOPIS_NOISE_LHS = %d" % (sc.PHILOX, sc.ANTITHETIC, sc.LHS) in hdr
    assert "kStratMaxK = 1 << 20" in eng and sc.MAX_K == 1 << 20
    for name in ("P0", "Q0", "P1", "Q1", "P2", "Q2"):                    # the coefficients, digit for digit
        body = re.search(r"const double %s\[\d\] = \{([^}]*)\}" % name, strat).group(1)
        assert [float(v) for v in body.replace("\n", " ").split(",")] == list(getattr(sc, name)), name
    from mpopis_amd import _lib
    assert _lib.NOISE_IDS == sc.KIND_IDS


@pytest.mark.parametrize("K", [1, 2, 3, 5, 63, 64, 65, 257, 4096])
def test_permutation_is_a_bijection(K):
    half = sc.half_bits(K)
    assert K == 1 or K <= 4 ** half < 4 * K                              # the Feistel domain: expected walks below 4
    keys = sc.round_keys(0x1234567890abcdef, 7, 3, np.arange(5))
    for r in range(5):
        pi, walks = sc.perm(K, keys[r])
        assert np.array_equal(np.sort(pi), np.arange(K))
        assert walks <= max(1, 4 ** half - K + 1)                        # the loop bound of strat_perm


def test_permutations_differ_between_rows_seeds_steps_and_iterations():
    K = 257
    base = dict(seed=20240001, step=5, it=2, r=3)
    ref = sc.perm(K, sc.round_keys(base["seed"], base["step"], base["it"], [base["r"]])[0])[0]
    for name, val in (("r", 4), ("seed", 20240002), ("seed", 20240001 + (1 << 32)), ("step", 6), ("it", 3)):
        a = dict(base)
        a[name] = val
        other = sc.perm(K, sc.round_keys(a["seed"], a["step"], a["it"], [a["r"]])[0])[0]
        assert not np.array_equal(ref, other), name
        assert np.mean(ref == other) < 0.05, name                        # (unrelated permutations agree in about 1 / K of the places)
    # the key stream and the jitter stream are disjoint from each other and from the tags in use
    assert sc.TAG_KEYS & sc.TAG_JITTER == 0 and (sc.TAG_KEYS | sc.TAG_JITTER) & 0xC0000000 == 0
    assert not np.array_equal(sc.round_keys(1, 0, 0, [0])[0, 0], sc.jitter_words(1, 0, 0, 0, 1)[0])


def test_permutation_is_uniform_at_K_8():
    """chi-square of the image of sample 0 and of sample 7 over 4096 rows of one seed against the uniform distribution on 8 strata: below the
    1 - 10^-6 quantile of chi-square with 7 degrees of freedom (40.52).  Found: 25.55 (k = 0) and 19.86 (k = 7)."""
    from scipy.stats import chi2
    keys = sc.round_keys(12345, 3, 1, np.arange(4096))
    P = np.stack([sc.perm(8, keys[r])[0] for r in range(4096)])
    limit = chi2.ppf(1 - 1e-6, 7)
    for k in (0, 7):
        cnt = np.bincount(P[:, k], minlength=8)
        stat = float(((cnt - 512.0) ** 2 / 512.0).sum())
        print("chi2 of pi_r(%d): %.3f (limit %.3f)" % (k, stat, limit))
        assert stat < limit


def test_jitter_words_are_the_documented_philox_call():
    from tests.helpers.sample_cases import philox_np
    seed, step, it, r, K = (1 << 32) + 77, 9, 1, 2, 5
    w = sc.jitter_words(seed, step, it, r, K)
    for k in range(K):
        assert w[k] == philox_np([[k, r, step, sc.TAG_JITTER | it, seed & 0xffffffff, seed >> 32]])[0, 0]
    assert np.array_equal(sc.round_keys(seed, step, it, [r])[0], philox_np([[r, 0, step, sc.TAG_KEYS | it, seed & 0xffffffff, seed >> 32]])[0])
    assert sc.xi_of(0) == 2.0 ** -33 and sc.xi_of(0xffffffff) == 1 - 2.0 ** -33


PHI_XI = (2.0 ** -33, 0.5, 1 - 2.0 ** -33)


@pytest.mark.parametrize("K", [1, 2, 3, 4096, 1 << 20])
def test_phi_inv_restatement_stays_inside_the_bound(K):
    pytest.importorskip("mpmath")
    strata = sorted({j for j in (0, 1, K // 2 - 1, K // 2, K - 1) if 0 <= j < K})
    j, xi = [a.ravel() for a in np.meshgrid(strata, PHI_XI, indexing="ij")]
    z = sc.phi_inv_f64(j, xi, K)
    err = sc.mp_err(z, sc.phi_inv_mp(j, xi, K))
    bound = sc.phi_inv_bound(j, xi, K)
    print("K %d: worst error %.3g, bounds %.3g .. %.3g, worst error / bound %.3f" % (K, err.max(), bound.min(), bound.max(), (err / bound).max()))
    assert np.all(bound < 1e-14) and np.all(bound > 2.0 ** -53)          # absolute, of order 1e-15, whatever |z| is (|z| reaches 8.2 here)
    assert np.all(err <= bound)
    # stratum j with jitter xi and stratum K - 1 - j with jitter 1 - xi: exact negatives
    assert np.array_equal(sc.phi_inv_f64(K - 1 - j, 1.0 - xi, K), -z)


def test_phi_inv_bound_on_random_device_inputs():
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(5)
    for K in (5, 257, 4096, 1 << 20):
        j = rng.integers(0, K, 150)
        xi = sc.xi_of(rng.integers(0, 1 << 32, 150, dtype=np.uint64))
        z = sc.phi_inv_f64(j, xi, K)
        assert np.all(sc.mp_err(z, sc.phi_inv_mp(j, xi, K)) <= sc.phi_inv_bound(j, xi, K))
        assert np.array_equal(sc.phi_inv_f64(K - 1 - j, 1.0 - xi, K), -z)


def test_phi_inv_bound_sees_a_wrong_coefficient(monkeypatch):
    """the bound is tight enough to notice the last printed digit of one coefficient changed by a few units"""
    pytest.importorskip("mpmath")
    j, xi, K = np.array([0, 3, 40, 400]), np.full(4, 0.5), 4096
    ref = sc.phi_inv_mp(j, xi, K)
    monkeypatch.setattr(sc, "P1", sc.P1[:4] + (sc.P1[4] * (1 + 1e-13),) + sc.P1[5:])
    assert np.any(sc.mp_err(sc.phi_inv_f64(j, xi, K), ref) > sc.phi_inv_bound(j, xi, K))


def test_truncation_constants_hold_on_a_coarser_grid():
    mp = pytest.importorskip("mpmath")
    with mp.workdps(40):
        for region in ("centre", "tail1", "tail2"):
            worst = max(abs(sc.formula_mp(p, region) - sc.truth_mp(p)) for p in sc.trunc_points(region, 150))
            print("%s: %.3g (constant %.3g)" % (region, float(worst), sc.TRUNC[region]))
            assert worst <= sc.TRUNC[region] / 2 * 1.0001


def test_slope_of_the_tail_correction_is_what_the_bound_assumes():
    """_ratio propagates the error of 1 / t with the polynomials' own slope bounds; they must dominate a finite difference of the formula"""
    z = np.linspace(1 / 8.6, 0.5, 400)
    for P, Q in ((sc.P1, sc.Q1), (sc.P2, sc.Q2)):
        v0, e0 = sc._ratio(z, 0.0, P, Q)
        v1, _ = sc._ratio(z + 1e-7, 0.0, P, Q)
        _, e = sc._ratio(z, 1e-7, P, Q)
        assert np.all(np.abs(v1 - v0) <= e)


def test_case_files_round_trip():
    seeds, active = sc.GEN_SEEDS, sc.GEN_ACTIVE
    op, B, ip, dp, arrays = hio.unpack_case(sc.MAGIC_IN, sc.case_gen(3, 5, 65, 1, 1, sc.LHS, seeds, active, 11, 2))
    assert (op, B, ip, dp) == (sc.OP_GEN, 3, [5, 65, 1, 1, sc.LHS, 11, 2, 1], [])
    assert [t for t, _ in arrays] == [hio.I32, hio.U64] and np.array_equal(arrays[1][1], np.array(seeds, dtype=np.uint64))
    op, B, ip, _, arrays = hio.unpack_case(sc.MAGIC_IN, sc.case_rows(sc.OP_JITTER, 3, 2, 7, seeds, active, 4, 0))
    assert (op, B, ip) == (sc.OP_JITTER, 3, [2, 7, 4, 0]) and np.array_equal(arrays[0][1], active)
    op, B, ip, _, arrays = hio.unpack_case(sc.MAGIC_IN, sc.case_phi_inv([0, 4095], [0, 0xffffffff], 4096))
    assert (op, B, ip) == (sc.OP_PHIINV, 1, [4096, 2]) and np.array_equal(arrays[2][1].view(np.uint32), [0, 0xffffffff])
    body = np.arange(6, dtype=np.float64)
    buf = hio.pack_result(sc.MAGIC_OUT, 0, [(hio.F64, np.concatenate([body, hio.poisoned(hio.GUARD)]))])
    got, guard = sc.unpack_result(buf)
    assert np.array_equal(got, body) and hio.is_poison(guard).all()
    assert len(sc.gen_shapes()) == 2 * 7 * (1 + 2 + 1)


def test_antithetic_source_columns():
    k0, sign, lin = sc.antithetic_source(2, 5, 2, 0)
    assert list(k0) == [0, 1, 2, 0, 1] and list(sign) == [1, 1, 1, -1, -1] and lin.shape == (2, 5)     # odd K: column 2 has no partner
    k0, sign, _ = sc.antithetic_source(1, 1, 1, 1)
    assert list(k0) == [0] and list(sign) == [1]


@pytest.mark.parametrize("fn", ["simulate_car_racing", "simulate_mountaincar", "simulate_cartpole"])
def test_examples_refuse_an_unknown_noise_kind_before_the_library(monkeypatch, fn):
    from mpopis_amd import examples, _lib

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(_lib.MPOPISError) as e:
        getattr(examples, fn)(num_trials=1, num_steps=1, noise="sobol", quiet=True)
    assert e.value.code == _lib.ERR_ARG and "sobol" in str(e.value)
    assert [_lib.noise_id(k) for k in ("philox", ":antithetic", "lhs")] == [0, 1, 2]


def test_python_surface_names_the_new_calls():
    from mpopis_amd import _lib, engine, policies
    for name in ("mpopis_set_noise_kind", "mpopis_get_noise_kind", "mpopis_draw_normals"):
        assert name in _lib.ABI_SYMBOLS
    assert all(hasattr(engine.Engine, n) for n in ("set_noise_kind", "noise_kind", "draw_normals"))
    assert isinstance(policies.AbstractPathIntegralPolicy.noise_kind, property)
