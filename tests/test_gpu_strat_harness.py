"""The antithetic / Latin-hypercube generator (kernels_strat.hip) and the pieces of strat.h it is made of, exercised directly through the C++
harness tools/kbench_strat.hip: one process per launch, inputs written by the test, the raw device output read back.  The permutation and the
jitter words must equal the NumPy restatement bit for bit; the inverse normal CDF and the full generator must stay within the derived bound
phi_inv_bound of the 40-digit value and be exactly antisymmetric; the antithetic draw's first half must be the Philox kind's normals, bit for
bit, and the rest their exact negations.  References: tests/helpers/strat_cases.py (proved on the CPU by tests/test_strat_cases_cpu.py), never
the engine.  The harness poisons the output first: an inactive slot's rows and the guard must stay untouched."""
import numpy as np
import pytest
from tests.helpers import harness_run as HR
from tests.helpers import strat_cases as sc

pytestmark = pytest.mark.gpu
B = 3
STEP, IT = sc.GEN_STREAM
MIRROR = {}                                                           # (cs, K) -> the PHIINV probe on the mirrored inputs of the LHS cases


@pytest.fixture(scope="module")
def harness():
    return HR.build("strat")


def _run(exe, tmp_path, case, shape):
    body, guard = sc.unpack_result(HR.run_case(exe, tmp_path, case))
    assert np.all(sc.is_poison(guard))
    return body.reshape(shape)


def _check_slots(a):
    """the inactive slot's rows untouched, no active entry left at the poison"""
    for b, on in enumerate(sc.GEN_ACTIVE):
        p = sc.is_poison(a[b])
        assert (not p.any()) if on else p.all(), b


@pytest.fixture(scope="module")
def lhs_ref():
    """{(cs, K): (j, x, 40-digit values of the active slots)}: shared by the cases of both orders"""
    pytest.importorskip("mpmath")
    cache = {}

    def get(cs, K):
        if (cs, K) not in cache:
            j, x = sc.lhs_inputs(sc.GEN_SEEDS, sc.GEN_ACTIVE, STEP, IT, cs, K)
            on = np.array(sc.GEN_ACTIVE, dtype=bool)
            cache[(cs, K)] = (j, x, sc.phi_inv_mp(j[on].ravel(), sc.xi_of(x[on].ravel()), K))
        return cache[(cs, K)]
    return get


@pytest.mark.parametrize("cs,K", [(cs, K) for cs in (1, 2, 5) for K in (1, 2, 3, 5, 64, 65, 257)])
def test_permutation_and_jitter_equal_the_restatement(harness, tmp_path, cs, K):
    j_ref, x_ref = sc.lhs_inputs(sc.GEN_SEEDS, sc.GEN_ACTIVE, STEP, IT, cs, K)
    on = np.array(sc.GEN_ACTIVE, dtype=bool)
    j = _run(harness, tmp_path, sc.case_rows(sc.OP_PERM, B, cs, K, sc.GEN_SEEDS, sc.GEN_ACTIVE, STEP, IT), (B, cs, K))
    _check_slots(j)
    assert np.array_equal(j[on], j_ref[on])
    assert np.array_equal(np.sort(j[on], axis=-1), np.broadcast_to(np.arange(K), (2, cs, K)))        # every row a permutation of the strata
    x = _run(harness, tmp_path, sc.case_rows(sc.OP_JITTER, B, cs, K, sc.GEN_SEEDS, sc.GEN_ACTIVE, STEP, IT), (B, cs, K))
    _check_slots(x)
    assert np.array_equal(x[on].view(np.uint32), x_ref[on])


@pytest.mark.parametrize("K", [1, 2, 3, 4096, 1 << 20])
def test_phi_inv_probe_within_the_bound_and_antisymmetric(harness, tmp_path, K):
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(K)
    strata = sorted({j for j in (0, 1, K // 2 - 1, K // 2, K - 1) if 0 <= j < K})
    xs = np.array([0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff], dtype=np.uint64)
    j, x = [a.ravel() for a in np.meshgrid(strata, xs, indexing="ij")]
    j = np.concatenate([j, rng.integers(0, K, 200)])
    x = np.concatenate([x, rng.integers(0, 1 << 32, 200, dtype=np.uint64)])
    jj, xx = np.concatenate([j, K - 1 - j]), np.concatenate([x, 0xffffffff - x])                       # every input and its mirror image
    z = _run(harness, tmp_path, sc.case_phi_inv(jj, xx, K), (2, j.size))
    assert not sc.is_poison(z).any()
    assert np.array_equal(z[1], -z[0])                                                                # exact negatives
    err = sc.mp_err(z[0], sc.phi_inv_mp(j, sc.xi_of(x), K))
    bound = sc.phi_inv_bound(j, sc.xi_of(x), K)
    print("PHIINV K %d: worst error %.3g, worst error / bound %.3f, off the restatement in %d of %d" % (
        K, err.max(), (err / bound).max(), int(np.sum(z[0] != sc.phi_inv_f64(j, sc.xi_of(x), K))), j.size))
    assert np.all(err <= bound)


@pytest.mark.parametrize("mppi,cs,K,as_", sc.gen_shapes())
def test_lhs_generator(harness, tmp_path, lhs_ref, mppi, cs, K, as_):
    j, x, ref = lhs_ref(cs, K)
    on = np.array(sc.GEN_ACTIVE, dtype=bool)
    Z = _run(harness, tmp_path, sc.case_gen(B, cs, K, as_, mppi, sc.LHS, sc.GEN_SEEDS, sc.GEN_ACTIVE, STEP, IT), (B, cs, K))
    _check_slots(Z)
    err = sc.mp_err(Z[on].ravel(), ref)
    assert np.all(err <= sc.phi_inv_bound(j[on].ravel(), sc.xi_of(x[on].ravel()), K))
    # one sample per stratum in every row: sorted by value, a row's samples come in the order of their strata
    assert np.array_equal(np.argsort(Z[on], axis=-1), np.argsort(j[on], axis=-1))
    # antisymmetry, bit for bit: the device's value for the mirrored input (K - 1 - j, ~x), from the probe (one launch per (cs, K))
    if (cs, K) not in MIRROR:
        MIRROR[(cs, K)] = _run(harness, tmp_path, sc.case_phi_inv((K - 1 - j[on]).ravel(), (0xffffffff - x[on].astype(np.uint64)).ravel(), K), Z[on].shape)
    assert np.array_equal(MIRROR[(cs, K)], -Z[on])


@pytest.mark.parametrize("mppi,cs,K,as_", sc.gen_shapes())
def test_antithetic_generator(harness, tmp_path, mppi, cs, K, as_):
    on = np.array(sc.GEN_ACTIVE, dtype=bool)
    Z = _run(harness, tmp_path, sc.case_gen(B, cs, K, as_, mppi, sc.ANTITHETIC, sc.GEN_SEEDS, sc.GEN_ACTIVE, STEP, IT), (B, cs, K))
    _check_slots(Z)
    P = _run(harness, tmp_path, sc.case_gen(B, cs, K, as_, mppi, sc.PHILOX, sc.GEN_SEEDS, sc.GEN_ACTIVE, STEP, IT), (B, cs, K))
    _check_slots(P)
    h = (K + 1) // 2
    assert np.array_equal(Z[on][:, :, :h], P[on][:, :, :h])                                           # the Philox kind's normals, bit for bit
    assert np.array_equal(Z[on][:, :, h:], -Z[on][:, :, :K - h])                                      # exact negations (odd K: column h - 1 alone)
    if K > 1:
        assert not np.array_equal(Z[on][:, :, h:], P[on][:, :, h:])


def test_generator_without_an_active_array(harness, tmp_path):
    """active == nullptr (how mpopis_draw_normals launches it): every slot is written"""
    for kind in (sc.ANTITHETIC, sc.LHS):
        Z = _run(harness, tmp_path, sc.case_gen(B, 2, 65, 2, 0, kind, sc.GEN_SEEDS, sc.GEN_ACTIVE, STEP, IT, no_active=True), (B, 2, 65))
        assert not sc.is_poison(Z).any()
        A = _run(harness, tmp_path, sc.case_gen(B, 2, 65, 2, 0, kind, sc.GEN_SEEDS, sc.GEN_ACTIVE, STEP, IT), (B, 2, 65))
        assert np.array_equal(Z[0], A[0]) and np.array_equal(Z[2], A[2])
