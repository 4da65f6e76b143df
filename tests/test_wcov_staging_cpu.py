"""The case list of tests/test_gpu_wcov_staging.py (tests/helpers/wcov_staging_cases.py) is well-formed and reaches what it claims, shown on the CPU:
every case takes the pair-list form with 64-column chunks, the row counts, column counts, split counts, weight sources, ones row on / off, gathered /
contiguous columns and the fourth-moment variant are all there, splits end empty, inside a chunk and on a chunk boundary, and a plain float64 evaluation
in the kernel's own plan stays within a quarter of every case's derived bound against the longdouble reference -- the bound tests the kernel, not the
input."""
import numpy as np
import pytest
from tests.helpers import mfma_cases as M
from tests.helpers import wcov_staging_cases as W

LD = M.LD


@pytest.fixture(scope="module")
def cases():
    return [W.build(s) for s in W.specs()]


def _src(c):
    return "cost" if c["cost"] is not None else "w" if c["w"] is not None else "none"


def test_every_case_takes_the_pair_list_with_64_column_chunks(cases):
    ids = [W.case_id(s) for s in W.specs()]
    assert len(set(ids)) == len(ids)
    for c in cases:
        partial, sq, aug, from_cost = M.case_form(c)
        assert partial == M.WCOV_PAIR64, (c["cs"], c["ksplit"])
        assert sq == (c["variant"] in ("ss", "lw")) and from_cost == (c["variant"] == "cost" and aug)
        assert M.unpack_case(c["data"])[0] == M.OP_WCOV


def test_the_list_reaches_what_it_claims(cases):
    plain = [c for c in cases if c["rscale"] is None]
    assert {c["cs"] for c in plain} == set(W.CS) == {96, 97, 100, 101, 111, 112, 20, 80}
    assert {(c["m"], c["ksplit"]) for c in plain if c["cs"] == 100 and c["idx"] is None and c["want_mu"]} == {(m, ks) for m in W.MS for ks in W.SPLITS}
    for m in W.MS[1:]:                                                    # (a lone column takes no +inf cost)
        assert {_src(c) for c in plain if c["cs"] == 100 and c["m"] == m and c["idx"] is None} == {"cost", "w", "none"}, m
    for ks in W.SPLITS:
        assert {_src(c) for c in plain if c["cs"] == 100 and c["ksplit"] == ks and c["idx"] is None} == {"cost", "w", "none"}, ks
    for cs in W.CS:
        assert {_src(c) for c in plain if c["cs"] == cs} == {"cost", "w", "none"}, cs
        assert len({c["m"] for c in plain if c["cs"] == cs}) >= 3 and {c["ksplit"] for c in plain if c["cs"] == cs} == {1, 2, 6}, cs
    assert {c["m"] for c in cases} == {1, 63, 64, 65, 130, 257}
    ends = set()
    for c in cases:
        ends |= W.chunk_ends(c)
    assert ends == {"empty", "mid", "boundary"}
    assert any(W.chunk_ends(c) == {"empty", "mid", "boundary"} for c in cases)           # m = 257 in six splits: four full, one of one column, one empty
    # ones row on and off, for gathered and for contiguous columns; the shapes without room for it never have it
    for gathered in (False, True):
        assert {M.case_form(c)[2] for c in plain if (c["idx"] is not None) == gathered and c["cs"] % 16} == {True, False}, gathered
    assert not any(M.case_form(c)[2] for c in cases if c["cs"] % 16 == 0)
    assert {c["variant"] for c in cases if c["idx"] is not None} >= {"idx", "idx_w", "ss", "lw"}
    sq = [c for c in cases if c["rscale"] is not None]
    assert len(sq) >= 3 and all(c["cs"] == 100 for c in sq)
    for c in cases:
        if c["cost"] is not None:                                         # a +inf cost: its weight is exactly 0
            assert np.all(np.isinf(c["cost"]).sum(axis=1) >= 1)
            w = M._wcov_inputs(dict(c, w=None), int(np.flatnonzero(c["active"])[0]))[1]
            assert np.all(w[np.isinf(c["cost"][int(np.flatnonzero(c["active"])[0])])] == 0) and w.max() == 1


def test_float64_emulation_is_well_inside_every_bound(cases):
    worst = {"S": 0.0, "mu": 0.0}
    for c in cases:
        for b in np.flatnonzero(c["active"]):
            ref = M.wcov_reference(c, b)
            S, mu = M.wcov_emulation(c, b)
            assert np.all(ref["S_bound"] >= 0) and np.all(np.isfinite(ref["S"].astype(np.float64)))
            err = np.abs(S.astype(LD) - ref["S"])
            assert np.all(err[ref["S_bound"] == 0] == 0)
            worst["S"] = max(worst["S"], float(np.max(np.where(ref["S_bound"] == 0, 0, err / np.where(ref["S_bound"] == 0, 1, ref["S_bound"])))))
            if mu is not None and c["mu"] is None:
                e = np.abs(mu.astype(LD) - ref["mean"])
                assert np.all(e[ref["mean_bound"] == 0] == 0)
                worst["mu"] = max(worst["mu"], float(np.max(np.where(ref["mean_bound"] == 0, 0, e / np.where(ref["mean_bound"] == 0, 1, ref["mean_bound"])))))
    print("worst emulation error / bound:", worst)
    assert worst["S"] <= 0.25 and worst["mu"] <= 0.25, worst


def test_the_poisoned_case_differs_only_where_nothing_may_read():
    c = W.build(dict(cs=100, K=W.GATHER_K, ksplit=2, variant="idx", m=65))
    p = W.poisoned(c)
    assert np.array_equal(p["idx"][:, :65], c["idx"][:, :65]) and not np.array_equal(p["idx"][:, 65:], c["idx"][:, 65:])
    for b in range(c["B"]):
        used = c["idx"][b, :65]
        assert np.array_equal(p["X"][b][:, used], c["X"][b][:, used])
        assert np.all(p["X"][b][:, p["idx"][b, 65:]] == 1e300) and int(np.sum(p["X"][b][0] == 1e300)) == W.GATHER_K - len(set(used.tolist()))
    op, B, ipar, dpar, arrays = M.unpack_case(p["data"])
    assert ipar == M.unpack_case(c["data"])[2] and np.array_equal(arrays[1][1].reshape(c["X"].shape), p["X"])
    assert [a.size for _, a in arrays] == [a.size for _, a in M.unpack_case(c["data"])[4]]
    pw = W.poisoned(W.build(dict(cs=97, K=W.GATHER_K, ksplit=2, variant="idx_w", m=65)))
    assert np.all(pw["w"][0][pw["idx"][0, 65:]] == 1e300) and np.all(pw["w"][0][pw["idx"][0, :65]] <= 1.0)
