"""CPU-side checks of the per-slot hyper-parameter seam (mpopis_set_slot_hyper, mpopis_get_slot_hyper, mpopis_set_Sigma_slots): the three
entry points are declared and exported, refuse a NULL handle, and the harnesses' per-trial split hands every rank the entries of its own
trials.  No compute."""
import os
import re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpopis_set_slot_hyper", "mpopis_get_slot_hyper", "mpopis_set_Sigma_slots")


@pytest.fixture(scope="module")
def L():
    from mpopis_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_declared_and_exported(L):
    from mpopis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mpopis.h")).read()
    declared = set(re.findall(r"\b(mpopis_[A-Za-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert L.mpopis_abi_version() == 5                      # support is detected by the symbol, not by the version


def test_null_handle_is_an_argument_error(L):
    assert L.mpopis_set_slot_hyper(None, None, None, None, None) == -1
    assert L.mpopis_get_slot_hyper(None, None, None, None, None) == -1
    assert L.mpopis_set_Sigma_slots(None, None, 2) == -1


def test_split_per_trial_one_rank():
    from mpopis_amd.examples import split_per_trial
    lam = [10.0, 2.5, 40.0, 7.0, 1.0]
    shared, slots = split_per_trial(lam, 5)
    assert shared is None and np.array_equal(slots, lam)    # trial k (1-based) gets entry k - 1
    shared, slots = split_per_trial(10.0, 5)
    assert shared == 10.0 and slots is None                 # a scalar keeps today's meaning


def test_split_per_trial_three_ranks():
    from mpopis_amd.examples import split_per_trial, shard_trials
    n = 7                                                   # not a multiple of 3: ranks hold 3, 2, 2 trials
    lam = np.arange(1.0, n + 1.0) * 1.5
    seen = []
    for rank in range(3):
        shared, slots = split_per_trial(lam, n, rank, 3)
        mine = shard_trials(n, rank, 3)
        assert shared is None and len(slots) == len(mine)
        assert np.array_equal(slots, [lam[k - 1] for k in mine])
        seen += mine
        assert split_per_trial(0.8, n, rank, 3) == (0.8, None)
    assert sorted(seen) == list(range(1, n + 1))
    assert [len(shard_trials(n, r, 3)) for r in range(3)] == [3, 2, 2]


def test_split_per_trial_covariances():
    from mpopis_amd.examples import split_per_trial
    n = 4
    vec = [0.0625, 0.1]
    assert split_per_trial(vec, n, cov=True) == (vec, None)                 # one diagonal, as today
    mat = np.array([[0.0625, 0.02], [0.02, 0.1]])
    shared, slots = split_per_trial(mat, n, cov=True)
    assert shared is mat and slots is None                                  # one matrix, as today
    vecs = np.array([[0.0625 * (1 + b), 0.1 / (1 + b)] for b in range(n)])
    shared, slots = split_per_trial(vecs, n, 1, 3, cov=True)                # rank 1 of 3 holds trials 2 (and 5, 8, ...)
    assert shared is None and np.array_equal(slots, vecs[[1]])
    mats = np.stack([np.diag(v) for v in vecs])
    shared, slots = split_per_trial(mats, n, 0, 3, cov=True)                # rank 0 holds trials 1 and 4
    assert shared is None and np.array_equal(slots, mats[[0, 3]])


def test_split_per_trial_wrong_length_raises():
    from mpopis_amd.examples import split_per_trial
    with pytest.raises(ValueError):
        split_per_trial([1.0, 2.0], 3)
    with pytest.raises(ValueError):
        split_per_trial([1.0, 2.0, 3.0, 4.0], 3, 0, 3)
    with pytest.raises(ValueError):
        split_per_trial(np.zeros((2, 3)), 4, cov=True)
    with pytest.raises(ValueError):
        split_per_trial(np.zeros((5, 2, 2)), 4, cov=True)


def test_split_per_trial_scalar_keyword_is_at_most_one_dimensional():
    from mpopis_amd.examples import split_per_trial
    with pytest.raises(ValueError):
        split_per_trial(np.ones((3, 2)), 3)                                 # num_trials rows, but a scalar keyword has one value per trial
    with pytest.raises(ValueError):
        split_per_trial(np.ones((3, 1)), 3)
    with pytest.raises(ValueError):
        split_per_trial([[10.0]], 1)


def test_split_per_trial_square_covariance_with_num_trials_rows(recwarn):
    from mpopis_amd.examples import split_per_trial
    sym = np.array([[0.0625, 0.02], [0.02, 0.1]])
    assert split_per_trial(sym, 2, cov=True)[0] is sym                      # one matrix, as before, and nothing to say about it
    assert split_per_trial(np.array([[0.0625, 0.0], [0.3, 0.1]]), 3, cov=True)[1] is None
    assert len(recwarn) == 0
    diags = np.array([[0.0625, 0.1], [0.125, 0.05]])                        # two trials of a one-car env: meant as per-trial diagonals
    with pytest.warns(UserWarning, match=r"\(2, 2, 2\)"):
        shared, slots = split_per_trial(diags, 2, cov=True)
    assert shared is diags and slots is None                                # still read as ONE matrix
    shared, slots = split_per_trial(np.stack([np.diag(v) for v in diags]), 2, cov=True)
    assert shared is None and slots.shape == (2, 2, 2)                      # the unambiguous spelling
