"""Per-slot tracks and env parameters, the parts that need no device: how simulate_car_racing / simulate_mountaincar / simulate_cartpole split
their `track`, `car_params` and `env_params` keywords over trials and ranks (mpopis_amd.examples.split_tracks_per_trial,
split_env_params_per_trial), and the two entry points' answer to a NULL handle (as tests/test_abi.py does for the older ones)."""
import numpy as np
import pytest


def _triple(n, r=50.0, w=15.0):
    a = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    return r * np.cos(a), r * np.sin(a), np.full(n, w)


def test_track_shared_versus_per_trial():
    from mpopis_amd.examples import split_tracks_per_trial
    t5 = _triple(5)
    assert split_tracks_per_trial("curve", 3) == ("curve", None)
    shared, per = split_tracks_per_trial(t5, 3)
    assert shared is t5 and per is None
    # three 1-D arrays of one length are ONE triple even when num_trials == 3; three names or three triples are one entry per trial
    shared, per = split_tracks_per_trial(_triple(3), 3)
    assert shared is not None and per is None
    shared, per = split_tracks_per_trial(["curve", "cubic", "curve1"], 3)
    assert shared is None and per == (["curve", "cubic", "curve1"], [0, 1, 2])
    shared, per = split_tracks_per_trial([_triple(5), _triple(6), _triple(7)], 3)
    assert shared is None and per[1] == [0, 1, 2] and [len(t[0]) for t in per[0]] == [5, 6, 7]
    # lists instead of arrays, and a mixed sequence
    shared, per = split_tracks_per_trial([[list(v) for v in _triple(4)], "cubic"], 2)
    assert shared is None and per[1] == [0, 1] and per[0][1] == "cubic"


def test_track_deduplication():
    from mpopis_amd.examples import split_tracks_per_trial
    _, (tracks, tos) = split_tracks_per_trial(["curve", "cubic", "curve", "cubic", "curve"], 5)
    assert tracks == ["curve", "cubic"] and tos == [0, 1, 0, 1, 0]
    a, b = _triple(5), _triple(5, r=51.0)
    a_again = tuple(np.array(v) for v in a)                    # equal numbers in other arrays: the same track
    _, (tracks, tos) = split_tracks_per_trial([b, a, a_again, b], 4)
    assert len(tracks) == 2 and tos == [0, 1, 1, 0] and tracks[0] is b and tracks[1] is a


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharding_five_trials(world):
    from mpopis_amd.examples import split_tracks_per_trial, split_env_params_per_trial, shard_trials
    names = ["curve", "cubic", "curve", "cubic1", "cubic"]
    params = np.arange(5 * 20, dtype=np.float64).reshape(5, 20)
    seen = []
    for rank in range(world):
        mine = shard_trials(5, rank, world)
        _, (tracks, tos) = split_tracks_per_trial(names, 5, rank, world)
        assert [tracks[i] for i in tos] == [names[k - 1] for k in mine]          # trial k gets entry k - 1
        assert len(set(tracks)) == len(tracks) and set(tracks) == {names[k - 1] for k in mine}
        shared, rows = split_env_params_per_trial(params, 20, 5, rank, world)
        assert shared is None and np.array_equal(rows, params[[k - 1 for k in mine]])
        seen += mine
    assert sorted(seen) == [1, 2, 3, 4, 5]


def test_env_params_shared_versus_per_trial():
    from mpopis_amd.examples import split_env_params_per_trial
    assert split_env_params_per_trial(None, 20, 3) == (None, None)
    shared, rows = split_env_params_per_trial(np.arange(20.0), 20, 3)
    assert rows is None and np.array_equal(shared, np.arange(20.0))
    shared, rows = split_env_params_per_trial(np.ones((3, 8)), 8, 3)
    assert shared is None and rows.shape == (3, 8)
    shared, rows = split_env_params_per_trial(np.ones((1, 11)), 11, 1)            # one trial, given as a row: still per trial
    assert shared is None and rows.shape == (1, 11)


def test_wrong_shapes_raise():
    from mpopis_amd.examples import split_tracks_per_trial, split_env_params_per_trial
    for bad in (np.ones(19), np.ones((3, 19)), np.ones((2, 20)), np.ones((3, 20, 1)), 1.0):
        with pytest.raises(ValueError):
            split_env_params_per_trial(bad, 20, 3)
    x, y, w = _triple(5)
    for bad in (["curve", "cubic"], (x, y), (x, y, w[:4]), [(x, y, w), (x, y)], 7, [(x[:1], y[:1], w[:1])] * 3, (x.reshape(5, 1), y, w)):
        with pytest.raises(ValueError):
            split_tracks_per_trial(bad, 3)


def test_simulate_keywords_are_checked_before_any_device_work():
    """a wrong shape raises in the splitting function, i.e. before the Engine is created (no device here)"""
    from mpopis_amd import simulate_car_racing, simulate_mountaincar, simulate_cartpole
    with pytest.raises(ValueError):
        simulate_car_racing(num_trials=3, track=["curve", "cubic"], seed=1, quiet=True)
    with pytest.raises(ValueError):
        simulate_car_racing(num_trials=3, car_params=np.ones((3, 19)), seed=1, quiet=True)
    with pytest.raises(ValueError):
        simulate_mountaincar(num_trials=2, env_params=np.ones((2, 11)), seed=1, quiet=True)
    with pytest.raises(ValueError):
        simulate_cartpole(num_trials=2, env_params=np.ones((3, 11)), seed=1, quiet=True)


def test_null_handle_is_an_argument_error():
    from mpopis_amd import build, _lib
    build.build()
    L = _lib.lib()
    assert L.mpopis_set_env_params_slots(None, None, 20) == _lib.ERR_ARG
    assert L.mpopis_set_tracks(None, 1, None, None, None, None, None) == _lib.ERR_ARG
