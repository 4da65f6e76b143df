"""The rollout kernels' distance to the centre line (ring table with unit tangents, cross product: car_dynamics.h ring_entry_project) at the places
where it can go wrong, against the oracle's literal projection: mpopis_rollout_costs for one car and for three cars on the default track, K = 130
(two full waves and a ragged one at one car), H = 3.  Every trial slot starts its cars where, within the three steps, the rollouts pass from one
nearest track point to the next, pass a track point (the chosen neighbour switches from predecessor to successor), and run along the lane edge
so that the steering noise puts rollouts on both sides of it.  The one-wave and the two-wave kernels must give identical bits."""
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "helpers", "projection_case.py")
K, T = 130, 3


def _start(track, i, along, offset, speed=25.0):
    """a car `along` metres past track point i on the segment to i + 1, `offset` metres to its left, heading along the segment"""
    tx, ty, _ = track
    P = len(tx)
    j = (i + 1) % P
    v = np.array([tx[j] - tx[i], ty[j] - ty[i]])
    t = v / np.hypot(*v)
    n = np.array([-t[1], t[0]])
    p = np.array([tx[i], ty[i]]) + along * t + offset * n
    return np.array([p[0], p[1], np.arctan2(t[1], t[0]), speed, 0.0, 0.0, 0.0, 0.0])


def _case(track, ncars):
    tx, ty, tw = track
    P = len(tx)
    seg = lambda i: float(np.hypot(tx[(i + 1) % P] - tx[i], ty[(i + 1) % P] - ty[i]))
    # per slot, what car 0 does in its 7.5 m: cross the midpoint of a segment (nearest point i -> i + 1), pass a track point (predecessor -> successor),
    # the wrap-around P-1 -> 0, and run 5 cm inside / outside the lane edge; the other cars take the same list from another track point
    slots = [lambda i: _start(track, i, 0.5 * seg(i) - 3.0, 2.0), lambda i: _start(track, i, -3.0, -4.0), lambda i: _start(track, P - 1, 0.5 * seg(P - 1) - 4.0, 0.0),
             lambda i: _start(track, i, 6.0, tw[i] - 0.05), lambda i: _start(track, i, 9.0, -(tw[i] + 0.05))]
    B = len(slots)
    x0 = np.stack([np.concatenate([slots[(b + c) % B](3 + 11 * c + 2 * b) for c in range(ncars)]) for b in range(B)])
    rng = np.random.default_rng(130 + ncars)
    cs = 2 * ncars * T
    U = np.zeros((B, cs)); U[:, 1::2] = 0.3
    E = rng.standard_normal((B, K, cs)) * np.tile([0.6, 0.3], ncars * T)          # steering noise up to the stops: +-0.2 m sideways within the horizon
    return x0, U, E


def _run(tmp, inp, env_extra):
    out = os.path.join(tmp, "out.npz")
    r = subprocess.run([sys.executable, CASE, inp, out], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env_extra), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return np.load(out)["cost"]


@pytest.mark.parametrize("ncars", [1, 3])
def test_rollout_costs_across_point_segment_and_lane_edge_switches(oracle, tmp_path, ncars):
    from mpopis_amd.engine import default_track
    track = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in default_track())
    x0, U, E = _case(track, ncars)
    B = len(x0)
    inp = os.path.join(str(tmp_path), "in.npz")
    np.savez(inp, tx=track[0], ty=track[1], tw=track[2], ncars=ncars, x0=x0, U=U, E=E)
    one = _run(str(tmp_path), inp, {"MPOPIS_ROLLOUT_DUO": "0"})
    duo = _run(str(tmp_path), inp, {"MPOPIS_ROLLOUT_DUO": "1000000"})
    assert one.tobytes() == duo.tobytes()                        # one-wave and two-wave kernels: identical bits
    env = oracle.OracleEnv("car", ncars, track=track)
    pol = oracle.OraclePolicy("gmppi", env, K, T, lam=10.0, U0=np.zeros(2 * ncars), cov=np.tile([0.0625, 0.1], ncars), nthreads=8)
    off = 0
    for b in range(B):
        env.state = x0[b]
        ref = pol.simulate_model(U[b], E[b].T)
        rel = np.max(np.abs(one[b] - ref) / (np.abs(ref) + 1e-9))
        print("\n[rollout projection] %d car(s), slot %d: max relative cost deviation %.2e, %d of %d rollouts leave the lane" % (ncars, b, rel, int(np.sum(ref > 9e5)), K))
        assert rel < 1e-8, (ncars, b, rel)                       # the project's per-rollout tolerance (tests/test_gpu_fullsize.py)
        nout = np.round(ref / 1e6)                               # reward evaluations off the road (-1e6 each) of every rollout
        off += int(nout.min() != nout.max())
    assert off >= 2                                              # in the lane-edge slots the rollouts differ in how often they are off the road: both sides occur
