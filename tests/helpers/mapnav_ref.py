"""Vectorised NumPy restatement of the waypoint-and-map env (mpopis_amd/env_examples/mapnav.hip: SS = 4, AS = 2, NP = 10, a data table of
2 P waypoint coordinates followed by a G x G map, row-major) and of simulate_model / rollout_model on it (src/mppi_mpopi_policies.jl:261-278,
src/utils.jl:55-67,129-144): the reference of the tests of envs with a table.  Plain products and sums, no FMA: against the device the
difference is rounding.

The map lookup is discontinuous: a position within rounding of a cell edge may fall into another cell on the device than here.  That is a
condition on the inputs, not a tolerance: every function that visits positions also returns the smallest distance of any position it looked
up to a cell edge that separates two cells (in cell units; inf when there is no such edge, G <= 1), and the tests require it to be >= MARGIN
for the seeds they use."""
import numpy as np

SS, AS, NP = 4, 2, 10
MARGIN = 1e-6
LO = np.array([-3.0, -2.0])
HI = np.array([2.0, 3.0])


def params(P, G, max_steps=200.0):
    """[dt, drag, P, G, origin, cell, w_path, w_map, w_vel, max_steps]: the map covers [-1, 1)^2 whatever G is"""
    return np.array([0.1, 0.2, float(P), float(G), -1.0, 2.0 / max(G, 1), 1.0, 0.5, 0.1, float(max_steps)])


def make_table(P, G, rng, pad=0):
    """P waypoints in [-1, 1]^2, then a G x G map of values in [0, 2); `pad` doubles behind it that no env reads"""
    return np.concatenate([rng.uniform(-1.0, 1.0, 2 * P), rng.uniform(0.0, 2.0, G * G), np.full(pad, 1e300)])


def _cells(x, p):
    """cell index along one axis (floor, clamped to 0..G-1) and the distance to the nearest edge between two cells, in cell units"""
    G = int(p[3])
    f = (x - p[4]) / p[5]
    c = np.floor(f)
    idx = np.where(c >= 0.0, np.minimum(c, G - 1), 0.0).astype(np.int64)
    if G < 2:
        return idx, np.inf
    edge = np.clip(np.rint(f), 1, G - 1)                          # the edges between cells sit at 1 .. G-1; outside them the clamp takes over
    return idx, float(np.min(np.abs(f - edge)))


def map_value(x, y, p, tab):
    """(map(x, y), edge margin) for positions of any shape"""
    P, G = int(p[2]), int(p[3])
    if G < 1:
        return np.zeros(np.shape(x)), np.inf
    ix, mx = _cells(x, p)
    iy, my = _cells(y, p)
    idx = 2 * P + iy * G + ix
    tab = np.asarray(tab, dtype=np.float64)
    ok = idx < tab.size                                           # a table shorter than the parameters promise counts as 0 there
    return np.where(ok, tab[np.where(ok, idx, 0)] if tab.size else 0.0, 0.0), min(mx, my)


def step(s, t, a, p, tab):
    """env(a) for a batch: s (..., 4), a (..., 2), t int -> (s', t', done, edge margin of the lookup)"""
    s = np.array(s, dtype=np.float64, copy=True)
    m, margin = map_value(s[..., 0], s[..., 1], p, tab)
    dt, damp = p[0], p[1] + m
    s[..., 2] = s[..., 2] + dt * (a[..., 0] - damp * s[..., 2])
    s[..., 3] = s[..., 3] + dt * (a[..., 1] - damp * s[..., 3])
    s[..., 0] = s[..., 0] + dt * s[..., 2]
    s[..., 1] = s[..., 1] + dt * s[..., 3]
    t = t + 1
    return s, t, int(t >= int(p[9])), margin


def reward(s, p, tab):
    """(reward(env), edge margin of the lookup)"""
    tab = np.asarray(tab, dtype=np.float64)
    P = min(int(p[2]), tab.size // 2)
    if P > 0:
        w = tab[:2 * P].reshape(P, 2)
        dx, dy = s[..., 0, None] - w[:, 0], s[..., 1, None] - w[:, 1]
        dmin = np.min(dx * dx + dy * dy, axis=-1)
    else:
        dmin = np.zeros(np.shape(s)[:-1])
    m, margin = map_value(s[..., 0], s[..., 1], p, tab)
    return -(p[6] * dmin + p[7] * m + p[8] * (s[..., 2] * s[..., 2] + s[..., 3] * s[..., 3])), margin


def rollout_costs(x0, U, E, p, tab, lo=LO, hi=HI, t0=0):
    """simulate_model for one slot: x0 (4,), U (cs,), E (K, cs) [row k = sample k] ->
    (cost (K,), trajectories (K, T, 4), edge margin over every lookup, number of looked-up positions outside the map)"""
    U, E = np.asarray(U, dtype=np.float64), np.asarray(E, dtype=np.float64)
    K, cs = E.shape
    T = cs // AS
    V = U[None, :] + E
    cost = np.zeros(K)
    s = np.tile(np.asarray(x0, dtype=np.float64), (K, 1))
    traj = np.zeros((K, T, SS))
    t, margin, outside = t0, np.inf, 0
    span = p[4] + p[5] * int(p[3])
    for i in range(T):
        a = np.clip(V[:, AS * i:AS * i + AS], lo, hi)
        outside += int(np.sum((s[:, :2] < p[4]) | (s[:, :2] >= span)))
        s, t, _, m1 = step(s, t, a, p, tab)
        r, m2 = reward(s, p, tab)
        cost = cost - r
        traj[:, i] = s
        margin = min(margin, m1, m2)
    outside += int(np.sum((s[:, :2] < p[4]) | (s[:, :2] >= span)))
    return cost, traj, margin, outside
