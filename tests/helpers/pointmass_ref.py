"""Vectorised NumPy restatement of the planar point mass (mpopis_amd/env_examples/pointmass.hip: SS = 5, AS = 3, NP = 9) and of
simulate_model / rollout_model on it (src/mppi_mpopi_policies.jl:261-278, src/utils.jl:55-67,129-144): the reference of the custom-env tests
whose sizes match no built-in env.  Plain products and sums, no FMA: against the device the difference is rounding (the step is a contraction
and the state O(1), so ~1e-14 over ten steps)."""
import numpy as np

SS, AS, NP = 5, 3, 9
#                  dt   drag  brake_gain goal_x goal_y w_pos w_vel w_effort max_steps
PARAMS = np.array([0.1, 0.2, 1.5, 1.0, -0.5, 1.0, 0.1, 0.05, 200.0])
LO = np.array([-1.0, -0.5, 0.0])
HI = np.array([0.7, 1.0, 1.0])


def step(s, t, a, p=PARAMS):
    """env(a) for a batch: s (..., 5), a (..., 3), t int -> (s', t', done)."""
    s = np.array(s, dtype=np.float64, copy=True)
    dt, damp = p[0], p[1] + p[2] * a[..., 2]
    s[..., 2] = s[..., 2] + dt * (a[..., 0] - damp * s[..., 2])
    s[..., 3] = s[..., 3] + dt * (a[..., 1] - damp * s[..., 3])
    s[..., 0] = s[..., 0] + dt * s[..., 2]
    s[..., 1] = s[..., 1] + dt * s[..., 3]
    s[..., 4] = 0.9 * s[..., 4] + dt * (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1])
    t = t + 1
    return s, t, int(t >= int(p[8]))


def reward(s, p=PARAMS):
    dx, dy = s[..., 0] - p[3], s[..., 1] - p[4]
    return -(p[5] * (dx * dx + dy * dy) + p[6] * (s[..., 2] * s[..., 2] + s[..., 3] * s[..., 3]) + p[7] * s[..., 4])


def rollout_costs(x0, U, E, p=PARAMS, lo=LO, hi=HI, U_orig=None, gamma=0.0, Sigma_inv=None, t0=0):
    """simulate_model for one slot: x0 (5,), U (cs,), E (K, cs) [row k = sample k] -> (cost (K,), trajectories (K, T, 5)).
    Control cost: gamma U_orig' Sigma_inv (V - U_orig) with the unclamped V (:272)."""
    U, E = np.asarray(U, dtype=np.float64), np.asarray(E, dtype=np.float64)
    K, cs = E.shape
    T = cs // AS
    Uo = U if U_orig is None else np.asarray(U_orig, dtype=np.float64)
    V = U[None, :] + E                                          # (K, cs)
    cost = np.zeros(K)
    if gamma != 0.0:
        g = gamma * (Uo @ np.asarray(Sigma_inv, dtype=np.float64))
        cost = cost + (V - Uo[None, :]) @ g
    s = np.tile(np.asarray(x0, dtype=np.float64), (K, 1))
    traj = np.zeros((K, T, SS))
    t = t0
    for i in range(T):
        a = np.clip(V[:, AS * i:AS * i + AS], lo, hi)
        s, t, _ = step(s, t, a, p)
        cost = cost - reward(s, p)
        traj[:, i] = s
    return cost, traj
