"""The expectation for a FLEET -- a MultiCarRacingEnv whose cars carry their own parameter vectors (multi-car_racing.jl:23-45) -- composed from
the per-car pieces the CPU oracle exports: oracle.car_step(params_c, s_c, a_c) for env.envs[c](a_c) (:200-207), orc_car_reward(params_c, ...)
for reward(env.envs[c]), and the pair terms of reward(env) (:145-158) restated here in the reference's order.  The oracle's own multi-car env
holds ONE vector; with equal vectors this composition reproduces its simulate_model (tests/test_car_fleet_cpu.py)."""
import ctypes as C
import math

import numpy as np

NPAR = 20


def graded_fleet(num_cars, base):
    """The fleet the tests drive: car c = the default vector with, at f = c / (num_cars - 1), m and Izz x (1 + 0.5 f), μf and μr x (1 - 0.4 f),
    Fxmax x (1 - 0.5 f), δmax x (1 - 0.3 f), β_limit x (1 - 0.5 f).  Car 0 keeps the defaults."""
    fl = np.tile(np.asarray(base, dtype=np.float64), (num_cars, 1))
    for c in range(num_cars):
        f = c / (num_cars - 1)
        fl[c, [0, 1]] *= 1 + 0.5 * f
        fl[c, [9, 10]] *= 1 - 0.4 * f
        fl[c, 13] *= 1 - 0.5 * f
        fl[c, 11] *= 1 - 0.3 * f
        fl[c, 17] *= 1 - 0.5 * f
    return fl


def car_reward(oracle, params, track, s):
    tx, ty, tw = track
    d = oracle._d
    return oracle.lib().orc_car_reward(d(oracle.f64(params)), C.c_int(len(tx)), d(tx), d(ty), d(tw), d(oracle.f64(s)))


def fleet_reward(oracle, fleet, track, s):
    """reward(env::MultiCarRacingEnv) with every car's own reward(en): s is (num_cars, 8)"""
    nc = len(fleet)
    rew = 0.0
    for i in range(nc):
        rew += car_reward(oracle, fleet[i], track, s[i])
        for j in range(i + 1, nc):
            dx, dy = s[j, 0] - s[i, 0], s[j, 1] - s[i, 1]
            dd = math.sqrt(dx * dx + dy * dy)
            rew += -dd
            if dd <= 4.0:
                rew += -11000.0
    return rew


def fleet_step(oracle, fleet, s, a):
    """env(a): car c steps with its own parameters and actions a[2c : 2c + 2]; returns the new (num_cars, 8) state"""
    return np.stack([oracle.car_step(fleet[c], s[c], a[2 * c:2 * c + 2]) for c in range(len(fleet))])


def fleet_rollout(oracle, fleet, track, x0, U, E, lo=None, hi=None, gamma=0.0, Sigma_inv=None, U_orig=None, log=False):
    """simulate_model (src/mppi_mpopi_policies.jl:261-278) + rollout_model (src/utils.jl:129-144) of one slot.  fleet (num_cars, 20), x0
    (8 num_cars,), U (cs,), E (K, cs) with row k = sample k, lo / hi (2 num_cars,) action bounds (default -1 / 1), gamma = λ (1 - α) with
    Sigma_inv (cs, cs) and U_orig (cs,) for the control cost.  Returns cost (K,), and with log also the states (K, T, 8 num_cars) after every step."""
    fleet = np.asarray(fleet, dtype=np.float64)
    nc = len(fleet)
    as_ = 2 * nc
    U, E = np.asarray(U, dtype=np.float64), np.asarray(E, dtype=np.float64)
    K, cs = E.shape
    T = cs // as_
    lo = -np.ones(as_) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.ones(as_) if hi is None else np.asarray(hi, dtype=np.float64)
    U_orig = U if U_orig is None else np.asarray(U_orig, dtype=np.float64)
    row = None
    if gamma != 0.0 and Sigma_inv is not None:
        row = (gamma * U_orig) @ np.asarray(Sigma_inv, dtype=np.float64)
    cost = np.zeros(K)
    traj = np.zeros((K, T, 8 * nc)) if log else None
    for k in range(K):
        V = U + E[k]
        cc = float(row @ (V - U_orig)) if row is not None else 0.0            # :272, the unclamped V
        A = np.clip(V.reshape(T, as_), lo, hi)                                  # get_model_controls (NaN passes)
        s = np.asarray(x0, dtype=np.float64).reshape(nc, 8).copy()
        c = 0.0
        for t in range(T):
            s = fleet_step(oracle, fleet, s, A[t])
            c -= fleet_reward(oracle, fleet, track, s)
            if log:
                traj[k, t] = s.reshape(-1)
        cost[k] = c + cc
    return (cost, traj) if log else cost
