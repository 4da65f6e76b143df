"""Inputs of tests/test_gpu_slot_env.py: small tracks, car parameter vectors and start states for handles whose trial slots differ in their
track and env parameters (mpopis_set_tracks / mpopis_set_env_params_slots).

Every start state has Vx >= 15 m/s, every horizon is at most 9 model steps of 0.1 s and every parameter vector keeps |Fx_min| / m <= 12 m/s^2:
at most ~11 m/s can be braked away in a rollout, so none reaches the standstill chatter regime that the waivers of tests/helpers/rollout_cases.py
exist for (the tests check the oracle's logged Vx all the same)."""
import numpy as np

COV = (0.0625, 0.1)
TRACK_OF_SLOT = [2, 0, 2, 1]          # non-monotonic and repeated: an index taken by slot where it should be taken by track fails


def ring(n, a, b=None, width=15.0):
    """n points on an ellipse with half-axes a, b (closed ring; n = 2: two points)"""
    th = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    b = a if b is None else b
    f = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    return f(a * np.cos(th)), f(b * np.sin(th)), f(np.full(n, width))


def tracks3(curve):
    """P = 48 (the bundled curve), 5 (a closed polygon) and 12 (an ellipse): every table in LDS"""
    return [tuple(np.ascontiguousarray(v, dtype=np.float64) for v in curve), ring(5, 45.0), ring(12, 80.0, 50.0)]


def car_params4(oracle):
    """Four parameter vectors (include/mpopis.h: m Izz h lf lr CD0 CD1 Caf Car muf mur dmax ddotmax Fxmax Fxmin lbrake ldrive blim dt ddt):
    dt/δt = 10 in slots 0, 1 and 5 in slots 2, 3; β_limit > π/2 in slot 1; λ_drive != 0 in slot 2; other m, C_αf, μ in slot 3."""
    p = np.stack([oracle.car_default_params() for _ in range(4)])
    p[0, 18], p[0, 19] = 0.1, 0.01
    p[1, 18], p[1, 19] = 0.1, 0.01
    p[1, 17] = 1.7
    p[2, 18], p[2, 19] = 0.1, 0.02
    p[2, 16] = 0.2 if p[2, 16] == 0.0 else 0.5 * p[2, 16]
    p[3, 18], p[3, 19] = 0.1, 0.02
    p[3, 0] *= 1.25; p[3, 7] *= 1.2; p[3, 9] = 0.8; p[3, 10] = 0.85
    assert np.all(np.abs(p[:, 14]) / p[:, 0] <= 12.0) and np.all(p[:, 18] <= 0.1 + 1e-12)
    return p


def start_state(trk, ncars, b, lateral=2.0):
    """cars of slot b on their own track: at point j heading for point j + 1, 7 m apart along the heading, Vx = 16 + b + c / 2"""
    tx, ty, tw = trk
    P = len(tx)
    j = (3 * b + 1) % P
    jn = (j + 1) % P
    head = np.arctan2(ty[jn] - ty[j], tx[jn] - tx[j])
    x = np.zeros(8 * ncars)
    for c in range(ncars):
        off = lateral * (1 if (b + c) % 2 else -1)
        pos = np.array([tx[j], ty[j]]) + off * np.array([-np.sin(head), np.cos(head)]) + 7.0 * c * np.array([np.cos(head), np.sin(head)])
        x[8 * c:8 * c + 8] = [pos[0], pos[1], head + 0.03 * (c - 1), 16.0 + b + 0.5 * c, 0.4 - 0.1 * c, 0.05, 0.02, 0.0]
    return x


def level1_inputs(rng, B, ncars, K, T):
    cs = 2 * ncars * T
    U = rng.uniform(-0.3, 0.3, (B, cs))
    U[:, 1::2] += 0.3
    E = rng.standard_normal((B, K, cs)) * np.tile([0.25, 0.32], ncars * T)
    E[:, :2] *= 6.0                                        # some samples far out: clamps, off the track, β penalties
    return U, E


def min_logged_vx(traj, ncars):
    """smallest Vx over an oracle trajectory log (K, T, 8 ncars)"""
    return float(min(traj[:, :, 8 * c + 3].min() for c in range(ncars)))


RTOL = 1e-8          # tests/test_gpu_parity.py: Level-1 costs and logged trajectories against the oracle


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-9)))


def mixed_tracks(sizes):
    return [ring(P, max(30.0, 6.0 * P / (2 * np.pi))) for P in sizes]


def level1_check(Engine, oracle, tracks, tos, params, nc, K, T, seed, log_slot=None):
    """rollout_costs of a per-slot handle against simulate_model of each slot's own oracle env; returns the worst relative deviation"""
    B = len(tos)
    rng = np.random.default_rng(seed)
    eng = Engine("car", nc, "gmppi", K, T, batch=B, lam=10.0, cov=np.tile(COV, nc), track=None, log_trajectories=log_slot is not None)
    eng.set_tracks(tracks, tos)
    eng.set_env_params_slots(params)
    U, E = level1_inputs(rng, B, nc, K, T)
    x0 = np.stack([start_state(tracks[tos[b]], nc, b) for b in range(B)])
    got = eng.rollout_costs(U, E, x0=x0)
    worst = 0.0
    for b in range(B):
        env = oracle.OracleEnv("car", nc, params=params[b], track=tracks[tos[b]])
        env.state = x0[b]
        pol = oracle.OraclePolicy("gmppi", env, K, T, lam=10.0, U0=np.zeros(2 * nc), cov=np.tile(COV, nc))
        ref, traj = pol.simulate_model(U[b], E[b].T, log=True)
        assert min_logged_vx(traj, nc) > 2.0                 # no rollout near the standstill regime (tests/helpers/slot_env_cases.py)
        err = rel_err(got[b], ref)
        print("[slot env level 1] cars %d K %d T %d slot %d (track %d, P %d): %.2e" % (nc, K, T, b, tos[b], len(tracks[tos[b]][0]), err))
        assert err < RTOL, (nc, K, T, b, err)
        worst = max(worst, err)
        if log_slot == b:
            tr = eng.get_trajectories()[b]
            assert rel_err(tr, traj) < RTOL
            if nc == 1:                                         # step by step: oracle.car_step under THIS slot's parameters from the logged state
                for k in range(min(K, 6)):
                    s = x0[b].copy()
                    for t in range(T):
                        s = oracle.car_step(params[b], s, np.clip(U[b, 2 * t:2 * t + 2] + E[b, k, 2 * t:2 * t + 2], -1.0, 1.0))
                        assert rel_err(tr[k, t], s) < RTOL, (k, t)
                        s = tr[k, t].copy()
    eng.close()
    return worst
