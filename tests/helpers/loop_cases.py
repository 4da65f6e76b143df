"""Cases, references and checks of the launch-level tests of the closed loop's other half -- k_env_step / k_env_query (kernels_reweight.hip),
k_harness_init / k_harness_update (kernels_harness.hip), k_trace_* (kernels_trace.hip), k_plan_* (kernels_plan.hip) -- as tools/kbench_loop.hip runs
them (file format: the comment at the top of that file).  tests/test_loop_cases_cpu.py proves the references, the cases and the checkers on the
CPU; tests/test_gpu_loop_harness.py runs the cases on the device.

References: bookkeeping_ref is a plain restatement of src/examples/car_example.jl:199-302 (and the simple envs' loops) in Python, written from
the Julia source; the env step and query are the oracle's (OracleEnv.step / reward, car_step, within_track, atan2); the plan order is
mpopis_amd.engine.plan_order; the state noise is oracle.philox_normals on the stream (step, 0x40000000) with the rotation in np.longdouble.

Bounds of the accumulated statistics (u = 2^-53; derived here, measured in the tests).  One step's term of vmean is (sum_c v_c) / NC with
v = sqrt(Vx^2 + Vy^2): two products and a sum (or one product and an fma, if the compiler fuses) put <= 2u on the radicand, the square root
halves that and adds its own u: <= 2u on v.  NC - 1 additions and one division: <= (NC + 2) u on the term.  The term of bmean starts from
|atan2(Vy, Vx)|, which OCML grants 2 ulp <= 4u: <= (NC + 4) u on the term.  n sequential additions of non-negative terms add <= (n - 1) u of the
sum.  So |sum_dev - sum_exact| <= gamma(NC + 2 + n - 1) sum_exact for vmean, gamma(NC + 4 + n - 1) sum_exact for bmean, gamma(k) = k u / (1 - k u)
(stat_bound).  vmax / bmax are one v / one |atan2|: 2u v <= 2 ulp and 2 ulp.  The noise: a device normal is within RNG_TOL = 1e-13 of the libm
normal (tests/helpers/sample_cases.py), so a position x + sigma z carries sigma RNG_TOL + its rounding; the noise cases keep sigma RNG_TOL below half
an ulp of the coordinate, which leaves <= 2 ulp.  The rotated velocity c Vx + s Vy: c and s are OCML's cos / sin (2 ulp <= 4u each) of an
angle that is off by d = sigma_psi RNG_TOL + u |dpsi|, then two products and a sum: <= (|Vx| + |Vy|) (d + 4u + 2u) (rot_bound)."""
import os, struct
import numpy as np
from mpopis_amd.engine import plan_order
from tests.helpers import harness_io as IO
from tests.helpers.harness_io import DT, GUARD, LD, U, bits, is_poison, poisoned, ulp_of, ulp_err      # (re-exported: the tests read them under this module's name)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MAGIC_IN, MAGIC_OUT = b"LOPCASE1", b"LOPRES01"
OP_STEP, OP_LOOP, OP_PLAN, OP_REORDER = 0, 1, 2, 3
ENV_MC, ENV_CAR, ENV_CP = 0, 1, 2
KIND_NAME = {ENV_MC: "mountaincar", ENV_CAR: "car", ENV_CP: "cartpole"}
ERR_NOT_PD, ERR_ACTION, ERR_HIP, ERR_NUMERIC = -2, -3, -4, -5
RNG_TOL = 1e-13                                                              # tests/helpers/sample_cases.py: device normal against the libm normal
ATAN2_ULP = 2                                                                # OCML's documented bound for the FP64 atan2
NOISE_STREAM = 0x40000000                                                    # k_harness_update: philox_normal_pair(seed, step, 0x40000000, 0 / 1)
(H_REW, H_CNT, H_LAP, H_PREV_Y, H_TRK, H_BETA, H_CRASH, H_VMEAN, H_VMAX, H_BMEAN, H_BMAX, H_LAP0, H_LAP1, H_LAP2, H_LAP3, H_ROLL) = range(16)
H_N = 16
EXACT_FIELDS = (H_REW, H_CNT, H_LAP, H_PREV_Y, H_TRK, H_BETA, H_CRASH, H_LAP0, H_LAP1, H_LAP2, H_LAP3, H_ROLL)
STEP_OUT = (("x", 0), ("t", 1), ("done", 1), ("reward", 0), ("status", 1), ("qreward", 0), ("within", 1), ("dist", 0), ("beta", 0))
LOOP_OUT = (("hs_log", 0), ("alive_log", 1), ("x_log", 0), ("reward_log", 0), ("q_within", 1), ("q_dist", 0), ("q_beta", 0), ("hs", 0), ("alive", 1), ("x", 0),
            ("actlog", 0), ("status", 1), ("t", 1), ("states", 0), ("rewards", 0), ("iters", 1), ("tr_within", 1), ("tr_dist", 0), ("tr_beta", 0))
PLAN_OUT = (("idx", 1), ("wsel", 0), ("controls", 0), ("Eplan", 0))
TR_STATES, TR_REWARDS, TR_ITERS, TR_WITHIN, TR_DIST, TR_BETA = 1, 2, 4, 8, 16, 32


def gamma(k):
    return k * U / (1.0 - k * U)


def stat_bound(field, ncars, n, total):
    """bound of |accumulated vmean / bmean - exact| after n steps (the module docstring derives it); total = the exact sum"""
    return gamma((ncars + (2 if field == H_VMEAN else 2 * ATAN2_ULP)) + max(n - 1, 0)) * abs(float(total))


def rot_bound(vx, vy, spsi, dpsi):
    return (abs(vx) + abs(vy)) * (spsi * RNG_TOL + U * abs(dpsi) + 6 * U)


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


# ================================================================ the harness's files =========================================================
def out_names(L):
    if L["op"] == OP_STEP:
        return STEP_OUT
    if L["op"] == OP_LOOP:
        return LOOP_OUT
    if L["op"] == OP_PLAN:
        return PLAN_OUT
    return (("out", 1 if L["elem"] == 4 else 0),)


def state_size(env):
    if env.get("ss"):
        return env["ss"]
    return 8 * env["ncars"] if env["kind"] == ENV_CAR else (4 if env["kind"] == ENV_CP else 2)


def action_size(env):
    return 2 * env["ncars"] if env["kind"] == ENV_CAR else 1


def _env_arrays(env, B):
    tr = env["track"] if env["track"] is not None else (None, None, None)
    sp, st = env.get("slot_params"), env.get("slot_tracks")
    if st is not None:
        assert len(st) == B
        sP = np.array([len(t[0]) for t in st], dtype=np.int32)
        sxyw = np.concatenate([np.concatenate([t[0], t[1], t[2]]) for t in st])
    else:
        sP = sxyw = None
    if sp is not None:
        assert np.shape(sp) == (B, 20)
    return [(0, env["params"]), (0, tr[0]), (0, tr[1]), (0, tr[2]), (0, env["lo"]), (0, env["hi"]), (0, sp), (1, sP), (0, sxyw)]


def _fields(L):
    B = L["B"]
    if L["op"] == OP_STEP:
        env = L["env"]
        ip = [env["kind"], env["ncars"], 0 if env["track"] is None else len(env["track"][0])] + [int(L["want"][n]) for n in ("reward", "within", "dist", "beta", "qreward")] + [int(L["skip_step"])]
        return ip, [], _env_arrays(env, B) + [(0, L["x"]), (1, L["t"]), (1, L["done"]), (0, L["action"]), (1, L["status"]), (1, L["alive"])]
    if L["op"] == OP_LOOP:
        env = L["env"]
        ip = [env["kind"], env["ncars"], 0 if env["track"] is None else len(env["track"][0]), L["nS"], L["num_steps"], L["laps"], L["K"], int(L["noise"] is not None),
              int(L["env_step"]), int(L["actlog"]), L["mask"], int(L["query"]), int(env.get("ss") or 0)]
        nz = L["noise"] if L["noise"] is not None else (0.0, 0.0, 0.0)
        return ip, list(nz), _env_arrays(env, B) + [(0, L["x0"]), (0, L["xs"]), (0, L["reward"]), (1, L["iters"]), (1, L["done_env"]), (0, L["control"]), (2, L["seeds"]), (1, L["alive0"])]
    if L["op"] == OP_PLAN:
        return [L["K"], L["top"], L["cs"]], [], [(0, L["w"]), (0, L["E"]), (0, L["Ucur"]), (0, L["Uin"]), (0, L["wn"]), (1, L["active"])]
    return [L["J"], L["per"], L["elem"]], [], [(1 if L["elem"] == 4 else 0, L["in"])]


def pack(launches):
    records = []
    for L in launches:
        ip, dp, arrays = _fields(L)
        records.append(IO.pack_launch(L["op"], L["B"], ip, dp, arrays))
    return IO.pack_launches(MAGIC_IN, records)


def pack_result(launches, results, guard_hit=None):
    """what the harness writes, from host-built results (name -> array or None): the CPU round trip.  guard_hit = (launch, name, index): one guard entry overwritten"""
    out = [MAGIC_OUT, struct.pack("<2q", GUARD, len(launches))]
    for li, (L, R) in enumerate(zip(launches, results)):
        names = out_names(L)
        out.append(struct.pack("<2q", L["op"], len(names)))
        for n, t in names:
            if R.get(n) is None:
                out.append(IO.pack_array(t, None))
                continue
            g = poisoned((GUARD,), t)
            if guard_hit and guard_hit[:2] == (li, n):
                g[guard_hit[2]] = 0
            a = np.ascontiguousarray(R[n], dtype=DT[t]).reshape(-1)
            out.append(IO.pack_array(t, np.concatenate([a, g])))
    return b"".join(out)


def unpack_result(buf, launches):
    """-> one dict per launch: every output by name, flat (None: no such buffer); asserts the header and that every guard entry is still poison"""
    assert buf[:8] == MAGIC_OUT, buf[:8]
    guard, n = struct.unpack_from("<2q", buf, 8)
    assert (guard, n) == (GUARD, len(launches)), (guard, n, len(launches))
    off, res = 24, []
    for L in launches:
        rh = struct.unpack_from("<2q", buf, off)
        off += 16
        names = out_names(L)
        assert rh == (L["op"], len(names)), rh
        R = {}
        for name, t in names:
            tt, cnt = struct.unpack_from("<2q", buf, off)
            off += 16
            assert tt == t, (name, tt)
            if cnt == 0:
                R[name] = None
                continue
            a = np.frombuffer(buf, dtype=DT[t], count=cnt, offset=off).copy()
            off += a.nbytes
            assert np.all(is_poison(a[cnt - GUARD:])), "guard entries written behind %s: %s" % (name, np.flatnonzero(~is_poison(a[cnt - GUARD:]))[:5])
            R[name] = a[:cnt - GUARD]
        res.append(R)
    assert off == len(buf), (off, len(buf))
    return res


# ================================================================ envs, tracks, states =========================================================
_cache = {}


def default_track():
    if "track" not in _cache:
        d = np.loadtxt(os.path.join(ROOT, "mpopis_amd", "data", "curve_sf20.csv"), delimiter=",")
        _cache["track"] = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in (d[:, 0], d[:, 1], np.full(d.shape[0], 15.0)))
    return _cache["track"]


def resampled_track(P, shift=(0.0, 0.0), width=15.0):
    """the default centre line resampled at P points evenly spaced along its length, moved by `shift`: another road with another P"""
    tx, ty, _ = default_track()
    x, y = np.append(tx, tx[0]), np.append(ty, ty[0])
    s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
    q = np.linspace(0.0, s[-1], P, endpoint=False)
    return (np.interp(q, s, x) + shift[0], np.interp(q, s, y) + shift[1], np.full(P, width))


def car_params(blim=None):
    if "params" not in _cache:
        _cache["params"] = _oracle().car_default_params()
    p = _cache["params"].copy()
    if blim is not None:
        p[17] = blim
    return p


def car_env(nc, track=None, params=None, lo=None, hi=None, slot_params=None, slot_tracks=None):
    return dict(kind=ENV_CAR, ncars=nc, params=car_params() if params is None else params, track=default_track() if track is None else track,
                lo=-np.ones(2 * nc) if lo is None else lo, hi=np.ones(2 * nc) if hi is None else hi, slot_params=slot_params, slot_tracks=slot_tracks)


def simple_env(kind, ss=None):
    """ss: a state size other than the env's own, for the harness and trace kernels alone (they take it as a plain number)"""
    O = _oracle()
    return dict(ss=ss, kind=kind, ncars=0, params=O.cartpole_default_params() if kind == ENV_CP else O.mountaincar_default_params(), track=None,
                lo=-np.ones(1), hi=np.ones(1), slot_params=None, slot_tracks=None)


def slot_track(env, b):
    return env["slot_tracks"][b] if env.get("slot_tracks") is not None else env["track"]


def slot_params(env, b):
    return env["slot_params"][b] if env.get("slot_params") is not None else env["params"]


def on_off_points(track):
    """a centre-line point more than 40 m from the origin (inside the lane, no lap logic nearby) and a point 500 m off the road"""
    tx, ty, _ = track
    i = int(np.flatnonzero(np.hypot(tx, ty) > 40.0)[0])
    return (float(tx[i]), float(ty[i])), (float(tx[i]) + 500.0, float(ty[i]) + 500.0)


def car8(x, y, psi=1.5, vx=10.0, vy=0.0):
    return np.array([x, y, psi, vx, vy, 0.0, 0.0, 0.0])


# ================================================================ bookkeeping_ref ==============================================================
def noise_ref(s8, seed, step, sig, dtype=LD):
    """car_example.jl:224-236 on one car's state in `dtype` (np.longdouble: the reference of the device's arithmetic; np.float64: the Julia code as it
    runs), the normals of oracle.philox_normals(seed, step, 0x40000000): -> (state, dpsi)"""
    z = _oracle().philox_normals(int(seed), int(step), NOISE_STREAM, 4).astype(dtype)
    s = np.asarray(s8, dtype=np.float64).astype(dtype)
    s[0] += dtype(sig[0]) * z[0]
    s[1] += dtype(sig[1]) * z[1]
    dpsi = dtype(sig[2]) * z[2]
    s[2] += dpsi
    c, sn, vx, vy = np.cos(dpsi), np.sin(dpsi), s[3], s[4]
    s[3] = c * vx + sn * vy
    s[4] = -sn * vx + c * vy
    return s, dpsi


def bookkeeping_ref(kind, ncars, xs, rewards, iters, dones, K, num_steps, laps, blim=None, within_fn=None, noise=None, dtype=np.float64):
    """The trial loop of src/examples/car_example.jl:199-302 (sim_type :cr / :mcr; the simple envs' loops keep lines 203-211 and env.done) on a scripted
    sequence: xs[s] = the state after env(act) of step s, rewards[s] = reward(env), iters[s], dones[s] = env.done of the simple envs.  noise = (seed,
    (sx, sy, spsi)) adds the state noise of :224-236 (one car only) before the logging.  Returns one dict per scripted step: hs = the accumulator in
    the device layout (H_*), alive, x = the state after the noise, and `tr` = what the step's branches saw.  After the loop's condition fails the
    entries repeat unchanged.  dtype: the type of the statistics (v, beta and their sums); counters and the reward sum are float64 always."""
    T = dtype
    rew = 0.0; cnt = 0; lap = 0; prev_y = T(0.0)
    trk_viol = beta_viol = crash_viol = 0
    v_mean_sum = T(0.0); b_mean_sum = T(0.0); v_max = T(-np.inf); b_max = T(-np.inf)
    lap_time = [0, 0, 0, 0]
    rollouts = 0.0
    env_done = False
    out = []
    x_after = None
    for s in range(len(xs)):
        tr = dict(ran=False)
        if (not env_done) and cnt <= num_steps:                              # while !env.done && cnt <= num_steps  (:203)
            tr["ran"] = True
            state = np.asarray(xs[s], dtype=np.float64).astype(T)
            rollouts += float(iters[s]) * K
            cnt += 1                                                         # :208
            step_rew = float(rewards[s])                                     # :210
            rew += step_rew                                                  # :211
            if kind != ENV_CAR:
                env_done = bool(dones[s])
                x_after = np.asarray(xs[s], dtype=np.float64).copy()
            else:
                if ncars == 1 and noise is not None:                         # :224-236 (sim_type == :cr)
                    sl, _ = noise_ref(xs[s], noise[0], s, noise[1], T)
                    x_after = sl.astype(np.float64)                          # the state the env holds from here on is a Float64 vector
                    state = x_after.astype(T)
                else:
                    x_after = np.asarray(xs[s], dtype=np.float64).copy()
                cars = state.reshape(ncars, 8)
                curr_y = min(c[1] for c in cars)                             # :241-243 (the rearmost car)
                vs = [np.sqrt(c[3] * c[3] + c[4] * c[4]) for c in cars]      # :244 / :247 norm(state[4:5])
                bs = [abs(np.arctan2(c[4], c[3])) for c in cars]             # :245 / :248
                v_mean_sum += sum(vs[1:], vs[0]) / T(ncars); b_mean_sum += sum(bs[1:], bs[0]) / T(ncars)      # :250-253 (mean of the logs = their sum / cnt at the end)
                v_max = max(v_max, max(vs)); b_max = max(b_max, max(bs))
                tr.update(viol=False, ex_b=None, within=None, temp_rew=None, crash=False)
                if step_rew < -4000:                                         # :256-263
                    c64 = np.asarray(x_after, dtype=np.float64).reshape(ncars, 8)
                    ex_b = any(abs(np.arctan2(c[4], c[3])) > blim for c in c64)      # exceed_β: any car
                    within_t = all(within_fn(c[:2]) for c in c64)                    # within_track: all cars
                    if ex_b: beta_viol += 1
                    if not within_t: trk_viol += 1
                    temp_rew = step_rew + (5000.0 if ex_b else 0.0) + (1000000.0 if not within_t else 0.0)
                    crash = temp_rew < -10500
                    if crash: crash_viol += 1
                    tr.update(viol=True, ex_b=ex_b, within=within_t, temp_rew=temp_rew, crash=crash)
                d = min(np.sqrt(c[0] * c[0] + c[1] * c[1]) for c in cars)     # :265-270 (the nearest car)
                lapped = bool(prev_y < 0.0 and curr_y >= 0.0 and d <= 15.0)   # :273
                if lapped:
                    lap += 1
                    if lap <= 4: lap_time[lap - 1] = cnt
                tr.update(curr_y=float(curr_y), prev_y=float(prev_y), d=float(d), lapped=lapped, trk=trk_viol, beta=beta_viol, lap=lap)
                if lap >= laps or trk_viol > 10 or beta_viol > 50:            # :277-279
                    env_done = True
                prev_y = curr_y
        hs = np.zeros(H_N, dtype=T)
        hs[[H_REW, H_CNT, H_LAP, H_PREV_Y, H_TRK, H_BETA, H_CRASH]] = [rew, cnt, lap, prev_y, trk_viol, beta_viol, crash_viol]
        hs[[H_VMEAN, H_VMAX, H_BMEAN, H_BMAX]] = [v_mean_sum, v_max, b_mean_sum, b_max]
        hs[H_LAP0:H_LAP0 + 4] = lap_time
        hs[H_ROLL] = rollouts
        out.append(dict(hs=hs, alive=int((not env_done) and cnt <= num_steps), x=None if x_after is None else x_after.copy(), tr=tr, cnt=cnt))
    return out


def record_of(hs, is_car=True):
    """mpopis_run_trials' record from the accumulator (car_example.jl:287-302)"""
    cnt = float(hs[H_CNT])
    r = dict(rew=float(hs[H_REW]), steps=cnt - 1, lap_t=[float(v) for v in hs[H_LAP0:H_LAP0 + 4]], beta_viol=float(hs[H_BETA]), trk_viol=float(hs[H_TRK]),
             crash_viol=float(hs[H_CRASH]), rollouts=float(hs[H_ROLL]))
    if is_car and cnt > 0:
        r.update(mean_v=hs[H_VMEAN] / cnt, max_v=hs[H_VMAX], mean_beta=hs[H_BMEAN] / cnt, max_beta=hs[H_BMAX])
    return r


# ================================================================ LOOP: scripted slots =========================================================
def _below(v):
    return float(np.nextafter(v, -np.inf))


def _above(v):
    return float(np.nextafter(v, np.inf))


def _vel(step, car, over=None, speed=None):
    """(Vx, Vy) of a scripted car: an everyday velocity that changes with step and car, or one at the slip angle `over` (radians)"""
    v = (9.0 + 0.7 * car + 0.31 * step) if speed is None else speed
    if over is None:
        return v, 0.4 * np.sin(1.3 * step + car)
    return v * np.cos(over), v * np.sin(over)


def script(name, nc, nS, track, blim, steps, notes=None):
    """one slot's script.  steps: {s: dict(pos=[(x, y)] * nc or one (x, y) for all, rew=, over={car: angle}, iters=, speed=)}; every other step is
    everyday: all cars on the centre-line point ON, reward -10, iters 3 + s % 4"""
    ON, OFF = on_off_points(track)
    xs, rew, its = np.zeros((nS, 8 * nc)), np.full(nS, -10.0), np.zeros(nS, dtype=np.int32)
    for s in range(nS):
        st = steps.get(s, {})
        pos = st.get("pos", ON)
        pos = [pos] * nc if isinstance(pos[0], float) else list(pos)
        pos = [OFF if p == "OFF" else ON if p == "ON" else p for p in pos]
        for c in range(nc):
            vx, vy = _vel(s, c, st.get("over", {}).get(c), st.get("speed"))
            xs[s, 8 * c:8 * c + 8] = car8(pos[c][0], pos[c][1], 1.5 + 0.01 * s, vx, vy)
        rew[s] = st.get("rew", -10.0 - 0.125 * s)
        its[s] = st.get("iters", 3 + s % 4)
    return dict(name=name, nc=nc, xs=xs, rew=rew, iters=its, notes=notes or {})


def update_scripts(nc, nS, track, blim):
    """The scripted slots of k_harness_update's car cases (laps = 4, num_steps = nS - 1 >= 52).  notes: what tests/test_loop_cases_cpu.py asserts on
    the reference's trace -- name -> (step, key, value) triples."""
    ON, OFF = on_off_points(track)
    far = [ON] * nc
    last = nc - 1
    def one_off(): return [OFF if c == last else ON for c in range(nc)]
    over = 1.5 * blim
    S = []
    # -4000 exactly is no violation; the next double below is (the car is off the road: the track counter moves)
    S.append(script("rew_4000", nc, nS, track, blim, {2: dict(rew=-4000.0, pos=one_off()), 3: dict(rew=_below(-4000.0), pos=one_off())},
                    {2: dict(viol=False), 3: dict(viol=True, within=False, ex_b=False, crash=False, trk=1)}))
    # temp_rew = -10500 exactly, then one ulp of step_rew below, for each (ex_b, !within)
    for eb, ow, base in ((0, 0, -10500.0), (1, 0, -15500.0), (0, 1, -1010500.0), (1, 1, -1015500.0)):
        st = dict(pos=one_off() if ow else far, over={last: over} if eb else {})
        S.append(script("crash_%d%d" % (eb, ow), nc, nS, track, blim, {1: dict(rew=base, **st), 2: dict(rew=_below(base), **st)},
                        {1: dict(viol=True, ex_b=bool(eb), within=not ow, temp_rew=-10500.0, crash=False), 2: dict(viol=True, ex_b=bool(eb), within=not ow, crash=True)}))
    # the 10th and the 11th track violation: the slot ends at the 11th
    S.append(script("trk_11", nc, nS, track, blim, {s: dict(rew=-1000010.0, pos=one_off()) for s in range(1, 12)},
                    {10: dict(trk=10, alive=1), 11: dict(trk=11, alive=0)}))
    # the 50th and the 51st beta violation
    S.append(script("beta_51", nc, nS, track, blim, {s: dict(rew=-5010.0, over={last: over}) for s in range(1, 52)},
                    {50: dict(beta=50, alive=1), 51: dict(beta=51, alive=0)}))
    # |beta| at blim (1 -+ 1e-9): the counter follows the state, whatever the supplied reward says
    S.append(script("beta_edge", nc, nS, track, blim, {1: dict(rew=-5010.0, over={last: blim * (1 + 1e-9)}), 2: dict(rew=-5010.0, over={last: blim * (1 - 1e-9)}),
                                                        3: dict(rew=-10.0, over={last: blim * (1 + 1e-9)})},
                    {1: dict(viol=True, ex_b=True, beta=1), 2: dict(viol=True, ex_b=False, beta=1), 3: dict(viol=False, beta=1)}))
    # laps: prev_y < 0 <= curr_y with curr_y = +0.0, -0.0, +-tiny; prev_y == 0.0 (+0.0 and -0.0) does not count, nor does the first step; the rearmost car's y decides
    tiny = 5e-324
    def at(y, x=3.0, lead=5.0): return [(x, y if c == last else y + lead) for c in range(nc)]          # car `last` is the rearmost
    S.append(script("lap_zero", nc, nS, track, blim, {0: dict(pos=at(1.0)), 1: dict(pos=at(-2.0)), 2: dict(pos=at(0.0)), 3: dict(pos=at(-2.0)), 4: dict(pos=at(-0.0)),
                                                      5: dict(pos=at(-2.0)), 6: dict(pos=at(tiny)), 7: dict(pos=at(-2.0)), 8: dict(pos=at(-tiny)), 9: dict(pos=at(3.0))},
                    {0: dict(lapped=False, prev_y=0.0), 2: dict(lapped=True, curr_y=0.0, lap=1), 4: dict(lapped=True, lap=2, neg_zero=True), 6: dict(lapped=True, lap=3),
                     8: dict(lapped=False, lap=3), 9: dict(lapped=True, lap=4, alive=0)}))
    S.append(script("lap_prev_zero", nc, nS, track, blim, {1: dict(pos=at(-2.0)), 2: dict(pos=at(0.0)), 3: dict(pos=at(2.0)), 4: dict(pos=at(-0.0)), 5: dict(pos=at(2.0))},
                    {2: dict(lapped=True, lap=1), 3: dict(lapped=False, prev_y=0.0), 5: dict(lapped=False, prev_y=-0.0, neg_zero_prev=True)}))
    # d = 15.0 exactly (3-4-5: 9, 12) counts, the next double above does not; the nearest car's d decides (the others are further out)
    def ring(p): return [p if c == 0 else (p[0] + 30.0, p[1] + 1.0 + c) for c in range(nc)]
    S.append(script("lap_d15", nc, nS, track, blim, {1: dict(pos=ring((9.0, -12.0))), 2: dict(pos=ring((9.0, 12.0))), 3: dict(pos=ring((0.0, -_above(15.0)))),
                                                     4: dict(pos=ring((0.0, _above(15.0))))},
                    {2: dict(lapped=True, d=15.0), 4: dict(lapped=False, d=_above(15.0))}))
    # a lap and a violation-triggered end in one step (the lap alone would not end the slot): several cars -- the 11th track violation of car 0 while the
    # rearmost car crosses the line; one car -- every point near the line is on the road, so the 51st beta violation instead
    if nc > 1:
        st = {s: dict(rew=-1000010.0, pos=one_off()) for s in range(1, 11)}
        st[11] = dict(pos=at(-2.0))
        st[12] = dict(rew=-1000010.0, pos=["OFF" if c == 0 else p for c, p in enumerate(at(1.0))])
        S.append(script("lap_and_end", nc, nS, track, blim, st, {12: dict(lap_and_end=True)}))
    else:
        st = {s: dict(rew=-5010.0, over={0: over}) for s in range(1, 52)}
        st[50]["pos"] = at(-2.0); st[51]["pos"] = at(1.0)
        S.append(script("lap_and_end", nc, nS, track, blim, st, {51: dict(lap_and_end=True)}))
    # nothing happens: alive through cnt == num_steps, dead at num_steps + 1
    S.append(script("plain", nc, nS, track, blim, {}, {nS - 2: dict(alive=1), nS - 1: dict(alive=0)}))
    return S


def loop_launch(env, scripts, slot_script, nS, num_steps, laps, K=7, noise=None, seeds=None, alive0=None, mask=63, query=True, actlog=True):
    """a scripted LOOP launch: slot b runs scripts[slot_script[b]]"""
    B, ss, as_ = len(slot_script), state_size(env), action_size(env)
    xs = np.stack([scripts[i]["xs"][:nS] for i in slot_script], axis=1)
    rew = np.stack([scripts[i]["rew"][:nS] for i in slot_script], axis=1)
    its = np.stack([scripts[i]["iters"][:nS] for i in slot_script], axis=1)
    dn = np.stack([scripts[i].get("done", np.zeros(nS, dtype=np.int32))[:nS] for i in slot_script], axis=1)
    rng = np.random.default_rng(B * 1000 + nS)
    control = rng.uniform(-1, 1, (nS, B, as_))
    x0 = rng.normal(size=(B, ss))
    return dict(op=OP_LOOP, B=B, env=env, nS=nS, num_steps=num_steps, laps=laps, K=K, noise=noise, env_step=False, actlog=actlog, mask=mask, query=query,
                x0=x0, xs=xs, reward=rew, iters=its, done_env=dn, control=control, seeds=seeds, alive0=alive0, scripts=scripts, slot_script=list(slot_script))


def slot_ref(L, b, oracle, dtype=np.float64, cache=None, xs=None):
    """bookkeeping_ref of slot b of a scripted LOOP launch (cached per script, env of the slot and noise seed: the result must not depend on B or b).
    xs: the states to book instead of the script's, with no noise -- the states the device held after ITS noise (check_noise holds those to the
    long-double noise; the bookkeeping is then checked on the very numbers it read)"""
    env = L["env"]
    car = env["kind"] == ENV_CAR
    if xs is not None:
        tk = slot_track(env, b)
        return bookkeeping_ref(env["kind"], env["ncars"], xs, L["reward"][:, b], L["iters"][:, b], L["done_env"][:, b], L["K"], L["num_steps"], L["laps"],
                               blim=float(slot_params(env, b)[17]), within_fn=lambda p: oracle.within_track(tk, p)[0], noise=None, dtype=dtype)
    key = (L["slot_script"][b], None if L["seeds"] is None else int(L["seeds"][b]), dtype, id(slot_track(env, b)) if car else 0, float(slot_params(env, b)[17]) if car else 0.0)
    if cache is not None and key in cache:
        return cache[key]
    tk = slot_track(env, b) if car else None
    ref = bookkeeping_ref(env["kind"], env["ncars"], L["xs"][:, b], L["reward"][:, b], L["iters"][:, b], L["done_env"][:, b], L["K"], L["num_steps"], L["laps"],
                          blim=float(slot_params(env, b)[17]) if car else None, within_fn=(lambda p: oracle.within_track(tk, p)[0]) if car else None,
                          noise=(L["seeds"][b], L["noise"]) if (L["noise"] is not None and L["seeds"] is not None) else None, dtype=dtype)
    if cache is not None:
        cache[key] = ref
    return ref


def init_hs():
    h = np.zeros(H_N)
    h[H_VMAX] = h[H_BMAX] = -np.inf
    return h


def loop_shapes(L, R):
    env, B, nS, S = L["env"], L["B"], L["nS"], L["num_steps"] + 1
    ss, as_, nc = state_size(env), action_size(env), max(1, env["ncars"])
    sh = dict(hs_log=(nS, B, H_N), alive_log=(nS, B), x_log=(nS, B, ss), reward_log=(nS, B), q_within=(nS, B), q_dist=(nS, B, nc), q_beta=(nS, B, nc), hs=(B, H_N), alive=(B,),
              x=(B, ss), actlog=(B, S, as_), status=(B,), t=(B,), states=(B, S + 1, ss), rewards=(B, S), iters=(B, S), tr_within=(B, S), tr_dist=(B, S, nc), tr_beta=(B, S, nc))
    return {k: (None if R[k] is None else R[k].reshape(sh[k])) for k in sh}


def check_loop(L, R, oracle, log=print, what="", cache=None):
    """A scripted LOOP launch against bookkeeping_ref, after EVERY step: counters, cnt, lap, lap times, prev_y, reward sum, rollouts and alive exact (bits);
    vmax / bmax within 2 ulp and vmean / bmean within stat_bound of the long-double restatement; a dead slot's hs, x, action log row and trace rows
    unchanged bit for bit; the action log; the trace rows gated by cnt == step + 1 and equal to k_env_query's read-out.  Returns the worst
    (vmean error / bound, bmean error / bound, vmax ulp, bmax ulp)."""
    env, B, nS, S = L["env"], L["B"], L["nS"], L["num_steps"] + 1
    car, nc = env["kind"] == ENV_CAR, max(1, env["ncars"])
    noisy = L["noise"] is not None and car and env["ncars"] == 1
    R = loop_shapes(L, R)
    alive0 = np.ones(B, dtype=np.int32) if L["alive0"] is None else np.asarray(L["alive0"])
    worst = [0.0, 0.0, 0.0, 0.0]
    for b in range(B):
        tag = "%s slot %d (%s)" % (what, b, L["scripts"][L["slot_script"][b]]["name"])
        if not alive0[b]:                                                     # dead from the start: everything stays as launch_harness_init / the poison left it
            for s in range(nS):
                assert np.array_equal(bits(R["hs_log"][s, b]), bits(init_hs())) and R["alive_log"][s, b] == 0, tag
                assert np.array_equal(bits(R["x_log"][s, b]), bits(L["xs"][s, b])), tag
            assert R["actlog"] is None or np.all(is_poison(R["actlog"][b])), tag
            for k in ("rewards", "iters", "tr_within", "tr_dist", "tr_beta"):
                assert R[k] is None or np.all(is_poison(R[k][b])), (tag, k)
            assert R["states"] is None or (np.all(is_poison(R["states"][b, 1:])) and np.array_equal(bits(R["states"][b, 0]), bits(L["x0"][b]))), tag
            continue
        held = R["x_log"][:, b] if noisy else None
        ref = slot_ref(L, b, oracle, np.float64, cache, xs=held)
        refl = slot_ref(L, b, oracle, LD, cache, xs=held) if car else None
        for s in range(nS):
            r, hs = ref[s], R["hs_log"][s, b]
            assert np.array_equal(bits(hs[list(EXACT_FIELDS)]), bits(r["hs"][list(EXACT_FIELDS)])), (tag, s, hs, r["hs"])
            assert R["alive_log"][s, b] == r["alive"], (tag, s)
            ran = r["tr"]["ran"]
            if not car:
                assert np.array_equal(bits(hs), bits(r["hs"])), (tag, s)                      # no car statistics: vmean .. bmax stay as initialised
            else:
                n, hl = r["cnt"], refl[s]["hs"]
                for j, (fm, fx) in enumerate(((H_VMEAN, H_VMAX), (H_BMEAN, H_BMAX))):
                    bound = stat_bound(fm, env["ncars"], n, hl[fm])
                    err = abs(float(LD(hs[fm]) - hl[fm]))
                    assert err <= bound, (tag, s, fm, err, bound)
                    if bound > 0: worst[j] = max(worst[j], err / bound)
                    e = float(ulp_err(hs[fx], hl[fx])) if n > 0 else 0.0
                    assert e <= 2.0, (tag, s, fx, e)
                    worst[2 + j] = max(worst[2 + j], e)
            # x: the script's state (the kernel writes it only through the noise)
            if noisy and ran:
                check_noise(L, b, s, R["x_log"][s, b], tag)
            else:
                assert np.array_equal(bits(R["x_log"][s, b]), bits(L["xs"][s, b])), (tag, s)
            if not ran and s > 0:
                assert np.array_equal(bits(hs), bits(R["hs_log"][s - 1, b])), (tag, s)        # a dead slot's accumulator: bit for bit
            # action log and trace rows of step s
            if R["actlog"] is not None:
                assert (np.array_equal(bits(R["actlog"][b, s]), bits(L["control"][s, b])) if ran else np.all(is_poison(R["actlog"][b, s]))), (tag, s)
            if R["states"] is not None:
                assert (np.array_equal(bits(R["states"][b, s + 1]), bits(R["x_log"][s, b])) if ran else np.all(is_poison(R["states"][b, s + 1]))), (tag, s)
            if R["rewards"] is not None:
                assert (bits(R["rewards"][b, s]) == bits(L["reward"][s, b]) if ran else is_poison(R["rewards"][b, s])), (tag, s)
            if R["iters"] is not None:
                assert (R["iters"][b, s] == L["iters"][s, b] if ran else is_poison(R["iters"][b, s])), (tag, s)
            if R["tr_within"] is not None:
                want = (R["q_within"][s, b] if R["q_within"] is not None else None) if car else 1
                assert (is_poison(R["tr_within"][b, s]) if not ran else (want is None or R["tr_within"][b, s] == want)), (tag, s)
                if ran and car:
                    tk = slot_track(env, b)
                    assert R["tr_within"][b, s] == int(all(oracle.within_track(tk, c[:2])[0] for c in R["x_log"][s, b].reshape(nc, 8))), (tag, s)
            for k, q in (("tr_dist", "q_dist"), ("tr_beta", "q_beta")):
                if R[k] is None:
                    continue
                if not ran or not car:
                    assert np.all(is_poison(R[k][b, s])), (tag, s, k)                        # simple envs write no dist / beta
                elif R[q] is not None:
                    assert np.array_equal(bits(R[k][b, s]), bits(R[q][s, b])), (tag, s, k)   # the kernel's claim: the same bits as k_env_query
        for s in range(nS, S):
            assert R["actlog"] is None or np.all(is_poison(R["actlog"][b, s])), (tag, s)
        if R["states"] is not None:
            assert np.array_equal(bits(R["states"][b, 0]), bits(L["x0"][b])), tag                # k_trace_start: row 0 only
            assert np.all(is_poison(R["states"][b, nS + 1:])), tag
        assert np.array_equal(bits(R["hs"][b]), bits(R["hs_log"][nS - 1, b])) and R["alive"][b] == R["alive_log"][nS - 1, b], tag
    if car and R["q_dist"] is not None:                                       # the query itself against the oracle (every slot, dead or not: it has no gate)
        for s in range(nS):
            for b in range(B):
                for c, st in enumerate(R["x_log"][s, b].reshape(nc, 8)):
                    w, d = oracle.within_track(slot_track(env, b), st[:2])
                    assert abs(R["q_dist"][s, b, c] - d) <= 1e-12 * max(1.0, abs(d)), (what, s, b, c)
                    assert abs(R["q_beta"][s, b, c] - np.arctan2(st[4], st[3])) <= ATAN2_ULP * ulp_of(np.arctan2(st[4], st[3])) + 2.0 ** -1074, (what, s, b, c)
    log("[loop %s] B %d, %s, %d cars: vmean err / bound %.3f, bmean err / bound %.3f, vmax %.2f ulp, bmax %.2f ulp" % (what, B, KIND_NAME[env["kind"]], env["ncars"], *worst))
    return worst


_noise_worst = dict(pos_ulp=0.0, rot_ratio=0.0)


def check_noise(L, b, s, got, tag=""):
    """the state after the noise of step s against the long-double reference: x, y, psi within 2 ulp, the rotated velocity within rot_bound, the rest untouched"""
    sig = L["noise"]
    ref, dpsi = noise_ref(L["xs"][s, b], L["seeds"][b], s, sig)
    e = ulp_err(got[:3], ref[:3])
    assert np.all(e <= 2.0), (tag, s, e)
    vx, vy = L["xs"][s, b][3], L["xs"][s, b][4]
    bound = rot_bound(vx, vy, sig[2], float(dpsi))
    dv = np.abs(got[3:5].astype(LD) - ref[3:5]).astype(np.float64)
    assert np.all(dv <= bound), (tag, s, dv, bound)
    assert np.array_equal(bits(got[5:]), bits(L["xs"][s, b][5:])), (tag, s)
    assert np.any(bits(got[:5]) != bits(L["xs"][s, b][:5])), (tag, s, "the noise must move the state")
    _noise_worst["pos_ulp"] = max(_noise_worst["pos_ulp"], float(e.max()))
    _noise_worst["rot_ratio"] = max(_noise_worst["rot_ratio"], float(dv.max() / bound))
    return float(e.max()), float(dv.max() / bound)


def noise_worst():
    return dict(_noise_worst)


def noise_scripts(nS):
    """one-car slots for the noise cases: coordinates in [64, 128) and psi in [2, 4), so that sigma RNG_TOL stays below half an ulp (NOISE_SIG)"""
    out = []
    for i in range(3):
        xs = np.zeros((nS, 8))
        for s in range(nS):
            xs[s] = [70.0 + 3.1 * s + i, -(90.0 + 1.7 * s + 2 * i), 2.0 + 0.11 * s + 0.3 * i, 11.0 + 0.5 * s, -0.7 + 0.2 * i + 0.05 * s, 0.1, 0.02, 0.3]
        out.append(dict(name="noise_%d" % i, nc=1, xs=xs, rew=np.full(nS, -12.5) - np.arange(nS), iters=np.full(nS, 2, dtype=np.int32), notes={}))
    return out


NOISE_SIG = (0.05, 0.03, 0.001)      # sigma RNG_TOL = 5e-15 / 3e-15 / 1e-16 <= half an ulp of 64 (7.1e-15) and of 2 (2.2e-16)


# ================================================================ STEP ========================================================================
def step_launch(env, x, action, t=None, done=None, status=None, alive=None, skip_step=False, want=None):
    B = len(x)
    w = dict(reward=True, within=True, dist=True, beta=True, qreward=True)
    w.update(want or {})
    return dict(op=OP_STEP, B=B, env=env, x=np.asarray(x, dtype=np.float64), t=np.zeros(B, dtype=np.int32) if t is None else np.asarray(t, dtype=np.int32),
                done=np.zeros(B, dtype=np.int32) if done is None else np.asarray(done, dtype=np.int32), action=None if action is None else np.asarray(action, dtype=np.float64),
                status=status, alive=alive, skip_step=skip_step, want=w)


def step_shapes(L, R):
    env, B = L["env"], L["B"]
    nc = max(1, env["ncars"])
    sh = dict(x=(B, state_size(env)), t=(B,), done=(B,), reward=(B,), status=(B,), qreward=(B,), within=(B,), dist=(B, nc), beta=(B, nc))
    return {k: (None if R[k] is None else R[k].reshape(sh[k])) for k in sh}


def in_bounds(L, b):
    env = L["env"]
    a = L["action"][b].reshape(-1)
    return bool(np.all((a >= env["lo"]) & (a <= env["hi"])))


def step_ref(oracle, L, b):
    """slot b after env(action): (state, t, done, reward) by the oracle -- car_step per car with the slot's parameters, OracleEnv.reward on the slot's track;
    the simple envs by OracleEnv.step"""
    env = L["env"]
    kind = KIND_NAME[env["kind"]]
    e = oracle.OracleEnv(kind, max(env["ncars"], 1) if env["kind"] == ENV_CAR else 0, params=slot_params(env, b), track=slot_track(env, b) if env["kind"] == ENV_CAR else None)
    if env["kind"] == ENV_CAR:
        nc = env["ncars"]
        x = np.concatenate([oracle.car_step(slot_params(env, b), L["x"][b, 8 * c:8 * c + 8], L["action"][b].reshape(nc, 2)[c]) for c in range(nc)])
        e.state = x
        return x, int(L["t"][b]) + 1, int(L["done"][b]), e.reward()
    e.state = L["x"][b]
    e.e.t, e.e.done = int(L["t"][b]), int(L["done"][b])
    assert e.step(L["action"][b].reshape(-1)) == 0
    return e.state, int(e.e.t), int(e.e.done), e.reward()


def query_ref(oracle, env, b, x, done=0):
    kind = KIND_NAME[env["kind"]]
    car = env["kind"] == ENV_CAR
    e = oracle.OracleEnv(kind, env["ncars"] if car else 0, params=slot_params(env, b), track=slot_track(env, b) if car else None)
    e.state = x
    e.e.done = int(done)
    if not car:
        return e.reward(), 1, None, None
    cars = np.asarray(x).reshape(env["ncars"], 8)
    wd = [oracle.within_track(slot_track(env, b), c[:2]) for c in cars]
    return e.reward(), int(all(w for w, _ in wd)), np.array([d for _, d in wd]), np.array([np.arctan2(c[4], c[3]) for c in cars])


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def pair_terms(x, nc):
    cars = np.asarray(x).reshape(nc, 8)
    return [float(np.hypot(cars[j, 0] - cars[i, 0], cars[j, 1] - cars[i, 1])) for i in range(nc) for j in range(i + 1, nc)]


def check_step(oracle, L, R, log=print, what=""):
    """STEP launch against the oracle at the tolerances of tests/test_gpu_parity.py (state 1e-10, reward 1e-9; the query's dist and reward 1e-12), the step
    counter, the action check and its precedence, dead slots untouched, null outputs, and step reward == query reward on the state the step left
    (one car: bit for bit; several cars: within 2 ulp of each pair term).  Returns (worst state dev, worst reward dev, multi-car step-vs-query worst in
    units of its bound, whether that held bitwise)."""
    env, B = L["env"], L["B"]
    car, nc = env["kind"] == ENV_CAR, max(1, env["ncars"])
    R = step_shapes(L, R)
    alive = np.ones(B, dtype=np.int32) if L["alive"] is None else np.asarray(L["alive"])
    st0 = None if L["status"] is None else np.asarray(L["status"])
    worst_x = worst_r = worst_sq = 0.0
    bitwise = True
    for b in range(B):
        tag = "%s slot %d" % (what, b)
        stepped = alive[b] and not L["skip_step"]
        if not stepped:
            assert np.array_equal(bits(R["x"][b]), bits(L["x"][b])) and R["t"][b] == L["t"][b] and R["done"][b] == L["done"][b], tag
            assert R["reward"] is None or is_poison(R["reward"][b]), tag
            assert R["status"] is None or R["status"][b] == st0[b], tag
        else:
            ok = in_bounds(L, b)
            checked = (not car) or env["ncars"] == 1                          # several cars: no check (multi-car_racing.jl:200-207)
            if R["status"] is not None:
                want = st0[b]
                if checked and not ok and st0[b] != ERR_HIP:
                    want = ERR_ACTION
                assert R["status"][b] == want, (tag, R["status"][b], want)
            assert R["t"][b] == L["t"][b] + 1 if car else True, tag
            finite = bool(np.all(np.isfinite(L["action"][b])))
            if ok or (car and not checked and finite and np.all(np.abs(L["action"][b]) <= 1.0)):
                x, t, d, rew = step_ref(oracle, L, b)
                ex = rel(R["x"][b], x)
                assert ex <= 1e-10, (tag, ex)
                assert (R["t"][b], R["done"][b]) == (t, d), (tag, R["t"][b], t, R["done"][b], d)
                worst_x = max(worst_x, ex)
                if R["reward"] is not None:
                    er = abs(R["reward"][b] - rew) / max(1.0, abs(rew))
                    assert er <= 1e-9, (tag, er, R["reward"][b], rew)
                    worst_r = max(worst_r, er)
            elif not car:
                assert R["t"][b] == L["t"][b] + 1, tag                        # the step counter advances whatever the action
        # the query on the state the launch left
        xq = R["x"][b]
        if np.all(np.isfinite(xq)):
            rew, win, dist, beta = query_ref(oracle, env, b, xq, R["done"][b])
            if R["qreward"] is not None:
                assert abs(R["qreward"][b] - rew) <= 1e-12 * max(1.0, abs(rew)), (tag, R["qreward"][b], rew)
            if R["within"] is not None:
                assert R["within"][b] == win, tag
            if car and R["dist"] is not None:
                assert np.all(np.abs(R["dist"][b] - dist) <= 1e-12 * np.maximum(1.0, np.abs(dist))), tag
            if car and R["beta"] is not None:
                assert np.all(np.abs(R["beta"][b] - beta) <= ATAN2_ULP * ulp_of(beta)), tag
            if not car:
                assert (R["dist"] is None or is_poison(R["dist"][b, 0])) and (R["beta"] is None or is_poison(R["beta"][b, 0])), tag
            if stepped and R["reward"] is not None and R["qreward"] is not None:
                if env["ncars"] <= 1:
                    assert bits(R["reward"][b]) == bits(R["qreward"][b]), (tag, R["reward"][b], R["qreward"][b])
                else:
                    # the pair distances are written in each kernel separately and may fuse differently: 2 ulp of each pair term (whether it held bit for
                    # bit is printed)
                    pt = pair_terms(xq, nc)
                    bound = 2.0 * float(np.sum(ulp_of(pt)))
                    dq = abs(R["reward"][b] - R["qreward"][b])
                    assert dq <= bound, (tag, dq, bound)
                    worst_sq = max(worst_sq, dq / bound)
                    bitwise &= bool(bits(R["reward"][b]) == bits(R["qreward"][b]))
    log("[step %s] %s, %d cars, B %d: worst state dev %.2e (1e-10), reward dev %.2e (1e-9); several cars step-vs-query %.3f of its bound, bitwise %s" %
        (what, KIND_NAME[env["kind"]], env["ncars"], B, worst_x, worst_r, worst_sq, bitwise))
    return worst_x, worst_r, worst_sq, bitwise


def parity_states(nc, B, seed):
    """car states on and around the road: the reset grid moved up the road, turned and at speed; slot 1 off the road; coincident cars 0 / 1 in slot 2"""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 8 * nc))
    for b in range(B):
        for c in range(nc):
            ii = c + 1
            gx = 0.0 if ii < 2 else ((ii / 2.0 * 5.0) if ii % 2 == 0 else ((1 - ii) / 2.0 * 5.0))
            x[b, 8 * c:8 * c + 8] = [gx + rng.uniform(-1, 1), 2.0 * b + rng.uniform(0, 3), np.pi / 2 + rng.uniform(-0.2, 0.2), rng.uniform(8, 18), rng.uniform(-1, 1),
                                     rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.5, 0.5)]
        if b == 1:
            x[b, 0] += 60.0
        if b == 2 and nc >= 2:
            x[b, 8:16] = x[b, 0:8]
    return x, rng.uniform(-1, 1, (B, 2 * nc))


def pair_edge_launches():
    """The pair term's edge dd <= 4.0.  By the query on given states: two cars exactly 4.0 apart along one axis (contact), the next double beyond (none), a
    3-4-5 offset (dd = 5 exactly: sqrt and comparison exact, none), coincident cars (contact).  No Pythagorean offset has the length 4.0 in binary, so the
    exact 4.0 is axis-aligned.  Through a step: identical states and actions 4 m apart along y inside one binade ([8, 16)): every rounding of the two
    cars is the same, x stays equal and the difference in y stays exactly 4.0 (contact); the same from the next double above 12 (none); coincident cars."""
    env = car_env(2)
    def two(p, q): return np.concatenate([car8(p[0], p[1], 1.5, 10.0, 0.2), car8(q[0], q[1], 1.5, 10.0, 0.2)])
    q = step_launch(env, np.stack([two((0.0, 0.0), (0.0, 4.0)), two((0.0, 0.0), (0.0, _above(4.0))), two((3.0, 0.0), (0.0, 4.0)), two((1.0, 2.0), (1.0, 2.0)),
                                   two((0.0, 1.0), (4.0, 1.0))]), None, skip_step=True)
    q["contact"] = [True, False, False, True, True]
    s0 = car8(0.0, 8.0, np.pi / 2, 10.0, 0.0)
    s1 = s0.copy(); s1[1] = 12.0
    s2 = s0.copy(); s2[1] = _above(12.0)
    act = np.tile(np.array([0.1, 0.3, 0.1, 0.3]), (3, 1))
    st = step_launch(env, np.stack([np.concatenate([s0, s1]), np.concatenate([s0, s2]), np.concatenate([s0, s0])]), act)
    st["contact"] = [True, False, True]
    return q, st


# ================================================================ PLAN ========================================================================
PLAN_K = (1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025, 2049)


def plan_tops(K):
    return sorted({t for t in (1, 2, K if K <= 64 else 64, 64) if t <= K})


def weight_rows(K, rng):
    """name -> weight row: the orders and ties the selection can get wrong"""
    rows = {}
    rows["equal"] = np.full(K, 1.0 / K)
    rows["two_values"] = np.where(rng.random(K) < 0.5, 0.25, 0.5)
    z = np.zeros(K); z[rng.integers(0, K, max(1, K // 50))] = rng.random(max(1, K // 50)); rows["mostly_zero"] = z
    rows["subnormal"] = rng.integers(1, 1000, K).astype(np.uint64).view(np.float64).copy()
    rows["descending"] = np.linspace(2.0, 1.0, K) if K > 1 else np.array([1.0])
    rows["ascending"] = np.linspace(1.0, 2.0, K) if K > 1 else np.array([1.0])
    t = rng.random(K) * 0.5
    for k in (0, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, K - 1):       # ties that straddle a wave, a 256-thread and a 1024-thread stride
        if 0 <= k < K:
            t[k] = 0.75
    rows["ties_across_strides"] = t
    rows["random"] = rng.random(K)
    return rows


def unsafe_rows(K, rng):
    """rows outside the kernel's contract (NaN, +inf, -0.0): only its safety claim is asserted on them"""
    r = rng.random(K)
    a, b, c = r.copy(), r.copy(), r.copy()
    a[rng.integers(0, K, max(1, K // 7))] = np.nan
    b[rng.integers(0, K, max(1, K // 9))] = np.inf
    c[rng.integers(0, K, max(1, K // 5))] = -0.0
    d = np.full(K, np.nan)
    e = r.copy(); e[::3] = np.nan; e[1::3] = -0.0; e[2::5] = np.inf
    return dict(some_nan=a, some_inf=b, neg_zero=c, all_nan=d, mixed=e)


def plan_launch(K, top, cs, rows, seed, active=None):
    rng = np.random.default_rng(seed)
    B = len(rows)
    return dict(op=OP_PLAN, B=B, K=K, top=top, cs=cs, w=np.stack(rows), E=rng.normal(size=(B, cs, K)), Ucur=rng.normal(size=(B, cs)), Uin=rng.normal(size=(B, cs)),
                wn=rng.normal(size=(B, cs)), active=active)


def plan_shapes(L, R):
    B, top, cs = L["B"], L["top"], L["cs"]
    return dict(idx=R["idx"].reshape(B, top), wsel=R["wsel"].reshape(B, top), controls=R["controls"].reshape(B, cs), Eplan=R["Eplan"].reshape(B, cs, top + 1))


def check_plan(L, R, safety_only=False):
    """idx == plan_order exactly, wsel == w[idx] bitwise, controls and column 0 the one addition, column j = E[r][idx[j-1]] + (Ucur - Uin) bitwise; an inactive slot
    untouched.  safety_only (NaN / inf / -0.0 rows): every index in [0, K) and all `top` distinct; the rest is then asserted against the indices the kernel chose"""
    R = plan_shapes(L, R)
    B, K, top = L["B"], L["K"], L["top"]
    act = np.ones(B, dtype=np.int32) if L["active"] is None else np.asarray(L["active"])
    for b in range(B):
        if not act[b]:
            assert all(np.all(is_poison(R[k][b])) for k in ("idx", "wsel", "controls", "Eplan")), ("inactive slot written", b)
            continue
        idx = R["idx"][b]
        assert np.all((idx >= 0) & (idx < K)), (b, idx)
        assert len(set(idx.tolist())) == top, (b, idx)
        if not safety_only:
            want = plan_order(L["w"][b], top)
            assert np.array_equal(idx, want), (b, K, top, idx[:8], want[:8])
        assert np.array_equal(bits(R["wsel"][b]), bits(L["w"][b][idx])), b
        assert np.array_equal(bits(R["controls"][b]), bits(L["Uin"][b] + L["wn"][b])), b
        assert np.array_equal(bits(R["Eplan"][b, :, 0]), bits(L["wn"][b])), b
        assert np.array_equal(bits(R["Eplan"][b, :, 1:]), bits(L["E"][b][:, idx] + (L["Ucur"][b] - L["Uin"][b])[:, None])), b


# ================================================================ REORDER =====================================================================
REORDER_PER = (1, 255, 256, 257, 1000)


def reorder_launches():
    Ls = []
    rng = np.random.default_rng(11)
    for per in REORDER_PER:
        for B in (1, 2, 5):
            for J in (1, 2, 5):
                for elem in (4, 8):
                    a = rng.integers(-2 ** 31, 2 ** 31 - 1, (J, B, per)).astype(np.int32) if elem == 4 else rng.normal(size=(J, B, per))
                    Ls.append({"op": OP_REORDER, "B": B, "J": J, "per": per, "elem": elem, "in": a})
    return Ls


def check_reorder(L, R):
    want = np.ascontiguousarray(np.transpose(L["in"], (1, 0, 2)))
    got = R["out"].reshape(want.shape)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (L["B"], L["J"], L["per"], L["elem"])
