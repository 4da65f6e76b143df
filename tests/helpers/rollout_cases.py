"""Cases, file format, references and checks for the direct tests of the rollout and step-begin launchers (tools/kbench_rollout.hip, which runs
launch_rollout / launch_extend_state / launch_step_begin on the launches of a case file): shared by tests/test_rollout_cases_cpu.py (which shows on the
CPU that the cases are what they claim, that every checker accepts a result built from the HOST build of car_dynamics.h and that named corruptions of
that result each fail the check meant for them) and tests/test_gpu_rollout_harness.py.  Nothing here touches the engine; references are the oracle,
np.longdouble and NumPy's exact integer arithmetic.  The check_* functions take the outputs in the harness's layout, whoever produced them.

A launch with a per-slot env (ops ROLLOUT_SLOTS / BEGIN_SLOTS: the SENV twins, the fleet body, slot_tk) carries "tracks" (the track table), "tos"
(track_of_slot) and "params" [B][np] or, with "fleet", [B][ncars][20]; slot_track / slot_params / car_params read them, so that every reference and check
below serves the shared and the per-slot launches alike (tests/test_gpu_rollout_slots_harness.py).

A launch is a dict (car_launch / simple_launch / begin_launch, slot_launch / simple_slot_launch / begin_slots_launch make them); pack() writes a list of them as one case file, unpack_result() reads the
result file back into one dict of arrays per launch and asserts that every guard entry is still poison."""
import os
import re
import struct
import numpy as np
from tests.helpers import harness_io as IO
from tests.helpers.harness_io import DT, GUARD, LD, U, bits, is_poison, poisoned      # (re-exported: the tests read them under this module's name)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "mpopis_amd", "csrc")
MAGIC_IN, MAGIC_OUT = b"ROLCASE1", b"ROLRES01"
OP_ROLLOUT, OP_BEGIN, OP_ROLLOUT_SLOTS, OP_BEGIN_SLOTS = 0, 1, 2, 3
ENV_MC, ENV_CAR, ENV_CP = 0, 1, 2
SIMPLE2, SIMPLE4, CUSTOM, TWO_WAVE, SPB1, SPB4, FLEET = range(7)            # engine.h: RolloutBody
BODY_NAME = {SIMPLE2: "simple-2", SIMPLE4: "simple-4", CUSTOM: "custom", TWO_WAVE: "two-wave", SPB1: "one-wave SPB 1", SPB4: "one-wave SPB 4", FLEET: "fleet"}
ERR_ACTION = -3
RTOL = 1e-8                                                                  # tests/test_gpu_parity.py, with its 1e-9 floor
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
DUO_ALWAYS = 1 << 30                                                         # MPOPIS_ROLLOUT_DUO: every launch without the logger takes the two-wave body
ROLLOUT_OUT = ("cost", "traj", "cmin", "status", "iters", "xext")
BEGIN_OUT = ("status", "active", "iters", "iters_acc", "Uin", "Ucur", "cmin", "xext", "xref")
OUT_TYPE = dict(cost=0, traj=0, cmin=2, status=1, iters=1, xext=0, active=1, iters_acc=2, Uin=0, Ucur=0, xref=0)


def cost_key(v):
    """engine.h: the order-preserving map double -> uint64 (unsigned comparison == numeric comparison, NaN sorts last)"""
    u = bits(v)
    return np.where(np.isnan(v), np.uint64(0xfff8000000000000), np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63)))      # every NaN, whatever its sign bit, after +inf


# ================================================================ constants read back from the sources ==========================================
def source_constants():
    """the thresholds rollout_form goes by, from the sources: a constant that moves changes expected_form, and a case written for one form fails"""
    roll = open(os.path.join(CSRC, "kernels_rollout.hip")).read()
    dyn = open(os.path.join(CSRC, "car_dynamics.h")).read()
    eng = open(os.path.join(CSRC, "engine.h")).read()

    def one(pat, s):
        m = re.findall(pat, s)
        assert len(m) == 1, (pat, m)
        return m[0]
    duo = one(r"constexpr int kDuoCarWaves = (\d+), kDuoCarsWaves = (\d+);", roll)
    # engine.h: fleet_static_lds(ncars) = ncars * (2 * 2 * 64 + 4) * sizeof(double); kernels_rollout.hip: counted against 64 * 1024
    fl = [int(v) for v in one(r"constexpr size_t fleet_static_lds\(int ncars\) \{ return \(size_t\)ncars \* \((\d+) \* (\d+) \* (\d+) \+ (\d+)\) \* sizeof\(double\); \}", eng)]
    return dict(fleet_static_per_car=(fl[0] * fl[1] * fl[2] + fl[3]) * 8,
                kFleetLdsDefault=int(one(r"f\.tlds = lds_all \+ fleet_static_lds\(NC\) <= (\d+) \* 1024;", roll)) * 1024,
                kDuoCarWaves=int(duo[0]), kDuoCarsWaves=int(duo[1]),
                spb4_K=int(one(r"a\.K >= (\d+) \? ROLLOUT_ONE_WAVE_SPB4", roll)),
                kRolloutDynLdsDefault=int(one(r"constexpr size_t kRolloutDynLdsDefault = (\d+) \* 1024;", roll)) * 1024,
                kRingStride=int(one(r"constexpr int kRingStride = (\d+);", dyn)), kRingPad=int(one(r"constexpr int kRingPad = (\d+);", dyn)),
                kCarExt=int(one(r"constexpr int kCarExt = (\d+);", dyn)), kTrackNbrW=int(one(r"constexpr int kTrackNbrW = (\d+);", dyn)))


def track_lds_bytes(P, W, all_tables, c):
    """kernels_rollout.hip: ring table [(P + 2 pad)][stride] + two certificates [2][P]; all: + x, y, w, |q|^2 [4][P] + neighbour distances and indices [P][W + 1]"""
    return (c["kRingStride"] * (P + 2 * c["kRingPad"]) + 2 * P) * 8 + ((4 * P * 8 + P * (W + 1) * (8 + 4)) if all_tables else 0)


def max_tlds_points(c):
    """the largest P whose tables all fit the default dynamic LDS"""
    P = 1
    while track_lds_bytes(P + 1, min(c["kTrackNbrW"], P + 1), True, c) <= c["kRolloutDynLdsDefault"]:
        P += 1
    return P


def fleet_static_lds(nc, c):
    """engine.h: static LDS of the fleet body (the position exchange + the per-car action bounds)"""
    return nc * c["fleet_static_per_car"]


def max_tlds_points_fleet(nc, c):
    """the largest P whose tables all fit beside the fleet body's static LDS: lds_all + fleet_static_lds(nc) <= 64 KiB"""
    P = 1
    while track_lds_bytes(P + 1, min(c["kTrackNbrW"], P + 1), True, c) + fleet_static_lds(nc, c) <= c["kFleetLdsDefault"]:
        P += 1
    return P


def samples_per_wave(nc):
    return 64 // nc


# ---- a launch with a per-slot env (op ROLLOUT_SLOTS / BEGIN_SLOTS): "tracks" = the track table, "tos" = track_of_slot, "params" [B][np] or, "fleet", [B][nc][20]
def is_rollout(L):
    return L["op"] in (OP_ROLLOUT, OP_ROLLOUT_SLOTS)


def has_slots(L):
    return L["op"] in (OP_ROLLOUT_SLOTS, OP_BEGIN_SLOTS)


def is_fleet(L):
    return bool(L.get("fleet"))


def slot_track(L, b):
    return L["tracks"][L["tos"][b]] if has_slots(L) else L["track"]


def slot_params(L, b):
    """slot b's parameter vector; a fleet: its [nc][20] vectors"""
    return L["params"][b] if has_slots(L) else L["params"]


def car_params(L, b, c):
    return slot_params(L, b)[c] if is_fleet(L) else slot_params(L, b)


def expected_form(L, duo=None, max_wg=None, c=None):
    """rollout_form restated: (body, log, tlds, dynamic LDS bytes).  duo: MPOPIS_ROLLOUT_DUO of the process (None: unset, then max_wg =
    MPOPIS_COOP_MAX_WG stands for the device's CU count)"""
    c = c or source_constants()
    log = bool(L["traj"])
    if L["kind"] != ENV_CAR:
        return (SIMPLE4 if L["kind"] == ENV_CP else SIMPLE2, log, False, 0)
    nc = L["ncars"]
    # per-slot tracks: the LARGEST track of the launch decides the placement and the LDS size (SlotEnv::lds_all / lds_ring)
    Ps = [len(slot_track(L, b)[0]) for b in range(L["B"])] if has_slots(L) else [L["P"]]
    lds = lambda all_tables: max(track_lds_bytes(P, min(c["kTrackNbrW"], P), all_tables, c) for P in Ps)
    if is_fleet(L):
        tlds = lds(True) + fleet_static_lds(nc, c) <= c["kFleetLdsDefault"]
        return (FLEET, log, tlds, lds(tlds))
    tlds = lds(True) <= c["kRolloutDynLdsDefault"]
    S = 64 // nc
    waves = L["B"] * ((L["K"] + S - 1) // S) * max(1, L["share"])
    limit = duo if duo is not None else (c["kDuoCarWaves"] if nc == 1 else c["kDuoCarsWaves"]) * max_wg
    body = TWO_WAVE if (not log and waves <= limit) else (SPB4 if L["K"] >= c["spb4_K"] else SPB1)
    return (body, log, tlds, lds(tlds))


# ================================================================ the harness's files =========================================================
def _track_table(L):
    """track_P, tx, ty, tw (concatenated), track_of_slot of a per-slot launch"""
    tr = L["tracks"]
    cat = lambda i: np.concatenate([np.asarray(t[i], dtype=np.float64) for t in tr])
    return np.array([len(t[0]) for t in tr], dtype=np.int32), cat(0), cat(1), cat(2), np.asarray(L["tos"], dtype=np.int32)


def _fields(L):
    if L["op"] == OP_ROLLOUT_SLOTS:
        car = L["kind"] == ENV_CAR
        tP, tx, ty, tw, tos = _track_table(L) if car else (None,) * 5
        ip = [L["kind"], L["ncars"], L["K"], L["T"], len(L["tracks"]) if car else 0, L["iter_n"], L["share"], int(L["traj"]), int(L["iters"]), L["begin"], int(is_fleet(L))]
        arrays = [(1, L["active"]), (0, L["params"]), (0, tx), (0, ty), (0, tw), (0, L["lo"]), (0, L["hi"]), (0, L["x0"]), (1, L["t0"]), (1, L["done0"]),
                  (0, L["U"]), (0, L["Uo"]), (0, L["E"]), (0, L["gvec"]), (2, L["cmin"]), (1, L["status"]), (1, tP), (1, tos)]
    elif L["op"] == OP_BEGIN_SLOTS:
        tP, tx, ty, tw, tos = _track_table(L)
        ip = [L["ncars"], L["cs"], len(L["tracks"])]
        arrays = [(1, L["alive"]), (1, L["status"]), (1, L["iters"]), (2, L["iters_acc"]), (0, L["U"]), (0, L["x"]), (0, tx), (0, ty), (0, tw), (2, L["cmin"]), (1, tP), (1, tos)]
    elif L["op"] == OP_ROLLOUT:
        ip = [L["kind"], L["ncars"], L["K"], L["T"], L["P"], L["iter_n"], L["share"], int(L["traj"]), int(L["iters"]), L["begin"]]
        tr = L["track"] if L["track"] is not None else (None, None, None)
        arrays = [(1, L["active"]), (0, L["params"]), (0, tr[0]), (0, tr[1]), (0, tr[2]), (0, L["lo"]), (0, L["hi"]), (0, L["x0"]), (1, L["t0"]), (1, L["done0"]),
                  (0, L["U"]), (0, L["Uo"]), (0, L["E"]), (0, L["gvec"]), (2, L["cmin"]), (1, L["status"])]
    else:
        ip = [L["ncars"], L["cs"], L["P"]]
        tr = L["track"] if L["track"] is not None else (None, None, None)
        arrays = [(1, L["alive"]), (1, L["status"]), (1, L["iters"]), (2, L["iters_acc"]), (0, L["U"]), (0, L["x"]), (0, tr[0]), (0, tr[1]), (0, tr[2]), (2, L["cmin"])]
    return ip, arrays


def pack(launches):
    records = []
    for L in launches:
        ip, arrays = _fields(L)
        records.append(IO.pack_launch(L["op"], L["B"], ip, [], arrays))
    return IO.pack_launches(MAGIC_IN, records)


def state_size(L):
    return 8 * L["ncars"] if L["kind"] == ENV_CAR else (4 if L["kind"] == ENV_CP else 2)


def out_shapes(L):
    """name -> shape of every output the launch was given a buffer for (None: not given)"""
    B = L["B"]
    if is_rollout(L):
        car = L["kind"] == ENV_CAR
        return dict(cost=(B, L["K"]), traj=(B, L["K"], state_size(L), L["T"]) if L["traj"] else None, cmin=(B,) if L["cmin"] is not None else None,
                    status=(B,) if L["status"] is not None else None, iters=(B,) if L["iters"] else None, xext=(B, L["ncars"], 13) if car else None)
    nc = L["ncars"]
    return dict(status=(B,) if L["status"] is not None else None, active=(B,), iters=(B,), iters_acc=(B,) if L["iters_acc"] is not None else None,
                Uin=(B, L["cs"]), Ucur=(B, L["cs"]), cmin=(B,) if L["cmin"] is not None else None, xext=(B, nc, 13) if nc > 0 else None,
                xref=(B, nc, 13) if (nc > 0 and L["x"] is not None) else None)


def pack_result(launches, results):
    """what the harness writes (the CPU round trip; puts a host-built result through the same unpacking): results = one dict name -> array per launch, with
    the key "form"; an entry "guard" = (name, index, value) writes one guard entry"""
    out = [MAGIC_OUT, struct.pack("<2q", GUARD, len(launches))]
    for L, R in zip(launches, results):
        names = ROLLOUT_OUT if is_rollout(L) else BEGIN_OUT
        out.append(struct.pack("<6q", L["op"], *[int(v) for v in R["form"]], len(names)))
        for n in names:
            shape, t = out_shapes(L)[n], OUT_TYPE[n]
            if shape is None:
                out.append(IO.pack_array(t, None))
                continue
            g = poisoned((GUARD,), t)
            if R.get("guard") and R["guard"][0] == n:
                g[R["guard"][1]] = R["guard"][2]
            a = np.ascontiguousarray(R[n], dtype=DT[t]).reshape(-1)
            assert a.size == int(np.prod(shape)), (n, a.size, shape)
            out.append(IO.pack_array(t, np.concatenate([a, g])))
    return b"".join(out)


def unpack_result(buf, launches):
    """-> one dict per launch: form = (body, log, tlds, lds) and every output by name in its shape (None: not given); asserts the header, the sizes
    and that every guard entry is still poison (nothing was written past the end)"""
    assert buf[:8] == MAGIC_OUT, buf[:8]
    guard, n = struct.unpack_from("<2q", buf, 8)
    assert (guard, n) == (GUARD, len(launches)), (guard, n, len(launches))
    off, res = 24, []
    for L in launches:
        rh = struct.unpack_from("<6q", buf, off)
        off += 48
        names = ROLLOUT_OUT if is_rollout(L) else BEGIN_OUT
        assert rh[0] == L["op"] and rh[5] == len(names), rh
        R = dict(form=(rh[1], bool(rh[2]), bool(rh[3]), rh[4]))
        shapes = out_shapes(L)
        for name in names:
            t, cnt = struct.unpack_from("<2q", buf, off)
            off += 16
            assert t == OUT_TYPE[name], (name, t)
            if shapes[name] is None:
                assert cnt == 0, (name, cnt)
                R[name] = None
                continue
            want = int(np.prod(shapes[name]))
            assert cnt == want + GUARD, (name, cnt, want)
            a = np.frombuffer(buf, dtype=DT[t], count=cnt, offset=off).copy()
            off += a.nbytes
            assert np.all(is_poison(a[want:])), "guard entries written behind %s: %s" % (name, np.flatnonzero(~is_poison(a[want:]))[:5])
            R[name] = a[:want].reshape(shapes[name])
        res.append(R)
    assert off == len(buf), (off, len(buf))
    return res


# ================================================================ tracks, start states, launches ===============================================
_cache = {}


def default_track():
    if "track" not in _cache:
        d = np.loadtxt(os.path.join(ROOT, "mpopis_amd", "data", "curve_sf20.csv"), delimiter=",")
        _cache["track"] = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in (d[:, 0], d[:, 1], np.full(d.shape[0], 15.0)))
    return _cache["track"]


def big_track(P):
    """the default centre line (a closed polyline) resampled at P points evenly spaced along its length: the same road with more points than the LDS holds"""
    if ("big", P) not in _cache:
        tx, ty, _ = default_track()
        x, y = np.append(tx, tx[0]), np.append(ty, ty[0])
        s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
        q = np.linspace(0.0, s[-1], P, endpoint=False)
        _cache[("big", P)] = (np.interp(q, s, x), np.interp(q, s, y), np.full(P, 15.0))
    return _cache[("big", P)]


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


def reset_state(nc):
    """car_racing.jl:215-223; multi-car_racing.jl:160-180 (the CPU test compares it with the oracle's reset)"""
    s = np.zeros(8 * nc)
    for c in range(nc):
        ii = c + 1
        if ii >= 2:
            s[8 * c] = (ii / 2.0 * 5.0) if ii % 2 == 0 else ((1 - ii) / 2.0 * 5.0)
        s[8 * c + 2] = 90.0 * (np.pi / 180.0)
        s[8 * c + 3] = 10.0
    return s


def start_states(nc, B):
    """slot 0: the reset grid.  slot 1: close_starts of tests/test_gpu_many_cars.py -- cars 0 / 1 coincident, car 2 3 m from car 0 (the -11000 contact term),
    the rest faster and shifted; one car: shifted and faster (tests/test_gpu_parity.py).  Further slots: the grid moved up the road, faster.  Vx >= 10 everywhere"""
    x0 = np.stack([reset_state(nc) for _ in range(B)])
    if B > 1:
        if nc == 1:
            x0[1, 0] += 2.0; x0[1, 3] = 17.0
        if nc >= 2:
            x0[1, 8:10] = x0[1, 0:2]
        if nc >= 3:
            x0[1, 16] = x0[1, 0] + 3.0; x0[1, 17] = x0[1, 1]
        for c in range(3, nc):
            x0[1, 8 * c + 1] += 1.5 * c; x0[1, 8 * c + 3] = 13.0
    for b in range(2, B):
        x0[b, 1::8] += 1.0 * b; x0[b, 3::8] = 10.0 + b
    return x0


def car_bounds(nc):
    """per-car action bounds inside RL.jl's [-1, 1]: different for every car, not symmetric"""
    lo, hi = np.zeros(2 * nc), np.zeros(2 * nc)
    for c in range(nc):
        lo[2 * c], hi[2 * c] = -1.0 + 0.05 * c, 0.6 + 0.04 * c
        lo[2 * c + 1], hi[2 * c + 1] = -0.9 + 0.1 * c, 1.0 - 0.06 * c
    return lo, hi


def car_launch(nc, B, K, T, seed, track=None, far=3, grid=False, **kw):
    """one launch_rollout of the car env.  E is kept in the device layout [B][cs][K], control row r = t * 2 nc + 2 c + i.  far: that many samples of slot 0
    get their noise x 8 (clamps, off the road, slip penalties).  grid: U and E on a 2^-20 grid (their sums are exact)"""
    rng = np.random.default_rng(seed)
    cs = 2 * nc * T
    track = default_track() if track is None else track
    Uc = rng.uniform(-0.3, 0.3, (B, cs)); Uc[:, 1::2] += 0.3
    E = rng.standard_normal((B, K, cs)) * np.tile([0.25, 0.32], nc * T)
    E[0, :min(far, K)] *= 8.0
    if grid:
        Uc, E = np.round(Uc * 2.0 ** 20) / 2.0 ** 20, np.round(E * 2.0 ** 20) / 2.0 ** 20
    lo, hi = car_bounds(nc)
    L = dict(op=OP_ROLLOUT, kind=ENV_CAR, ncars=nc, B=B, K=K, T=T, P=len(track[0]), track=track, params=_oracle().car_default_params(), lo=lo, hi=hi,
             x0=start_states(nc, B), t0=None, done0=None, U=Uc, Uo=Uc.copy(), E=np.ascontiguousarray(E.transpose(0, 2, 1)), gvec=None, active=None, cmin=None,
             status=None, traj=False, iters=False, iter_n=3, share=1, begin=0)
    L.update(kw)
    return L


def simple_launch(kind, B, K, T, seed, x0, t0=None, done0=None, **kw):
    rng = np.random.default_rng(seed)
    O = _oracle()
    E = rng.standard_normal((B, K, T)) * 1.2                              # beyond the action bounds in a third of the steps
    Uc = rng.uniform(-0.2, 0.2, (B, T))
    L = dict(op=OP_ROLLOUT, kind=kind, ncars=0, B=B, K=K, T=T, P=0, track=None, params=O.cartpole_default_params() if kind == ENV_CP else O.mountaincar_default_params(),
             lo=np.array([-1.0]), hi=np.array([1.0]), x0=np.asarray(x0, dtype=np.float64), t0=t0, done0=done0, U=Uc, Uo=Uc.copy(),
             E=np.ascontiguousarray(E.transpose(0, 2, 1)), gvec=None, active=None, cmin=None, status=None, traj=False, iters=False, iter_n=3, share=1, begin=0)
    L.update(kw)
    return L


def active_slots(L):
    return [b for b in range(L["B"]) if L["active"] is None or L["active"][b]]


def controls(L, b, lo=None, hi=None):
    """V = U + E[:, k] and the clamped actions of slot b, both [cs][K] (simulate_model :271, get_model_controls: NaN passes through)"""
    lo, hi = (L["lo"] if lo is None else lo), (L["hi"] if hi is None else hi)
    a = len(lo)
    V = L["U"][b][:, None] + L["E"][b]
    l, h = np.tile(lo, L["T"])[:, None], np.tile(hi, L["T"])[:, None]
    with np.errstate(invalid="ignore"):
        return V, np.where(V > h, h, np.where(V < l, l, V))


# ================================================================ references ===================================================================
def oracle_costs(oracle, L, log=False):
    """OraclePolicy.simulate_model per active slot -> {b: cost [K]} (log: {b: (cost, traj [K][T][ss])}).  A per-slot launch: the env of slot b's own
    parameters and track; a fleet: car_fleet_ref.fleet_rollout, the oracle's per-car step and reward composed in the reference's order"""
    kind = {ENV_CAR: "car", ENV_MC: "mountaincar", ENV_CP: "cartpole"}[L["kind"]]
    a = len(L["lo"])
    if is_fleet(L):
        from tests.helpers import car_fleet_ref as FR
        return {b: FR.fleet_rollout(oracle, slot_params(L, b), slot_track(L, b), L["x0"][b], L["U"][b], np.ascontiguousarray(L["E"][b].T), lo=L["lo"], hi=L["hi"], log=log)
                for b in active_slots(L)}

    def make(b):
        env = oracle.OracleEnv(kind, L["ncars"], params=slot_params(L, b), track=slot_track(L, b) if L["kind"] == ENV_CAR else None)
        pol = oracle.OraclePolicy("gmppi", env, L["K"], L["T"], lam=10.0, U0=np.zeros(a), cov=np.ones(a), nthreads=8)
        for i in range(a):
            pol.p.lo[i], pol.p.hi[i] = L["lo"][i], L["hi"][i]
        return env, pol
    if not has_slots(L):
        env, pol = make(0)
    out = {}
    for b in active_slots(L):
        if has_slots(L):
            env, pol = make(b)
        env.state = L["x0"][b]
        env.e.t = int(L["t0"][b]) if L["t0"] is not None else 0
        env.e.done = int(L["done0"][b]) if L["done0"] is not None else 0
        out[b] = pol.simulate_model(L["U"][b], L["E"][b], log=log)
    return out


def rel_err(a, b):
    """tests/test_gpu_parity.py"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-9)))


def check_form(L, R, duo=None, max_wg=None, want_body=None):
    want = expected_form(L, duo, max_wg)
    assert tuple(R["form"]) == want, ("rollout_form", R["form"], "restated", want)
    assert want_body is None or want[0] == want_body, ("this case was written for", BODY_NAME[want_body], "and runs", BODY_NAME[want[0]])


def check_slots(L, R):
    """inactive slots keep their poison in cost, traj and iters and their value in cmin and status; active slots are written everywhere and report iter_n"""
    act = active_slots(L)
    for b in range(L["B"]):
        if b in act:
            assert not is_poison(R["cost"][b]).any(), ("cost: untouched entries in slot", b)
            if R["traj"] is not None:
                assert not is_poison(R["traj"][b]).any(), ("traj: untouched entries in slot", b)
            if R["iters"] is not None:
                assert R["iters"][b] == L["iter_n"], ("iters", b, R["iters"][b])
        else:
            assert is_poison(R["cost"][b]).all(), ("cost written in the inactive slot", b)
            assert R["traj"] is None or is_poison(R["traj"][b]).all(), ("traj written in the inactive slot", b)
            assert R["iters"] is None or is_poison(R["iters"][b]), ("iters written in the inactive slot", b)
            assert R["cmin"] is None or R["cmin"][b] == np.uint64(L["cmin"][b]), ("cmin written in the inactive slot", b)
            assert R["status"] is None or R["status"][b] == L["status"][b], ("status written in the inactive slot", b)


def check_parity(oracle, L, R, log=print, what="", ref=None):
    """cost (and traj, when logged) of every active slot against simulate_model at RTOL -> the worst deviation.  Costs and the car env's trajectories by
    rel_err (floor 1e-9); the simple envs' trajectories relative to max(1, |ref|), a different metric (see below).  ref: oracle_costs of this launch,
    computed by the caller (with log when the launch logs) and shared between the launches that have the same inputs"""
    ref = oracle_costs(oracle, L, log=bool(L["traj"])) if ref is None else ref
    worst = 0.0
    for b, r in ref.items():
        c = r[0] if L["traj"] else r
        fin = np.isfinite(c)
        assert np.array_equal(np.isfinite(R["cost"][b]), fin), (what, "finite costs differ", b)
        e = rel_err(R["cost"][b][fin], c[fin]) if fin.any() else 0.0
        assert e < RTOL, (what, "slot", b, "cost deviates", e, int(np.argmax(np.abs(R["cost"][b] - c))))
        worst = max(worst, e)
        if L["traj"]:
            t = np.transpose(r[1], (0, 2, 1))                               # [K][T][ss] -> [K][ss][T]
            # the simple envs' states are sums of O(1) terms that pass through zero (an angle of 1e-4 carries the rounding of its O(1) history): their
            # deviation is taken relative to max(1, |ref|), as dynamics_cases.check_step takes a state's
            e = rel_err(R["traj"][b], t) if L["kind"] == ENV_CAR else float(np.max(np.abs(R["traj"][b] - t) / np.maximum(1.0, np.abs(t))))
            assert e < RTOL, (what, "slot", b, "trajectory deviates", e)
            worst = max(worst, e)
    return worst


def check_cmin(L, R):
    """cmin[b] = min(the value before the launch, min_k cost_key(cost[b][k])) compared as u64; status: MPOPIS_ERR_ACTION exactly where a cost is not finite"""
    if R["cmin"] is None:
        assert R["status"] is None or np.array_equal(R["status"], L["status"]), ("status written without cmin", R["status"])
        return
    for b in active_slots(L):
        want = min(int(np.uint64(L["cmin"][b])), int(cost_key(R["cost"][b]).min()))
        assert int(R["cmin"][b]) == want, ("cmin", b, hex(int(R["cmin"][b])), hex(want))
        if R["status"] is not None:
            bad = not np.all(np.isfinite(R["cost"][b]))
            assert R["status"][b] == (ERR_ACTION if bad else L["status"][b]), ("status", b, R["status"][b], bad)


def _psi_dev(got, ref):
    d = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    d[..., 2] = np.minimum(d[..., 2], np.abs(np.abs(got[..., 2] - ref[..., 2]) - 2 * np.pi))      # the heading's wrap may land on either side at exactly +-pi
    return d


def check_logger(oracle, L, R, log=print, what=""):
    """The logger form step by step (layout [B][K][8 nc][T]): every logged state against oracle.car_step -- under the parameters of THAT car of that slot -- from the state logged before it (the first from x0)
    under clamp(U + E) at dynamics_cases.check_step's 1e-11 -- cases whose sign(Vx) is decided within rounding of zero would be set aside (deviation beyond
    1e-9), counted and capped; these driving starts allow none -- and the cost against the long-double sum over t of the oracle's reward AT THE LOGGED STATES
    plus the control cost: each reward held to check_slip's 1e-12 max(1, |r|), the summation to 2 (T nc + 8) u sum |terms|.  -> (worst state deviation, worst cost ratio)"""
    nc, K, T = L["ncars"], L["K"], L["T"]
    worst, ratio = 0.0, 0.0
    for b in active_slots(L):
        if is_fleet(L):                                                      # every car's own reward under its own parameters + the pair terms (car_fleet_ref)
            from tests.helpers import car_fleet_ref as FR
            reward = lambda x, b=b: FR.fleet_reward(oracle, slot_params(L, b), slot_track(L, b), x)
        else:
            env = oracle.OracleEnv("car", nc, params=slot_params(L, b), track=slot_track(L, b))

            def reward(x, env=env):
                env.state = x.reshape(-1)
                return env.reward()
        V, A = controls(L, b)
        X = R["traj"][b].reshape(K, nc, 8, T).transpose(0, 1, 3, 2)          # [K][nc][T][8]
        A = A.reshape(T, nc, 2, K).transpose(3, 1, 0, 2)                     # [K][nc][T][2]
        prev = np.concatenate([np.broadcast_to(L["x0"][b].reshape(1, nc, 1, 8), (K, nc, 1, 8)), X[:, :, :-1]], axis=2)
        ref = np.empty_like(X)
        for k in range(K):
            for c in range(nc):
                for t in range(T):
                    ref[k, c, t] = oracle.car_step(car_params(L, b, c), prev[k, c, t], A[k, c, t])
        dev = _psi_dev(X, ref).max(axis=-1)
        aside = dev > 1e-9
        assert int(aside.sum()) == 0, (what, "slot", b, "states set aside", int(aside.sum()), "cap 0 (driving)", float(dev.max()))
        assert dev.max() < 1e-11, (what, "slot", b, "state deviates", float(dev.max()), np.unravel_index(int(np.argmax(dev)), dev.shape))
        worst = max(worst, float(dev.max()))
        r = np.empty((K, T))
        for k in range(K):
            for t in range(T):
                r[k, t] = reward(np.ascontiguousarray(X[k, :, t]))
        cc = np.zeros(K, dtype=LD)
        if L["gvec"] is not None:
            cc = (L["gvec"][b].astype(LD)[:, None] * (V.astype(LD) - L["Uo"][b].astype(LD)[:, None])).sum(axis=0)
        refc = (-r.astype(LD)).sum(axis=1) + cc
        mag = np.abs(r).sum(axis=1) + np.abs(cc)
        bound = (1e-12 * np.maximum(1.0, np.abs(r))).sum(axis=1) + 2 * (T * nc + 8) * U * mag
        q = float(np.max(np.abs(R["cost"][b].astype(LD) - refc) / bound))
        assert q <= 1.0, (what, "slot", b, "cost against the rewards at the logged states", q)
        ratio = max(ratio, q)
    return worst, ratio


def gvec_of(L, gamma, Sigma_inv):
    """gvec = gamma U_orig' Sigma^-1 in long double, rounded once"""
    return np.stack([(gamma * L["Uo"][b].astype(LD)) @ Sigma_inv.astype(LD) for b in range(L["B"])]).astype(np.float64)


def cost_terms_sum(oracle, L, b):
    """sum over steps and cars of |the car's own reward| + |its pair terms| along the oracle's trajectories [K]: no partial sum of a sample's cost exceeds it"""
    nc, K, T = L["ncars"], L["K"], L["T"]
    _, traj = oracle_costs(oracle, L, log=True)[b]
    ones = [oracle.OracleEnv("car", 1, params=car_params(L, b, c), track=slot_track(L, b)) for c in range(nc if is_fleet(L) else 1)]
    tot = np.zeros(K)
    for k in range(K):
        for t in range(T):
            for c in range(nc):
                one = ones[c if is_fleet(L) else 0]
                one.state = traj[k, t, 8 * c:8 * c + 8]
                tot[k] += abs(one.reward())
                for q in range(c + 1, nc):
                    dd = np.hypot(*(traj[k, t, 8 * q:8 * q + 2] - traj[k, t, 8 * c:8 * c + 2]))
                    tot[k] += dd + (11000.0 if dd <= 4.0 else 0.0)
    return tot


def check_gamma(oracle, L, R, R0, log=print, what=""):
    """cost - cost(gamma = 0) against sum_r gvec_r (V_r - U_orig_r) in long double; bound 2 (cs + 8) u sum |terms| + u |cost| -> the worst ratio.
    The bound's second term is the one rounding of cost + control cost.  With nc cars the kernels add each car's control cost to that car's cost and then
    sum the cars, in both launches: nc + 2 (nc - 1) roundings, each of at most u (C + sum |terms|) with C = cost_terms_sum, of which the first term of the
    bound has to carry 3 nc - 3.  It does where 2 (cs + 8) sum |terms| >= (3 nc - 3) (C + sum |terms|), which this check demands of its case
    (gamma_launches: the project's own covariance scale, no contact and no off-road penalties in the costs) instead of assuming it."""
    nc = L["ncars"]
    cs = 2 * nc * L["T"]
    ratio = 0.0
    for b in active_slots(L):
        V, _ = controls(L, b)
        terms = L["gvec"][b].astype(LD)[:, None] * (V.astype(LD) - L["Uo"][b].astype(LD)[:, None])
        mag = np.abs(terms).sum(axis=0)
        if nc > 1:
            C = cost_terms_sum(oracle, L, b)
            assert np.all(2 * (cs + 8) * mag >= (3 * nc - 3) * (C + mag)), (what, "the case does not carry the bound", float(mag.min()), float(C.max()))
        bound = 2 * (cs + 8) * U * mag + U * np.abs(R["cost"][b])
        q = float(np.max(np.abs((R["cost"][b].astype(LD) - R0["cost"][b].astype(LD)) - terms.sum(axis=0)) / bound))
        ratio = max(ratio, q)
    return ratio


# ================================================================ step-begin cases ============================================================
BEGIN_P = (1, 2, 5, 63, 64, 65, 255, 256, 257, 300, 2048)
BEGIN_CS = (1, 255, 256, 257, 800)


def tie_classes(P):
    """the index sets a start position is made equidistant from, by where k_step_begin's 256-thread search meets them: in one thread (i, i + 256), in
    different waves (i, i + 64), in neighbouring lanes (i, i + 1), across the wrap (0, P - 1), and all of one thread, two waves (i, i + 64, i + 256)"""
    out = {}
    if P >= 257:
        i = min(5, P - 257); out["thread"] = (i, i + 256)
        out["three"] = (i, i + 64, i + 256)
    if P >= 65:
        i = min(7, P - 65); out["waves"] = (i, i + 64)
    if P >= 2:
        i = min(9, P - 2); out["lanes"] = (i, i + 1)
    if P >= 3:
        out["wrap"] = (0, P - 1)
    if P == 1:
        out["single"] = (0,)
    return out


def tie_track(P, idx):
    """P track points on small integer coordinates, far from the origin (x = 1000 + k, y = 2000 + k mod 7), except the points of idx: (3, 4), (4, 3) and
    (-4, -3) -- each 5 from the origin, the first two mirror images in the line y = x.  Every search key is an integer far below 2^53, hence exact"""
    k = np.arange(P)
    x, y = 1000.0 + k, 2000.0 + (k % 7)
    for (px, py), i in zip(((3.0, 4.0), (4.0, 3.0), (-4.0, -3.0)), idx):
        x[i], y[i] = px, py
    return x, y, np.full(P, 3.0)


def begin_launch(P, nc, name, seed, B=2, cs=6, flags=0):
    """launch_step_begin + launch_extend_state on the tie class `name` of tie_classes(P) (or "random": no designed tie).  Two-point ties: car c of slot b
    stands at (-(c + b), -(c + b)), on the line y = x; three-point ties: every car at the origin.  flags: bit 0 alive given, bit 1 status given,
    bit 2 iters_acc given, bit 3 cmin given"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, nc, 8))
    if name == "random":
        track = tie_track(P, ())
        pick = rng.integers(0, P, (B, nc))
        x[:, :, 0] = track[0][pick] + rng.integers(-3, 4, (B, nc)); x[:, :, 1] = track[1][pick] + rng.integers(-3, 4, (B, nc))
        idx = None
    else:
        idx = tie_classes(P)[name]
        track = tie_track(P, idx)
        for b in range(B):
            for c in range(nc):
                x[b, c, 0] = x[b, c, 1] = 0.0 if len(idx) != 2 else -float(c + b)
    return dict(op=OP_BEGIN, B=B, ncars=nc, cs=cs, P=P, track=track, x=x, U=rng.standard_normal((B, cs)), alive=np.array([1, 0] * B, dtype=np.int32)[:B] if flags & 1 else None,
                status=np.array([-2, 7] * B, dtype=np.int32)[:B] if flags & 2 else None, iters=np.array([5, 7] * B, dtype=np.int32)[:B],
                iters_acc=np.array([100, 1 << 40] * B, dtype=np.uint64)[:B] if flags & 4 else None, cmin=np.array([17, 1 << 63] * B, dtype=np.uint64)[:B] if flags & 8 else None,
                tie=idx, name=name)


def copy_launch(cs, seed, B=2, nc=3):
    """launch_step_begin without start states (x == nullptr): the U copies at cs, every flag given, xext allocated and left alone"""
    rng = np.random.default_rng(seed)
    return dict(op=OP_BEGIN, B=B, ncars=nc, cs=cs, P=0, track=None, x=None, U=rng.standard_normal((B, cs)), alive=np.array([0, 1] * B, dtype=np.int32)[:B],
                status=np.array([-3, 0] * B, dtype=np.int32)[:B], iters=np.array([2, 9] * B, dtype=np.int32)[:B], iters_acc=np.array([0, 12345] * B, dtype=np.uint64)[:B],
                cmin=np.array([0, 99] * B, dtype=np.uint64)[:B], tie=None, name="copy")


def exact_argmin(track, px, py):
    """NumPy's first minimum of the squared distance in exact integer arithmetic -> (index, all indices at the minimum)"""
    tx, ty = track[0].astype(np.int64), track[1].astype(np.int64)
    assert np.array_equal(tx, track[0]) and np.array_equal(ty, track[1]) and px == int(px) and py == int(py), "integer coordinates only"
    d2 = (tx - int(px)) ** 2 + (ty - int(py)) ** 2
    return int(np.argmin(d2)), np.flatnonzero(d2 == d2.min())


def check_begin(L, R):
    B, nc, cs = L["B"], L["ncars"], L["cs"]
    if L["status"] is not None:
        assert np.all(R["status"] == 0), ("status", R["status"])
    else:
        assert R["status"] is None
    assert np.array_equal(R["active"], L["alive"] if L["alive"] is not None else np.ones(B, dtype=np.int32)), ("active", R["active"], L["alive"])
    assert np.all(R["iters"] == 0), ("iters", R["iters"])
    if L["iters_acc"] is not None:
        assert np.array_equal(R["iters_acc"], L["iters_acc"] + L["iters"].astype(np.uint64)), ("iters_acc", R["iters_acc"])
    if L["cmin"] is not None:
        assert np.all(R["cmin"] == ALL_ONES), ("cmin", R["cmin"])
    assert np.array_equal(bits(R["Uin"]), bits(L["U"])) and np.array_equal(bits(R["Ucur"]), bits(L["U"])), "U copies"
    if L["x"] is None:
        assert R["xext"] is None or is_poison(R["xext"]).all(), "xext written without start states"
        return
    assert np.array_equal(bits(R["xext"][:, :, :12]), bits(R["xref"][:, :, :12])), "xext[0..11] differs from launch_extend_state's"
    assert np.array_equal(bits(R["xext"][:, :, :8]), bits(L["x"])), "xext[0..7] is not the state"
    for b in range(B):
        tie = L["ties"][b] if has_slots(L) else L["tie"]                      # per-slot tracks: the first minimum on THIS slot's track
        for c in range(nc):
            first, allmin = exact_argmin(slot_track(L, b), L["x"][b, c, 0], L["x"][b, c, 1])
            if tie is not None:
                assert np.array_equal(allmin, np.sort(tie)), ("the designed tie is not the minimum", L["name"], b, c, allmin, tie)
            got, ext = R["xext"][b, c, 12], R["xref"][b, c, 12]
            assert got == first and ext == first, ("anchor", L["name"], "P", len(slot_track(L, b)[0]), "slot", b, "car", c, "step_begin", got, "extend_state", ext, "first minimum", first, "tied", allmin)


# ================================================================ the case lists ===============================================================
T_FULL, T_SHORT = (1, 2, 3, 4, 5, 8, 9), (1, 5)
BIG_P = 240                                                                  # beyond the LDS limit (max_tlds_points: 190)


def k_edges(nc):
    """K = 1, and K below, at and just above the S = 64 / nc samples of a wave, and three waves with a ragged last one"""
    S = samples_per_wave(nc)
    return sorted({1, S - 1, S, S + 1, 2 * S + 3})


def spb4_K(nc):
    """the smallest ragged K that takes four sample-waves per workgroup: a full workgroup's worth below the threshold would not"""
    return source_constants()["spb4_K"] + samples_per_wave(nc) + 1


def duo_of(body):
    """the MPOPIS_ROLLOUT_DUO that pins a launch without the logger to this body"""
    return DUO_ALWAYS if body == TWO_WAVE else 0


def parity_launches(nc, body):
    """(b): every K edge x every T of the car count in one body (SPB 4: its one K), alternating between the two ways to make the start state, and the
    three-wave case on the track beyond the LDS limit"""
    Ts = T_FULL if nc in (1, 3) else T_SHORT
    Ks = [spb4_K(nc)] if body == SPB4 else k_edges(nc)
    out = [car_launch(nc, 2, K, T, 1000 * nc + 10 * K + T, begin=(i + j) % 2) for i, K in enumerate(Ks) for j, T in enumerate(Ts)]
    out.append(car_launch(nc, 2, Ks[-1], 5, 1000 * nc + 7, track=big_track(BIG_P), begin=1))
    return out


def logger_launches(nc):
    """(c): SPB 1 and SPB 4 x both table placements at T = 9, with traj"""
    S = samples_per_wave(nc)
    return [car_launch(nc, B, K, 9, 3000 + 10 * nc + i, track=tr, traj=True, iters=True)
            for i, (B, K, tr) in enumerate([(2, S + 1, default_track()), (2, S + 1, big_track(BIG_P)), (1, spb4_K(nc), default_track()), (1, spb4_K(nc), big_track(BIG_P))])]


def form_cases():
    """(a): (name, launch, environment of the harness process, the body the case was written for)"""
    c = source_constants()
    pmax = max_tlds_points(c)
    duo = lambda n: {"MPOPIS_ROLLOUT_DUO": str(n)}
    wg = {"MPOPIS_COOP_MAX_WG": "2"}
    one, cars = 2 * c["kDuoCarWaves"], 2 * c["kDuoCarsWaves"]              # the default limits of a two-CU device
    th = c["spb4_K"]
    L = car_launch
    return [
        ("1 car at the limit", L(1, 1, 192, 2, 1), duo(3), TWO_WAVE), ("1 car over the limit", L(1, 1, 193, 2, 2), duo(3), SPB1),
        ("3 cars at the limit", L(3, 2, 84, 2, 3), duo(8), TWO_WAVE), ("3 cars over the limit", L(3, 2, 85, 2, 4), duo(8), SPB1),
        ("share 2 at the limit", L(1, 1, 192, 2, 5, share=2), duo(6), TWO_WAVE), ("share 2 over the limit", L(1, 1, 193, 2, 6, share=2), duo(6), SPB1),
        ("K below the SPB 4 threshold", L(1, 1, th - 1, 1, 7), duo(0), SPB1), ("K at the SPB 4 threshold", L(1, 1, th, 1, 8), duo(0), SPB4),
        ("5 cars below the SPB 4 threshold", L(5, 1, th - 1, 1, 9), duo(0), SPB1), ("5 cars at the SPB 4 threshold", L(5, 1, th, 1, 10), duo(0), SPB4),
        ("two-wave at K >= threshold", L(1, 1, 1024, 1, 11), duo(16), TWO_WAVE), ("one wave more", L(1, 1, 1025, 1, 12), duo(16), SPB4),
        ("traj is never two-wave", L(1, 1, 65, 2, 13, traj=True), duo(DUO_ALWAYS), SPB1), ("traj is never two-wave, large K", L(2, 1, th, 1, 14, traj=True), duo(DUO_ALWAYS), SPB4),
        ("largest track in LDS, two-wave", L(2, 1, 40, 2, 15, track=big_track(pmax)), duo(DUO_ALWAYS), TWO_WAVE),
        ("smallest track beyond, two-wave", L(2, 1, 40, 2, 16, track=big_track(pmax + 1)), duo(DUO_ALWAYS), TWO_WAVE),
        ("largest track in LDS, one-wave", L(2, 1, 40, 2, 15, track=big_track(pmax)), duo(0), SPB1), ("smallest track beyond, one-wave", L(2, 1, 40, 2, 16, track=big_track(pmax + 1)), duo(0), SPB1),
        ("default limit, 1 car at it", L(1, 1, 64 * one, 1, 17), wg, TWO_WAVE), ("default limit, 1 car over it", L(1, 1, 64 * one + 1, 1, 18), wg, SPB4 if 64 * one + 1 >= th else SPB1),
        ("default limit, 2 cars at it", L(2, 1, 32 * cars, 1, 19), wg, TWO_WAVE), ("default limit, 2 cars over it", L(2, 1, 32 * cars + 1, 1, 20), wg, SPB4 if 32 * cars + 1 >= th else SPB1),
    ]


def env_form_args(env):
    """the (duo, max_wg) arguments of expected_form for a harness environment"""
    return (int(env["MPOPIS_ROLLOUT_DUO"]) if "MPOPIS_ROLLOUT_DUO" in env else None, int(env["MPOPIS_COOP_MAX_WG"]) if "MPOPIS_COOP_MAX_WG" in env else None)


def slot_alone(L, b):
    """slot b as a launch of its own; a per-slot launch: with its one-slot SlotEnv (the slot's track as the whole table)"""
    out = dict(L, B=1, active=None)
    for k in ("x0", "U", "Uo", "E", "gvec", "cmin", "status"):
        if L[k] is not None:
            out[k] = L[k][b:b + 1].copy()
    if has_slots(L):
        out.update(params=L["params"][b:b + 1].copy(), tracks=[slot_track(L, b)], tos=[0])
    return out


def permute_slots(L, order):
    """slot i of the result is slot order[i] of L: track_of_slot, parameters, states and inputs move together"""
    order = list(order)
    out = dict(L)
    for k in ("x0", "U", "Uo", "E", "gvec", "cmin", "status", "active", "params", "t0", "done0"):
        if L[k] is not None:
            out[k] = np.ascontiguousarray(np.asarray(L[k])[order])
    out["tos"] = [L["tos"][i] for i in order]
    return out


def permute_cars(L, perm):
    """car i of the result is car perm[i] of the fleet launch L: parameters, start states, bounds, the rows of U, Uo, E (and gvec)"""
    perm = np.asarray(perm)
    nc, T, B = L["ncars"], L["T"], L["B"]
    out = dict(L, params=np.ascontiguousarray(L["params"][:, perm]), x0=np.ascontiguousarray(L["x0"].reshape(B, nc, 8)[:, perm].reshape(B, 8 * nc)),
               lo=np.ascontiguousarray(L["lo"].reshape(nc, 2)[perm].reshape(-1)), hi=np.ascontiguousarray(L["hi"].reshape(nc, 2)[perm].reshape(-1)))
    for k in ("U", "Uo", "gvec"):
        if L[k] is not None:
            out[k] = np.ascontiguousarray(L[k].reshape(B, T, nc, 2)[:, :, perm].reshape(B, -1))
    out["E"] = np.ascontiguousarray(L["E"].reshape(B, T, nc, 2, L["K"])[:, :, perm].reshape(B, 2 * nc * T, L["K"]))
    return out


def invariant_launches(nc, make=None, S=None, nan_cars=None, two_wave=True):
    """(d): -> (launches of the one-wave process by name, names also run in the two-wave process, notes).  make: the launch factory (car_launch; (l): a
    per-slot or fleet one), S: the samples of a wave (the fleet body: 64), nan_cars: the cars that get the NaN of the three nan_* cases (default: the last)"""
    car_launch = make or globals()["car_launch"]
    S = S or samples_per_wave(nc)
    K, Kbig, T, seed = 2 * S + 3, source_constants()["spb4_K"] + S + 1, 5, 7000 + nc
    cs = 2 * nc * T
    rng = np.random.default_rng(seed)
    small = cost_key(np.array([-1e30]))[0]                                   # a smaller key than any cost: it survives
    common = dict(active=np.array([1, 0, 1], dtype=np.int32), cmin=np.array([ALL_ONES, POISON64, small], dtype=np.uint64), status=np.array([0, 7, 0], dtype=np.int32),
                  iters=True, iter_n=4)
    base = car_launch(nc, 3, K, T, seed, **common)
    A = dict(base=base, logged=dict(base, traj=True))
    perm = rng.permutation(K)
    A["perm"] = dict(base, E=np.ascontiguousarray(base["E"][:, :, perm]))
    A["slot0"], A["slot2"] = slot_alone(base, 0), slot_alone(base, 2)
    A["zero_gvec"] = dict(base, gvec=np.zeros((3, cs)))
    g, d = car_launch(nc, 3, K, T, seed + 1, grid=True, **common), 2.0 ** -6
    A["grid"], A["grid_shift"] = g, dict(g, U=g["U"] + d, E=g["E"] - d)
    assert np.array_equal((g["U"] + d)[:, :, None] + (g["E"] - d), g["U"][:, :, None] + g["E"]) and np.array_equal((g["U"] + d) - d, g["U"]) and np.array_equal((g["E"] - d) + d, g["E"])
    big = car_launch(nc, 1, Kbig, T, seed + 2)
    A["big"], A["big_head"] = big, dict(big, K=K, E=np.ascontiguousarray(big["E"][:, :, :K]))
    kn, cn = S + 1, nc - 1                                                   # the NaN: the last car of the second wave's second sample, in slot 2
    nan_names = []
    for car in (nan_cars or [cn]):
        for name, t in (("nan_t0", 0), ("nan_mid", 2), ("nan_last", T - 1)):
            name = name if car == cn else "%s_car%d" % (name, car)
            E = base["E"].copy(); E[2, t * 2 * nc + 2 * car + (t % 2), kn] = np.nan
            A[name] = dict(base, E=E); A[name + "_nocmin"] = dict(base, E=E, cmin=None)
            nan_names.append(name)
    E, Er = base["E"].copy(), base["E"].copy()
    for k, r, v in ((1, 0, np.inf), (2, cs - 1, -np.inf), (K - 1, cs // 2, np.inf)):
        E[0, r, k], Er[0, r, k] = v, np.sign(v) * 1e300
    A["inf"], A["inf_ref"] = dict(base, E=E), dict(base, E=Er)
    Un = base["U"].copy(); Un[0, 2 * cn] = np.nan                            # the last car's first steering command of slot 0: every sample of the slot
    A["all_nan"] = dict(base, U=Un)
    if has_slots(base):                                                      # (l): the slots in another order, the inactive one staying in the middle
        A["slot_perm"] = permute_slots(base, [2, 1, 0])
    return A, (("base", "big", "grid", "grid_shift", "nan_mid", "inf", "all_nan") if two_wave else ()), dict(perm=perm, K=K, kn=kn, small=small, nan_names=nan_names)


def check_invariants(nc, A, RA, RB, two_wave_names, notes):
    """the exact invariants of (d), bit for bit; RA / RB: results by name of the one-wave and the two-wave process"""
    act = (0, 2)
    same = lambda x, y: np.array_equal(bits(x), bits(y))
    for R, names in ((RA, list(A)), (RB, two_wave_names)):
        for n in names:
            check_slots(A[n], R[n])
            check_cmin(A[n], R[n])
    for n in two_wave_names:                                                 # two-wave equals one-wave, K < 1024 and K >= 1024
        assert same(RA[n]["cost"], RB[n]["cost"]), ("two-wave differs from one-wave", n)
        for f in ("cmin", "status", "iters"):
            assert RA[n][f] is None or np.array_equal(RA[n][f], RB[n][f]), ("two-wave differs from one-wave", n, f)
    for R in ((RA, RB) if two_wave_names else (RA,)):
        base = R["base"]["cost"]
        assert R["base"]["cmin"][2] == notes["small"], "a smaller cmin than every cost must survive"
        assert same(R["grid_shift"]["cost"], R["grid"]["cost"]), "(U + d, E - d) differs from (U, E)"
        c = R["nan_mid"]["cost"]
        assert not np.isfinite(c[2, notes["kn"]]) and same(np.delete(c, notes["kn"], axis=1), np.delete(base, notes["kn"], axis=1)), "a NaN reached another sample"
        assert np.array_equal(R["nan_mid"]["status"], [0, 7, ERR_ACTION])
        assert np.all(np.isfinite(R["inf"]["cost"][[0, 2]])) and np.array_equal(R["inf"]["status"], [0, 7, 0]), "+-inf must be clamped, not reported"
        c = R["all_nan"]["cost"]
        assert not np.isfinite(c[0]).any() and same(c[2], base[2]) and np.array_equal(R["all_nan"]["status"], [ERR_ACTION, 7, 0])
        assert int(R["all_nan"]["cmin"][0]) > int(cost_key(np.array([np.inf]))[0]) and R["all_nan"]["cmin"][0] != ALL_ONES, "the key of a NaN orders after every number"
    base = RA["base"]["cost"]
    for b in act:
        assert same(RA["perm"]["cost"][b], base[b][notes["perm"]]), ("permuted columns, slot", b)
        assert same(RA["slot%d" % b]["cost"][0], base[b]), ("slot alone", b)
        assert RA["slot%d" % b]["cmin"][0] == RA["base"]["cmin"][b]
    assert same(RA["zero_gvec"]["cost"], base), "an all-zero gvec changes the costs"
    assert same(RA["big_head"]["cost"][0], RA["big"]["cost"][0, :notes["K"]]), "a sample's cost depends on more than its column"
    assert same(RA["inf"]["cost"], RA["inf_ref"]["cost"]), "+-inf is not clamped like +-1e300"
    if "slot_perm" in A:
        assert same(RA["slot_perm"]["cost"][[0, 2]], RA["base"]["cost"][[2, 0]]), "permuting the slots with their tracks and parameters does not permute the costs"
        for f in ("cmin", "status", "iters"):
            assert np.array_equal(RA["slot_perm"][f][[0, 2]], RA["base"][f][[2, 0]]), ("permuting the slots does not permute", f)
    for n in notes.get("nan_names", ("nan_t0", "nan_mid", "nan_last")):
        c = RA[n]["cost"]
        assert not np.isfinite(c[2, notes["kn"]]), (n, "the NaN sample's cost is finite")
        assert same(np.delete(c, notes["kn"], axis=1), np.delete(base, notes["kn"], axis=1)), (n, "a NaN reached another sample")
        assert np.array_equal(RA[n]["status"], [0, 7, ERR_ACTION]), (n, RA[n]["status"])
        assert np.array_equal(RA[n + "_nocmin"]["status"], [0, 7, 0]) and same(RA[n + "_nocmin"]["cost"], c), (n, "without cmin")


def gamma_launches(nc, make=None, S=None):
    """(e): the same launch with gvec = gamma U_orig' Sigma^-1 and without.  Sigma is the project's own proposal covariance diag(0.0625, 0.1) per step with a
    random coupling of a tenth of it, gamma = lambda (1 - alpha) = 10 x 1; the cars start on the reset grid and no sample is far out (check_gamma says why)"""
    S = S or samples_per_wave(nc)
    T = 5
    cs = 2 * nc * T
    L0 = (make or car_launch)(nc, 1, 2 * S + 3, T, 5000 + nc, far=0)
    rng = np.random.default_rng(5100 + nc)
    M = rng.standard_normal((cs, cs))
    sd = np.sqrt(np.tile([0.0625, 0.1], nc * T))
    Sigma = np.diag(sd * sd) + 0.1 * (M @ M.T / cs) * np.outer(sd, sd)
    L0["Uo"] = rng.uniform(-0.3, 0.3, (1, cs))
    L1 = dict(L0)
    L1["gvec"] = gvec_of(L0, 10.0, np.linalg.inv(Sigma))
    return L1, L0


SIMPLE_K, SIMPLE_T = (1, 63, 64, 65, 130), (1, 15)
SIMPLE_X0 = {ENV_MC: [[-0.5, 0.0], [-0.4, 0.01]], ENV_CP: [[0.0, 0.0, 0.02, 0.0], [0.1, -0.2, -0.05, 0.3]]}


def simple_launches(kind):
    """(f): K x T with t0 / done0 given and null and traj on every other launch; then a slot that starts done, termination inside the rollout (the step
    limit; CartPole also the pole falling), and a NaN action (the launch before it is the same without the NaN)"""
    i32 = lambda *v: np.array(v, dtype=np.int32)
    out = []
    for i, K in enumerate(SIMPLE_K):
        for j, T in enumerate(SIMPLE_T):
            given = (i + j) % 2 == 0
            out.append(simple_launch(kind, 2, K, T, 9000 + 100 * kind + 10 * i + j, SIMPLE_X0[kind], t0=i32(3, 0) if given else None, done0=i32(0, 0) if given else None, traj=(i % 2 == 0)))
    ms = int(out[0]["params"][10 if kind == ENV_CP else 7])
    out.append(simple_launch(kind, 2, 65, 15, 9901, SIMPLE_X0[kind], t0=i32(ms + 3, 0), done0=i32(1, 0), traj=True))
    out.append(simple_launch(kind, 2, 65, 15, 9902, SIMPLE_X0[kind], t0=i32(ms - 5, ms - 1), done0=i32(0, 0), traj=True))
    if kind == ENV_CP:
        out.append(simple_launch(kind, 2, 65, 15, 9903, [[0.0, 0.0, 0.19, 0.6], [2.3, 1.5, 0.0, 0.0]], traj=True))
    base = simple_launch(kind, 2, 65, 15, 9904, SIMPLE_X0[kind])
    E = base["E"].copy(); E[0, 7, 3] = np.nan; E[1, 14, 64] = np.nan
    return out + [base, dict(base, E=E)]


def begin_launches():
    """(g): every tie class of every P for 1, 3 and 8 cars (three-point ties: one car), a launch without designed ties per P, and the U copies"""
    out, flags = [], 0
    for P in BEGIN_P:
        for nc in (1, 3, 8):
            for name, idx in tie_classes(P).items():
                if len(idx) == 3 and nc != 1:
                    continue
                out.append(begin_launch(P, nc, name, 100 * P + nc, flags=flags % 16)); flags += 1
            out.append(begin_launch(P, nc, "random", 100 * P + nc + 50, flags=flags % 16)); flags += 5
    return out + [copy_launch(cs, 40 + cs) for cs in BEGIN_CS]


# ================================================================ per-slot envs and fleets: (h) .. (o) ==========================================
SLOT_TOS = [2, 0, 1]                                                         # (i): not the identity, so an index taken by slot where it should be taken by track fails
FLEET_K = (1, 63, 64, 65, 131)                                               # lane = sample in the fleet body: the wave edge is 64 at every car count
BIG_TRACK_P = 2048                                                           # kMaxTrackPoints: the raised dynamic-LDS limit


def ring_track(P):
    """slot_env_cases.ring at the two sizes the per-slot cases use: a triangle (P = 3: below the five-point tier of the ring search) and a 12-point ellipse"""
    from tests.helpers import slot_env_cases as SE
    if ("ring", P) not in _cache:
        _cache[("ring", P)] = SE.ring(3, 60.0) if P == 3 else SE.ring(P, 80.0, 50.0)
    return _cache[("ring", P)]


def small_tracks():
    """the track table of (i) and (l): 48, 3 and 12 points"""
    return [default_track(), ring_track(3), ring_track(12)]


def _on_the_road(track):
    """the bundled centre line or a resampling of it: start_states' grid stands on it"""
    return track is default_track() or any(track is v for k, v in _cache.items() if isinstance(k, tuple) and k[0] == "big")


def slot_params3(which=(1, 3, 0)):
    """three of the four vectors of slot_env_cases.car_params4 (1: beta_limit > pi / 2; 2: dt / 10 = 0.02, lambda_drive != 0; 3: 0.02, other m, C_af, mu; 0: the defaults)"""
    from tests.helpers import slot_env_cases as SE
    return np.ascontiguousarray(SE.car_params4(_oracle())[list(which)])


def fleet_params(nc, B):
    """slot 0: car_fleet_ref.graded_fleet; slot 1: its cars in reverse order at dt / 5 = 0.02 (nsub differs per slot); slot 2: rotated by one car, 0.02"""
    from tests.helpers import car_fleet_ref as FR
    g = FR.graded_fleet(nc, _oracle().car_default_params())
    out = np.stack([g, g[::-1], np.roll(g, 1, axis=0)][:B] if B <= 3 else [g] * B)
    out[1:, :, 19] = 0.02
    return np.ascontiguousarray(out)


def slot_launch(nc, B, K, T, seed, tracks=None, tos=None, params=None, fleet=False, **kw):
    """car_launch with a per-slot env: slot b drives on tracks[tos[b]] under params[b] ([20], fleet: [nc][20]).  Start states: start_states' row b where
    the slot's track is the bundled road (slot 1 keeps the coincident cars and the car 3 m off), slot_env_cases.start_state on the slot's own track otherwise"""
    from tests.helpers import slot_env_cases as SE
    tracks = [default_track()] if tracks is None else list(tracks)
    tos = [0] * B if tos is None else list(tos)
    assert len(tos) == B and all(0 <= t < len(tracks) for t in tos)
    if params is None:
        params = fleet_params(nc, B) if fleet else slot_params3()[:B]
    params = np.ascontiguousarray(params, dtype=np.float64)
    assert params.shape == ((B, nc, 20) if fleet else (B, 20)), params.shape
    L = car_launch(nc, B, K, T, seed, **kw)
    if "x0" not in kw:
        for b in range(B):
            if not _on_the_road(tracks[tos[b]]):
                L["x0"][b] = SE.start_state(tracks[tos[b]], nc, b)
    L.update(op=OP_ROLLOUT_SLOTS, tracks=tracks, tos=tos, params=params, fleet=fleet, track=None, P=0)
    return L


def twin_launch(nc, B, K, T, seed, **kw):
    """the per-slot twin of car_launch on the three small tracks"""
    kw.setdefault("tracks", small_tracks()); kw.setdefault("tos", SLOT_TOS[:B] if B == 3 else [1, 0][:B])
    return slot_launch(nc, B, K, T, seed, **kw)


def fleet_launch(nc, B, K, T, seed, **kw):
    return slot_launch(nc, B, K, T, seed, fleet=True, **kw)


def shared_as_slots(L, fleet=False):
    """the launch L (op ROLLOUT) as a per-slot launch whose SlotEnv holds B copies of the shared parameters and track: the first cross-body comparison
    (fleet: every car of every slot with the shared vector -- the second)"""
    B, nc = L["B"], L["ncars"]
    prm = np.tile(L["params"], (B, nc, 1)) if fleet else np.tile(L["params"], (B, 1))
    return dict(L, op=OP_ROLLOUT_SLOTS, tracks=[L["track"]], tos=[0] * B, params=np.ascontiguousarray(prm), fleet=fleet, track=None, P=0)


def one_car_of(L, c):
    """car c of the fleet launch L as a one-car shared launch per slot parameters -- B one-slot launches (op ROLLOUT takes one vector), each with that car's
    parameters, bounds, start state and control rows, on the slot's track, with the logger: the third cross-body comparison"""
    nc, T, K = L["ncars"], L["T"], L["K"]
    out = []
    for b in range(L["B"]):
        rows = lambda a: np.ascontiguousarray(a[b].reshape((T, nc, 2) + a[b].shape[1:])[:, c].reshape((1, 2 * T) + a[b].shape[1:]))
        trk = slot_track(L, b)
        out.append(dict(L, op=OP_ROLLOUT, B=1, ncars=1, fleet=False, track=trk, P=len(trk[0]), params=np.ascontiguousarray(L["params"][b, c]), lo=L["lo"][2 * c:2 * c + 2].copy(),
                        hi=L["hi"][2 * c:2 * c + 2].copy(), x0=L["x0"][b:b + 1, 8 * c:8 * c + 8].copy(), U=rows(L["U"]), Uo=rows(L["Uo"]), E=rows(L["E"]), gvec=None, active=None, cmin=None,
                        status=None, traj=True))
    return out


# ---- (h) form
def slot_form_cases():
    """(h): (name, launch, environment of the harness process, the body the case was written for).  Placement goes by the LARGEST track of the launch: a
    3-point slot beside one of pmax points runs with every table in LDS, beside pmax + 1 ring-only; the fleet on both sides of max_tlds_points_fleet(nc);
    and the raised dynamic-LDS limit with a 2048-point track in the launch"""
    c = source_constants()
    pmax, th = max_tlds_points(c), c["spb4_K"]
    duo = lambda n: {"MPOPIS_ROLLOUT_DUO": str(n)}
    out = []
    for body, env, nc, K in ((TWO_WAVE, duo(DUO_ALWAYS), 1, 65), (SPB1, duo(0), 3, 22), (SPB4, duo(0), 2, th + 1)):
        for P in (pmax, pmax + 1):
            out.append(("%s twin, 3 points beside %d" % (BODY_NAME[body], P), twin_launch(nc, 2, K, 2, 100 + P + nc, tracks=[ring_track(3), big_track(P)], tos=[0, 1], begin=P % 2), env, body))
    out.append(("logger twin, 3 points beside %d" % (pmax + 1), twin_launch(1, 2, 65, 2, 120, tracks=[ring_track(3), big_track(pmax + 1)], tos=[0, 1], traj=True), duo(DUO_ALWAYS), SPB1))
    for nc in (2, 8):
        pf = max_tlds_points_fleet(nc, c)
        for P in (pf, pf + 1):
            for traj in (False, True):
                out.append(("fleet of %d, %d points%s" % (nc, P, ", logged" if traj else ""), fleet_launch(nc, 2, 65, 2, 130 + P + nc, tracks=[ring_track(3), big_track(P)], tos=[0, 1], traj=traj),
                            duo(DUO_ALWAYS), FLEET))
    big = big_track(BIG_TRACK_P)
    out.append(("two-wave twin with a 2048-point track", twin_launch(1, 2, 65, 2, 140, tracks=[big, ring_track(12)], tos=[1, 0]), duo(DUO_ALWAYS), TWO_WAVE))
    out.append(("fleet of 8 with a 2048-point track", fleet_launch(8, 2, 65, 2, 141, tracks=[big, ring_track(12)], tos=[1, 0]), duo(0), FLEET))
    return out


# ---- (i) twin parity
def twin_parity_launches(nc, body):
    """(i): parity_launches' K and T edges on three slots with their own tracks (48, 3, 12 points through track_of_slot = [2, 0, 1]) and parameter vectors
    (one with dt / 5), and the three-wave case with the track beyond the LDS limit as one of the three"""
    Ts = T_FULL if nc in (1, 3) else T_SHORT
    Ks = [spb4_K(nc)] if body == SPB4 else k_edges(nc)
    out = [twin_launch(nc, 3, K, T, 2000 * nc + 10 * K + T, begin=(i + j) % 2) for i, K in enumerate(Ks) for j, T in enumerate(Ts)]
    out.append(twin_launch(nc, 3, Ks[-1], 5, 2000 * nc + 7, tracks=[big_track(BIG_P), ring_track(3), ring_track(12)], begin=1))
    return out


# ---- (j) fleet parity
def fleet_parity_launches(nc):
    """(j): two fleets (graded; reversed at dt / 5) x K in FLEET_K x T (1, 2, 3: the buffer-reuse edges of the exchange; 4, 5, 8, 9: the renormalisation
    steps), every other launch with per-slot tracks (slot 0 on the 12-point ellipse), and one ring-only launch.  The test runs each with and without the logger"""
    Ts = T_FULL if nc in (2, 3, 8) else (1, 2, 5)
    out = []
    for i, K in enumerate(FLEET_K):
        for j, T in enumerate(Ts):
            kw = dict(tracks=[default_track(), ring_track(12)], tos=[1, 0]) if (i + j) % 2 else {}
            out.append(fleet_launch(nc, 2, K, T, 3000 * nc + 10 * K + T, begin=(i + j) % 2, **kw))
    out.append(fleet_launch(nc, 2, 65, 5, 3000 * nc + 7, tracks=[big_track(BIG_P), ring_track(12)], tos=[0, 1], begin=1))
    return out


# ---- (k) logger
def slot_logger_launches(nc, fleet):
    """(k): T = 9, K = 65, two slots, with traj, in both table placements.  Twins: 48 and 12 points, then 240 and 12; fleets: both slots on the road (the inputs
    whose logged Vx the issue's premise was measured on), then on its 240-point resampling"""
    make = fleet_launch if fleet else twin_launch
    if fleet:
        tr = [dict(), dict(tracks=[big_track(BIG_P)], tos=[0, 0])]
    else:
        tr = [dict(tracks=[default_track(), ring_track(12)], tos=[1, 0]), dict(tracks=[big_track(BIG_P), ring_track(12)], tos=[1, 0])]
    return [make(nc, 2, 65, 9, 4000 + 10 * nc + i, traj=True, iters=True, **kw) for i, kw in enumerate(tr)]


# ---- (l) invariants
def twin_invariant_launches(nc):
    """(l), twins: invariant_launches on three slots whose INACTIVE middle slot has a valid but different SlotEnv entry (the 3-point track, its own vector)"""
    make = lambda nc, B, K, T, seed, **kw: twin_launch(nc, B, K, T, seed, tos=[2, 1, 0][:B] if B == 3 else [0], params=slot_params3((2, 0, 3))[:B], **kw)
    return invariant_launches(nc, make=make)


def fleet_invariant_launches(nc):
    """(l), fleets: the same on three fleets (64 samples per wave; no two-wave form), the NaN in car 0, a middle car and the last car at t = 0, 2, T - 1, and
    the car permutation: the logged launch with its cars in another order"""
    make = lambda nc, B, K, T, seed, **kw: fleet_launch(nc, B, K, T, seed, tracks=small_tracks(), tos=[2, 1, 0][:B] if B == 3 else [0], **kw)
    A, two, notes = invariant_launches(nc, make=make, S=64, nan_cars=sorted({0, nc // 2, nc - 1}), two_wave=False)
    rng = np.random.default_rng(70 + nc)
    perm = np.roll(np.arange(nc), 1)                                         # a derangement (every car moves to another wave): the first random one, else the rotation
    for _ in range(100):
        cand = rng.permutation(nc)
        if not np.any(cand == np.arange(nc)):
            perm = cand
            break
    A["car_perm"] = permute_cars(A["logged"], perm)
    notes["car_perm"] = perm
    return A, two, notes


def check_car_permutation(oracle, L, R, Lp, Rp, perm):
    """the fleet with its cars permuted: each car's dynamics do not depend on the others, so its logged 8 x T block equals its block of the unpermuted run bit
    for bit; the costs change their summation order and are held to 2 (T nc + 8) u sum |terms| (cost_terms_sum) -> the worst cost ratio"""
    nc, K, T = L["ncars"], L["K"], L["T"]
    ratio = 0.0
    for b in active_slots(L):
        X, Xp = R["traj"][b].reshape(K, nc, 8 * T), Rp["traj"][b].reshape(K, nc, 8 * T)
        for i in range(nc):
            assert np.array_equal(bits(Xp[:, i]), bits(X[:, perm[i]])), ("slot", b, "car", int(perm[i]), "logs another trajectory as car", i, "of the permuted fleet")
        bound = 2 * (T * nc + 8) * U * cost_terms_sum(oracle, L, b)
        ratio = max(ratio, float(np.max(np.abs(R["cost"][b].astype(LD) - Rp["cost"][b].astype(LD)) / bound)))
    assert ratio <= 1.0, ("costs of the permuted fleet", ratio)
    return ratio


# ---- (n) the simple envs per slot
def simple_params3(kind):
    """three parameter vectors per launch (mountaincar: power, gravity; cartpole: gravity, pole mass and length, force) with the derived entries kept consistent"""
    O = _oracle()
    if kind == ENV_CP:
        p = np.stack([O.cartpole_default_params() for _ in range(3)])
        p[1, 0], p[1, 2], p[1, 4], p[1, 6] = 9.0, 0.15, 0.6, 12.0
        p[2, 0], p[2, 2], p[2, 4], p[2, 6] = 10.5, 0.08, 0.45, 8.0
        p[:, 3] = p[:, 1] + p[:, 2]; p[:, 5] = p[:, 2] * p[:, 4]           # totalmass, polemasslength
    else:
        p = np.stack([O.mountaincar_default_params() for _ in range(3)])
        p[1, 5], p[1, 6] = 0.002, 0.003
        p[2, 5], p[2, 6] = 0.001, 0.002
    return p


def simple_slot_launch(kind, K, T, seed, x0, params, t0=None, done0=None, **kw):
    L = simple_launch(kind, 3, K, T, seed, x0, t0=t0, done0=done0, **kw)
    L.update(op=OP_ROLLOUT_SLOTS, params=np.ascontiguousarray(params), tracks=None, tos=None, fleet=False)
    return L


def simple_slot_launches(kind):
    """(n): K x T with t0 / done0 given and null, traj on every other launch; then a slot whose OWN step limit ends the episode inside the rollout while
    its neighbours' do not (same t0), and a NaN action (the launch before it is the same without the NaN)"""
    i32 = lambda *v: np.array(v, dtype=np.int32)
    x0 = SIMPLE_X0[kind] + [[-0.6, 0.02] if kind == ENV_MC else [-0.1, 0.1, 0.03, -0.2]]
    prm = simple_params3(kind)
    out = []
    for i, K in enumerate(SIMPLE_K):
        for j, T in enumerate(SIMPLE_T):
            given = (i + j) % 2 == 0
            out.append(simple_slot_launch(kind, K, T, 9500 + 100 * kind + 10 * i + j, x0, prm, t0=i32(3, 0, 7) if given else None, done0=i32(0, 0, 0) if given else None, traj=(i % 2 == 0)))
    ends = prm.copy(); ends[1, 10 if kind == ENV_CP else 7] = 25                # slot 1's own step limit: reached 5 steps into the rollout
    out.append(simple_slot_launch(kind, 65, 15, 9951, x0, ends, t0=i32(20, 20, 20), done0=i32(0, 0, 0), traj=True))
    base = simple_slot_launch(kind, 65, 15, 9952, x0, prm)
    E = base["E"].copy(); E[0, 7, 3] = np.nan; E[2, 14, 64] = np.nan
    return out + [base, dict(base, E=E)]


# ---- (o) step begin with per-slot tracks
BEGIN_SLOT_P = (1, 2, 5, 64, 65, 257, 2048)


def begin_slots_launch(Ps, nc, seed, flags=0, cs=6):
    """launch_step_begin + launch_extend_state with slot_tk: slot b on its own tie_track of Ps[b] points (the table holds them in another order than the slots),
    every car on a designed exact tie of ITS track whose first minimum differs from the index slot 0's track would give (asserted here)"""
    B = len(Ps)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, nc, 8))
    ties, tracks = [None] * B, [None] * B
    for b in range(B):
        classes = [idx for idx in tie_classes(Ps[b]).values() if len(idx) != 3 or nc == 1]
        if b == 0:                                                           # slot 0: a real tie away from index 0 where its track has one (P = 1, 2 have none)
            classes.sort(key=lambda idx: not (len(idx) > 1 and min(idx) > 0))
        for idx in classes:
            xb = x[b].copy()
            for c in range(nc):
                xb[c, 0] = xb[c, 1] = 0.0 if len(idx) != 2 else -float(c + b)
            trk = tie_track(Ps[b], idx)
            own = [exact_argmin(trk, xb[c, 0], xb[c, 1])[0] for c in range(nc)]
            other = [exact_argmin(tracks[0], xb[c, 0], xb[c, 1])[0] for c in range(nc)] if b else None
            if b == 0 or all(o != w for o, w in zip(own, other)):
                ties[b], tracks[b], x[b] = idx, trk, xb
                break
        assert tracks[b] is not None, ("no tie class of P = %d gives another anchor than slot 0's track" % Ps[b], Ps)
    for b in range(1, B):                                                    # the premise: on slot 0's track every car of the other slots would get another anchor
        for c in range(nc):
            assert exact_argmin(tracks[b], x[b, c, 0], x[b, c, 1])[0] != exact_argmin(tracks[0], x[b, c, 0], x[b, c, 1])[0], (Ps, b, c)
    order = list(np.roll(np.arange(B), 1))                                   # table entry i = the track of slot order[i]
    tos = [order.index(b) for b in range(B)]
    return dict(op=OP_BEGIN_SLOTS, B=B, ncars=nc, cs=cs, P=0, track=None, tracks=[tracks[i] for i in order], tos=tos, ties=ties, x=x, U=rng.standard_normal((B, cs)),
                alive=np.array([1, 0] * B, dtype=np.int32)[:B] if flags & 1 else None, status=np.array([-2, 7] * B, dtype=np.int32)[:B] if flags & 2 else None,
                iters=np.array([5, 7] * B, dtype=np.int32)[:B], iters_acc=np.array([100, 1 << 40] * B, dtype=np.uint64)[:B] if flags & 4 else None,
                cmin=np.array([17, 1 << 63] * B, dtype=np.uint64)[:B] if flags & 8 else None, tie=None, name="slots %s" % (Ps,))


def begin_slots_launches():
    """(o): B = 3, each slot on a different track, every P of BEGIN_SLOT_P in every position, for 1, 3 and 8 cars"""
    out, flags = [], 0
    n = len(BEGIN_SLOT_P)
    for nc in (1, 3, 8):
        for i in range(n):
            Ps = [BEGIN_SLOT_P[i], BEGIN_SLOT_P[(i + 2) % n], BEGIN_SLOT_P[(i + 4) % n]]
            out.append(begin_slots_launch(Ps, nc, 600 + 10 * i + nc, flags=flags % 16)); flags += 3
    return out
