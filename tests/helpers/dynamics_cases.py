"""Inputs, file format, references and checks for the direct tests of the car model's device arithmetic (tools/kbench_dynamics.hip, which runs
mpopis_amd/csrc/car_dynamics.h one lane per case): shared by tests/test_dynamics_cases_cpu.py (which shows on the CPU that the cases are what they
claim, and holds the header's HOST build to the same bounds through tests/shim/host_shim.cpp) and tests/test_gpu_dynamics_harness.py.  Also the
home of the state / parameter generators of tests/test_dynamics_shim.py and of the long-double projection of tests/test_track_projection_cpu.py.
Nothing here touches the engine; references are np.longdouble, exact rationals, NumPy and the oracle.  The check_* functions take the raw output
arrays in the harness's layout, whoever produced them (device = True: the harness; False: the host shim)."""
import struct
from fractions import Fraction
import numpy as np
from tests.helpers.harness_io import GUARD, LD, U, bits, is_poison      # (re-exported: the tests read them under this module's name)

OP_PRIMS, OP_STEP, OP_REWARD = 0, 1, 2
MAGIC_IN, MAGIC_OUT = b"DYNCASE1", b"DYNRES01"
PRIM_IN, PRIM_OUT, STEP_IN, STEP_OUT, REW_IN, REW_OUT = 14, 16, 14, 12, 5, 12
OUT_WIDTH = {OP_PRIMS: PRIM_OUT, OP_STEP: STEP_OUT, OP_REWARD: REW_OUT}
REGIMES = ("driving", "crawling", "stopped", "backwards", "spinning")
REGIME_SEED = {"driving": 1, "crawling": 2, "stopped": 3, "backwards": 4, "spinning": 5}
NSUBS = (1, 2, 3, 5, 7, 10, 13, 20)
TINY_ANGLE = 1.0 / 32.0
# columns of the primitives' input and output (tools/kbench_dynamics.hip)
X, Q, ANG, CV, CLO, CHI, SV, STHR, FA, FB, FC, MUFZ, CA, FXT = range(14)
O_RCP1, O_RCP, O_SQRT, O_RSQ_S, O_RSQ_R, O_SIN, O_COS, O_CSYM, O_CU, O_CVV, O_FMA, O_FYMAX, O_THR, O_K2, O_K3, O_SPARE = range(16)


# ================================================================ moved from tests/test_dynamics_shim.py ======================================
def states(rng, n, regime):
    s = np.zeros((n, 8))
    s[:, 0] = rng.uniform(-50, 50, n); s[:, 1] = rng.uniform(-50, 50, n); s[:, 2] = rng.uniform(-np.pi, np.pi, n)
    s[:, 6] = rng.uniform(-0.45, 0.45, n); s[:, 7] = rng.uniform(-1, 1, n)
    if regime == "driving":
        s[:, 3] = rng.uniform(2.0, 35.0, n); s[:, 4] = rng.uniform(-1.5, 1.5, n); s[:, 5] = rng.uniform(-0.8, 0.8, n)
    elif regime == "crawling":
        s[:, 3] = rng.uniform(1e-3, 1.2, n); s[:, 4] = rng.uniform(-0.3, 0.3, n); s[:, 5] = rng.uniform(-0.3, 0.3, n)
    elif regime == "stopped":
        s[:, 3] = 0.0; s[:, 4] = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(-0.2, 0.2, n)); s[:, 5] = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(-0.2, 0.2, n))
    elif regime == "backwards":
        s[:, 3] = -rng.uniform(1e-3, 6.0, n); s[:, 4] = rng.uniform(-1.0, 1.0, n); s[:, 5] = rng.uniform(-0.6, 0.6, n)
    elif regime == "spinning":
        s[:, 3] = rng.uniform(-3.0, 8.0, n); s[:, 4] = rng.uniform(-8.0, 8.0, n); s[:, 5] = rng.uniform(-3.0, 3.0, n)
    return s


def random_car_params(rng, base):
    """one random CarRacingEnvParams / dt / δt set (the draws of test_model_step_with_random_car_parameters, in its order)"""
    p = base.copy()
    p[0] *= rng.uniform(0.6, 1.6); p[1] *= rng.uniform(0.6, 1.6)                    # m, Izz
    p[2] *= rng.uniform(0.5, 1.5)                                                    # h
    p[3] *= rng.uniform(0.8, 1.25); p[4] *= rng.uniform(0.8, 1.25)                   # lf, lr
    p[5] *= rng.uniform(0.0, 2.0); p[6] *= rng.uniform(0.0, 2.0)                     # CD0, CD1
    p[7] *= rng.uniform(0.5, 1.8); p[8] *= rng.uniform(0.5, 1.8)                     # Caf, Car
    p[9] = rng.uniform(0.4, 1.2); p[10] = rng.uniform(0.4, 1.2)                      # mu_f, mu_r
    p[11] = np.deg2rad(rng.uniform(10.0, 45.0))                                      # delta_max
    p[12] = np.deg2rad(rng.choice([30.0, 90.0, 150.0, 400.0, 900.0]))                # delta_dot_max (the last two: beyond the small-angle range per sub-step)
    p[13] *= rng.uniform(0.5, 1.5); p[14] *= rng.uniform(0.5, 1.5)                   # Fx_max, Fx_min
    p[15] = rng.uniform(0.3, 0.9); p[16] = rng.uniform(0.0, 1.0)                     # lambda_brake, lambda_drive
    p[17] = np.deg2rad(rng.uniform(15.0, 80.0))                                      # beta_limit
    nsub = int(rng.choice([1, 2, 3, 5, 7, 10, 13, 20]))
    p[19] = float(rng.choice([0.005, 0.01, 0.02])); p[18] = nsub * p[19]             # delta_t, dt
    return p


# ================================================================ moved from tests/test_track_projection_cpu.py ===============================
def tracks():
    from mpopis_amd.engine import default_track, BUNDLED_TRACKS
    out = [(n, default_track(name=n)) for n in BUNDLED_TRACKS]
    for P in (3, 5):
        a = np.linspace(0, 2 * np.pi, P, endpoint=False)
        out.append(("ring%d" % P, (30 * np.cos(a), 30 * np.sin(a), np.full(P, 15.0))))
    return [(n, tuple(np.ascontiguousarray(a, dtype=np.float64) for a in t)) for n, t in out]


def exact(track, p):
    """car_racing_tracks.jl:68-92 in long double: nearest point (first minimum), the nearer ring neighbour (ties -> predecessor), distance from the line"""
    X, Y = track[0].astype(LD), track[1].astype(LD)
    P = len(X)
    px, py = LD(p[0]), LD(p[1])
    d2 = (X - px) ** 2 + (Y - py) ** 2
    i = int(np.argmin(d2))
    im, ip = (i - 1) % P, (i + 1) % P

    def line(j):
        vx, vy, ux, uy = X[j] - X[i], Y[j] - Y[i], px - X[i], py - Y[i]
        return abs(ux * vy - uy * vx) / np.sqrt(vx * vx + vy * vy)
    rest = np.delete(d2, i)
    return dict(i=i, prev=bool(d2[im] <= d2[ip]), dm2=d2[im], dp2=d2[ip], d_prev=line(im), d_next=line(ip), u=np.sqrt(d2[i]),
                clear=bool(rest.min() > d2[i] * (1 + LD(1e-9)) + LD(1e-9)))          # the nearest point is not in doubt


def normal(track, i, j):
    vx, vy = track[0][j] - track[0][i], track[1][j] - track[1][i]
    n = np.hypot(vx, vy)
    return np.array([vx / n, vy / n]), np.array([-vy / n, vx / n])


def positions(track, rng):
    """(kind, position) pairs for every track point"""
    tx, ty, tw = track
    P = len(tx)
    out = []
    for i in range(P):
        q = np.array([tx[i], ty[i]])
        im, ip = (i - 1) % P, (i + 1) % P
        out.append(("point", q.copy()))
        for j in (im, ip):
            t, n = normal(track, i, j)
            seg = np.hypot(tx[j] - tx[i], ty[j] - ty[i])
            out.append(("segment", q + t * seg * rng.uniform(0.02, 0.45)))
            out.append(("near", q + t * seg * rng.uniform(0.02, 0.4) + n * rng.normal(0.0, 3.0)))
            for side in (-1.0, 1.0):                              # the lane edge, 1e-9 m inside and outside: moved onto it along the segment's normal below
                for eps in (-1e-9, 1e-9):
                    out.append(("edge", q + t * seg * rng.uniform(0.02, 0.3) + n * side * (tw[i] + eps)))
        # the switch: the point of the perpendicular bisector of (predecessor, successor) closest to q, then one ulp either way along the chord
        a, b = np.array([tx[im], ty[im]]), np.array([tx[ip], ty[ip]])
        mid, ch = 0.5 * (a + b), (b - a) / np.hypot(*(b - a))
        perp = np.array([-ch[1], ch[0]])
        for s in (np.dot(q - mid, perp), np.dot(q - mid, perp) + 2.0, np.dot(q - mid, perp) - 2.0):
            p = mid + s * perp
            k = int(np.argmax(np.abs(ch)))
            for step in (0, 1, -1):
                pp = p.copy()
                if step:
                    pp[k] = np.nextafter(pp[k], pp[k] + step * np.sign(ch[k]))
                out.append(("switch", pp))
    return out


# ================================================================ the harness's files =========================================================
def _f64(x, shape):
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.shape == shape, (x.shape, shape)
    return x.tobytes()


def pack_prims(inp, lo, hi):
    n = inp.shape[0]
    return b"".join([MAGIC_IN, struct.pack("<7q", OP_PRIMS, n, 0, 0, 0, 0, 0), struct.pack("<2d", lo, hi), _f64(inp, (n, PRIM_IN))])


def pack_steps(groups):
    """groups: dicts psi, renorm, p20, bnd (lo0, hi0, lo1, hi1), inp [n][14]"""
    out = [MAGIC_IN, struct.pack("<7q", OP_STEP, 0, len(groups), 0, 0, 0, 0)]
    for g in groups:
        n = g["inp"].shape[0]
        out += [struct.pack("<4q", int(g["psi"]), int(g["renorm"]), n, 0), _f64(g["p20"], (20,)), _f64(g["bnd"], (4,)), _f64(g["inp"], (n, STEP_IN))]
    return b"".join(out)


def pack_reward(p20, track, inp):
    n, P = inp.shape[0], len(track[0])
    return b"".join([MAGIC_IN, struct.pack("<7q", OP_REWARD, n, 0, P, 0, 0, 0), _f64(p20, (20,))] + [_f64(t, (P,)) for t in track] + [_f64(inp, (n, REW_IN))])


def unpack_case(buf):
    """inverse of the three pack functions (what the harness parses)"""
    assert buf[:8] == MAGIC_IN
    op, n, G, P = struct.unpack_from("<4q", buf, 8)
    off = 64

    def take(dt, cnt):
        nonlocal off
        a = np.frombuffer(buf, dtype=dt, count=cnt, offset=off).copy()
        off += a.nbytes
        return a
    c = dict(op=op, n=n, G=G, P=P)
    if op == OP_PRIMS:
        c["lo"], c["hi"] = take(np.float64, 2)
        c["inp"] = take(np.float64, n * PRIM_IN).reshape(n, PRIM_IN)
    elif op == OP_STEP:
        c["groups"] = []
        for _ in range(G):
            gh = take(np.int64, 4)
            c["groups"].append(dict(psi=bool(gh[0]), renorm=bool(gh[1]), p20=take(np.float64, 20), bnd=take(np.float64, 4), inp=take(np.float64, gh[2] * STEP_IN).reshape(gh[2], STEP_IN)))
    else:
        c["p20"] = take(np.float64, 20)
        c["track"] = tuple(take(np.float64, P) for _ in range(3))
        c["inp"] = take(np.float64, n * REW_IN).reshape(n, REW_IN)
    assert off == len(buf)
    return c


def pack_result(op, outs):
    """what the harness writes (used by the CPU round trip and to put the host shim's outputs through the same unpacking): outs = one [n][width] array per launch"""
    body = [np.concatenate([np.ascontiguousarray(o, np.float64).reshape(-1), np.frombuffer(b"\xa5" * (8 * GUARD), dtype=np.float64)]).tobytes() for o in outs]
    return b"".join([MAGIC_OUT, struct.pack("<3q", op, GUARD, len(outs))] + body)


def unpack_result(buf, op, ns):
    """-> one [n][width] array per launch; asserts the header and that every guard entry is still poison (nothing was written past the end)"""
    assert buf[:8] == MAGIC_OUT, buf[:8]
    rop, guard, launches = struct.unpack_from("<3q", buf, 8)
    assert (rop, guard, launches) == (op, GUARD, len(ns)), (rop, guard, launches)
    off, w, outs = 32, OUT_WIDTH[op], []
    for n in ns:
        a = np.frombuffer(buf, dtype=np.float64, count=n * w + GUARD, offset=off).copy()
        off += a.nbytes
        assert np.all(is_poison(a[n * w:])), "guard entries overwritten"
        outs.append(a[:n * w].reshape(n, w))
    assert off == len(buf)
    return outs


# ================================================================ exact arithmetic =============================================================
def fma_exact(a, b, c):
    """the correctly rounded a b + c of finite doubles (exact rationals; the conversion back rounds once, to nearest even)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def ulps(got, ref):
    """|got - ref| in units of the last place of the (long double, finite, nonzero) reference as a double"""
    ref = np.asarray(ref, dtype=LD)
    _, e = np.frexp(ref)
    return np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref) / np.ldexp(LD(1.0), e - 53)


def clampd_ref(v, lo, hi):
    """clampd of car_dynamics.h: v > hi ? hi : (v < lo ? lo : v) -- a NaN fails both comparisons and comes back"""
    return np.where(v > hi, hi, np.where(v < lo, lo, v))


# ================================================================ 1. primitives ================================================================
def _edges(kmin, kmax):
    """powers of two with their two neighbours; the lower neighbour is the mantissa of all ones"""
    p = 2.0 ** np.arange(kmin, kmax + 1, dtype=np.float64)
    return np.concatenate([p, np.nextafter(p, 0.0), np.nextafter(p, np.inf)])


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _fill(head, n, tail):
    head = np.asarray(head, dtype=np.float64)
    assert head.size <= n, (head.size, n)
    return np.concatenate([head, tail(n - head.size)])


def prim_inputs(n=65536 + 37, lo=-1.0, hi=1.0, seed=11):
    """[n][14] inputs of the primitives: the edges first, then log-uniform draws over the model's own ranges (see the checks for what each column feeds)"""
    assert n % 64 != 0 and n >= 1500
    rng = np.random.default_rng(seed)
    inp = np.zeros((n, PRIM_IN))
    e = _edges(-40, 11)                                                                # Vx xq: 1e-12 .. 2e3
    inp[:, X] = _fill(np.concatenate([e, -e, [np.nan, 1e-12, 2e3]]), n, lambda m: _logu(rng, 1e-12, 2e3, m) * np.where(rng.random(m) < 0.25, -1.0, 1.0))
    e = _edges(-40, 34)                                                                # fy_max^2: 1e-8 .. 1e10; Vx^2 + Vy^2: 0 .. 1e4
    inp[:, Q] = _fill(np.concatenate([[0.0, 0.0, np.nan, 1e-8, 1e10, 1e4], e]), n, lambda m: np.where(rng.random(m) < 0.5, _logu(rng, 1e-8, 1e10, m), _logu(rng, 1e-12, 1e4, m)))
    e = _edges(-60, -5); e = e[e <= TINY_ANGLE]
    inp[:, ANG] = _fill(np.concatenate([[0.0, TINY_ANGLE, -TINY_ANGLE, np.nan], e, -e]), n,
                        lambda m: np.where(rng.random(m) < 0.5, rng.uniform(-TINY_ANGLE, TINY_ANGLE, m), _logu(rng, 1e-12, TINY_ANGLE, m) * rng.choice([-1.0, 1.0], m)))
    # clamps: per-lane bounds clo <= chi (every 7th lane clo == chi), the value by category
    a, b = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    clo, chi = np.minimum(a, b), np.maximum(a, b)
    chi[::7] = clo[::7]
    cat = np.arange(n) % 12
    w = rng.random(n)
    cv = np.select([cat == 0, cat == 1, cat == 2, cat == 3, cat == 4, cat == 5, cat == 6, cat == 7, cat == 8, cat == 9, cat == 10],
                   [clo + w * (chi - clo), clo - _logu(rng, 1e-16, 1e3, n), chi + _logu(rng, 1e-16, 1e3, n), clo, chi, np.inf, -np.inf, np.nan,
                    np.full(n, lo), np.full(n, hi), lo + w * (hi - lo)], rng.standard_normal(n) * 2.0)
    inp[:, CV], inp[:, CLO], inp[:, CHI] = cv, clo, chi
    thr = np.abs(rng.standard_normal(n)) * 2.0
    thr[::11] = 0.0; thr[5::97] = np.inf
    sv = rng.standard_normal(n) * 3.0
    sv[1::6] = thr[1::6]; sv[2::6] = -thr[2::6]; sv[3::60] = np.inf; sv[4::60] = -np.inf
    sv[7::6] = np.nextafter(thr[7::6], np.inf); sv[8::6] = -np.nextafter(thr[8::6], np.inf)
    inp[:, SV], inp[:, STHR] = sv, thr
    # fma: random scales; every 4th lane c = -round(a b), so that the result is the product's rounding error (what only a fused operation returns)
    fa = rng.standard_normal(n) * 2.0 ** rng.integers(-30, 31, n); fb = rng.standard_normal(n) * 2.0 ** rng.integers(-30, 31, n)
    fc = rng.standard_normal(n) * 2.0 ** rng.integers(-30, 31, n)
    fc[::4] = -(fa[::4] * fb[::4]); fc[1::16] = 0.0
    fc[2::16] = -(fa[2::16] * fb[2::16]) * (1.0 + 2.0 ** -30)
    inp[:, FA], inp[:, FB], inp[:, FC] = fa, fb, fc
    # tyre constants: mu f_z and C over the ranges random parameters reach; fxt as a fraction of mu f_z incl. exactly +-1 (the 1e-8 floor) and beyond
    mufz = _logu(rng, 1e2, 3e4, n)
    frac = rng.uniform(-0.98, 0.98, n)
    frac[::16] = 1.0; frac[1::16] = -1.0; frac[2::64] = 1.25; frac[3::64] = 1.0 - 1e-9; frac[4::64] = 0.0
    inp[:, MUFZ], inp[:, CA], inp[:, FXT] = mufz, _logu(rng, 2e4, 3e5, n), frac * mufz
    inp[5::64, FXT] = np.sqrt(np.maximum(mufz[5::64] ** 2 - rng.uniform(1e-8, 1e-3, mufz[5::64].size), 0.0))     # fy_max^2 at the floor and just above
    return inp


# relative bounds of the four tyre constants in units of u = 2^-53, from the operation count of tire_fymax / tire_from_fymax with the documented classes
# of their inputs (every IEEE operation and every rounded constant: 1 u; fy_max = fast_sqrt: 1 ulp <= 2 u; rf within 1 ulp of 1 / fy_max: 2 u, plus the
# 2 u of fy_max itself against the exact root = 4 u against 1 / sqrt):
#   fymax                               : 2
#   thr = (3 fymax) (1 / C)             : 2 (fymax) + 1 (3 x) + 1 (1 / C) + 1 (x)                          = 5
#   k2  = ((C C) (1/3)) rf              : 1 (C C) + 1 (the constant 1/3) + 1 (x) + 4 (rf) + 1 (x)          = 8
#   k3  = ((C C C) (1/27)) (rf rf)      : 2 (C C C) + 1 (1/27) + 1 (x) + (4 + 4 + 1) (rf rf) + 1 (x)       = 14
# plus 1 % for the second-order terms and the reference's own 2^-64 arithmetic.  The reference takes fy_max^2 = max(mufz^2 - fl(fxt^2), 1e-8) with the
# fma EXACT (the cancellation of that difference belongs to the formula, which the literal model shares, not to the operations under test).
TIRE_BOUND_U = {"fymax": 2, "thr": 5, "k2": 8, "k3": 14}


def check_prims(inp, out, lo, hi, device, log=print):
    """-> dict of the measured worst figures; asserts every bound of the primitives"""
    assert np.finfo(LD).eps <= 2.0 ** -63, "needs an extended-precision long double for the reference"
    n = inp.shape[0]
    assert out.shape == (n, PRIM_OUT) and np.all(is_poison(out[:, O_SPARE]))              # the column nobody writes is still poison
    fig = {}
    # ---- reciprocals
    x = inp[:, X]; ok = ~np.isnan(x)
    assert np.all(np.isnan(out[~ok, O_RCP1])) and np.all(np.isnan(out[~ok, O_RCP])) and (~ok).any()
    ref = LD(1.0) / x[ok].astype(LD)
    fig["fast_rcp1"] = float(ulps(out[ok, O_RCP1], ref).max()); fig["fast_rcp"] = float(ulps(out[ok, O_RCP], ref).max())
    assert fig["fast_rcp1"] <= 19.0, fig
    assert fig["fast_rcp"] <= 1.0, fig
    # ---- square roots
    q = inp[:, Q]; nan = np.isnan(q); zero = q == 0.0; ok = ~nan & ~zero
    assert nan.any() and zero.any()
    assert np.all(np.isnan(out[nan, O_SQRT])) and np.all(np.isnan(out[nan, O_RSQ_S])) and np.all(np.isnan(out[nan, O_RSQ_R]))
    assert np.all(out[zero, O_SQRT] == (1e-150 if device else 0.0)), out[zero, O_SQRT]   # the 1e-300 bias of the device form: an exact 0 stays finite
    fig["fast_sqrt"] = float(ulps(out[ok, O_SQRT], np.sqrt(q[ok].astype(LD))).max())
    assert fig["fast_sqrt"] <= 1.0, fig
    assert np.array_equal(bits(out[~nan, O_RSQ_S]), bits(out[~nan, O_SQRT]))             # fast_sqrt_rsq: the root has the bits of fast_sqrt
    rs_ok = ok | (zero & device)
    fig["fast_sqrt_rsq 1/s"] = float(ulps(out[rs_ok, O_RSQ_R], LD(1.0) / out[rs_ok, O_RSQ_S].astype(LD)).max())
    assert fig["fast_sqrt_rsq 1/s"] <= 1.0, fig                                           # the class of fast_rcp(s); the value is printed, not asserted
    # ---- sin / cos of a small angle
    v = inp[:, ANG]; ok = ~np.isnan(v); nz = ok & (v != 0.0)
    assert np.all(np.abs(v[ok]) <= TINY_ANGLE) and (~ok).any() and np.all(np.isnan(out[~ok, O_SIN])) and np.all(np.isnan(out[~ok, O_COS]))
    assert np.all(out[ok & ~nz, O_SIN] == 0.0) and (ok & ~nz).any()
    fig["sincos_tiny sin"] = float(ulps(out[nz, O_SIN], np.sin(v[nz].astype(LD))).max())
    fig["sincos_tiny cos"] = float(ulps(out[ok, O_COS], np.cos(v[ok].astype(LD))).max())
    assert fig["sincos_tiny sin"] <= 1.0 and fig["sincos_tiny cos"] <= 1.0, fig
    # ---- clamps (equal as numbers: the sign of a zero is not asserted)
    cv, clo, chi = inp[:, CV], inp[:, CLO], inp[:, CHI]
    nan = np.isnan(cv)
    for col, l, h in ((O_CU, np.full(n, lo), np.full(n, hi)), (O_CVV, clo, chi)):
        want = clampd_ref(cv, l, h)
        assert np.all(np.isnan(out[nan, col])) and nan.any(), "a NaN was clamped away"
        assert np.array_equal(out[~nan, col], want[~nan]), np.flatnonzero(out[:, col] != want)[:5]
        f = ~nan
        seen = [np.any(f & (cv > l) & (cv < h)) or not np.any(l < h), np.any(f & (cv < l)), np.any(f & (cv > h)), np.any(f & (cv == l)), np.any(f & (cv == h)), np.any(np.isposinf(cv)), np.any(np.isneginf(cv))]
        assert all(seen), seen
    assert np.any(clo == chi)
    sv, thr = inp[:, SV], inp[:, STHR]
    assert not np.isnan(sv).any() and np.all(thr >= 0.0)
    assert np.array_equal(out[:, O_CSYM], np.maximum(np.minimum(sv, thr), -thr))
    # ---- fma: the bits of the correctly rounded result, unless that is a zero
    want = np.array([fma_exact(a, b, c) for a, b, c in inp[:, [FA, FB, FC]]])
    assert np.all(np.isfinite(want))
    assert np.array_equal(out[:, O_FMA], want) and np.array_equal(bits(out[want != 0.0, O_FMA]), bits(want[want != 0.0]))
    assert np.sum((inp[:, FC] == -(inp[:, FA] * inp[:, FB])) & (want != 0.0)) > n // 8       # the lanes only a fused operation gets right
    # ---- tyre constants
    mufz, Ca, fxt = inp[:, MUFZ], inp[:, CA], inp[:, FXT]
    arg = np.array([fma_exact(m, m, -t) for m, t in zip(mufz, fxt * fxt)])
    floor = arg <= 1e-8
    assert floor.sum() > n // 16 and np.any(fxt == mufz) and np.any(fxt == -mufz) and np.any((arg > 1e-8) & (arg < 1.0))
    fy = np.sqrt(np.maximum(arg, 1e-8).astype(LD)); C = Ca.astype(LD)
    refs = {"fymax": (O_FYMAX, fy), "thr": (O_THR, 3 * fy / C), "k2": (O_K2, C * C / (3 * fy)), "k3": (O_K3, C * C * C / (27 * fy * fy))}
    for name, (col, r) in refs.items():
        rel = np.abs(out[:, col].astype(LD) - r) / r
        fig["tire_consts " + name] = float(rel.max() / U)
        assert fig["tire_consts " + name] <= TIRE_BOUND_U[name] * 1.01, (name, fig)
    for k, val in fig.items():
        log("[dynamics %s] %-20s worst %.4f %s" % ("device" if device else "host", k, val, "u relative" if k.startswith("tire") else "ulp"))
    return fig


# ================================================================ 2. one model step ============================================================
EPS = (0.0, 2.0 ** -52, -2.0 ** -52, 2.0 ** -50, -2.0 ** -50)          # the drift a rollout's (sin, cos) pairs carry between renormalisations
VARIANTS = [(psi, renorm) for psi in (True, False) for renorm in (True, False)]
ACTION_BOUNDS = np.array([-1.0, 1.0, -1.0, 1.0])
_cache = {}


def default_step_cases(oracle):
    """the five regimes of tests/test_dynamics_shim.py::test_model_step_matches_the_literal_reference_step (its generator, seeds and action mix), 1500 cases
    each, sorted by regime, with the oracle's step of every case -> S [7500][8], A [7500][2], regime index [7500], ref [7500][8]"""
    if "default" not in _cache:
        p = oracle.car_default_params()
        Ss, As, Rs = [], [], []
        for r, regime in enumerate(REGIMES):
            rng = np.random.default_rng(REGIME_SEED[regime])
            n = 1500
            S = states(rng, n, regime)
            A = rng.uniform(-1, 1, (n, 2))
            A[rng.random(n) < 0.15, 1] = -1.0
            A[rng.random(n) < 0.10, 1] = 1.0
            A[rng.random(n) < 0.10, 0] = rng.choice([-1.0, 1.0])
            A[rng.random(n) < 0.05] = 0.0
            Ss.append(S); As.append(A); Rs.append(np.full(n, r))
        S, A, R = np.concatenate(Ss), np.concatenate(As), np.concatenate(Rs)
        ref = np.stack([oracle.car_step(p, S[i], A[i]) for i in range(len(S))])
        for a in (S, A, R, ref):
            a.setflags(write=False)
        _cache["default"] = (p, S, A, R, ref)
    return _cache["default"]


def step_inp(S, A, eps=None):
    """[n][14]: the state, sin / cos of psi and delta scaled by 1 + eps (lane i: EPS[i % 5] unless given), the two raw actions"""
    n = len(S)
    e = np.array(EPS)[np.arange(n) % len(EPS)] if eps is None else np.broadcast_to(eps, (n,))
    f = 1.0 + e
    return np.column_stack([S, np.sin(S[:, 2]) * f, np.cos(S[:, 2]) * f, np.sin(S[:, 6]) * f, np.cos(S[:, 6]) * f, A])


def interleave_order(R):
    """round robin over the regimes (R sorted, equal counts): lane k holds case (k % 5) * 1500 + k // 5 -- every wave mixes hot and general lanes"""
    n, m = len(R), len(REGIMES)
    k = np.arange(n)
    return (k % m) * (n // m) + k // m


def random_param_groups(oracle, seed=78, ngroups=40, per_regime=6):
    """about 40 random parameter sets of 30 lanes (6 per regime), every sub-step count of NSUBS five times, steering rates of both classes (even groups
    30 / 90 deg/s: small-angle increments; odd groups 400 / 900 deg/s: beyond 1/32 rad per sub-step where the target is far enough) -> [(p20, S, A, R, ref)]"""
    key = ("random", seed, ngroups, per_regime)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        base = oracle.car_default_params()
        out = []
        for g in range(ngroups):
            p = random_car_params(rng, base)
            p[12] = np.deg2rad(rng.choice([400.0, 900.0]) if g % 2 else rng.choice([30.0, 90.0]))
            p[18] = NSUBS[g % len(NSUBS)] * p[19]
            Ss, As, Rs = [], [], []
            for r, regime in enumerate(REGIMES):
                S = states(rng, per_regime, regime)
                S[:, 6] = rng.uniform(-0.9, 0.9, per_regime) * p[11]
                Ss.append(S); As.append(rng.uniform(-1, 1, (per_regime, 2))); Rs.append(np.full(per_regime, r))
            S, A, R = np.concatenate(Ss), np.concatenate(As), np.concatenate(Rs)
            out.append((p, S, A, R, np.stack([oracle.car_step(p, S[i], A[i]) for i in range(len(S))])))
        _cache[key] = out
    return _cache[key]


def steer_increment(p, S, A):
    """the steering increment of one sub-step (car_racing.jl:295-296, :301): beyond 1/32 rad the model takes the library sin / cos"""
    tgt = A[:, 0] * p[11] - S[:, 6]
    return np.sign(tgt) * np.minimum(np.abs(tgt) / p[18], p[12]) * p[19]


def oracle_vx_trace(oracle, p, s, a):
    """the oracle's Vx before every sub-step of one action: the step rerun with dt cut to k sub-steps, the steering command scaled so that the steering rate
    min(|target| / dt, rate limit) is the full step's"""
    nsub = int(round(p[18] / p[19]))
    tgt = a[0] * p[11] - s[6]
    out = [s[3]]
    for k in range(1, nsub):
        q = p.copy(); q[18] = k * p[19]
        out.append(oracle.car_step(q, s, [(s[6] + tgt * k / nsub) / p[11], a[1]])[3])
    return np.array(out)


def check_step(oracle, p, inp, out, ref, R, psi, renorm, tol, what, log=print):
    """one group's output against the oracle's step -> (worst deviation per regime, indices set aside)"""
    n = inp.shape[0]
    assert out.shape == (n, STEP_OUT) and ref.shape == (n, 8) and not np.isnan(out).any()
    got = out[:, :8]
    d = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    d[:, 2] = np.minimum(d[:, 2], np.abs(np.abs(got[:, 2] - ref[:, 2]) - 2 * np.pi))      # the heading's wrap to (-pi, pi] may land on either side at exactly +-pi
    cols = list(range(8)) if psi else [0, 1, 3, 4, 5, 6, 7]
    if not psi:
        assert np.array_equal(bits(out[:, 2]), bits(inp[:, 2])), "PSI = false must leave psi alone"
    dev = d[:, cols].max(axis=1)
    aside = dev > 1e-9                                                                     # sign(Vx) decided within rounding of zero (tests/test_dynamics_shim.py)
    worst = {}
    for r, regime in enumerate(REGIMES):
        m = R == r
        if not m.any():
            continue
        cap = int(m.sum()) // 100 if regime in ("crawling", "stopped") else 0
        assert int((m & aside).sum()) <= cap, (what, regime, "set aside", int((m & aside).sum()), "cap", cap, "worst", float(dev[m].max()))
        worst[regime] = float(dev[m & ~aside].max())
        assert worst[regime] < tol, (what, regime, worst[regime], int(np.argmax(np.where(m & ~aside, dev, 0.0))))
    for i in np.flatnonzero(aside):                                                        # each one: the oracle's own Vx passes within rounding of zero in a sub-step
        vx = oracle_vx_trace(oracle, p, inp[i, :8], inp[i, 12:14])
        assert np.abs(vx).min() < 1e-10, (what, int(i), vx)
    k = ~aside
    pair = np.max(np.abs(np.column_stack([out[k, 8] - np.sin(ref[k, 2]), out[k, 9] - np.cos(ref[k, 2]), out[k, 10] - np.sin(ref[k, 6]), out[k, 11] - np.cos(ref[k, 6])])))
    assert pair <= 1e-11, (what, pair)
    log("[dynamics step] %s PSI=%d renorm=%d: worst relative state deviation %s, (sin, cos) pairs %.2e, %d set aside" %
        (what, psi, renorm, " ".join("%s %.2e" % kv for kv in worst.items()), pair, int(aside.sum())))
    return worst, np.flatnonzero(aside)


def nan_action_cases(oracle):
    """NaN steering / NaN pedal on a hot lane (driving) and on general lanes (rolling backwards, stopped), and two clean lanes -> S, A, which lanes must be poisoned"""
    hot = [0.0, 0.0, 0.5, 10.0, 0.1, 0.05, 0.02, 0.3]
    back = [1.0, -2.0, -0.7, -2.0, 0.3, 0.1, -0.05, -0.2]
    stop = [3.0, 4.0, 2.0, 0.0, 0.0, 0.0, 0.1, 0.0]
    nan = float("nan")
    rows = [(hot, (nan, 0.2)), (hot, (0.1, nan)), (back, (nan, 0.2)), (back, (0.1, nan)), (stop, (nan, -0.5)), (stop, (0.3, nan)), (hot, (0.1, 0.2)), (back, (0.1, 0.2))]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([True] * 6 + [False] * 2)


# ================================================================ 3. reward and nearest-point paths ===========================================
def ring_tables(track):
    """n2 and the two certificates as build_track_tables / ring_cert_radius2 derive them"""
    tx, ty, _ = track
    P = len(tx)
    j = np.arange(P)
    c3, c5 = np.full(P, np.inf), np.full(P, np.inf)
    for i in range(P):
        step = np.minimum(np.abs(j - i), P - np.abs(j - i))
        d2 = (tx - tx[i]) * (tx - tx[i]) + (ty - ty[i]) * (ty - ty[i])
        if (step > 1).any():
            c3[i] = d2[step > 1].min() * (1.0 - 1e-9)
        if (step > 2).any():
            c5[i] = d2[step > 2].min() * (1.0 - 1e-9)
    return tx * tx + ty * ty, c3, c5


def ring_masks_np(track, tables, a, px, py):
    """The conditions of the Track comment for one lane, restated: anchor present, 4 |p - q_a|^2 < certificate, three pairwise different keys (five keys
    with a single smallest one).  -> (mask3, rel3, mask5, rel5, margin3, margin5); margin: 4 |p - q_a|^2 is at least 1e-6 relative away from the certificate.
    Keys are the kernels' own two fused multiply-adds, evaluated exactly and rounded once each."""
    tx, ty, _ = track
    n2, c3, c5 = tables
    P = len(tx)
    if a < 0:
        return False, 0, False, 0, True, True
    m2x, m2y = -2.0 * px, -2.0 * py
    key = lambda i: fma_exact(ty[i % P], m2y, fma_exact(tx[i % P], m2x, n2[i % P]))
    d = {s: key(a + s) for s in (-2, -1, 0, 1, 2)}
    D4 = 4.0 * (d[0] + fma_exact(px, px, py * py))
    near = lambda c: np.isinf(c) or abs(D4 - c) >= 1e-6 * c
    mask3 = bool(D4 < c3[a]) and d[0] != d[-1] and d[0] != d[1] and d[-1] != d[1]
    rel3 = -1 if (d[-1] < d[0] and d[-1] < d[1]) else (1 if (d[1] < d[0] and d[1] < d[-1]) else 0)
    best = min(d.values())
    mask5 = P >= 5 and bool(D4 < c5[a]) and sum(v == best for v in d.values()) == 1
    rel5 = 0
    for s in (-1, 1, -2, 2):                                           # the order ring5_candidates replaces its best in (strict <)
        if d[s] < d[rel5]:
            rel5 = s
    return mask3, rel3, mask5, rel5, near(c3[a]), near(c5[a])


def projection_cases(track, rng):
    """the positions of positions() as tests/test_track_projection_cpu.py uses them: edge samples slid onto lane_w -+ 1e-9 m of the exact distance, and only
    those whose nearest point is not in doubt -> [dict(kind, p, ex)]"""
    tx, ty, tw = track
    P = len(tx)
    out = []
    for kind, p in positions(track, rng):
        ex = exact(track, p)
        if kind == "edge":
            j = (ex["i"] - 1) % P if ex["prev"] else (ex["i"] + 1) % P
            _, n = normal(track, ex["i"], j)
            d = float(ex["d_prev"] if ex["prev"] else ex["d_next"])
            eps = 1e-9 if d > tw[ex["i"]] else -1e-9
            sgn = np.sign(np.dot(p - np.array([tx[ex["i"]], ty[ex["i"]]]), n))
            p = p + n * sgn * ((tw[ex["i"]] + eps) - d)
            ex2 = exact(track, p)
            if ex2["i"] != ex["i"] or ex2["prev"] != ex["prev"]:
                continue
            ex = ex2
        if ex["clear"]:
            out.append(dict(kind=kind, p=p, ex=ex))
    return out


ARRANGEMENTS = ("a", "b", "c")


def reward_lanes(name, track):
    """The lanes of one track under the three anchor arrangements.  Every wave of 64 is one SPECIAL lane (lane 0) + up to 63 regular lanes.
    Regular lanes: one per position, anchored at the nearest point or a ring neighbour (cycling; an anchor is taken only where the restated three-point
    test -- and, from five points on, the five-point test -- holds for it with margin); positions with no such anchor (exact switch ties, far out on a
    sparse stretch) are anchored at their nearest point and collected in the LAST waves, whose tier is not asserted (the last wave before them is
    filled up with repeated positions).
    Special lane: a position whose nearest point lies two ring steps from an anchor inside that anchor's five-point certificate ("seed"; on the 3-point
    ring, where two steps on are one step back, any position).  (a) it is anchored like a regular lane, (b) at the seed's anchor two steps away, (c) not
    at all.  -> dict(cases, case [n], inp {arr: [n][5]}, intent {arr: [waves] tier 1 / 2 / 3 or 0 = not asserted}, seeds)"""
    key = ("reward", name)
    if key in _cache:
        return _cache[key]
    tx, ty, tw = track
    P = len(tx)
    tables = ring_tables(track)
    rng = np.random.default_rng(len(name) * 1000 + P)
    cases = projection_cases(track, rng)
    good, poor, seeds = [], [], []
    for k, c in enumerate(cases):
        i, (px, py) = c["ex"]["i"], c["p"]
        c["anchor"] = None
        for a in np.roll([i, (i - 1) % P, (i + 1) % P], -(k % 3)):
            m3, r3, m5, r5, g3, g5 = ring_masks_np(track, tables, int(a), px, py)
            if m3 and g3 and (a + r3) % P == i and (P < 5 or (m5 and g5 and (a + r5) % P == i)):
                c["anchor"] = int(a)
                break
        (good if c["anchor"] is not None else poor).append(k)
        if c["anchor"] is None:
            c["anchor"] = i
            continue
        for a in ((i + 2) % P, (i - 2) % P):
            m3, r3, m5, r5, g3, g5 = ring_masks_np(track, tables, a, px, py)
            if P >= 5 and not m3 and g3 and m5 and g5 and (a + r5) % P == i:
                seeds.append((k, a))
    if P < 5:
        seeds = [(k, (cases[k]["ex"]["i"] + 2) % P) for k in good[:8]]
    assert seeds, name
    good_set = set(good)
    assert good
    pad = (-len(good)) % 63 if poor else 0                              # the uncertified positions start a wave of their own: the last certified wave is filled up with repeats
    order = good + [good[k % len(good)] for k in range(pad)] + poor
    lane_case, anchors, intent = [], {arr: [] for arr in ARRANGEMENTS}, {arr: [] for arr in ARRANGEMENTS}
    for w, at in enumerate(range(0, len(order), 63)):
        regs = order[at:at + 63]
        sk, sa = seeds[w % len(seeds)]
        lane_case += [sk] + regs
        reg_anchors = [cases[k]["anchor"] for k in regs]
        anchors["a"] += [cases[sk]["anchor"]] + reg_anchors
        anchors["b"] += [sa] + reg_anchors
        anchors["c"] += [-1] + reg_anchors
        pure = all(k in good_set for k in regs)
        intent["a"].append(1 if pure else 0)
        intent["b"].append((2 if pure else 0) if P >= 5 else 0)
        intent["c"].append(3)
    if len(lane_case) % 64 == 0:                                        # a ragged last wave, always
        lane_case.append(order[0])
        for arr in ARRANGEMENTS:
            anchors[arr].append(cases[order[0]]["anchor"])
    lane_case = np.array(lane_case)
    pos = np.array([cases[k]["p"] for k in lane_case])
    inp = {arr: np.column_stack([pos, np.zeros((len(pos), 2)), np.array(anchors[arr], dtype=np.float64)]) for arr in ARRANGEMENTS}     # cars at rest: no speed term, no slip penalty
    _cache[key] = dict(cases=cases, case=lane_case, inp=inp, intent=intent, seeds=seeds, tables=tables, good=len(good), poor=len(poor))
    return _cache[key]


def wave_tiers(out):
    """which tier of car_reward each wave of 64 lanes took, from the lanes' own mask bits: 1 = every lane passed the three-point test, 2 = not that, but every
    lane passed the five-point test, 3 = the general search"""
    n = out.shape[0]
    t = []
    for at in range(0, n, 64):
        o = out[at:at + 64]
        t.append(1 if np.all(o[:, 2] == 1.0) else (2 if np.all(o[:, 4] == 1.0) else 3))
    return t


def check_wave_masks(out):
    """device only: the masks every lane of a wave saw are ONE value, whose bits are the lanes' own bits, and exec is the wave's population"""
    n = out.shape[0]
    for at in range(0, n, 64):
        o = out[at:at + 64]
        cnt = o.shape[0]
        ex = bits(o[:, 11])
        assert np.all(ex == np.uint64((1 << cnt) - 1)), (at, hex(int(ex[0])), cnt)
        for col, bit in ((9, 2), (10, 4)):
            m = bits(o[:, col])
            assert np.all(m == m[0]), (at, col)
            want = sum(1 << l for l in range(cnt) if o[l, bit] == 1.0)
            assert int(m[0]) & ((1 << cnt) - 1) == want, (at, col, hex(int(m[0])), hex(want))


def check_reward_positions(name, track, L, outs, device, log=print):
    """outs: {arrangement: [n][12]} -> the worst distance error in units of u |p - p1|; asserts everything section 3 of the test's docstring lists"""
    tx, ty, tw = track
    P = len(tx)
    n = len(L["case"])
    worst, nedge_in, nedge_out, seen, nmask = 0.0, 0, 0, set(), 0
    o_a = outs["a"]
    for arr in ARRANGEMENTS:
        o = outs[arr]
        assert o.shape == (n, REW_OUT) and not np.isnan(o[:, :9]).any()
        # identical bits whichever way the nearest point was found: reward, outgoing anchor, and the unanchored search's verdict, distance and point
        for col in (0, 1, 6, 7, 8):
            assert np.array_equal(bits(o[:, col]), bits(o_a[:, col])), (name, arr, col, np.flatnonzero(bits(o[:, col]) != bits(o_a[:, col]))[:5])
        tiers = wave_tiers(o)
        for w, (got, want) in enumerate(zip(tiers, L["intent"][arr])):
            assert want == 0 or got == want, (name, arr, "wave", w, "took tier", got, "intended", want)
        if device:
            check_wave_masks(o)
        for l in range(n):
            a = int(L["inp"][arr][l, 4])
            m3, r3, m5, r5, g3, g5 = ring_masks_np(track, L["tables"], a, *L["inp"][arr][l, :2])
            if g3:
                assert o[l, 2] == float(m3) and (not m3 or o[l, 3] == r3), (name, arr, l, o[l, 2:4], m3, r3)
            if g5:
                assert o[l, 4] == float(m5) and (not m5 or o[l, 5] == r5), (name, arr, l, o[l, 4:6], m5, r5)
            nmask += g3 + g5
    for l in range(n):
        c = L["cases"][L["case"][l]]
        ex, kind = c["ex"], c["kind"]
        i = ex["i"]
        rew, anchor, within, d, anchor_u = o_a[l, 0], int(o_a[l, 1]), bool(o_a[l, 6]), o_a[l, 7], int(o_a[l, 8])
        assert anchor == i and anchor_u == i, (name, kind, l, anchor, anchor_u, i)                         # the long-double nearest point
        tie = abs(ex["dm2"] - ex["dp2"]) <= 4 * U * (ex["dm2"] + ex["dp2"])
        cands = [ex["d_prev"], ex["d_next"]] if tie else [ex["d_prev"] if ex["prev"] else ex["d_next"]]
        bound = 4 * U * float(ex["u"])                                                                      # derived in tests/test_track_projection_cpu.py
        err = min(abs(LD(d) - cc) for cc in cands)
        assert err <= bound, (name, kind, l, d, [float(cc) for cc in cands], float(err), bound)
        if ex["u"] > 0:
            worst = max(worst, float(err) / (U * float(ex["u"])))
        want = (0.0 if within else -1000000.0) + -d
        if kind == "point" or ex["u"] == 0:
            assert d == 0.0, (name, l, d)                                                                   # on a track point: exactly 0
        if d == 0.0:                                                                                        # a car at rest ON the centre line: nothing absorbs the
            assert rew in ((2e-150, 0.0) if device else (0.0,)), (name, l, rew)                            # device's 2 fast_sqrt(0) = 2e-150
        else:
            assert rew == want, (name, kind, l, rew, want)
        if kind == "edge":
            ref = float(cands[0])
            assert abs(abs(ref - tw[i]) - 1e-9) < 1e-12, (name, l, ref)
            assert within == (ref < tw[i]), (name, l, d, ref)
            nedge_in += within; nedge_out += not within
        seen.add(kind)
    assert seen == {"point", "segment", "near", "edge", "switch"} and nedge_in > 0 and nedge_out > 0 and nmask > 3 * n
    log("[dynamics reward %s] %s: worst distance error %.2f u |p - p1| (bound 4), %d lanes (%d with a certified anchor, %d without), edge in / out %d / %d, waves per tier (a) %s (b) %s (c) %s"
        % ("device" if device else "host", name, worst, n, L["good"], L["poor"], nedge_in, nedge_out, *[np.bincount(wave_tiers(outs[arr]), minlength=4)[1:].tolist() for arr in ARRANGEMENTS]))
    return worst


def tie_track():
    """a closed track on small integer coordinates: every squared distance and every search key below is an integer far below 2^53, hence exact"""
    xs = [0, 4, 8, 8, 8, 4, 0, 0]
    ys = [0, 0, 0, 4, 8, 8, 8, 4]
    return tuple(np.array(a, dtype=np.float64) for a in (xs, ys, [3.0] * 8))


def tie_cases():
    """positions with integer coordinates on the perpendicular bisector of two consecutive track points (the pair P-1, 0 included), nearer to those two than to
    any other point, anchored at either of the two, at the ring neighbours on both sides and not at all -> track, inp [n][5], the lower index of each lane's pair"""
    track = tie_track()
    tx, ty, _ = track
    P = len(tx)
    rows, low = [], []
    for i in range(P):
        j = (i + 1) % P
        mx, my = (tx[i] + tx[j]) / 2, (ty[i] + ty[j]) / 2
        nx, ny = (ty[j] - ty[i]) / 4, -(tx[j] - tx[i]) / 4                       # unit normal (the segments are 4 long and axis-parallel)
        for s in (-1.0, 0.0, 1.0):
            p = (mx + s * nx, my + s * ny)
            d2 = (tx - p[0]) ** 2 + (ty - p[1]) ** 2
            if not (d2[i] == d2[j] and np.all(np.delete(d2, [i, j]) > d2[i])):
                continue
            for a in (i, j, (i - 1) % P, (j + 1) % P, -1):
                rows.append([p[0], p[1], 0.0, 0.0, float(a)]); low.append(min(i, j))
    return track, np.array(rows), np.array(low)


def slip_cases(oracle, track):
    """the 4000 random states of tests/test_dynamics_shim.py::test_reward_matches_the_reference_reward (its draws), then cars at rest, Vx = 0 with Vy != 0 and
    reversed cars on both sides of the slip limit; odd lanes carry no anchor, even lanes their nearest point -> inp [n][5], the oracle's reward [n]"""
    key = "slip"
    if key not in _cache:
        tx, ty, tw = track
        env = oracle.OracleEnv("car", 1, track=track)
        rng = np.random.default_rng(9)
        S = []
        for i in range(4000):
            j = int(rng.integers(0, len(tx)))
            off = rng.normal(0.0, 6.0, 2) if i % 4 else rng.normal(0.0, 25.0, 2)
            S.append([tx[j] + off[0], ty[j] + off[1], rng.uniform(-np.pi, np.pi), rng.uniform(-3, 30), rng.uniform(-6, 6), rng.uniform(-1, 1), rng.uniform(-0.4, 0.4), rng.uniform(-1, 1)])
        for i in range(141):
            j = int(rng.integers(0, len(tx)))
            off = rng.normal(0.0, 5.0, 2)
            v = [(0.0, 0.0), (0.0, rng.uniform(-3, 3)), (-rng.uniform(0.1, 10), rng.uniform(-0.5, 0.5)), (-rng.uniform(0.01, 2), rng.uniform(-4, 4)), (-rng.uniform(1, 5), 0.0)][i % 5]
            S.append([tx[j] + off[0], ty[j] + off[1], 0.3, v[0], v[1], 0.0, 0.0, 0.0])
        S = np.array(S)
        ref = np.zeros(len(S))
        for i, s in enumerate(S):
            env.state = s
            ref[i] = env.reward()
        near = np.array([int(np.argmin((tx - s[0]) ** 2 + (ty - s[1]) ** 2)) for s in S])
        anchor = np.where(np.arange(len(S)) % 2, -1, near).astype(np.float64)
        _cache[key] = (np.column_stack([S[:, 0], S[:, 1], S[:, 3], S[:, 4], anchor]), ref)
    return _cache[key]


def check_slip(inp, out, ref, log=print):
    dev = np.abs(out[:, 0] - ref) / np.maximum(1.0, np.abs(ref))
    kinds = {(r < -9e5, -9e5 <= r < -4000) for r in ref}
    assert len(kinds) >= 3                                                # on the road, off the road and beyond the slip limit all occurred
    vx, vy = inp[:, 2], inp[:, 3]
    assert np.any((vx == 0) & (vy == 0)) and np.any((vx == 0) & (vy != 0)) and np.any(vx < 0)
    log("[dynamics reward] slip / speed terms: worst relative deviation from the oracle's reward %.2e over %d states" % (dev.max(), len(ref)))
    assert dev.max() < 1e-12, (dev.max(), int(np.argmax(dev)))
    return float(dev.max())


def check_ties(inp, out, low):
    """exact ties: both ring tests say "not applicable" from every anchor, and the general search returns the lower index, anchored or not"""
    assert out.shape == (len(inp), REW_OUT)
    assert np.all(out[:, 2] == 0.0) and np.all(out[:, 4] == 0.0), np.flatnonzero((out[:, 2] != 0.0) | (out[:, 4] != 0.0))
    assert np.array_equal(out[:, 1], low.astype(np.float64)) and np.array_equal(out[:, 8], low.astype(np.float64)), (out[:, 1], low)


def check_pair_drift(inp, out, renorm):
    """what renorm does, over a few thousand lanes fed pairs 1 + eps off the unit circle: renorm = false carries the drift on (the squared norm of the returned
    (sin psi, cos psi) follows 2 eps: correlation above 0.9, the rest is the rounding of the rotations), renorm = true removes it (correlation below 0.2)"""
    n = inp.shape[0]
    assert n >= 5000
    e2 = inp[:, 8] ** 2 + inp[:, 9] ** 2 - 1.0
    assert len(set(np.round(e2 * 2.0 ** 50).tolist())) >= 5                # the inputs do carry the five drifts
    c = float(np.corrcoef(out[:, 8] ** 2 + out[:, 9] ** 2 - 1.0, e2)[0, 1])
    assert (abs(c) < 0.2) if renorm else (c > 0.9), (renorm, c)
    return c


def boundary_cases():
    """On the integer track, anchored at the origin (point 0: its key is exactly 0, so 4 |p - q_a|^2 = 4 fl(px^2 + fl(py^2)) with one rounding each): positions for
    which that is EXACTLY the three-point (five-point) certificate -- the strict < must say "not applicable" -- and, one step of px lower, a few ulp below it -- applicable.
    The certificates of this track are exact integers times (1 - 1e-9), one IEEE multiplication: the same bits here and in the header's tables, so these
    lanes are checked against the restated conditions without the 1e-6 margin.  -> track, inp [4][5], (mask3, mask5) the restated conditions give"""
    track = tie_track()
    tables = ring_tables(track)
    rows, want = [], []
    for c, y0 in ((tables[1][0], 0.125), (tables[2][0], 0.25)):
        found = None
        for k in range(4000):
            py = y0 + k * 2.0 ** -20
            px0 = float(np.sqrt(c / 4.0 - py * py))
            for px in (px0, np.nextafter(px0, 0.0), np.nextafter(px0, 9.0)):
                if 4.0 * fma_exact(px, px, py * py) == c:
                    found = (px, py)
                    break
            if found:
                break
        assert found, c
        px, py = found
        below = px
        while 4.0 * fma_exact(below, below, py * py) >= c:
            below = float(np.nextafter(below, 0.0))
        for x in (px, below):
            rows.append([x, py, 0.0, 0.0, 0.0])
            m = ring_masks_np(track, tables, 0, x, py)
            want.append((m[0], m[2]))
    return track, np.array(rows), np.array(want)


def check_boundary(inp, out, want):
    assert np.array_equal(out[:, 2] == 1.0, want[:, 0]) and np.array_equal(out[:, 4] == 1.0, want[:, 1]), (out[:, [2, 4]], want)
    # whichever tier ran, the nearest point is the general search's
    assert np.array_equal(out[:, 1], out[:, 8])
