"""CPU check of the distance from a position to the track's centre line as the rollout kernels compute it (mpopis_amd/csrc/car_dynamics.h:
track_prev_nearer + track_line_dist, the cross product of p - p1 with the tabulated unit tangent of the chosen segment) against a long-double
point-to-line distance, through the host build of the header (tests/shim/host_shim.cpp: shim_within_ring, shim_within_anchor, shim_car_reward).

Bound on |dist - exact|: 4 u |p - p1| |t^| with u = 2^-53, absolute.  Where it comes from: the components of p - p1 carry one rounding each (u),
those of t^ half an ulp (the table rounds a long-double quotient once), the product uy tx and the final fma one rounding each, so to first order
|error| <= (|ux ty| + |uy tx|) (u + u/2 + u) + u dist <= 3.5 u |p - p1| |t^| (Cauchy-Schwarz; dist <= |p - p1|); 4 u leaves the second-order
terms and the reference's own 2^-64 arithmetic.  On a track point p - p1 = 0 and the distance must be exactly 0.

Positions: on every track point, on the segments, at the switch between predecessor and successor (equidistant, and one ulp to either side),
within 1e-9 m of the lane edge on both sides, around the wrap-around P-1 -> 0 (every point of every track is visited), all bundled tracks plus a
3-point and a 5-point ring.  The ring paths and the general search (anchored and unanchored) must return identical bits."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from tests.helpers.dynamics_cases import tracks as _tracks, exact as _exact, normal as _normal, positions as _positions

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "shim", "host_shim.cpp")
SHIM_SO = os.path.join(HERE, "shim", "libhost_shim.so")
HDR = os.path.join(os.path.dirname(HERE), "mpopis_amd", "csrc", "car_dynamics.h")
dp = C.POINTER(C.c_double)
LD = np.longdouble
U = 2.0 ** -53


@pytest.fixture(scope="module")
def shim():
    if (not os.path.exists(SHIM_SO)) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(SHIM_SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", SHIM_SO, SHIM_SRC])
    L = C.CDLL(SHIM_SO)
    L.shim_within_anchor.argtypes = [C.c_int, dp, dp, dp, C.c_double, C.c_double, C.POINTER(C.c_int), dp]
    L.shim_within_ring.argtypes = [C.c_int, dp, dp, dp, C.c_double, C.c_double, C.POINTER(C.c_int), dp, C.POINTER(C.c_int)]
    L.shim_car_reward.argtypes = [dp, C.c_int, dp, dp, dp, dp]
    L.shim_car_reward.restype = C.c_double
    return L


TRACKS = _tracks()                                               # kept alive: the shim caches the tables of a track by the address of its x array
_DUMMY = tuple(np.ascontiguousarray(a) for a in (np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.ones(3)))


def _call(shim, track, p, anchor, ring):
    tx, ty, tw = track
    a, d, fast = C.c_int(anchor), C.c_double(), C.c_int(-1)
    args = (len(tx), tx.ctypes.data_as(dp), ty.ctypes.data_as(dp), tw.ctypes.data_as(dp), float(p[0]), float(p[1]))
    w = shim.shim_within_ring(*args, C.byref(a), C.byref(d), C.byref(fast)) if ring else shim.shim_within_anchor(*args, C.byref(a), C.byref(d))
    return bool(w), a.value, d.value, fast.value


@pytest.mark.parametrize("name,track", TRACKS, ids=[n for n, _ in TRACKS])
def test_cross_product_projection_matches_a_long_double_distance(shim, oracle, name, track):
    assert np.finfo(LD).eps <= 2.0 ** -63, "needs an extended-precision long double for the reference"
    tx, ty, tw = track
    P = len(tx)
    rng = np.random.default_rng(len(name) * 1000 + P)
    for t in (_DUMMY, track):                                    # make the shim's two cached-track slots rebuild for THIS track (they key on addresses)
        _call(shim, t, (0.0, 0.0), -1, True); _call(shim, t, (0.0, 0.0), -1, False)
    p20 = oracle.car_default_params()
    worst, seen, nring, nedge_in, nedge_out, nswitch = 0.0, set(), 0, 0, 0, 0
    for kind, p in _positions(track, rng):
        ex = _exact(track, p)
        if kind == "edge":                                       # slide along the chosen segment's normal until the exact distance is lane_w -+ 1e-9
            j = (ex["i"] - 1) % P if ex["prev"] else (ex["i"] + 1) % P
            _, n = _normal(track, ex["i"], j)
            d = float(ex["d_prev"] if ex["prev"] else ex["d_next"])
            eps = 1e-9 if d > tw[ex["i"]] else -1e-9
            sgn = np.sign(np.dot(p - np.array([tx[ex["i"]], ty[ex["i"]]]), n))
            p = p + n * sgn * ((tw[ex["i"]] + eps) - d)
            ex2 = _exact(track, p)
            if ex2["i"] != ex["i"] or ex2["prev"] != ex["prev"]:
                continue                                         # (the move changed the segment: not an edge sample of this segment)
            ex = ex2
        if not ex["clear"]:
            continue                                             # two track points equally near: the search's tie rules, not the projection, decide
        i = ex["i"]
        # every path from every anchor that can reach this point: ring tiers from the point itself and its ring neighbours, the general search
        # anchored there and unanchored -- identical bits
        got = [_call(shim, track, p, a, True) for a in (i, (i - 1) % P, (i + 1) % P)] + [_call(shim, track, p, a, False) for a in (i, (i + 1) % P, -1)]
        nring += sum(g[3] > 0 for g in got[:3])
        w, a, d, _ = got[0]
        for g in got[1:]:
            assert g[:3] == (w, a, d), (name, kind, p, got)
        assert a == i, (name, kind, p, a, i)
        # which segment: the long-double choice, unless the two squared distances agree to within the rounding of the double comparison
        tie = abs(ex["dm2"] - ex["dp2"]) <= 4 * U * (ex["dm2"] + ex["dp2"])
        cands = [ex["d_prev"], ex["d_next"]] if tie else [ex["d_prev"] if ex["prev"] else ex["d_next"]]
        bound = 4 * U * float(ex["u"]) * 1.0
        err = min(abs(LD(d) - c) for c in cands)
        if kind == "point":
            assert d == 0.0, (name, p, d)
        assert err <= bound, (name, kind, p, d, [float(c) for c in cands], float(err), bound)
        if ex["u"] > 0:
            worst = max(worst, float(err) / (U * float(ex["u"])))
        seen.add(kind)
        nswitch += kind == "switch" and tie
        if kind == "edge":
            ref = float(cands[0])
            assert abs(abs(ref - tw[i]) - 1e-9) < 1e-12, (name, p, ref)
            assert w == (ref < tw[i]), (name, p, d, ref)         # 1e-9 m is 10^5 error bounds away from the edge: the verdict is not in doubt
            nedge_in += w; nedge_out += not w
            # the same through the reward: -dist on the road, -1e6 - dist off it (a car at rest: no speed term, no slip penalty)
            s = np.array([p[0], p[1], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
            rew = shim.shim_car_reward(p20.ctypes.data_as(dp), P, tx.ctypes.data_as(dp), ty.ctypes.data_as(dp), tw.ctypes.data_as(dp), s.ctypes.data_as(dp))
            assert rew == ((0.0 if w else -1000000.0) + -d), (name, p, rew, d)
    print("\n[projection] %s: worst error %.2f u |p - p1| (bound 4), %d ring-path evaluations, edge in / out %d / %d, exact switches %d"
          % (name, worst, nring, nedge_in, nedge_out, nswitch))
    assert seen == {"point", "segment", "near", "edge", "switch"}
    assert nring > 0 and nedge_in > 0 and nedge_out > 0
