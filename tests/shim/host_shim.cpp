// Test-only host build of the engine's shared dynamics header (mpopis_amd/csrc/car_dynamics.h), so
// the fast-path algebra used by the HIP rollout kernel can be checked against the CPU oracle on a
// machine without a GPU.  Not part of the product; never loaded by mpopis_amd.
#include "../../mpopis_amd/csrc/car_dynamics.h"
#include <vector>
#include <cstring>
using namespace mpopis;
extern "C" {
void shim_car_action_step(const double* p20, double* s8, double a0, double a1) {
    CarParams p = make_car_params(p20);
    CarState c; car_state_from8(c, s8);
    car_action_step(p, c, a0, a1);
    car_state_to8(c, s8);
}
double shim_car_reward(const double* p20, int P, const double* tx, const double* ty, const double* tw, const double* s8) {
    CarParams p = make_car_params(p20);
    const TrackHost th(P, tx, ty, tw); const Track tk = th.view();
    return car_reward(p, tk, s8[0], s8[1], s8[3], s8[4]);
}
// full single-car rollout: controls as x T (already clamped); returns -sum(reward)
double shim_car_rollout(const double* p20, int P, const double* tx, const double* ty, const double* tw,
                        double* s8, const double* ctrl, int T) {
    CarParams p = make_car_params(p20);
    const TrackHost th(P, tx, ty, tw); const Track tk = th.view();
    double c = 0.0;
    CarState st; car_state_from8(st, s8);          // sin/cos evaluated once, then carried (as in the kernel)
    for (int t = 0; t < T; ++t) { car_action_step(p, st, ctrl[2 * t], ctrl[2 * t + 1]); c -= car_reward(p, tk, st.x, st.y, st.Vx, st.Vy, &st.near); }
    car_state_to8(st, s8);
    return c;
}
void shim_mc_step(const double* p8, double* s2, int* t, int* done, double f) { McParams p = make_mc_params(p8); mc_step(p, s2, t, done, f); }
double shim_mc_reward(const double* p8, const double* s2, int done) { McParams p = make_mc_params(p8); return mc_reward(p, s2, done); }
}
extern "C" int shim_within_anchor(int P, const double* tx, const double* ty, const double* tw, double px, double py, int* anchor, double* dist) {
    static TrackHost th; static Track tk; static const double* last = nullptr;
    if (last != tx) { th = TrackHost(P, tx, ty, tw); tk = th.view(); last = tx; }
    return within_track(tk, px, py, dist, anchor) ? 1 : 0;
}
// the rollout kernels' path: ring fast path when it applies, general search otherwise (car_dynamics.h: car_reward); *fast = which one ran
extern "C" int shim_within_ring(int P, const double* tx, const double* ty, const double* tw, double px, double py, int* anchor, double* dist, int* fast) {
    static TrackHost th; static Track tk; static const double* last = nullptr;
    if (last != tx) { th = TrackHost(P, tx, ty, tw); tk = th.view(); last = tx; }
    int rel = 0;
    bool ok = ring_candidates(tk.ring, tk.ring_cert, *anchor, px, py, -2.0 * px, -2.0 * py, &rel);
    *fast = ok ? 1 : 0;
    if (!ok && tk.P >= 5) {                                    // second tier of car_reward: five candidates under the wider certificate
        ok = ring5_candidates(tk.ring, tk.ring_cert + tk.P, *anchor, px, py, -2.0 * px, -2.0 * py, &rel);
        if (ok) *fast = 2;
    }
    if (ok) {
        const bool w = ring_project(tk.ring, *anchor, rel, px, py, dist);
        *anchor = ring_wrap(*anchor + rel, tk.P);
        return w ? 1 : 0;
    }
    return within_track(tk, px, py, dist, anchor) ? 1 : 0;
}
// ---- the lane programs of tools/kbench_dynamics.hip on the host (tests/test_dynamics_cases_cpu.py): same inputs, same output layout, one call = one "wave" of one lane
extern "C" void shim_dyn_prims(int n, const double* in, double* out, double lo, double hi) {
    for (int i = 0; i < n; ++i) {
        const double* a = in + (size_t)i * 14; double* o = out + (size_t)i * 16;
        o[0] = fast_rcp1(a[0]); o[1] = fast_rcp(a[0]); o[2] = fast_sqrt(a[1]);
        double rs; o[3] = fast_sqrt_rsq(a[1], &rs); o[4] = rs;
        sincos_tiny(a[2], &o[5], &o[6]);
        o[7] = clamp_sym(a[6], a[7]); o[8] = clampd_u(a[3], lo, hi); o[9] = clampd_v(a[3], a[4], a[5]); o[10] = fma_v(a[8], a[9], a[10]);
        const TireK k = tire_consts(a[11], a[12], a[13]);
        o[11] = k.fymax; o[12] = k.thr; o[13] = k.k2; o[14] = k.k3;
    }
}
// 12-double CarState (the 8 state doubles + sp, cp, sd, cd as given) and two raw actions per lane; PSI and renorm as arguments
extern "C" void shim_dyn_step(const double* p20, int psi, int renorm, const double* bnd, int n, const double* in, double* out) {
    const CarParams p = make_car_params(p20);
    for (int i = 0; i < n; ++i) {
        const double* a = in + (size_t)i * 14; double* o = out + (size_t)i * 12;
        CarState c;
        c.x = a[0]; c.y = a[1]; c.psi = a[2]; c.Vx = a[3]; c.Vy = a[4]; c.r = a[5]; c.delta = a[6]; c.pedal = a[7];
        c.sp = a[8]; c.cp = a[9]; c.sd = a[10]; c.cd = a[11]; c.near = -1;
        const double a0 = clampd_u(a[12], bnd[0], bnd[1]), a1 = clampd_u(a[13], bnd[2], bnd[3]);
        if (psi) car_action_step<true>(p, c, a0, a1, renorm != 0); else car_action_step<false>(p, c, a0, a1, renorm != 0);
        o[0] = c.x; o[1] = c.y; o[2] = c.psi; o[3] = c.Vx; o[4] = c.Vy; o[5] = c.r; o[6] = c.delta; o[7] = c.pedal;
        o[8] = c.sp; o[9] = c.cp; o[10] = c.sd; o[11] = c.cd;
    }
}
// reward, the two ring masks (bit 0 = the single caller) with rel, and the unanchored search; in[n][5] = { px, py, Vx, Vy, anchor }
extern "C" void shim_dyn_reward(const double* p20, int P, const double* tx, const double* ty, const double* tw, int n, const double* in, double* out) {
    const CarParams p = make_car_params(p20);
    const TrackHost th(P, tx, ty, tw); const Track tk = th.view();
    for (int i = 0; i < n; ++i) {
        const double* a = in + (size_t)i * 5; double* o = out + (size_t)i * 12;
        const double px = a[0], py = a[1], m2x = -2.0 * px, m2y = -2.0 * py;
        const int a_in = (int)a[4];
        int anchor = a_in, rel3 = 0, rel5 = 0, none = -1;
        o[0] = car_reward(p, tk, px, py, a[2], a[3], &anchor); o[1] = (double)anchor;
        const unsigned long long m3 = ring_candidates(tk.ring, tk.ring_cert, a_in, px, py, m2x, m2y, &rel3);
        const unsigned long long m5 = (P >= 5) ? ring5_candidates(tk.ring, tk.ring_cert + P, a_in, px, py, m2x, m2y, &rel5) : 0ull;
        o[2] = (double)(m3 & 1ull); o[3] = (double)rel3; o[4] = (double)(m5 & 1ull); o[5] = (double)rel5;
        double dist = 0.0;
        o[6] = within_track(tk, px, py, &dist, &none) ? 1.0 : 0.0; o[7] = dist; o[8] = (double)none;
        const unsigned long long ex = 1ull;
        memcpy(&o[9], &m3, 8); memcpy(&o[10], &m5, 8); memcpy(&o[11], &ex, 8);
    }
}
// ---- one car of a rollout as kernels_rollout.hip carries it (tests/test_rollout_cases_cpu.py): the start state extended once (sin / cos; the anchor of the
// first search by the full scan, as write_xext), the actions as given (already clamped), the unit-circle renormalisation every 4th step.  n cars at once on
// one track: states[n][T][8] after every step, rew[n][T] the car's own reward of the step (no pair terms: the caller adds them), near[n] the start anchor
extern "C" void shim_car_rollout_log(const double* p20, int P, const double* tx, const double* ty, const double* tw, int n, const double* s8, const double* ctrl, int T,
                                     double* states, double* rew, int* near) {
    const CarParams p = make_car_params(p20);
    const TrackHost th(P, tx, ty, tw); const Track tk = th.view();
    for (int i = 0; i < n; ++i) {
        CarState st; car_state_from8(st, s8 + (size_t)i * 8);
        double dist; int a = -1;
        (void)within_track(tk, st.x, st.y, &dist, &a);
        st.near = a; near[i] = a;
        for (int t = 0; t < T; ++t) {
            car_action_step<true>(p, st, ctrl[((size_t)i * T + t) * 2], ctrl[((size_t)i * T + t) * 2 + 1], (t & 3) == 0);
            rew[(size_t)i * T + t] = car_reward(p, tk, st.x, st.y, st.Vx, st.Vy, &st.near);
            car_state_to8(st, states + ((size_t)i * T + t) * 8);
        }
    }
}
// the two simple envs' step and reward (engine.h's simple_env_step / simple_env_reward restated on the header's functions): kind 0 mountaincar (p8), 2 cartpole (p11)
extern "C" double shim_simple_step(int kind, const double* prm, double* s, int* t, int* done, double a) {
    if (kind == 2) { const CpParams p = make_cp_params(prm); cp_step(p, s, t, done, a); return cp_reward(*done); }
    const McParams p = make_mc_params(prm); mc_step(p, s, t, done, a); return mc_reward(p, s, *done);
}
