// Example environment for the env SDK (include/mpopis_env.h): a planar point mass that is steered to a goal.
//
//   state  s = [x, y, vx, vy, effort]        (SS = 5)    effort: a leaky integral of the squared thrust
//   action a = [ax, ay, brake]               (AS = 3)    thrust per axis and a brake that adds drag; bounds per action, e.g.
//                                                        lo = [-1, -0.5, 0], hi = [0.7, 1, 1] (mpopis_set_action_bounds)
//   params p = [dt, drag, brake_gain, goal_x, goal_y, w_pos, w_vel, w_effort, max_steps]      (NP = 9)
//
//   env(a):       v += dt (a_xy - (drag + brake_gain * brake) v);  x += dt v;  effort = 0.9 effort + dt |a_xy|^2;  t += 1;  done = t >= max_steps
//   reward(env):  -(w_pos |x - goal|^2 + w_vel |v|^2 + w_effort effort)        smooth: no sample sits on a discontinuity
//
// Build and run it under any policy:
//     from mpopis_amd import CustomEnv, GMPPI_Policy, pointmass_source
//     env = CustomEnv(pointmass_source(), 5, 3, params=[0.1, 0.2, 1.5, 1.0, -0.5, 1.0, 0.1, 0.05, 200], lo=[-1, -0.5, 0], hi=[0.7, 1, 1])
//     pol = GMPPI_Policy(env, num_samples=1024, horizon=20, λ=1.0, U0=[0.0, 0.0, 0.0], cov_mat=[0.3, 0.3, 0.1])
//     env(pol(env))
// Every index into s, a and p is a compile-time constant, so state and action stay in registers (see the rules in mpopis_env.h).
#include "mpopis_env.h"

MPOPIS_ENV_FN void pointmass_step(double* s, int* t, int* done, const double* a, const double* p) {
    const double dt = p[0], damp = p[1] + p[2] * a[2];
    s[2] += dt * (a[0] - damp * s[2]);
    s[3] += dt * (a[1] - damp * s[3]);
    s[0] += dt * s[2];
    s[1] += dt * s[3];
    s[4] = 0.9 * s[4] + dt * (a[0] * a[0] + a[1] * a[1]);
    *t += 1;
    *done = *t >= (int)p[8] ? 1 : 0;
}

MPOPIS_ENV_FN double pointmass_reward(const double* s, int t, int done, const double* p) {
    (void)t; (void)done;
    const double dx = s[0] - p[3], dy = s[1] - p[4];
    return -(p[5] * (dx * dx + dy * dy) + p[6] * (s[2] * s[2] + s[3] * s[3]) + p[7] * s[4]);
}

MPOPIS_DEFINE_ENV(5, 3, 9, pointmass_step, pointmass_reward)
