// MountainCar through the env SDK (include/mpopis_env.h): RL.jl MountainCarEnv(continuous = true) with the reward override of
// src/examples/mountaincar_example.jl:4-22, restated with the built-in env's parameter vector (mpopis.h: 8 doubles
// {min_pos, max_pos, max_speed, goal_pos, goal_velocity, power, gravity, max_steps}).  Test infrastructure.
#include "mpopis_env.h"

MPOPIS_ENV_FN double mc_clamp(double v, double lo, double hi) { return v > hi ? hi : (v < lo ? lo : v); }

MPOPIS_ENV_FN void mountaincar_step(double* s, int* t, int* done, const double* a, const double* p) {
    *t += 1;
    double x = s[0], v = s[1];
    v += a[0] * p[5] + cos(3 * x) * (-p[6]);
    v = mc_clamp(v, -p[2], p[2]);
    x += v;
    x = mc_clamp(x, p[0], p[1]);
    if (x == p[0] && v < 0) v = 0;
    *done = ((x >= p[3] && v >= p[4]) || (*t >= (int)p[7])) ? 1 : 0;
    s[0] = x; s[1] = v;
}

MPOPIS_ENV_FN double mountaincar_reward(const double* s, int t, int done, const double* p) {
    (void)t;
    double rew = 0.0;
    if (s[0] >= p[3] && s[1] >= p[4]) rew += 100000;
    rew += fabs(s[1]);
    rew += done ? 0.0 : -1.0;
    return rew;
}

MPOPIS_DEFINE_ENV(2, 1, 8, mountaincar_step, mountaincar_reward)
