// CartPole through the env SDK (include/mpopis_env.h): RL.jl CartPoleEnv(continuous = true) driven by the functor of
// src/examples/cartpole_example.jl:3-6, restated with the built-in env's parameter vector (mpopis.h: 11 doubles
// {gravity, masscart, masspole, totalmass, halflength, polemasslength, forcemag, dt, thetathreshold, xthreshold, max_steps}).
// Test infrastructure: the oracle's CartPole checks the SDK path end to end through it.
#include "mpopis_env.h"

MPOPIS_ENV_FN void cartpole_step(double* s, int* t, int* done, const double* a, const double* p) {
    *t += 1;
    const double gravity = p[0], masspole = p[2], totalmass = p[3], halflength = p[4], polemasslength = p[5], dt = p[7];
    const double force = a[0] * p[6];
    const double xdot = s[1], theta = s[2], thetadot = s[3];
    const double costheta = cos(theta), sintheta = sin(theta);
    const double tmp = (force + polemasslength * (thetadot * thetadot) * sintheta) / totalmass;
    const double thetaacc = (gravity * sintheta - costheta * tmp) / (halflength * (4.0 / 3.0 - masspole * (costheta * costheta) / totalmass));
    const double xacc = tmp - polemasslength * thetaacc * costheta / totalmass;
    s[0] += dt * xdot;
    s[1] += dt * xacc;
    s[2] += dt * thetadot;
    s[3] += dt * thetaacc;
    *done = (fabs(s[0]) > p[9] || fabs(s[2]) > p[8] || *t > (int)p[10]) ? 1 : 0;
}

MPOPIS_ENV_FN double cartpole_reward(const double* s, int t, int done, const double* p) {
    (void)s; (void)t; (void)p;
    return done ? 0.0 : 1.0;
}

MPOPIS_DEFINE_ENV(4, 1, 11, cartpole_step, cartpole_reward)
