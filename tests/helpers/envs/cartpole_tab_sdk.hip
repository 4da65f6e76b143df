// cartpole_sdk.hip with its eleven parameters in the env's TABLE instead of the parameter vector (NP = 0, tab[0..10] in the order of
// mpopis.h: {gravity, masscart, masspole, totalmass, halflength, polemasslength, forcemag, dt, thetathreshold, xthreshold, max_steps}).
// Test infrastructure: ties the table kernels of MPOPIS_DEFINE_ENV_TABLE to the built-in CartPole and to the oracle's.
#include "mpopis_env.h"

MPOPIS_ENV_FN void cartpole_step(double* s, int* t, int* done, const double* a, const double* p, const double* tab, int ntab) {
    (void)p; (void)ntab;
    *t += 1;
    const double gravity = tab[0], masspole = tab[2], totalmass = tab[3], halflength = tab[4], polemasslength = tab[5], dt = tab[7];
    const double force = a[0] * tab[6];
    const double xdot = s[1], theta = s[2], thetadot = s[3];
    const double costheta = cos(theta), sintheta = sin(theta);
    const double tmp = (force + polemasslength * (thetadot * thetadot) * sintheta) / totalmass;
    const double thetaacc = (gravity * sintheta - costheta * tmp) / (halflength * (4.0 / 3.0 - masspole * (costheta * costheta) / totalmass));
    const double xacc = tmp - polemasslength * thetaacc * costheta / totalmass;
    s[0] += dt * xdot;
    s[1] += dt * xacc;
    s[2] += dt * thetadot;
    s[3] += dt * thetaacc;
    *done = (fabs(s[0]) > tab[9] || fabs(s[2]) > tab[8] || *t > (int)tab[10]) ? 1 : 0;
}

MPOPIS_ENV_FN double cartpole_reward(const double* s, int t, int done, const double* p, const double* tab, int ntab) {
    (void)s; (void)t; (void)p; (void)tab; (void)ntab;
    return done ? 0.0 : 1.0;
}

MPOPIS_DEFINE_ENV_TABLE(4, 1, 0, cartpole_step, cartpole_reward)
