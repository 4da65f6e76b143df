// A damped pendulum through the env SDK (include/mpopis_env.h) whose two functions carry the obvious names `step` and `reward`, and which
// reads no parameters (NP = 0): state [angle, angular velocity], one torque.  Test infrastructure: the names must not collide with anything
// the SDK macro generates, on the device as on the host.
#include "mpopis_env.h"

MPOPIS_ENV_FN void step(double* s, int* t, int* done, const double* a, const double* p) {
    (void)p;
    s[1] += 0.1 * (a[0] - 0.5 * s[1] - sin(s[0]));
    s[0] += 0.1 * s[1];
    *t += 1;
    *done = *t >= 50 ? 1 : 0;
}

MPOPIS_ENV_FN double reward(const double* s, int t, int done, const double* p) {
    (void)t; (void)done; (void)p;
    const double d = s[0] - 1.0;
    return -(d * d + 0.1 * s[1] * s[1]);
}

MPOPIS_DEFINE_ENV(2, 1, 0, step, reward)
