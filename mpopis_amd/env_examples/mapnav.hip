// Example environment with a data table (include/mpopis_env.h, MPOPIS_DEFINE_ENV_TABLE): a planar point that follows a list of waypoints
// across a cost map.  The table is data sized at run time -- the same code object runs on a table of 3 doubles and on one of 20 000.
//
//   state  s = [x, y, vx, vy]                (SS = 4)
//   action a = [ax, ay]                      (AS = 2)
//   params p = [dt, drag, P, G, origin, cell, w_path, w_map, w_vel, max_steps]               (NP = 10)
//   table    = [wx_0, wy_0, ..., wx_{P-1}, wy_{P-1},  map[0][0], map[0][1], ..., map[G-1][G-1]]    (2 P + G G doubles, mpopis_set_env_table)
//              P waypoints, then a G x G map, row-major (row = y cell, column = x cell) over the square [origin, origin + G cell)^2.
//              A position outside the square takes the nearest cell (the index is clamped).  P = 0 and G = 0 are legal: no path term,
//              a map that is 0 everywhere -- which is also what an env sees before any table is set (ntab == 0).
//
//   env(a):       v += dt (a - (drag + map(x, y)) v);  x += dt v;  t += 1;  done = t >= max_steps       the map is extra drag (mud)
//   reward(env):  -(w_path min_i |x - w_i|^2 + w_map map(x, y) + w_vel |v|^2)
//
// The waypoint loop runs over a wave-uniform index, the map lookup over a per-lane one; both are plain tab[...] reads.  Entries past ntab
// are never read: a table shorter than the parameters promise counts as 0 there.
//
//     from mpopis_amd import CustomEnv, GMPPI_Policy, mapnav_source
//     table = np.concatenate([waypoints.ravel(), cost_map.ravel()])
//     env = CustomEnv(mapnav_source(), 4, 2, params=[0.1, 0.2, len(waypoints), G, -1.0, 2.0 / G, 1.0, 0.5, 0.1, 200], table=table)
//     pol = GMPPI_Policy(env, num_samples=1024, horizon=20, λ=1.0, U0=[0.0, 0.0], cov_mat=[0.3, 0.3])
//     env(pol(env))
#include "mpopis_env.h"

// cell index along one axis: floor, clamped to 0..G-1 (NaN -> 0)
MPOPIS_ENV_FN int mapnav_cell(double x, double origin, double cell, int G) {
    const double c = floor((x - origin) / cell);
    return !(c >= 0.0) ? 0 : (c > (double)(G - 1) ? G - 1 : (int)c);
}

MPOPIS_ENV_FN double mapnav_map(double x, double y, const double* p, const double* tab, int ntab) {
    const int P = (int)p[2], G = (int)p[3];
    if (G < 1) return 0.0;
    const int idx = 2 * P + mapnav_cell(y, p[4], p[5], G) * G + mapnav_cell(x, p[4], p[5], G);
    return idx < ntab ? tab[idx] : 0.0;
}

MPOPIS_ENV_FN void mapnav_step(double* s, int* t, int* done, const double* a, const double* p, const double* tab, int ntab) {
    const double dt = p[0], damp = p[1] + mapnav_map(s[0], s[1], p, tab, ntab);
    s[2] += dt * (a[0] - damp * s[2]);
    s[3] += dt * (a[1] - damp * s[3]);
    s[0] += dt * s[2];
    s[1] += dt * s[3];
    *t += 1;
    *done = *t >= (int)p[9] ? 1 : 0;
}

MPOPIS_ENV_FN double mapnav_reward(const double* s, int t, int done, const double* p, const double* tab, int ntab) {
    (void)t; (void)done;
    const int P = (int)p[2] < ntab / 2 ? (int)p[2] : ntab / 2;
    double dmin = 0.0;
    for (int i = 0; i < P; ++i) {
        const double dx = s[0] - tab[2 * i], dy = s[1] - tab[2 * i + 1];
        const double d = dx * dx + dy * dy;
        dmin = (i == 0 || d < dmin) ? d : dmin;
    }
    return -(p[6] * dmin + p[7] * mapnav_map(s[0], s[1], p, tab, ntab) + p[8] * (s[2] * s[2] + s[3] * s[3]));
}

MPOPIS_DEFINE_ENV_TABLE(4, 2, 10, mapnav_step, mapnav_reward)
