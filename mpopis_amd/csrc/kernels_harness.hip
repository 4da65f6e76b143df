// kernels_harness.hip -- the bookkeeping of the closed-loop trial harness (engine_harness.hip), one lane per trial slot:
//   simulate_car_racing trial loop   src/examples/car_example.jl:199-302
//   simulate_mountaincar trial loop  src/examples/mountaincar_example.jl:125-180
//   simulate_cartpole trial loop     src/examples/cartpole_example.jl:110-160
// A kernel-only translation unit: mpopis_handle::run_trials and tools/kbench_loop.hip reach the kernels through the launchers of engine.h.
#include "engine.h"
#include "philox.h"
#include <math.h>

namespace mpopis {

__global__ void k_harness_init(double* hs, int* alive, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    for (int i = 0; i < kH_N; ++i) hs[(size_t)b * kH_N + i] = 0.0;
    hs[(size_t)b * kH_N + kH_vmax] = -INFINITY; hs[(size_t)b * kH_N + kH_bmax] = -INFINITY;
    alive[b] = 1;
}

// after env(act): cnt += 1; rew += reward(env); logging; violations; lap counter; termination
__global__ void k_harness_update(EnvDesc env, double* x, const int* done_env, const double* reward, const int* iters,
                                 double* hs, int* alive, const double* control, double* actlog, int step, int num_steps, int laps, int K, int B,
                                 StateNoise nz, SlotEnv senv) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B || !alive[b]) return;
    slot_env_into(env, senv, b);                                               // blim and within_track of the slot's own car and track
    double* h = hs + (size_t)b * kH_N;
    if (nz.seeds && env.kind == MPOPIS_ENV_CAR && env.ncars == 1) {            // :224-236 (sim_type == :cr only), after reward(env)
        double z0, z1, z2, z3;
        philox_normal_pair(nz.seeds[b], (uint32_t)step, 0x40000000u, 0, nz.rng_tab, &z0, &z1);      // (tables read from global memory: a few lanes per step)
        philox_normal_pair(nz.seeds[b], (uint32_t)step, 0x40000000u, 1, nz.rng_tab, &z2, &z3);
        double* s = x + (size_t)b * 8;
        s[0] += nz.sx * z0; s[1] += nz.sy * z1;
        const double dpsi = nz.spsi * z2;
        s[2] += dpsi;
        const double c = cos(dpsi), sn = sin(dpsi), vx = s[3], vy = s[4];      // passive rotation matrix [c s; -s c]
        s[3] = c * vx + sn * vy; s[4] = -sn * vx + c * vy;
    }
    if (actlog) for (int i = 0; i < env.as; ++i) actlog[((size_t)b * (num_steps + 1) + step) * env.as + i] = control[(size_t)b * env.as + i];
    h[kH_rollouts] += (double)iters[b] * K;
    const double step_rew = reward[b];
    h[kH_rew] += step_rew;                                                     // :210-211
    const double cnt = h[kH_cnt] + 1.0;                                        // :208
    h[kH_cnt] = cnt;
    bool done = false;
    if (env.kind != MPOPIS_ENV_CAR) {
        done = done_env[b] != 0;                                               // env.done from RL.jl _step!
    } else {
        const int NC = env.ncars;
        const double* xb = x + (size_t)b * 8 * NC;
        double curr_y = xb[1], vmean = 0, vmax = -INFINITY, bmean = 0, bmax = -INFINITY, d = INFINITY;   // :241-253,:265-270
        bool ex_b = false, within_t = true;
        for (int c = 0; c < NC; ++c) {
            const double* s = xb + 8 * c;
            if (s[1] < curr_y) curr_y = s[1];
            const double v = sqrt(s[3] * s[3] + s[4] * s[4]);
            const double be = fabs(atan2(s[4], s[3]));
            vmean += v; bmean += be; vmax = fmax(vmax, v); bmax = fmax(bmax, be);
            d = fmin(d, sqrt(s[0] * s[0] + s[1] * s[1]));
            if (be > (senv.cars ? senv.cars[(size_t)b * NC + c].blim : env.car.blim)) ex_b = true;      // (a fleet: car c's own β limit)
            double dist;
            if (!within_track(env.track, s[0], s[1], &dist, nullptr)) within_t = false;
        }
        h[kH_vmean] += vmean / NC; h[kH_bmean] += bmean / NC;
        h[kH_vmax] = fmax(h[kH_vmax], vmax); h[kH_bmax] = fmax(h[kH_bmax], bmax);
        if (step_rew < -4000) {                                                // :256-263
            if (ex_b) h[kH_beta] += 1;
            if (!within_t) h[kH_trk] += 1;
            const double temp_rew = step_rew + (ex_b ? 5000.0 : 0.0) + (!within_t ? 1000000.0 : 0.0);
            if (temp_rew < -10500) h[kH_crash] += 1;
        }
        if (h[kH_prev_y] < 0.0 && curr_y >= 0.0 && d <= 15.0) {                // :273-276
            h[kH_lap] += 1;
            const int lap = (int)h[kH_lap];
            if (lap >= 1 && lap <= 4) h[kH_lap0 + lap - 1] = cnt;
        }
        if (h[kH_lap] >= laps || h[kH_trk] > 10 || h[kH_beta] > 50) done = true;   // :277-279
        h[kH_prev_y] = curr_y;
    }
    if (done || !(cnt <= num_steps)) alive[b] = 0;                              // while !env.done && cnt <= num_steps
}

void launch_harness_init(double* hs, int* alive, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_harness_init, dim3((B + 63) / 64), dim3(64), 0, s, hs, alive, B);
}

void launch_harness_update(const EnvDesc& env, double* x, const int* done_env, const double* reward, const int* iters, double* hs, int* alive,
                           const double* control, double* actlog, int step, int num_steps, int laps, int K, int B, const StateNoise& nz,
                           const SlotEnv& senv, hipStream_t s) {
    hipLaunchKernelGGL(k_harness_update, dim3((B + 63) / 64), dim3(64), 0, s, env, x, done_env, reward, iters, hs, alive, control, actlog, step,
                       num_steps, laps, K, B, nz, senv);
}

}  // namespace mpopis
