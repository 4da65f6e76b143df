// kernels_rollout_fleet.hip -- the car rollout of a FLEET handle (mpopis_set_env_params_cars): every car of a multi-car slot
// integrates with its own CarParams, as env.envs[c] of the reference's MultiCarRacingEnv owns its params (multi-car_racing.jl:23-45, :200-207).
//
// Mapping: one WAVE per car.  A workgroup is NC waves of 64 lanes for 64 samples; wave c integrates and rewards car c of each.  The lane-packed
// kernels of kernels_rollout.hip put the cars of a sample into different lanes of ONE wave, where parameters that differ per car would be per-lane
// values: 38 doubles = 76 VGPRs on top of kernels that sit at 165-168 VGPRs.  Here c is wave-uniform, so car c's CarParams arrive like the one-car
// kernel's -- scalar loads through the constant address space into SGPRs -- and car_action_step / car_reward run unchanged.  The price is the pair
// terms of the multi-car reward (:145-158): the cars of a sample now sit in different waves, so each wave publishes its 64 (x, y) in LDS after every
// model step and the workgroup meets at one barrier per step.
// The pieces shared with the lane-packed kernels (track staging, control stream, start state, epilogue, the launcher that raises the LDS limit) come
// from kernels_rollout.hip, included as text like kernels_rollout_slots.hip does; with MPOPIS_ROLLOUT_FLEET it instantiates no kernel of its own.
#if defined(MPOPIS_ROLL_PROF) || defined(MPOPIS_PATH_STATS)
#error "the dev builds instrument kernels_rollout.hip only"
#endif
#define MPOPIS_ROLLOUT_SLOT_TWINS
#define MPOPIS_ROLLOUT_FLEET
#include "kernels_rollout.hip"

namespace mpopis {

// The exchange: buffer t & 1 holds the positions after model step t, [car][x, y][lane].  Wave c writes its row, the workgroup barrier of step t
// follows, then every wave reads the rows q > c.  Step t + 1 writes the OTHER buffer, and its barrier separates the reads of buffer t & 1 from the
// writes of step t + 2 into it.  After the last step the buffer of step T (last read in step T - 2, two barriers ago) carries the per-car costs.
template <int NC>
struct FleetExchange {
    double xy[2][NC][2][64];
};
static_assert(sizeof(FleetExchange<kMaxCars>) + sizeof(double) * kMaxCars * 4 == fleet_static_lds(kMaxCars), "rollout_form counts this");

// Three waves per SIMD: 147-162 VGPRs and no spill.  At the one-car kernel's four (128 VGPRs) the body spills 12-14 VGPRs without the logger and
// 24-38 with it, and measured slower: 224 against 208 us per launch at one three-car trial of K = 4096, 1483 against 1419 us at 64.
template <int NC, bool LOG, bool TLDS>
__global__ void __launch_bounds__(64 * NC) __attribute__((amdgpu_waves_per_eu(3, 3))) k_rollout_fleet(RolloutArgs a) {
    static_assert(NC >= 2 && NC <= kMaxCars, "2..8 cars (a one-car handle has no fleet)");
    const int b = blockIdx.y;
    const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);            // this wave's car
    CarParams p; Track slot_tk;
    slot_const_copy(p, a.senv.cars + ((size_t)b * NC + c));                    // wave-uniform address: scalar loads, as the one-car per-slot kernel's
    slot_const_copy(slot_tk, a.senv.track + b);
    if (!rollout_slot_begin(a, b)) return;                                     // (uniform per workgroup: no wave is left waiting at a barrier)
    const CarLane<1> l(blockIdx.x, a.K);                                       // lane = sample; lanes past K load from sample K - 1 and take part in every barrier
    const int T = a.T;
    extern __shared__ __attribute__((aligned(16))) double sh_dyn[];
    __shared__ FleetExchange<NC> ex;
    __shared__ double sh_bnd[NC][4];
    const Track tk = stage_track<TLDS>(slot_tk, sh_dyn, threadIdx.x, 64 * NC); // once per workgroup, shared by its NC waves
    stage_action_bounds<NC>(a.env, sh_bnd);
    __syncthreads();
    CarState s = load_start_state<NC>(a, b, c);
    double* tr = LOG ? a.traj + ((size_t)b * a.K + l.kk) * (size_t)(8 * NC * T) : nullptr;
    const ControlStream<NC> ctl(a, b, c, l.kk);

    double cost = 0.0, cc = 0.0;
    double e0 = ctl.Eb[0], e1 = ctl.Eb[a.K], u0 = ctl.Ub[0], u1 = ctl.Ub[1];
    for (int t = 0; t < T; ++t) {
        double v0, v1;
        ctl.next(t, T, a.K, e0, e1, u0, u1, v0, v1, cc);
        const double a0 = clamp_action<NC>(a.env, sh_bnd, c, 0, v0), a1 = clamp_action<NC>(a.env, sh_bnd, c, 1, v1);
        car_action_step<LOG>(p, s, a0, a1, (t & 3) == 0);                      // unit-circle renormalisation every 4th step
        double (*xy)[2][64] = ex.xy[t & 1];
        xy[c][0][l.lane] = s.x; xy[c][1][l.lane] = s.y;
        double rew = car_reward(p, tk, s.x, s.y, s.Vx, s.Vy, &s.near);         // (the other waves' positions arrive meanwhile)
        __syncthreads();
        for (int q = c + 1; q < NC; ++q) {                                     // multi-car_racing.jl:145-158, as add_pair_terms: ascending q, same arithmetic
            const double dx = xy[q][0][l.lane] - s.x, dy = xy[q][1][l.lane] - s.y;
            const double dd = fast_sqrt(fma(dx, dx, dy * dy));
            rew += -dd;
            if (dd <= 4.0) rew += -11000.0;
        }
        cost -= rew;                                                           // utils.jl:138
        if (LOG && l.valid) {                                                  // trajectories[k][t, :] utils.jl:140
            double s8[8];
            car_state_to8(s, s8);
#pragma unroll
            for (int i = 0; i < 8; ++i) tr[(size_t)(8 * c + i) * T + t] = s8[i];
        }
    }
    cost += cc;
    // the sample's cost: the sum over its cars in car order, formed by wave 0 (cost_0 + cost_1 + ...) as sum_over_cars forms it
    double (*fin)[2][64] = ex.xy[T & 1];
    fin[c][0][l.lane] = cost;
    __syncthreads();
    if (c != 0) return;
    double total = cost;
#pragma unroll
    for (int q = 1; q < NC; ++q) total += fin[q][0][l.lane];
    rollout_epilogue<1>(a, b, l, total);
}

// dynamic LDS beyond which the kernel's limit is raised: what the default 64 KB leaves beside the static part; raised, the ring table of the largest
// track (131 360 B) + the static part stay inside the CU's 160 KB
constexpr int kFleetDynLdsRaised = 132 * 1024;
static_assert((size_t)(kRingStride * (kMaxTrackPoints + 2 * kRingPad) + 2 * kMaxTrackPoints) * sizeof(double) <= (size_t)kFleetDynLdsRaised
              && (size_t)kFleetDynLdsRaised + fleet_static_lds(kMaxCars) <= 160 * 1024, "ring table of the largest track + the exchange must fit a CU's LDS");

template <int NC, bool LOG, bool TLDS>
static void launch_fleet_kernel(const RolloutArgs& a, size_t lds, hipStream_t st) {
    static std::atomic<unsigned long long> seen{0};
    const void* fn = (const void*)k_rollout_fleet<NC, LOG, TLDS>;
    if (lds + fleet_static_lds(NC) > 64 * 1024) ensure_dyn_lds(fn, kFleetDynLdsRaised, seen);
    hipLaunchKernelGGL((k_rollout_fleet<NC, LOG, TLDS>), dim3((a.K + 63) / 64, a.B), dim3(64 * NC), lds, st, a);
}

template <int NC = 2>
static bool launch_fleet(const RolloutArgs& a, const RolloutForm& f, hipStream_t st) {
    if (a.env.ncars != NC) {
        if constexpr (NC < kMaxCars) return launch_fleet<NC + 1>(a, f, st);
        else return false;
    }
    if (a.traj) { if (f.tlds) launch_fleet_kernel<NC, true, true>(a, f.lds, st); else launch_fleet_kernel<NC, true, false>(a, f.lds, st); }
    else        { if (f.tlds) launch_fleet_kernel<NC, false, true>(a, f.lds, st); else launch_fleet_kernel<NC, false, false>(a, f.lds, st); }
    return true;
}

bool launch_car_rollout_fleet(const RolloutArgs& a, const RolloutForm& f, hipStream_t st) {
    if (!a.senv.cars || !a.senv.track) return false;
    return launch_fleet(a, f, st);
}

}  // namespace mpopis
