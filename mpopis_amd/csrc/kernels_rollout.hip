// kernels_rollout.hip -- the fused model-rollout kernel: replaces, per sample k,
//   simulate_model            src/mppi_mpopi_policies.jl:261-278  (V = pol.U + E[:,k], control cost, clamp)
//   calculate_trajectory_costs(::MPPI_Policy) inner loop  :198-214
//   get_model_controls        src/utils.jl:55-67
//   rollout_model             src/utils.jl:129-144
//   env(a) + reward(env)      car_racing.jl:238-344,201-213; multi-car_racing.jl:200-207,145-158;
//                             mountaincar_example.jl:4-22
// in ONE launch, state in registers, no per-sample env copies (the reference deep-copies the env
// per sample, :270).
//
// Mapping (CDNA4): lane = one car of one sample.  A wave = S = 64/NC samples x NC cars, lane = c * S + j, so the cars of one sample sit in ONE
// wave and exchange (x,y) for the pairwise terms of the multi-car reward by lane shuffles -- no LDS exchange, no barrier in the time loop (round 2
// ran wave = car with a workgroup barrier per model step: 5.9 cycles per VALU instruction at 64 trials against 4.8 for the one-car kernel).  One
// car (S = 64): E is [cs][K] (K fastest) so each per-step control load is one coalesced 512-B transaction per wave; the nominal control U, the env
// state, the action bounds and the 48-point track are wave-uniform and arrive through the scalar cache / LDS broadcasts.  The kernels are
// FP64-VALU bound; HBM traffic is 8*cs bytes per sample.
// Two device bodies serve 1..8 cars: rollout_one_wave (each wave integrates and rewards its samples) and rollout_two_wave (a dynamics wave hands
// the state to a reward wave, for few rollouts).  The entry points k_rollout_car / k_rollout_car_duo (one car) and k_rollout_cars /
// k_rollout_cars_duo (2..8 cars) are one call each into them, with their own launch bounds and occupancy.
// The per-slot-env twins of the car kernels are compiled from this same text as a translation unit of their own,
// kernels_rollout_slots.hip (it defines MPOPIS_ROLLOUT_SLOT_TWINS and includes this file): the kernel templates and the launcher templates are
// shared, everything else -- the simple envs, the start-state kernels, rollout_form, launch_rollout -- exists here only.  The build stays as
// long as its longest file that way; with both sets in one file it took twice the time.
// A third unit, kernels_rollout_fleet.hip (one wave per car, for handles whose cars carry their own parameters), includes
// this text with MPOPIS_ROLLOUT_FLEET as well and takes the pieces only: no kernel or launcher of this file is instantiated there.
#include "engine.h"

namespace mpopis {
#ifdef MPOPIS_ROLLOUT_SLOT_TWINS
constexpr bool kSlotTwins = true;
#else
constexpr bool kSlotTwins = false;
#endif
bool launch_car_rollout_slots(const RolloutArgs& a, const RolloutForm& f, hipStream_t st);      // kernels_rollout_slots.hip: the SENV instantiations

// Track tables into LDS (dynamic LDS layout: ring table [(P+6)][6] + certification radii [2][P]; with ALL: + x, y, w, |q|^2 [4][P] + neighbour
// distances [P][W+1] + neighbour indices [P][W+1]).  Returns the Track the rollout uses; the caller synchronises.
template <bool ALL>
__device__ __forceinline__ Track stage_track(const Track& g, double* sh, int tid, int nthreads) {
    const int P = g.P, W = g.nbrw, NS = P * (W + 1);
    double* sh_ring = sh;
    double* sh_cert = sh + kRingStride * (P + 2 * kRingPad);
    for (int i = tid; i < kRingStride * (P + 2 * kRingPad); i += nthreads) sh_ring[i] = g.ring[i];
    for (int i = tid; i < 2 * P; i += nthreads) sh_cert[i] = g.ring_cert[i];      // three-point and five-point certificates
    if (!ALL) return Track{g.x, g.y, g.w, g.n2, P, g.nbr_idx, g.nbr_dist, W, sh_ring, sh_cert};
    double* sh_trk = sh_cert + 2 * P;
    double* sh_nd = sh_trk + 4 * P;
    int* sh_ni = reinterpret_cast<int*>(sh_nd + NS);
    for (int i = tid; i < P; i += nthreads) { sh_trk[i] = g.x[i]; sh_trk[P + i] = g.y[i]; sh_trk[2 * P + i] = g.w[i]; sh_trk[3 * P + i] = g.n2[i]; }
    for (int i = tid; i < NS; i += nthreads) { sh_nd[i] = g.nbr_dist[i]; sh_ni[i] = g.nbr_idx[i]; }
    return Track{sh_trk, sh_trk + P, sh_trk + 2 * P, sh_trk + 3 * P, P, sh_ni, sh_nd, W, sh_ring, sh_cert};
}

// TLDS: every track table fits the default 64 KB of dynamic LDS (P <= 190 points: all bundled tracks).  Otherwise only the ring table of the
// straight-line nearest-point search is staged (64 B per point) and the general search -- first step of a rollout, lanes far off their
// anchor -- reads the coordinate / neighbour tables from global memory.
#ifdef MPOPIS_ROLL_PROF
// dev build (tools/roll_prof.sh): start / end time (s_memrealtime, 100 MHz) and hardware id of every wave of the last 1-car launch.
// What it showed (C5, 64 trials, 4 waves per SIMD): the waves of a SIMD do not progress together -- issue arbitration is oldest-first, the oldest
// wave runs at the lone-wave rate and ends at ~146 us, the youngest at ~376 us -- but evening them out with rotating s_setprio levels (per action,
// by wave slot and clock) narrowed the spread to 259..374 us WITHOUT shortening the launch: the SIMD's throughput is the same either way,
// ~5.0 cycles per FP64 instruction at 4 waves (tools/mfma_rate.hip measures 5.0 for bare v_fma_f64 streams at 4 waves per SIMD, 4.6 at 8), and
// 43.0 k instructions x 4 waves x 5.0 cycles = the measured launch.  The kernel is at the attainable issue rate; only fewer instructions help.
__device__ unsigned long long g_roll_prof[3 * 8192];
extern "C" int mpopis_debug_roll_prof(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_roll_prof), sizeof(g_roll_prof)); }
#endif
#ifdef MPOPIS_PATH_STATS
extern "C" int mpopis_debug_path_stats(unsigned long long* out, int reset) {      // dev build: read (and optionally clear) the path counters of car_dynamics.h
    int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_path_stats), sizeof(g_path_stats));
    if (reset) { unsigned long long z[8] = {0}; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_path_stats), z, sizeof z); }
    return rc;
}
extern "C" int mpopis_debug_sick(unsigned char* out, int n, int reset) {       // per-thread flags of the launches since the last reset
    int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sick), (size_t)n);
    if (reset) { void* p = nullptr; rc |= (int)hipGetSymbolAddress(&p, HIP_SYMBOL(g_sick)); rc |= (int)hipMemset(p, 0, sizeof(g_sick)); }
    return rc;
}
#endif

// ---- the pieces of a rollout, each written once ----

// Slots with active == 0 are skipped (AIS early break); the slot's first thread records the iteration.  False: skip this slot.
__device__ __forceinline__ bool rollout_slot_begin(const RolloutArgs& a, int b) {
    if (a.active && !a.active[b]) return false;
    if (a.iters && blockIdx.x == 0 && threadIdx.x == 0) a.iters[b] = a.iter_n;
    return true;
}

// lane = c * S + j: car c of sample j, S = 64 / NC samples per wave (the 64 - NC S lanes past them idle as duplicates: 1 at NC = 3, 7; 4 at 5, 6).
// wave_id numbers the slot's sample-waves; kk is a sample index that idle lanes may load from.
template <int NC>
struct CarLane {
    static constexpr int S = 64 / NC;
    int lane, c, j, k, kk;
    bool valid;
    __device__ __forceinline__ CarLane(int wave_id, int K)
        : lane(threadIdx.x & 63), c(min(lane / S, NC - 1)), j(lane - c * S), k(wave_id * S + j), kk(min(k, K - 1)), valid((j < S) & (k < K)) {}
};

// car c's start state in slot b: the 8 state doubles, sin / cos of psi and delta, and the nearest track point (launch_extend_state)
template <int NC>
__device__ __forceinline__ CarState load_start_state(const RolloutArgs& a, int b, int c) {
    const double* xe = a.x0ext + ((size_t)b * NC + c) * kCarExt;
    CarState s;
    s.x = xe[0]; s.y = xe[1]; s.psi = xe[2]; s.Vx = xe[3]; s.Vy = xe[4]; s.r = xe[5]; s.delta = xe[6]; s.pedal = xe[7];
    s.sp = xe[8]; s.cp = xe[9]; s.sd = xe[10]; s.cd = xe[11]; s.near = (int)xe[12];
    return s;
}

// The controls of car c in sample kk (simulate_model, :271-272).  next() forms V = pol.U + E[:,k] of step t from the values the caller holds
// (e0, e1: noise, u0, u1: nominal control, loaded one step ahead), starts their loads for step t + 1 -- the next step's noise (global) and nominal
// control (scalar at one car) are in flight during this step -- and adds the control cost of the unclamped V (γ = 0 in every reference config).
// The prefetched values and T, K stay with the caller: kept as members, they changed the code of the time loops (3.6 % slower two-wave 3-car rollouts).
template <int NC>
struct ControlStream {
    static constexpr int as = 2 * NC;
    const double *Eb, *Ub, *Uo, *gv;
    __device__ __forceinline__ ControlStream(const RolloutArgs& a, int b, int c, int kk)
        : Eb(a.E + (size_t)b * a.cs * a.K + (size_t)(2 * c) * a.K + kk), Ub(a.Ucur + (size_t)b * a.cs + 2 * c), Uo(a.Uorig + (size_t)b * a.cs + 2 * c),
          gv(a.gvec ? a.gvec + (size_t)b * a.cs + 2 * c : nullptr) {}
    __device__ __forceinline__ void next(int t, int T, int K, double& e0, double& e1, double& u0, double& u1, double& v0, double& v1, double& cc) const {
        v0 = u0 + e0; v1 = u1 + e1;
        if (t + 1 < T) {
            e0 = Eb[(size_t)(t + 1) * as * K]; e1 = Eb[(size_t)(t + 1) * as * K + K];
            u0 = Ub[(t + 1) * as]; u1 = Ub[(t + 1) * as + 1];
        }
        if (__builtin_expect(gv != nullptr, 0)) cc += control_cost_term(gv[t * as], v0 - Uo[t * as], gv[t * as + 1], v1 - Uo[t * as + 1]);
    }
};

// The action bounds of get_model_controls (NaN passes through).  One car: wave-uniform kernel arguments, clamped against scalar registers
// (clampd_u).  NC cars: the bounds differ between the cars of a wave, so every lane reads its car's from the LDS table bnd (clampd_v), which
// stage_action_bounds fills before the workgroup barrier.
template <int NC>
__device__ __forceinline__ void stage_action_bounds(const EnvDesc& env, double (*bnd)[4]) {
    if (NC > 1 && threadIdx.x < NC) {
        const int q = threadIdx.x;
        bnd[q][0] = env.lo[2 * q]; bnd[q][1] = env.hi[2 * q]; bnd[q][2] = env.lo[2 * q + 1]; bnd[q][3] = env.hi[2 * q + 1];
    }
}
template <int NC>
__device__ __forceinline__ double clamp_action(const EnvDesc& env, const double (*bnd)[4], int c, int i, double v) {
    if constexpr (NC == 1) return clampd_u(v, env.lo[i], env.hi[i]);
    else return clampd_v(v, bnd[c][2 * i], bnd[c][2 * i + 1]);
}

// multi-car_racing.jl:145-158: the distance from car c to each car behind it in the env's order, and the collision penalty.  The other cars' (x, y)
// come from the lanes of the same sample by shuffles (every lane takes part in each).  Nothing at one car.
template <int NC>
__device__ __forceinline__ double add_pair_terms(double rew, double x, double y, int c, int j) {
    constexpr int S = 64 / NC;
#pragma unroll
    for (int q = 1; q < NC; ++q) {
        const double xq = __shfl(x, q * S + j, 64), yq = __shfl(y, q * S + j, 64);
        if (q > c) {
            const double dx = xq - x, dy = yq - y;
            const double dd = fast_sqrt(fma(dx, dx, dy * dy));                 // 1 ulp (car_dynamics.h); coincident cars give 1e-150, not 0
            rew += -dd;
            if (dd <= 4.0) rew += -11000.0;
        }
    }
    return rew;
}

// the sample's cost, the sum over its cars in car order: meaningful on the car-0 lanes (cost_0 + cost_1 + ...)
template <int NC>
__device__ __forceinline__ double sum_over_cars(double cost, int j) {
    constexpr int S = 64 / NC;
    double total = cost;
#pragma unroll
    for (int q = 1; q < NC; ++q) total += __shfl(cost, q * S + j, 64);
    return total;
}

// The car-0 lane of a valid sample writes its cost.  ρ = minimum(costs) (utils.jl:81) accumulates into cmin, one atomic per wave, so that the AIS
// reweighting can be folded into the moments kernel (launch_wcov_mfma, weights from costs) instead of a launch of its own between the two.
template <int NC>
__device__ __forceinline__ void rollout_epilogue(const RolloutArgs& a, int b, const CarLane<NC>& l, double total) {
    const bool writer = l.valid && l.c == 0;
    if (writer) a.cost[(size_t)b * a.K + l.k] = total;
    if (a.cmin) {
        unsigned long long key = writer ? cost_key(total) : ~0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(key, o, 64); key = (t < key) ? t : key; }
        if (l.lane == 0) atomicMin(&a.cmin[b], key);
        if (writer && !(fabs(total) < INFINITY) && a.status) status_raise(&a.status[b], MPOPIS_ERR_ACTION);   // non-finite cost <=> NaN action (car_racing.jl:239)
    }
}

// The two-slot LDS mailbox of rollout_two_wave: the dynamics wave publishes (x, y, Vx, Vy) of every lane after model step t, the reward wave
// consumes them; release / acquire at workgroup scope.  After the last step the dynamics wave leaves its control cost and publishes T + 1.
struct RolloutMailbox {
    double state[2][4][64];
    double cc[64];
    int ready, done;                                                           // model steps published by wave 0 / consumed by wave 1
    __device__ __forceinline__ void publish(int t, int lane, const CarState& s) {
        const int slot = t & 1;
        if (t >= 2) while (__hip_atomic_load(&done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < t - 1) __builtin_amdgcn_s_sleep(1);   // slot free again?
        state[slot][0][lane] = s.x; state[slot][1][lane] = s.y; state[slot][2][lane] = s.Vx; state[slot][3][lane] = s.Vy;
        __hip_atomic_store(&ready, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ void consume(int t, int lane, double& x, double& y, double& Vx, double& Vy) {
        while (__hip_atomic_load(&ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < t + 1) __builtin_amdgcn_s_sleep(1);
        const int slot = t & 1;
        x = state[slot][0][lane]; y = state[slot][1][lane]; Vx = state[slot][2][lane]; Vy = state[slot][3][lane];
        __hip_atomic_store(&done, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);       // (release: the reads above are complete)
    }
    __device__ __forceinline__ void close(int T, int lane, double c) {
        cc[lane] = c;
        __hip_atomic_store(&ready, T + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ double control_cost(int T, int lane) {
        while (__hip_atomic_load(&ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < T + 1) __builtin_amdgcn_s_sleep(1);
        return cc[lane];
    }
};

// The env of slot b.  SENV (a handle after mpopis_set_env_params_slots / mpopis_set_tracks): the slot's own CarParams and Track descriptor, copied
// from the [B] arrays at the top of the kernel through the constant address space, at an address every lane of the workgroup shares
// (b = blockIdx.y) -- so the copies are scalar loads into SGPRs, where the shared form keeps its kernel arguments.  The setters are setup calls
// (they wait for the handle's queued work), so nothing writes these arrays under a running kernel.  A car handle with either per-slot part
// in force passes BOTH arrays (the other one holds copies of the shared value, mpopis_handle::sync_slot_env): choosing between an array and the
// kernel argument here would make the address generic and the loads vector loads, 80 VGPRs of parameters.
template <class P>
__device__ __forceinline__ void slot_const_copy(P& dst, const P* src) {
    typedef const P __attribute__((address_space(4))) * CP;      // the constant address space: what makes the copy scalar loads
    __builtin_memcpy(&dst, (CP)src, sizeof(P));
}

// ---- the two bodies ----

// One wave integrates and rewards S samples x NC cars; SPB sample-waves per workgroup share one LDS copy of the track tables.
// LOG: the trajectory logger is on (a.traj != nullptr) -- only then is the heading angle psi itself tracked.
template <int NC, int SPB, bool LOG, bool TLDS, bool SENV>
__device__ __forceinline__ void rollout_one_wave(const RolloutArgs& a) {
#ifdef MPOPIS_ROLL_PROF
    const unsigned long long prof_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    const int b = blockIdx.y;
    CarParams slot_car; Track slot_tk;
    if constexpr (SENV) { slot_const_copy(slot_car, a.senv.car + b); slot_const_copy(slot_tk, a.senv.track + b); }
    if (!rollout_slot_begin(a, b)) return;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);           // sample-wave of the workgroup
    const CarLane<NC> l(blockIdx.x * SPB + g, a.K);
    const int T = a.T;
    const CarParams& p = SENV ? slot_car : a.env.car;
    // stage the (wave-uniform, read-only) track in LDS: uniform-address ds_reads broadcast to all lanes
    extern __shared__ __attribute__((aligned(16))) double sh_dyn[];
    __shared__ double sh_bnd[NC][4];
    const Track tk = stage_track<TLDS>(SENV ? slot_tk : a.env.track, sh_dyn, threadIdx.x, 64 * SPB);
    stage_action_bounds<NC>(a.env, sh_bnd);
    __syncthreads();
    CarState s = load_start_state<NC>(a, b, l.c);
    double* tr = LOG ? a.traj + ((size_t)b * a.K + l.kk) * (size_t)(8 * NC * T) : nullptr;
    const ControlStream<NC> ctl(a, b, l.c, l.kk);

    double cost = 0.0, cc = 0.0;
    double e0 = ctl.Eb[0], e1 = ctl.Eb[a.K], u0 = ctl.Ub[0], u1 = ctl.Ub[1];
    for (int t = 0; t < T; ++t) {
        double v0, v1;
        ctl.next(t, T, a.K, e0, e1, u0, u1, v0, v1, cc);
        const double a0 = clamp_action<NC>(a.env, sh_bnd, l.c, 0, v0), a1 = clamp_action<NC>(a.env, sh_bnd, l.c, 1, v1);
        car_action_step<LOG>(p, s, a0, a1, (t & 3) == 0);                      // unit-circle renormalisation every 4th step
        const double rew = add_pair_terms<NC>(car_reward(p, tk, s.x, s.y, s.Vx, s.Vy, &s.near), s.x, s.y, l.c, l.j);
        cost -= rew;                                                           // utils.jl:138
        if (LOG && l.valid) {                                                  // trajectories[k][t, :] utils.jl:140
            double s8[8];
            car_state_to8(s, s8);
#pragma unroll
            for (int i = 0; i < 8; ++i) tr[(size_t)(8 * l.c + i) * T + t] = s8[i];
        }
    }
    cost += cc;
    const double total = sum_over_cars<NC>(cost, l.j);
#ifdef MPOPIS_PATH_STATS
    if constexpr (NC == 1) {   // dev build, one car: rollouts of this launch that took the general sub-step at least once / that end stopped (per launch: flags cleared)
        const size_t t_ = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
        const bool went = t_ < sizeof(g_sick) && (g_sick[t_] & 1);
        if (t_ < sizeof(g_sick)) g_sick[t_] = 0;
        const int nw = __popcll(__ballot(went)), ns = __popcll(__ballot(!(s.Vx > 0.5)));
        if (l.lane == 0) { atomicAdd(&g_path_stats[6], (unsigned long long)nw); atomicAdd(&g_path_stats[7], (unsigned long long)ns); }
    }
#endif
    rollout_epilogue(a, b, l, total);
#ifdef MPOPIS_ROLL_PROF
    if (NC == 1 && l.lane == 0) {
        const int w = (blockIdx.y * gridDim.x + blockIdx.x) * SPB + g;
        if (w < 8192) {
            unsigned hwid; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            g_roll_prof[3 * w] = prof_t0; g_roll_prof[3 * w + 1] = __builtin_amdgcn_s_memrealtime(); g_roll_prof[3 * w + 2] = ((unsigned long long)xcc << 32) | hwid;
        }
    }
#endif
}

// Few rollouts (up to two rollout waves per SIMD -- one trial of K <= 4096, or the 8 .. 32-trials-per-GPU share of a strong-scaled run).  A wave
// alone on a SIMD issues one FP64 instruction per ~8.4 cycles whatever it does, so a rollout costs its instruction count and most of the chip
// idles.  Here a workgroup is TWO waves for S samples: wave 0 integrates the dynamics of every car (V = U + E, clamp, car_action_step) and hands
// (x, y, Vx, Vy) after every model step to wave 1 through the mailbox; wave 1 evaluates the reward (nearest-point search, lane test, drift
// penalty: ~110 of the ~885 instructions of a one-car model step) and the pair terms, accumulates the cost and sums it over the cars.  Same
// arithmetic in the same order as rollout_one_wave -- bit-identical costs -- with the dynamics wave's chain 11 % shorter at one car.  The reward
// wave is ~8x faster than the dynamics wave, so the producer practically never waits for a free slot.
template <int NC, bool TLDS, bool SENV>
__device__ __forceinline__ void rollout_two_wave(const RolloutArgs& a) {
    const int b = blockIdx.y;
    CarParams slot_car; Track slot_tk;
    if constexpr (SENV) { slot_const_copy(slot_car, a.senv.car + b); slot_const_copy(slot_tk, a.senv.track + b); }
    if (!rollout_slot_begin(a, b)) return;
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // 0: dynamics, 1: reward
    const CarLane<NC> l(blockIdx.x, a.K);
    const int T = a.T;
    const CarParams& p = SENV ? slot_car : a.env.car;
    extern __shared__ __attribute__((aligned(16))) double sh_dyn[];
    __shared__ double sh_bnd[NC][4];
    __shared__ RolloutMailbox mb;
    const Track tk = stage_track<TLDS>(SENV ? slot_tk : a.env.track, sh_dyn, threadIdx.x, 128);
    stage_action_bounds<NC>(a.env, sh_bnd);
    if (threadIdx.x == 0) { mb.ready = 0; mb.done = 0; }
    __syncthreads();
    if (role == 0) {
        CarState s = load_start_state<NC>(a, b, l.c);
        const ControlStream<NC> ctl(a, b, l.c, l.kk);
        double cc = 0.0;
        double e0 = ctl.Eb[0], e1 = ctl.Eb[a.K], u0 = ctl.Ub[0], u1 = ctl.Ub[1];
        for (int t = 0; t < T; ++t) {
            double v0, v1;
            ctl.next(t, T, a.K, e0, e1, u0, u1, v0, v1, cc);
            const double a0 = clamp_action<NC>(a.env, sh_bnd, l.c, 0, v0), a1 = clamp_action<NC>(a.env, sh_bnd, l.c, 1, v1);
            car_action_step<false>(p, s, a0, a1, (t & 3) == 0);
            mb.publish(t, l.lane, s);
        }
        mb.close(T, l.lane, cc);
        return;
    }
    double cost = 0.0;
    int near = load_start_state<NC>(a, b, l.c).near;                            // the anchor of the first search: the track point nearest to the start position
    for (int t = 0; t < T; ++t) {
        double x, y, Vx, Vy;
        mb.consume(t, l.lane, x, y, Vx, Vy);
        const double rew = add_pair_terms<NC>(car_reward(p, tk, x, y, Vx, Vy, &near), x, y, l.c, l.j);
        cost -= rew;                                                           // utils.jl:138
    }
    cost += mb.control_cost(T, l.lane);
    rollout_epilogue(a, b, l, sum_over_cars<NC>(cost, l.j));
}

// ---- the entry points ----

// One car (CarRacingEnv), 4 waves per SIMD
template <int NC, int SPB, bool LOG, bool TLDS, bool SENV = false>
__global__ void __launch_bounds__(64 * NC * SPB) __attribute__((amdgpu_waves_per_eu(4, 4))) k_rollout_car(RolloutArgs a) {
    static_assert(NC == 1, "multi-car envs run k_rollout_cars");
    rollout_one_wave<NC, SPB, LOG, TLDS, SENV>(a);
}

// One car, two waves: held to 128 VGPRs = 4 waves per SIMD, so two dynamics and two reward waves share a SIMD
template <bool TLDS, bool SENV = false>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(4, 4))) k_rollout_car_duo(RolloutArgs a) {
    rollout_two_wave<1, TLDS, SENV>(a);
}

// NC >= 2 cars (MultiCarRacingEnv).  The launch runs it at WPE = 3 waves per SIMD: 168 VGPRs, no spills, 1411 us at 64 three-car trials,
// against 1509 us at 4 (128 VGPRs, 33 spills).
template <int NC, int SPB, bool LOG, int WPE, bool TLDS, bool SENV = false>
__global__ void __launch_bounds__(64 * SPB) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) k_rollout_cars(RolloutArgs a) {
    static_assert(NC >= 2 && NC <= kMaxCars, "2..8 cars");
    rollout_one_wave<NC, SPB, LOG, TLDS, SENV>(a);
}

// NC >= 2 cars, two waves, 3 waves per SIMD
template <int NC, bool TLDS, bool SENV = false>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(3, 3))) k_rollout_cars_duo(RolloutArgs a) {
    static_assert(NC >= 2 && NC <= kMaxCars, "2..8 cars");
    rollout_two_wave<NC, TLDS, SENV>(a);
}

#ifndef MPOPIS_ROLLOUT_SLOT_TWINS
// MountainCar (ss = 2) and CartPole (ss = 4): scalar action, a handful of flops per step
template <int SS, bool SENV = false>
__global__ void __launch_bounds__(64) k_rollout_simple(RolloutArgs a) {
    const int b = blockIdx.y;
    if (!rollout_slot_begin(a, b)) return;
    if constexpr (SENV) slot_env_into(a.env, a.senv, b);
    const int k = blockIdx.x * 64 + threadIdx.x;
    const int K = a.K, T = a.T;
    const bool valid = k < K;
    const int kk = valid ? k : K - 1;
    double s[SS];
#pragma unroll
    for (int i = 0; i < SS; ++i) s[i] = a.x0[b * SS + i];
    int t_env = a.t0 ? a.t0[b] : 0, done = a.done0 ? a.done0[b] : 0;
    const double* Eb = a.E + (size_t)b * a.cs * K + kk;
    const double* Ub = a.Ucur + (size_t)b * a.cs;
    const double* Uo = a.Uorig + (size_t)b * a.cs;
    const double* gv = a.gvec ? a.gvec + (size_t)b * a.cs : nullptr;
    double* tr = a.traj ? a.traj + ((size_t)b * K + kk) * (size_t)(SS * T) : nullptr;
    double cost = 0.0, cc = 0.0;
    for (int t = 0; t < T; ++t) {
        const double v = Ub[t] + Eb[(size_t)t * K];
        if (gv) cc += gv[t] * (v - Uo[t]);
        const double act = clampd(v, a.env.lo[0], a.env.hi[0]);
        // a NaN action: RL.jl's act! asserts `a in action_space(env)` and the rollout dies there.  MountainCar's reward carries the NaN state into the cost by
        // itself; CartPole's reward (1 until done) does not look at the state's values, so the cost is poisoned explicitly -- a non-finite cost is what raises
        // MPOPIS_ERR_ACTION (round 6, tests/test_gpu_edge_cases.py)
        if (act != act) cost = act;
        simple_env_step(a.env, s, &t_env, &done, act);
        cost -= simple_env_reward(a.env, s, done);
        if (tr && valid) {
#pragma unroll
            for (int i = 0; i < SS; ++i) tr[i * T + t] = s[i];
        }
    }
    if (valid) a.cost[(size_t)b * K + k] = cost + cc;
}

// x0ext[b][car][12] = env state + sin/cos(psi), sin/cos(delta): evaluated once per trial and car
// instead of once per sample (the start state is shared by all K rollouts).
// ... and the track point nearest to the start position (full scan, once per trial and car): the anchor of every rollout's first nearest-point
// search, which then takes the ring paths like every later step instead of sending the whole wave through the general search
__device__ __forceinline__ void write_xext(const double* x8, double* o, const Track& tk) {
    CarState c;
    car_state_from8(c, x8);
    o[0] = c.x; o[1] = c.y; o[2] = c.psi; o[3] = c.Vx; o[4] = c.Vy; o[5] = c.r; o[6] = c.delta; o[7] = c.pedal;
    o[8] = c.sp; o[9] = c.cp; o[10] = c.sd; o[11] = c.cd;
    int near = -1;
    if (tk.P > 0) { double dist; (void)within_track(tk, c.x, c.y, &dist, &near); }
    o[12] = (double)near;
}
__global__ void k_extend_state(const double* x, double* xext, int n_cars_total, Track tk, const Track* slot_tk, int ncars) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_cars_total) return;
    if (slot_tk) tk = slot_tk[i / ncars];
    write_xext(x + (size_t)i * 8, xext + (size_t)i * kCarExt, tk);
}
void launch_extend_state(const double* x, double* xext, int B, int ncars, hipStream_t st, const Track& tk, const Track* slot_tk) {
    const int n = B * ncars;
    hipLaunchKernelGGL(k_extend_state, dim3((n + 63) / 64), dim3(64), 0, st, x, xext, n, tk, slot_tk, std::max(1, ncars));
}

// Start of an MPC step, one launch instead of seven (at one trial the step is a chain of dependent launches, each boundary costs 2-4 us):
// status = 0 (unless sticky), active = alive gate (or 1), iters = 0, U_orig = the loop's pol.U = pol.U, and the car start states extended
// with sin/cos of psi / delta (as k_extend_state).
__global__ void __launch_bounds__(256) k_step_begin(int* status, int* active, const int* alive, int* iters, const double* U, double* Uin, double* Ucur,
                                                    int cs, const double* x, double* xext, int ncars, unsigned long long* cmin, Track tk, unsigned long long* iters_acc, const Track* slot_tk) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (slot_tk) tk = slot_tk[b];
    if (tid == 0) {
        if (iters_acc) iters_acc[b] += (unsigned long long)iters[b];          // the previous step's executed iterations (CE / CMA early breaks counted as run)
        if (status) status[b] = 0; active[b] = alive ? alive[b] : 1; iters[b] = 0; if (cmin) cmin[b] = ~0ull;
    }
    for (int i = tid; i < cs; i += 256) { const double u = U[(size_t)b * cs + i]; Uin[(size_t)b * cs + i] = u; Ucur[(size_t)b * cs + i] = u; }
    if (!x) return;
    if (tid < ncars) {
        const size_t i = (size_t)b * ncars + tid;
        write_xext(x + i * 8, xext + i * kCarExt, Track{nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr});      // (nearest point: below)
    }
    // the track point nearest to each car's start position -- the first minimum of |q_i|^2 - 2 q_i.p, exactly what within_track's full scan
    // returns -- found by the whole workgroup (one thread scanning the track serially put 3-4 us on the critical path of EVERY MPC step: C2 0.130 -> 0.134 ms)
    __shared__ double sh_v[4]; __shared__ int sh_i[4];
    for (int c = 0; c < ncars; ++c) {
        const double* s8 = x + ((size_t)b * ncars + c) * 8;
        const double m2x = -2.0 * s8[0], m2y = -2.0 * s8[1];
        double bv = 0.0; int bi = -1;
        for (int i = tid; i < tk.P; i += 256) {
            const double d = track_key(tk.x, tk.y, tk.n2, i, m2x, m2y);        // the same key and order as within_track (car_dynamics.h)
            if (bi < 0 || track_key_before(d, i, bv, bi)) { bv = d; bi = i; }  // ascending i within a thread: its first minimum
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (oi >= 0 && (bi < 0 || track_key_before(ov, oi, bv, bi))) { bv = ov; bi = oi; }
        }
        __syncthreads();
        if ((tid & 63) == 0) { sh_v[tid >> 6] = bv; sh_i[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) if (sh_i[w] >= 0 && (bi < 0 || track_key_before(sh_v[w], sh_i[w], bv, bi))) { bv = sh_v[w]; bi = sh_i[w]; }
            xext[((size_t)b * ncars + c) * kCarExt + 12] = (double)bi;
        }
    }
}
void launch_step_begin(int* status, int* active, const int* alive, int* iters, const double* U, double* Uin, double* Ucur, int B, int cs,
                       const double* x, double* xext, int ncars, hipStream_t st, unsigned long long* cmin, const Track& tk, unsigned long long* iters_acc, const Track* slot_tk) {
    hipLaunchKernelGGL(k_step_begin, dim3(B), dim3(256), 0, st, status, active, alive, iters, U, Uin, Ucur, cs, x, xext, ncars, cmin, tk, iters_acc, slot_tk);
}

#endif      // !MPOPIS_ROLLOUT_SLOT_TWINS

// Dynamic LDS a rollout kernel may request without raising its limit: the default 64 KB minus the kernels' STATIC LDS (two-wave kernels:
// mailbox 4 KB + control-cost column 0.5 KB + flags + per-car bounds, ~4.7 KB).  Beyond it the limit is raised before the launch, once per
// kernel and device, to what the largest supported track needs: the ring-only layout at kMaxTrackPoints (64 P + 288 B = 131 360 B at P = 2048)
// plus the static part, rounded up -- 144 KB of the CU's 160 KB.
constexpr size_t kRolloutDynLdsDefault = 56 * 1024;
constexpr int kRolloutDynLdsRaised = 144 * 1024;
static_assert((size_t)(kRingStride * (kMaxTrackPoints + 2 * kRingPad) + 2 * kMaxTrackPoints) * sizeof(double) + 8 * 1024 <= (size_t)kRolloutDynLdsRaised,
              "ring table of the largest track + static LDS must fit the raised limit");
// one `seen` mask per kernel (non-type template parameter): large tracks need the dynamic-LDS limit raised, per device
template <void (*KERNEL)(RolloutArgs)>
static void launch_rollout_kernel(dim3 grid, int block, size_t lds, hipStream_t st, const RolloutArgs& a) {
    static std::atomic<unsigned long long> seen{0};
    if (lds > kRolloutDynLdsDefault) ensure_dyn_lds((const void*)KERNEL, kRolloutDynLdsRaised, seen);
    hipLaunchKernelGGL(KERNEL, grid, dim3(block), lds, st, a);
}

// The one-wave form: one wave per S = 64 / NC samples, SPB waves per workgroup.  LOG: the trajectory logger; TLDS: every track table in LDS.
// (SENV = kSlotTwins: this translation unit instantiates the shared kernels, kernels_rollout_slots.hip their per-slot-env twins)
template <int NC, int SPB, bool LOG, bool TLDS>
static void launch_one_wave_kernel(const RolloutArgs& a, size_t lds, hipStream_t st) {
    const dim3 grid((a.K + SPB * (64 / NC) - 1) / (SPB * (64 / NC)), a.B);
    if constexpr (NC == 1) launch_rollout_kernel<k_rollout_car<1, SPB, LOG, TLDS, kSlotTwins>>(grid, 64 * SPB, lds, st, a);
    else launch_rollout_kernel<k_rollout_cars<NC, SPB, LOG, 3, TLDS, kSlotTwins>>(grid, 64 * SPB, lds, st, a);
}
template <int NC, int SPB>
static void launch_one_wave(const RolloutArgs& a, bool tl, size_t lds, hipStream_t st) {
    if (a.traj) { if (tl) launch_one_wave_kernel<NC, SPB, true, true>(a, lds, st); else launch_one_wave_kernel<NC, SPB, true, false>(a, lds, st); }
    else        { if (tl) launch_one_wave_kernel<NC, SPB, false, true>(a, lds, st); else launch_one_wave_kernel<NC, SPB, false, false>(a, lds, st); }
}
// The two-wave form: two waves per S samples (no logger).
template <int NC>
static void launch_two_wave(const RolloutArgs& a, bool tl, size_t lds, hipStream_t st) {
    const dim3 grid((a.K + 64 / NC - 1) / (64 / NC), a.B);
    if constexpr (NC == 1) { if (tl) launch_rollout_kernel<k_rollout_car_duo<true, kSlotTwins>>(grid, 128, lds, st, a); else launch_rollout_kernel<k_rollout_car_duo<false, kSlotTwins>>(grid, 128, lds, st, a); }
    else { if (tl) launch_rollout_kernel<k_rollout_cars_duo<NC, true, kSlotTwins>>(grid, 128, lds, st, a); else launch_rollout_kernel<k_rollout_cars_duo<NC, false, kSlotTwins>>(grid, 128, lds, st, a); }
}

#ifndef MPOPIS_ROLLOUT_SLOT_TWINS
// The two-wave form takes launches of up to this many rollout waves per CU (all parts of a multi-stream schedule together).  Measured crossovers:
// one car 8, i.e. 2 per SIMD (C5 shapes: 3.49 vs 3.95 ms at 32 trials, 5.36 vs 4.71 at 48); 2..8 cars (3 waves per SIMD) 5 (C4 shapes: 5.53 ->
// 4.86 ms at one trial, 7.18 -> 6.66 at 6 (1176 waves), 7.49 -> 7.68 at 8).  MPOPIS_ROLLOUT_DUO, read once per process, replaces the limit by a
// wave count for the whole chip; 0: never.
constexpr int kDuoCarWaves = 8, kDuoCarsWaves = 5;
static long long rollout_duo_max_waves(int ncars) {
    static const int env_duo = [] { const char* e = getenv("MPOPIS_ROLLOUT_DUO"); return e ? atoi(e) : -1; }();
    return env_duo >= 0 ? env_duo : (long long)(ncars == 1 ? kDuoCarWaves : kDuoCarsWaves) * coop_max_workgroups();
}

#endif

// NC cars (compile-time dispatch over 1..kMaxCars): the body rollout_form chose.  False: no kernel for this car count.
template <int NC = 1>
static bool launch_car_rollout(const RolloutArgs& a, const RolloutForm& f, hipStream_t st) {
    if (a.env.ncars != NC) {
        if constexpr (NC < kMaxCars) return launch_car_rollout<NC + 1>(a, f, st);
        else return false;
    }
    if (f.body == ROLLOUT_TWO_WAVE) launch_two_wave<NC>(a, f.tlds, f.lds, st);
    else if (f.body == ROLLOUT_ONE_WAVE_SPB4) launch_one_wave<NC, 4>(a, f.tlds, f.lds, st);
    else launch_one_wave<NC, 1>(a, f.tlds, f.lds, st);
    return true;
}

#if defined(MPOPIS_ROLLOUT_FLEET)
// (kernels_rollout_fleet.hip takes the pieces above and instantiates none of the kernels)
#elif defined(MPOPIS_ROLLOUT_SLOT_TWINS)
bool launch_car_rollout_slots(const RolloutArgs& a, const RolloutForm& f, hipStream_t st) { return launch_car_rollout(a, f, st); }
#else
// A caller's env (include/mpopis_env.h): the rollout kernel of its code object, same grid as k_rollout_simple.  The built-in kernels treat
// every kind that is not the car as one of the two simple envs, so a custom handle must never reach them.
// An env with a table: four-wave workgroups; a table the code object's LDS kernel can stage goes there with ntab * 8 bytes of dynamic LDS (a small
// table costs no occupancy), a larger one to the kernel that reads it from global memory.
static bool launch_custom_rollout(const RolloutArgs& a, const RolloutForm& f, hipStream_t st, hipError_t* err) {
    const CustomEnv* ce = a.env.custom;
    if (!ce || !ce->rollout) { if (err) *err = hipErrorInvalidHandle; return false; }
    mpopis_env_rollout_tab_args kt{};
    mpopis_env_rollout_args& k = kt.r;
    k.x0 = (uint64_t)a.x0; k.t0 = (uint64_t)a.t0; k.done0 = (uint64_t)a.done0; k.Ucur = (uint64_t)a.Ucur; k.Uorig = (uint64_t)a.Uorig;
    k.E = (uint64_t)a.E; k.gvec = (uint64_t)a.gvec; k.cost = (uint64_t)a.cost; k.traj = (uint64_t)a.traj; k.active = (uint64_t)a.active;
    k.iters = (uint64_t)a.iters; k.params = (uint64_t)ce->d_params;
    k.B = a.B; k.K = a.K; k.T = a.T; k.cs = a.cs; k.iter_n = a.iter_n;
    for (int i = 0; i < kMaxAs; ++i) { k.lo[i] = a.env.lo[i]; k.hi[i] = a.env.hi[i]; }
    hipError_t e;
    if (ce->has_table) {
        kt.table = (uint64_t)ce->table_view; kt.table_stride = ce->table_stride; kt.ntab = ce->ntab;
        const bool lds = f.tlds;                                             // rollout_form: the table fits what the code object's LDS kernel stages
        constexpr int WG = MPOPIS_ENV_TABLE_THREADS;
        void* params[] = {&kt};
        e = hipModuleLaunchKernel(lds ? ce->rollout : ce->rollout_gtab, (a.K + WG - 1) / WG, a.B, 1, WG, 1, 1, (unsigned)f.lds, st, params, nullptr);
    } else {
        void* params[] = {&k};
        e = hipModuleLaunchKernel(ce->rollout, (a.K + 63) / 64, a.B, 1, 64, 1, 1, 0, st, params, nullptr);
    }
    if (err) *err = e;
    return e == hipSuccess;
}

// The kernel launch_rollout picks (engine.h).  The car env: the two-wave form for few rollout waves (never with the logger), otherwise the one-wave
// form with one sample-wave per workgroup for small K (every wave on its own CU) or 4 sharing the LDS tables for large K.
RolloutForm rollout_form(const RolloutArgs& a) {
    RolloutForm f;
    f.log = a.traj != nullptr;
    if (a.env.kind == MPOPIS_ENV_CUSTOM) {
        const CustomEnv* ce = a.env.custom;
        f.body = ROLLOUT_CUSTOM;
        if (ce && ce->has_table && ce->ntab <= ce->table_lds_doubles) { f.tlds = true; f.lds = (size_t)ce->ntab * 8u; }
        return f;
    }
    if (a.env.kind == MPOPIS_ENV_MOUNTAINCAR || a.env.kind == MPOPIS_ENV_CARTPOLE) {
        f.body = a.env.kind == MPOPIS_ENV_CARTPOLE ? ROLLOUT_SIMPLE4 : ROLLOUT_SIMPLE2;     // state size 4 / 2
        return f;
    }
    const int P = a.env.track.P, W = a.env.track.nbrw, NC = a.env.ncars;
    // every table in LDS when that fits the default 64 KB (all bundled tracks: 48-60 points); larger tracks (beyond 190 points; Track(infile; sample_factor = 1):
    // ~1000 points) stage the ring table only (64 P + 288 B: 128.3 KB at the 2048-point limit; the kernels' dynamic-LDS limit is raised to 144 KB once)
    // Per-slot tracks: every slot of the launch runs ONE kernel, so the handle's largest track decides the placement and the LDS size (senv.lds_all /
    // lds_ring, formed by mpopis_set_tracks); each workgroup stages its own slot's P points into it.
    const size_t lds_all = a.senv.track ? a.senv.lds_all : track_lds_bytes(P, W, true);
    f.tlds = lds_all <= kRolloutDynLdsDefault;      // (static LDS of the two-wave kernels counted: P = 221, 222 used to total 65.7-66 KB without the limit being raised)
    f.lds = f.tlds ? lds_all : a.senv.track ? a.senv.lds_ring : track_lds_bytes(P, W, false);
    if (NC < 1 || NC > kMaxCars) { f.body = ROLLOUT_ONE_WAVE_SPB1; return f; }           // (no kernel: launch_rollout returns false)
    if (a.senv.cars) {
        // A fleet: always the one-wave-per-car body, whose static LDS -- the position exchange, 16 KB at 8 cars -- counts
        // against the default 64 KB where the placement is decided (the largest-track rule above holds: a fleet handle always passes senv.track)
        f.body = ROLLOUT_FLEET;
        f.tlds = lds_all + fleet_static_lds(NC) <= 64 * 1024;
        f.lds = f.tlds ? lds_all : a.senv.track ? a.senv.lds_ring : track_lds_bytes(P, W, false);
        return f;
    }
    const int S = 64 / NC;
    const long long waves = (long long)a.B * ((a.K + S - 1) / S) * std::max(1, a.share);
    // (a per-slot-env handle takes the same body as a shared one: every instantiation has its twin)
    if (!a.traj && waves <= rollout_duo_max_waves(NC)) f.body = ROLLOUT_TWO_WAVE;
    else f.body = a.K >= 1024 ? ROLLOUT_ONE_WAVE_SPB4 : ROLLOUT_ONE_WAVE_SPB1;
    return f;
}

bool launch_rollout(const RolloutArgs& a, hipStream_t st, hipError_t* custom_err) {
    const RolloutForm f = rollout_form(a);
    if (f.body == ROLLOUT_CUSTOM) return launch_custom_rollout(a, f, st, custom_err);
    if (f.body == ROLLOUT_SIMPLE2 || f.body == ROLLOUT_SIMPLE4) {
        const auto kernel = a.senv.mc || a.senv.cp ? (f.body == ROLLOUT_SIMPLE4 ? k_rollout_simple<4, true> : k_rollout_simple<2, true>)
                                                   : (f.body == ROLLOUT_SIMPLE4 ? k_rollout_simple<4> : k_rollout_simple<2>);
        hipLaunchKernelGGL(kernel, dim3((a.K + 63) / 64, a.B), dim3(64), 0, st, a);
        return true;
    }
    if (f.body == ROLLOUT_FLEET) return launch_car_rollout_fleet(a, f, st);
    return a.senv.car && a.senv.track ? launch_car_rollout_slots(a, f, st) : launch_car_rollout(a, f, st);
}
#endif      // !MPOPIS_ROLLOUT_SLOT_TWINS

}  // namespace mpopis
