/*
 * mpopis_env.h -- device-side SDK: run every policy of libmpopis_hip.so on YOUR environment.
 *
 * The reference's plug-in seam is Julia dispatch on (policy type, env type): any AbstractEnv with env(a), reward(env), state(env) and
 * action_space(env) runs under all its policies (rollout_model(env::AbstractEnv, ...) src/utils.jl:129-144, simulate_model(pol,
 * env::AbstractEnv, ...) src/mppi_mpopi_policies.jl:261-278).  Here the same seam is a gfx950 code object: you write env(a) and reward(env)
 * as two functions, one macro line turns them into the engine's rollout / env-step / env-query kernels, you compile the file with
 *
 *     hipcc --genco --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -I include my_env.hip -o my_env.hsaco
 *
 * (mpopis_amd.build.build_env does exactly that) and hand the bytes to the C ABI's custom-env create call of include/mpopis.h.  The engine
 * loads the module at create time and launches its kernels where it launches its built-in rollout kernels; no host is in the loop.
 *
 *     #include "mpopis_env.h"
 *     MPOPIS_ENV_FN void   my_step  (double* s, int* t, int* done, const double* a, const double* p) { ... }   // env(a): advance s in place
 *     MPOPIS_ENV_FN double my_reward(const double* s, int t, int done, const double* p) { ... }               // reward(env) after the step
 *     MPOPIS_DEFINE_ENV(SS, AS, NP, my_step, my_reward)
 *
 *   s     state(env), SS doubles                      a   the action, AS doubles, already clamped to action_space(env)
 *   t     the env's step counter (you advance it)     p   NP parameter doubles (mpopis_set_env_params), wave-uniform
 *   done  the env's terminated flag (you set it)
 *
 * Rules for the two functions.  Index s, a and p with compile-time constants only (write loops over them with #pragma unroll and constant
 * trip counts): state and action then live in registers.  A per-thread array indexed at run time lands in scratch memory and costs an
 * order of magnitude; `-Rpass-analysis=kernel-resource-usage` must report ScratchSize 0 for mpopis_env_rollout.  No statics, no I/O, no
 * dependence on the thread index: the same function steps one of K model rollouts and the real env.
 *
 * A host compiler sees MPOPIS_ENV_FN as `static inline` and MPOPIS_DEFINE_ENV as two plain C functions (mpopis_env_host_step,
 * mpopis_env_host_reward) plus the constant, so the same source builds into a CPU shim for testing the dynamics without a GPU
 * (g++ -x c++ -shared -fPIC -I include my_env.hip).
 *
 * An env with a data table -- a reference path, an obstacle list, a cost grid, a lookup curve: data sized at run time -- takes two more
 * arguments and the second macro:
 *
 *     MPOPIS_ENV_FN void   my_step  (double* s, int* t, int* done, const double* a, const double* p, const double* tab, int ntab) { ... }
 *     MPOPIS_ENV_FN double my_reward(const double* s, int t, int done, const double* p, const double* tab, int ntab) { ... }
 *     MPOPIS_DEFINE_ENV_TABLE(SS, AS, NP, my_step, my_reward)
 *
 *   tab   the ntab doubles the handle holds for this trial slot (mpopis_set_env_table: one table for all slots, or one per slot), read-only.
 *         Index it at run time, wave-uniformly (a loop over waypoints) or per lane (the grid cell under a position); ntab == 0 until a table
 *         is set, and tab must not be dereferenced then.  The rules for s, a and p stay as above.
 *
 * A table of up to MPOPIS_ENV_TABLE_LDS_DOUBLES doubles is staged in LDS once per workgroup of four waves (mpopis_env_rollout_tab); a larger one,
 * up to MPOPIS_ENV_MAX_TABLE, is read from global memory through the constant address space (mpopis_env_rollout_gtab).  The engine picks the
 * kernel by the size of the table that is set; the two functions are the same source in both, and in the host build.
 */
#ifndef MPOPIS_ENV_H
#define MPOPIS_ENV_H
#include <stdint.h>
#include <math.h>

#define MPOPIS_ENV_SDK_VERSION 1
#define MPOPIS_ENV_MAX_STATE 64      /* SS in 1..64 */
#define MPOPIS_ENV_MAX_ACTION 16     /* AS in 1..16 */
#define MPOPIS_ENV_MAX_PARAMS 64     /* NP in 0..64 */
#define MPOPIS_ENV_ERR_ACTION (-3)   /* == MPOPIS_ERR_ACTION of mpopis.h */
#define MPOPIS_ENV_TABLE_VERSION 1
#define MPOPIS_ENV_TABLE_LDS_DOUBLES 4096      /* largest table staged in LDS: 32 KiB, up to five workgroups per CU */
#define MPOPIS_ENV_MAX_TABLE (1 << 20)         /* ntab in 0..2^20 doubles per slot */
#define MPOPIS_ENV_TABLE_THREADS 256           /* workgroup of the two table rollout kernels: four waves */

/* Kernel arguments: plain data with fixed-width fields, shared by the generated kernels and the engine that launches them (both include
 * this header).  Every uint64_t is a device address (0 = absent). */
typedef struct {
    uint64_t x0;        /* const double [B][SS]      start state of every slot                                        */
    uint64_t t0;        /* const int32  [B]          env step counter                                                 */
    uint64_t done0;     /* const int32  [B]          env terminated flag                                              */
    uint64_t Ucur;      /* const double [B][cs]      pol.U of the running AIS iteration                               */
    uint64_t Uorig;     /* const double [B][cs]      U_orig                                                           */
    uint64_t E;         /* const double [B][cs][K]   noise, row t*AS + j, K fastest                                   */
    uint64_t gvec;      /* const double [B][cs] or 0 gamma U_orig' Sigma^-1 (control cost)                            */
    uint64_t cost;      /* double       [B][K]       out                                                              */
    uint64_t traj;      /* double [B][K][SS][T] or 0 logger (state after every model step)                            */
    uint64_t active;    /* const int32 [B] or 0      slots with active == 0 are skipped                               */
    uint64_t iters;     /* int32 [B] or 0            iters[b] = iter_n for every slot worked on                       */
    uint64_t params;    /* const double [NP]                                                                          */
    int32_t B, K, T, cs, iter_n, reserved;
    double lo[MPOPIS_ENV_MAX_ACTION], hi[MPOPIS_ENV_MAX_ACTION];      /* action_space(env) per action                   */
} mpopis_env_rollout_args;

typedef struct {
    uint64_t x;         /* double [B][SS]  resident env state (stepped in place; read only by the query kernel)               */
    uint64_t t, done;   /* int32  [B]                                                                                         */
    uint64_t action;    /* const double [B][AS]   (step kernel)                                                               */
    uint64_t reward;    /* double [B] or 0        out                                                                         */
    uint64_t status;    /* int32 [B] or 0         MPOPIS_ENV_ERR_ACTION is raised for an action outside [lo, hi] (step kernel) */
    uint64_t alive;     /* const int32 [B] or 0   slots with alive == 0 are skipped (step kernel)                             */
    uint64_t within;    /* int32 [B] or 0         out: 1 (query kernel)                                                       */
    uint64_t params;    /* const double [NP]                                                                                  */
    int32_t B, reserved;
    double lo[MPOPIS_ENV_MAX_ACTION], hi[MPOPIS_ENV_MAX_ACTION];
} mpopis_env_step_args;

/* Arguments of the table kernels (MPOPIS_DEFINE_ENV_TABLE): the fields above, then the table. */
typedef struct {
    mpopis_env_rollout_args r;
    uint64_t table;         /* const double [ntab], or [B][table_stride] when every slot has its own; 0 when ntab == 0 */
    int64_t table_stride;   /* doubles from one slot's table to the next; 0: one table shared by all slots              */
    int32_t ntab, pad;
} mpopis_env_rollout_tab_args;

typedef struct {
    mpopis_env_step_args s;
    uint64_t table;
    int64_t table_stride;
    int32_t ntab, pad;
} mpopis_env_step_tab_args;

#define MPOPIS_ENV_CHECK_SIZES_(SS, AS, NP)                                                                            \
    static_assert((SS) >= 1 && (SS) <= MPOPIS_ENV_MAX_STATE, "MPOPIS_DEFINE_ENV: state size must be 1..64");           \
    static_assert((AS) >= 1 && (AS) <= MPOPIS_ENV_MAX_ACTION, "MPOPIS_DEFINE_ENV: action size must be 1..16");         \
    static_assert((NP) >= 0 && (NP) <= MPOPIS_ENV_MAX_PARAMS, "MPOPIS_DEFINE_ENV: parameter count must be 0..64");

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MPOPIS_ENV_FN __host__ __device__ __forceinline__

namespace mpopis_env {

/* U, U_orig, gvec, the parameters and the start state are the same for every lane of a wave and are not written while a rollout kernel
 * runs: read through the constant address space they arrive by scalar loads, off the vector memory path that carries E. */
typedef const __attribute__((address_space(4))) double* uniform_f64;
typedef const __attribute__((address_space(4))) int32_t* uniform_i32;
__device__ __forceinline__ uniform_f64 as_uniform_f64(uint64_t a) { return (uniform_f64)a; }
__device__ __forceinline__ uniform_i32 as_uniform_i32(uint64_t a) { return (uniform_i32)a; }
/* everything else is global memory (not the generic address space a plain pointer made from an integer would mean) */
typedef __attribute__((address_space(1))) double* global_f64;
typedef __attribute__((address_space(1))) int32_t* global_i32;
__device__ __forceinline__ global_f64 as_global_f64(uint64_t a) { return (global_f64)a; }
__device__ __forceinline__ global_i32 as_global_i32(uint64_t a) { return (global_i32)a; }

/* the user's two functions travel as template arguments: MPOPIS_DEFINE_ENV names them at file scope, where no name of this header can hide them */
typedef void (*step_fn)(double* s, int* t, int* done, const double* a, const double* p);
typedef double (*reward_fn)(const double* s, int t, int done, const double* p);
typedef void (*step_tab_fn)(double* s, int* t, int* done, const double* a, const double* p, const double* tab, int ntab);
typedef double (*reward_tab_fn)(const double* s, int t, int done, const double* p, const double* tab, int ntab);

/* One body per kernel serves both kinds of env: it is instantiated on the two functions themselves and calls them by their type. */
template <class F> struct takes_table { static constexpr bool value = false; };
template <> struct takes_table<step_tab_fn> { static constexpr bool value = true; };
template <> struct takes_table<reward_tab_fn> { static constexpr bool value = true; };

/* get_model_controls' clamp (src/utils.jl:55-67); NaN passes through */
__device__ __forceinline__ double clamp(double v, double lo, double hi) { return v > hi ? hi : (v < lo ? lo : v); }

/* Per-slot error codes merge by precedence (mpopis.h: HIP > ACTION > NOT_PD > NUMERIC): ACTION replaces 0, NOT_PD (-2) and NUMERIC (-5). */
__device__ __forceinline__ void raise_action(global_i32 p) {
    int cur = *p;
    while (cur >= 0 || cur == -2 || cur == -5) {
        const int seen = atomicCAS((int*)p, cur, MPOPIS_ENV_ERR_ACTION);
        if (seen == cur) break;
        cur = seen;
    }
}

/* simulate_model + rollout_model for one slot's K samples: lane = one rollout, workgroups of WG threads (MPOPIS_DEFINE_ENV: one wave), grid (ceil(K / WG), B).
 *   V = pol.U + E[:, k]; control cost of the unclamped V; a = clamp(V); env(a); cost -= reward(env); logger     (:261-278, utils.jl:129-144)
 * State and action are registers (every loop over SS / AS is unrolled); E is read coalesced over k; everything else is wave-uniform. */
template <int SS, int AS, int NP, auto STEP, auto REWARD, int WG = 64, bool GATE = true>
__device__ __forceinline__ void rollout(const mpopis_env_rollout_args& a, const double* tab = nullptr, int ntab = 0) {
    const int b = blockIdx.y;
    if (GATE && a.active && !as_uniform_i32(a.active)[b]) return;             /* AIS early break (GATE = false: the caller has looked) */
    const int K = a.K, T = a.T;
    const int k = blockIdx.x * WG + threadIdx.x;
    const bool valid = k < K;
    const int kk = valid ? k : K - 1;                                          /* idle lanes duplicate the last sample and do not store */
    const size_t cs = (size_t)AS * T;
    const uniform_f64 x0 = as_uniform_f64(a.x0) + (size_t)b * SS;
    const uniform_f64 Ub = as_uniform_f64(a.Ucur) + (size_t)b * cs;
    const uniform_f64 Uo = as_uniform_f64(a.Uorig) + (size_t)b * cs;
    const uniform_f64 gv = as_uniform_f64(a.gvec) + (size_t)b * cs;
    const bool has_g = a.gvec != 0;
    const double* p = (const double*)as_uniform_f64(a.params);
    const global_f64 Eb = as_global_f64(a.E) + (size_t)b * cs * K + kk;
    const global_f64 tr = as_global_f64(a.traj) + ((size_t)b * K + kk) * ((size_t)SS * T);
    const bool log = a.traj != 0 && valid;
    double s[SS];
#pragma unroll
    for (int i = 0; i < SS; ++i) s[i] = x0[i];
    int t_env = a.t0 ? as_uniform_i32(a.t0)[b] : 0, done = a.done0 ? as_uniform_i32(a.done0)[b] : 0;
    double cost = 0.0, cc = 0.0;
    for (int t = 0; t < T; ++t) {
        double act[AS];
        bool nan_action = false;
#pragma unroll
        for (int j = 0; j < AS; ++j) {
            const size_t r = (size_t)t * AS + j;
            const double v = Ub[r] + Eb[r * K];
            if (has_g) cc += gv[r] * (v - Uo[r]);                              /* gamma U_orig' Sigma^-1 (V - U_orig), :272 */
            act[j] = clamp(v, a.lo[j], a.hi[j]);
            nan_action |= act[j] != act[j];
        }
        /* a NaN action: RL.jl's act! asserts `a in action_space(env)` and the rollout dies there.  A reward need not look at the state's
         * values, so the cost is poisoned here: a non-finite cost is what raises MPOPIS_ERR_ACTION when the weights are formed */
        if (nan_action) cost = NAN;
        if constexpr (takes_table<decltype(STEP)>::value) {
            STEP(s, &t_env, &done, act, p, tab, ntab);
            cost -= REWARD(s, t_env, done, p, tab, ntab);
        } else {
            STEP(s, &t_env, &done, act, p);
            cost -= REWARD(s, t_env, done, p);                                /* utils.jl:138 */
        }
        if (log) {                                                             /* trajectories[k][t, :] utils.jl:140 */
#pragma unroll
            for (int i = 0; i < SS; ++i) tr[(size_t)i * T + t] = s[i];
        }
    }
    if (valid) as_global_f64(a.cost)[(size_t)b * K + k] = cost + cc;
    /* the slot's first lane records the iteration (last: a lane-dependent branch ahead of the loop would cost the slot offsets their uniformity) */
    if (a.iters && blockIdx.x == 0 && threadIdx.x == 0) as_global_i32(a.iters)[b] = a.iter_n;
}

/* MPOPIS_DEFINE_ENV_TABLE: four waves per workgroup.  LDS form: the workgroup copies the slot's table into dynamic LDS (ntab * 8 bytes, sized at
 * launch: a small table costs no occupancy), coalesced and with eight loads in flight per thread; after the one barrier, waves without a sample
 * leave.  Global form: the table is wave-uniform and not written while the kernel runs (mpopis_set_env_table waits for the handle's streams),
 * so it is read like the parameters: uniform indices by scalar loads, per-lane indices by vector loads. */
template <int SS, int AS, int NP, bool LDS, step_tab_fn STEP, reward_tab_fn REWARD>
__device__ __forceinline__ void rollout_tab(const mpopis_env_rollout_tab_args& a) {
    constexpr int WG = MPOPIS_ENV_TABLE_THREADS;
    const int b = blockIdx.y;
    if (a.r.active && !as_uniform_i32(a.r.active)[b]) return;                 /* the whole workgroup, ahead of the barrier */
    const int ntab = a.ntab;
    if constexpr (LDS) {
        extern __shared__ double mpopis_env_tab_lds[];
        const global_f64 src = as_global_f64(a.table) + (size_t)b * a.table_stride;
        const int tid = threadIdx.x;
        for (int e0 = tid; e0 < ntab; e0 += WG * 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[min(e0 + u * WG, ntab - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (e0 + u * WG < ntab) mpopis_env_tab_lds[e0 + u * WG] = v[u];
        }
        __syncthreads();
        if ((int)(threadIdx.x & ~63u) >= a.r.K - WG * (int)blockIdx.x) return;         /* a wave with no sample at all */
        rollout<SS, AS, NP, STEP, REWARD, WG, false>(a.r, mpopis_env_tab_lds, ntab);
    } else {
        if ((int)(threadIdx.x & ~63u) >= a.r.K - WG * (int)blockIdx.x) return;
        rollout<SS, AS, NP, STEP, REWARD, WG, false>(a.r, (const double*)(as_uniform_f64(a.table) + (size_t)b * a.table_stride), ntab);
    }
}

/* the cold kernels read a slot's table from global memory (one lane per slot: nothing to stage for) */
__device__ __forceinline__ const double* slot_table(uint64_t table, int64_t stride, int b) { return (const double*)(as_global_f64(table) + (size_t)b * stride); }

/* env(action); reward(env) for the B resident envs, one lane per slot */
template <int SS, int AS, int NP, auto STEP, auto REWARD>
__device__ __forceinline__ void env_step(const mpopis_env_step_args& a, uint64_t table = 0, int64_t table_stride = 0, int ntab = 0) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    if (a.alive && !as_global_i32(a.alive)[b]) return;
    const double* p = (const double*)as_uniform_f64(a.params);
    const global_f64 ab = as_global_f64(a.action) + (size_t)b * AS;
    double act[AS];
    bool inside = true;
#pragma unroll
    for (int j = 0; j < AS; ++j) { act[j] = ab[j]; inside &= act[j] >= a.lo[j] && act[j] <= a.hi[j]; }
    if (!inside && a.status) raise_action(as_global_i32(a.status) + b);        /* "Action is not in action space" (NaN included) */
    const global_f64 xb = as_global_f64(a.x) + (size_t)b * SS;
    double s[SS];
#pragma unroll
    for (int i = 0; i < SS; ++i) s[i] = xb[i];
    int t = as_global_i32(a.t)[b], done = as_global_i32(a.done)[b];
    if constexpr (takes_table<decltype(STEP)>::value) STEP(s, &t, &done, act, p, slot_table(table, table_stride, b), ntab);
    else STEP(s, &t, &done, act, p);
#pragma unroll
    for (int i = 0; i < SS; ++i) xb[i] = s[i];
    as_global_i32(a.t)[b] = t; as_global_i32(a.done)[b] = done;
    if (a.reward) {
        if constexpr (takes_table<decltype(REWARD)>::value) as_global_f64(a.reward)[b] = REWARD(s, t, done, p, slot_table(table, table_stride, b), ntab);
        else as_global_f64(a.reward)[b] = REWARD(s, t, done, p);
    }
}
/* reward(env) of the resident state without stepping */
template <int SS, int AS, int NP, auto STEP, auto REWARD>
__device__ __forceinline__ void env_query(const mpopis_env_step_args& a, uint64_t table = 0, int64_t table_stride = 0, int ntab = 0) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const double* p = (const double*)as_uniform_f64(a.params);
    const global_f64 xb = as_global_f64(a.x) + (size_t)b * SS;
    double s[SS];
#pragma unroll
    for (int i = 0; i < SS; ++i) s[i] = xb[i];
    if (a.reward) {
        const int t = as_global_i32(a.t)[b], done = as_global_i32(a.done)[b];
        if constexpr (takes_table<decltype(REWARD)>::value) as_global_f64(a.reward)[b] = REWARD(s, t, done, p, slot_table(table, table_stride, b), ntab);
        else as_global_f64(a.reward)[b] = REWARD(s, t, done, p);
    }
    if (a.within) as_global_i32(a.within)[b] = 1;
}

}  /* namespace mpopis_env */

/* The engine finds the kernels and the constant by these names: {sdk version, SS, AS, NP}. */
#define MPOPIS_DEFINE_ENV(SS, AS, NP, STEP, REWARD)                                                                                          \
    MPOPIS_ENV_CHECK_SIZES_(SS, AS, NP)                                                                                                      \
    extern "C" __device__ __attribute__((used)) const int32_t mpopis_env_abi[4] = {MPOPIS_ENV_SDK_VERSION, (SS), (AS), (NP)};                \
    extern "C" __global__ void __launch_bounds__(64) mpopis_env_rollout(mpopis_env_rollout_args a) {                                         \
        mpopis_env::rollout<(SS), (AS), (NP), STEP, REWARD>(a);                                                                              \
    }                                                                                                                                        \
    extern "C" __global__ void __launch_bounds__(64) mpopis_env_step(mpopis_env_step_args a) {                                               \
        mpopis_env::env_step<(SS), (AS), (NP), STEP, REWARD>(a);                                                                             \
    }                                                                                                                                        \
    extern "C" __global__ void __launch_bounds__(64) mpopis_env_query(mpopis_env_step_args a) {                                              \
        mpopis_env::env_query<(SS), (AS), (NP), STEP, REWARD>(a);                                                                            \
    }

/* An env with a table: the same constant, a second one {table version, largest table the LDS kernel stages} -- its presence tells the engine that
 * the env takes a table -- and four kernels under names of their own. */
#define MPOPIS_DEFINE_ENV_TABLE(SS, AS, NP, STEP, REWARD)                                                                                    \
    MPOPIS_ENV_CHECK_SIZES_(SS, AS, NP)                                                                                                      \
    extern "C" __device__ __attribute__((used)) const int32_t mpopis_env_abi[4] = {MPOPIS_ENV_SDK_VERSION, (SS), (AS), (NP)};                \
    extern "C" __device__ __attribute__((used)) const int32_t mpopis_env_table_abi[2] = {MPOPIS_ENV_TABLE_VERSION, MPOPIS_ENV_TABLE_LDS_DOUBLES};  \
    extern "C" __global__ void __launch_bounds__(MPOPIS_ENV_TABLE_THREADS) mpopis_env_rollout_tab(mpopis_env_rollout_tab_args a) {           \
        mpopis_env::rollout_tab<(SS), (AS), (NP), true, STEP, REWARD>(a);                                                                    \
    }                                                                                                                                        \
    extern "C" __global__ void __launch_bounds__(MPOPIS_ENV_TABLE_THREADS) mpopis_env_rollout_gtab(mpopis_env_rollout_tab_args a) {          \
        mpopis_env::rollout_tab<(SS), (AS), (NP), false, STEP, REWARD>(a);                                                                   \
    }                                                                                                                                        \
    extern "C" __global__ void __launch_bounds__(64) mpopis_env_step_tab(mpopis_env_step_tab_args a) {                                       \
        mpopis_env::env_step<(SS), (AS), (NP), STEP, REWARD>(a.s, a.table, a.table_stride, a.ntab);                                            \
    }                                                                                                                                        \
    extern "C" __global__ void __launch_bounds__(64) mpopis_env_query_tab(mpopis_env_step_tab_args a) {                                      \
        mpopis_env::env_query<(SS), (AS), (NP), STEP, REWARD>(a.s, a.table, a.table_stride, a.ntab);                                            \
    }

#else  /* host compiler: the env as two C functions */
#define MPOPIS_ENV_FN static inline
#define MPOPIS_DEFINE_ENV(SS, AS, NP, STEP, REWARD)                                                                                          \
    MPOPIS_ENV_CHECK_SIZES_(SS, AS, NP)                                                                                                      \
    extern "C" const int32_t mpopis_env_abi[4] = {MPOPIS_ENV_SDK_VERSION, (SS), (AS), (NP)};                                                 \
    extern "C" void mpopis_env_host_step(double* s, int* t, int* done, const double* a, const double* p) { STEP(s, t, done, a, p); }         \
    extern "C" double mpopis_env_host_reward(const double* s, int t, int done, const double* p) { return REWARD(s, t, done, p); }
#define MPOPIS_DEFINE_ENV_TABLE(SS, AS, NP, STEP, REWARD)                                                                                    \
    MPOPIS_ENV_CHECK_SIZES_(SS, AS, NP)                                                                                                      \
    extern "C" const int32_t mpopis_env_abi[4] = {MPOPIS_ENV_SDK_VERSION, (SS), (AS), (NP)};                                                 \
    extern "C" const int32_t mpopis_env_table_abi[2] = {MPOPIS_ENV_TABLE_VERSION, MPOPIS_ENV_TABLE_LDS_DOUBLES};                             \
    extern "C" void mpopis_env_host_step(double* s, int* t, int* done, const double* a, const double* p, const double* tab, int ntab) {      \
        STEP(s, t, done, a, p, tab, ntab);                                                                                                   \
    }                                                                                                                                        \
    extern "C" double mpopis_env_host_reward(const double* s, int t, int done, const double* p, const double* tab, int ntab) {               \
        return REWARD(s, t, done, p, tab, ntab);                                                                                             \
    }
#endif

#endif  /* MPOPIS_ENV_H */
