// engine.h -- internal declarations shared by the HIP translation units of libmpopis_hip.so.
//
// Data layout in HBM: per handle, B trial slots, every per-slot buffer [B][...], FP64 unless its type says otherwise.  The record of the buffers
// and their per-slot extents is the declaration table in create_handle (engine_api.hip), from which the slot views are derived too.
//   E      [B][cs][K]     noise, ROW-MAJOR BY CONTROL ROW (K fastest).  The reference stores E as
//                         cs x K column-major (sample k contiguous); here lanes = samples, so the
//                         transpose makes every rollout-kernel load and every reduction over k
//                         coalesced.  The C ABI transposes on upload/download.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <string>
#include <vector>
#include "../../include/mpopis.h"
#include "../../include/mpopis_env.h"
#include "car_dynamics.h"

namespace mpopis {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE setting: a process that keeps one handle per GPU
//  must configure each large-LDS kernel once on every device it launches on.
// `seen` = the call site's static bit mask of configured device ordinals (atomic: handles may live on different threads).
inline void ensure_dyn_lds(const void* fn, int bytes, std::atomic<unsigned long long>& seen) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const unsigned long long bit = 1ull << (dev & 63);
    if (seen.load(std::memory_order_relaxed) & bit) return;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    seen.fetch_or(bit, std::memory_order_relaxed);
}

// Wave issue priority (s_setprio 0..3, default 0): the latency-bound kernels of the per-slot chain raise it.  Whenever kernels of
// different streams share the chip (the part-chain schedule of policy_step_enqueue, the side chains of the CMA update, several
// handles on one device), the short links then win the SIMD issue arbitration against long-running throughput waves instead of being
// starved by them (measured: k_weights 9 us alone, 155 us next to a rollout kernel at equal priority).
#define MPOPIS_HI_PRIO() __builtin_amdgcn_s_setprio(3)

constexpr int kMaxCars = MPOPIS_MAX_CARS;      // include/mpopis.h; the rollout kernels are instantiated for 1..8 cars
constexpr int kMaxAs = 2 * kMaxCars;
static_assert(kMaxAs == MPOPIS_ENV_MAX_ACTION && MPOPIS_ENV_ERR_ACTION == MPOPIS_ERR_ACTION, "include/mpopis_env.h restates these");

// A caller-supplied env (MPOPIS_ENV_CUSTOM, include/mpopis_env.h): the loaded code object, its three kernels and the device parameter
// buffer.  Owned by the handle; the launchers below reach it through EnvDesc::custom (a HOST pointer: kernels never look at it).
// An env built with MPOPIS_DEFINE_ENV_TABLE (has_table) has four kernels instead -- rollout is then the LDS form, rollout_gtab the global one --
// and the table mpopis_set_env_table uploaded: ntab doubles per slot, shared (table_stride 0) or one per slot (table_stride == ntab).
struct CustomEnv {
    hipModule_t module = nullptr;
    hipFunction_t rollout = nullptr, step = nullptr, query = nullptr, rollout_gtab = nullptr;
    double* d_params = nullptr;
    int nparams = 0;
    bool has_table = false;
    int table_lds_doubles = 0;        // largest table the code object's LDS kernel stages (mpopis_env_table_abi[1])
    double* d_table = nullptr;        // the buffer (not in mpopis_handle::allocs: it grows); table_cap doubles
    size_t table_cap = 0;
    const double* table_view = nullptr;   // the table of the handle's first slot: d_table, moved with the slot views (shift_slots); null while ntab == 0
    int64_t table_stride = 0;
    int ntab = 0;
};

constexpr int kEnvTableLdsMaxDoubles = 8192;      // 64 KiB of dynamic LDS: what a kernel may be launched with without its limit being raised

struct EnvDesc {
    int kind;        // MPOPIS_ENV_*
    int ncars;
    int ss, as;
    CarParams car;
    McParams mc;
    CpParams cp;
    Track track;     // device pointers
    double lo[kMaxAs], hi[kMaxAs];
    const CustomEnv* custom;   // MPOPIS_ENV_CUSTOM only
};

// dynamic LDS the rollout kernels' stage_track fills for a track of P points with W-wide neighbour tables (kernels_rollout.hip): the ring table and its
// certificates, with `all` also x, y, w, |q|^2 and the neighbour tables
inline size_t track_lds_bytes(int P, int W, bool all) {
    return (size_t)(kRingStride * (P + 2 * kRingPad) + 2 * P) * sizeof(double) + (all ? (size_t)4 * P * sizeof(double) + (size_t)P * (W + 1) * (sizeof(double) + sizeof(int)) : 0);
}

// The env of a handle whose trial slots differ (mpopis_set_env_params_slots / mpopis_set_tracks): [B] arrays of ready-made
// parameter structs and track descriptors that move with the slot views.  A null pointer: that part of the shared EnvDesc holds in every slot.
// lds_all / lds_ring: track_lds_bytes of the handle's LARGEST track with every table / the ring table only -- every slot of a launch runs one kernel.
struct SlotEnv {
    const CarParams* car = nullptr;
    const McParams* mc = nullptr;
    const CpParams* cp = nullptr;
    const Track* track = nullptr;
    size_t lds_all = 0, lds_ring = 0;
    // A fleet (mpopis_set_env_params_cars): [B][ncars] structs, car c of slot b at cars[b * ncars + c]; null: no fleet.  With it
    // `track` is set too and `car` is null: the rollout runs the one-wave-per-car body (kernels_rollout_fleet.hip), the small kernels read cars[].
    const CarParams* cars = nullptr;
    bool any() const { return car || mc || cp || track || cars; }
};
// lds_all / lds_ring of a SlotEnv from the HOST copy of its [n] track descriptors (mpopis_set_tracks; tools/kbench_rollout.hip forms its SlotEnv
// through this too, so a harness launch gets the LDS size a handle's launch gets)
inline void slot_tracks_lds(const Track* host, size_t n, size_t* lds_all, size_t* lds_ring) {
    size_t all = 0, ring = 0;
    for (size_t b = 0; b < n; ++b) {
        const size_t a = track_lds_bytes(host[b].P, host[b].nbrw, true), r = track_lds_bytes(host[b].P, host[b].nbrw, false);
        all = a > all ? a : all; ring = r > ring ? r : ring;
    }
    *lds_all = all; *lds_ring = ring;
}
// the small kernels (env step / query, harness bookkeeping, the simple envs' rollout) overwrite their by-value EnvDesc with slot b's parts
__device__ __forceinline__ void slot_env_into(EnvDesc& env, const SlotEnv& se, int b) {
    if (se.car) env.car = se.car[b];
    if (se.mc) env.mc = se.mc[b];
    if (se.cp) env.cp = se.cp[b];
    if (se.track) env.track = se.track[b];
}

// the two scalar-action classic-control envs share one code path ("simple" envs): ss = 2 or 4, as = 1
MP_HD void simple_env_step(const EnvDesc& env, double* s, int* t, int* done, double a) {
    if (env.kind == MPOPIS_ENV_CARTPOLE) cp_step(env.cp, s, t, done, a);
    else mc_step(env.mc, s, t, done, a);
}
MP_HD double simple_env_reward(const EnvDesc& env, const double* s, int done) {
    return env.kind == MPOPIS_ENV_CARTPOLE ? cp_reward(done) : mc_reward(env.mc, s, done);
}

// Arguments of the fused rollout kernel (== simulate_model + rollout_model + env step + reward)
struct RolloutArgs {
    EnvDesc env;
    int B, K, T, cs;
    const double* x0;      // [B][ss]   (MountainCar)
    const double* x0ext;   // [B][ncars][kCarExt] car start states + sin/cos + nearest track point (launch_extend_state)
    const int* t0;         // [B] (MountainCar step counter) or nullptr
    const int* done0;      // [B]
    const double* Ucur;    // [B][cs]
    const double* Uorig;   // [B][cs]
    const double* E;       // [B][cs][K]   (G-variants)  /  [B][T*as][K] (:mppi, same thing)
    const double* gvec;    // [B][cs] = (γ U_orig' Σ_inv) or nullptr when γ == 0
    double* cost;          // [B][K]
    double* traj;          // nullptr or [B][K][ss][T] (Julia (T x ss) column-major per sample)
    const int* active;     // nullptr or [B]: slots with active==0 are skipped (AIS early break)
    int* iters;            // nullptr or [B]: iters[b] = iter_n for every slot this launch works on (AIS iterations executed)
    int iter_n;
    unsigned long long* cmin;   // nullptr or [B]: running minimum of the slot's costs as an order-preserving key (cost_key), car kernels only
    int* status;                // with cmin: a non-finite cost sets MPOPIS_ERR_ACTION here (what k_weights reports when it runs)
    int share = 1;              // launches of this size in flight at once (multi-stream schedule): kernel choice goes by the chip's total load
    SlotEnv senv;               // per-slot env (last: the kernel-argument offsets of everything above are those of a handle without one)
};
// order-preserving map double -> uint64 (unsigned comparison == numeric comparison, NaN sorts last) for atomicMin on costs.  Every NaN maps to the key
// of the positive quiet NaN: the rollout's cost -= reward leaves a NaN with the sign bit SET, whose raw pattern would sort before every number.
__host__ __device__ __forceinline__ unsigned long long cost_key(double v) {
    unsigned long long u; memcpy(&u, &v, 8);
    if (v != v) return 0xfff8000000000000ull;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double cost_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v; memcpy(&v, &u, 8);
    return v;
}

// Per-slot error codes merge by PRECEDENCE, on the device like on the host (include/mpopis.h: HIP > ACTION > NOT_PD > NUMERIC -- the codes of
// ABI version 1 keep their order and the newer MPOPIS_ERR_NUMERIC never hides one of them).  Every kernel that reports into status[b] goes
// through status_raise: a plain atomicMin would let an earlier NUMERIC (-5) mask a later NOT_PD (-2) / ACTION (-3) of the same slot.
__host__ __device__ __forceinline__ int status_rank(int c) {
    return c == MPOPIS_ERR_HIP ? 4 : c == MPOPIS_ERR_ACTION ? 3 : c == MPOPIS_ERR_NOT_PD ? 2 : c == MPOPIS_ERR_NUMERIC ? 1 : c < 0 ? 5 : 0;
}
__device__ __forceinline__ void status_raise(int* p, int code) {
    int cur = *p;
    while (status_rank(code) > status_rank(cur)) {
        const int seen = atomicCAS(p, cur, code);
        if (seen == cur) break;
        cur = seen;
    }
}

// A quantity that is one number for the whole batch or one per trial slot (mpopis_set_slot_hyper).  A kernel that consumes one is a template
// over the type of that one argument -- double, or const double* indexed by the slot -- so both forms come from one body.
__device__ __forceinline__ double slot_val(double v, int) { return v; }
__device__ __forceinline__ double slot_val(const double* v, int b) { return v[b]; }
struct SlotVal { double v; const double* per_slot; };   // per_slot == nullptr: v in every slot; else per_slot[b] (a [B] device array that moves with the slot views)

// The kernel launch_rollout picks, as a pure function of the launch's arguments (the launcher switches on it; tools/kbench_rollout.hip writes it into
// its result so that a test written for one form fails when a threshold moves): the body, whether the trajectory logger is on, whether every track
// table is staged in LDS (car bodies: otherwise the ring table only; custom body: the env's data table goes to the code object's LDS kernel), and the dynamic LDS of one workgroup.  MPOPIS_ROLLOUT_DUO is read once per process.
enum RolloutBody { ROLLOUT_SIMPLE2 = 0, ROLLOUT_SIMPLE4 = 1, ROLLOUT_CUSTOM = 2, ROLLOUT_TWO_WAVE = 3, ROLLOUT_ONE_WAVE_SPB1 = 4, ROLLOUT_ONE_WAVE_SPB4 = 5,
                   ROLLOUT_FLEET = 6 /* one wave per car of 64 samples: a handle whose cars carry their own parameters */ };
struct RolloutForm { RolloutBody body = ROLLOUT_SIMPLE2; bool log = false, tlds = false; size_t lds = 0; };
RolloutForm rollout_form(const RolloutArgs& a);
// kernels_rollout_fleet.hip: static LDS of the fleet body for ncars cars (the position exchange [2][ncars][2][64] doubles + the per-car action bounds),
// which rollout_form counts against the default 64 KB, and its launcher (false: no kernel for this car count)
constexpr size_t fleet_static_lds(int ncars) { return (size_t)ncars * (2 * 2 * 64 + 4) * sizeof(double); }
bool launch_car_rollout_fleet(const RolloutArgs& a, const RolloutForm& f, hipStream_t st);
bool launch_rollout(const RolloutArgs& a, hipStream_t s, hipError_t* custom_err = nullptr);      // false: nothing launched -- no rollout kernel for this env, or the custom env's launch failed (*custom_err says why)
// kernels_risk.hip (scenario handles): cost[b][k] = the risk aggregate (MPOPIS_RISK_*: kind, tail in 1..M, theta) of the M
// scenario costs sc[m * pstride + b * K + k]; slots with active == 0 are skipped; cmin / status (nullable) as in the rollout's epilogue.
// false: no kernel for this M (outside 1..MPOPIS_MAX_SCENARIOS)
bool launch_risk(const double* sc, size_t pstride, int M, double* cost, int B, int K, int kind, int tail, double theta, const int* active,
                 unsigned long long* cmin, int* status, hipStream_t s);
void launch_extend_state(const double* x, double* xext, int B, int ncars, hipStream_t s, const Track& tk, const Track* slot_tk = nullptr /* [B], or null: tk in every slot */);
// (iters_acc: per-slot running sum of the iteration counts of earlier steps, folded in before iters is cleared; may be null)
void launch_step_begin(int* status, int* active, const int* alive, int* iters, const double* U, double* Uin, double* Ucur, int B, int cs,
                       const double* x, double* xext, int ncars, hipStream_t st, unsigned long long* cmin, const Track& tk, unsigned long long* iters_acc = nullptr, const Track* slot_tk = nullptr);

// compute_weights (utils.jl:79-86) per slot: w = exp(-(1/λ)(c-min c)) / Σ, given -1/λ
void launch_weights(const double* cost, double* w, int B, int K, SlotVal neg_inv_lambda, const int* active,
                    int* status, hipStream_t s, double* wsum = nullptr);
// which form of k_weights launch_weights runs for K samples (the workgroup size decides: the register form covers K <= 8 x blockDim)
enum WeightsForm { WEIGHTS_REG_256 = 0, WEIGHTS_REG_1024 = 1, WEIGHTS_3PASS_1024 = 2 };
int weights_block(int K);
WeightsForm weights_form(int K);

// out[b][r] = Σ_k w[b][k] * (E[b][r][k] + shift[b][r]) / (norm ? Σ_k w : 1)
void launch_wmean(const double* E, const double* w, const double* shiftA, const double* shiftB,
                  double* out, int B, int cs, int K, int normalize, const int* active, hipStream_t s);

// functor tail: wc = U + wn; control = clamp(wc[1:as]); roll U (utils.jl:88-101)
void launch_finalize_env(const double* wn, double* U, double* control, int B, int cs, int as, int T,
                         const EnvDesc& env, hipStream_t s);

// layout converters between the ABI's cs x K column-major and the engine's [cs][K]
void launch_transpose_in(const double* src_colmajor, double* dst_rows, int B, int cs, int K, hipStream_t s, size_t src_stride = 0 /* 0: cs*K */);
void launch_transpose_out(const double* src_rows, const double* shiftA, const double* shiftB,
                          double* dst_colmajor, int B, int cs, int K, hipStream_t s);

// real env step + reward for the resident envs
// (both return the launch status of a custom env's kernel; hipSuccess for the built-in envs, whose launches show in hipGetLastError)
hipError_t launch_env_step(const EnvDesc& env, double* x, int* t, int* done, const double* action,
                           double* reward, int* status, const int* alive, int B, hipStream_t s, const SlotEnv& senv = SlotEnv());

hipError_t launch_env_query(const EnvDesc& env, const double* x, const int* t, const int* done, double* reward, int* within, double* dist, double* beta, int B, hipStream_t s, const SlotEnv& senv = SlotEnv());

// kernels_harness.hip: the bookkeeping of the closed-loop trial harness (mpopis_run_trials).  hs [B][kH_N]: the per-slot accumulator (doubles)
enum { kH_rew = 0, kH_cnt, kH_lap, kH_prev_y, kH_trk, kH_beta, kH_crash, kH_vmean, kH_vmax, kH_bmean, kH_bmax,
       kH_lap0, kH_lap1, kH_lap2, kH_lap3, kH_rollouts, kH_N = 16 };
// state noise of the one-car env (car_example.jl:224-236): seeds == nullptr switches it off; rng_tab = the table of launch_rng_tab_init
struct StateNoise { double sx, sy, spsi; const uint64_t* seeds; const double* rng_tab; };
// hs = 0 (vmax = bmax = -inf), alive = 1
void launch_harness_init(double* hs, int* alive, int B, hipStream_t s);
// after env(act), for the slots with alive != 0: state noise, action log row `step` ([B][num_steps + 1][as], nullable), cnt += 1, rew += reward,
// rollouts += iters K, the car statistics, violation counters, lap counter; alive = 0 when the trial ends
void launch_harness_update(const EnvDesc& env, double* x, const int* done_env, const double* reward, const int* iters, double* hs, int* alive,
                           const double* control, double* actlog, int step, int num_steps, int laps, int K, int B, const StateNoise& nz,
                           const SlotEnv& senv, hipStream_t s);

// kernels_sample.hip
void launch_sample_normal(double* Z, int B, int cs, int K, int as, int mppi_order, const uint64_t* seeds,
                          uint32_t slo, uint32_t shi, const double* dscale, const int* active, hipStream_t s, const double* rng_tab);
// which kernel launch_sample_normal runs: four normals per Philox call (G order, 4 | cs), two (the members of a draw pair sit in adjacent rows: cs
// even in G order, as even in :mppi order), or one normal per thread
enum SampleNormalForm { SAMPLE_NORMAL_SINGLE = 0, SAMPLE_NORMAL_PAIR = 1, SAMPLE_NORMAL_QUAD = 2 };
SampleNormalForm sample_normal_form(int cs, int as, int mppi_order);
void launch_rng_tab_init(double* gtab, hipStream_t s);      // philox.h: kRngTabDoubles doubles (Box-Muller tables), once per handle
void launch_sample_resample_draws(int32_t* di, double* du, int B, int K, const uint64_t* seeds, uint32_t slo, uint32_t shi,
                                  const int* active, hipStream_t s);
// kernels_strat.hip: Z[b][r][k] = plain standard normals of the antithetic (kind MPOPIS_NOISE_ANTITHETIC) or Latin-hypercube (MPOPIS_NOISE_LHS,
// K <= 2^20) draw of (seed, step, iter); both orders; rows of inactive slots are not written
constexpr int kStratMaxK = 1 << 20;
void launch_sample_strat(double* Z, int B, int cs, int K, int as, int mppi_order, int kind, const uint64_t* seeds, uint32_t step, uint32_t iter,
                         const int* active, hipStream_t s, const double* rng_tab);


// Workspace of the cooperative ("cluster") kernels: several workgroups per matrix that exchange through global memory and therefore need
// to be co-resident.  Co-residency is planned (grid <= coop_max_workgroups() of the device) but never assumed: every wait is bounded, a
// cluster that gives up marks its slot in `redo`, counts the event in `timeouts`, and the launch is followed by the one-workgroup kernel
// predicated on `redo` -- a slot is only ever reported failed by the kernel that needs no partner.  The host disables the cooperative
// kernels of a handle after the first recorded time-out (sync_status), so a device that cannot hold the clusters (partitioned GPU, many
// handles / processes) pays the bounded wait once.
struct CoopCtx {
    unsigned long long* flags = nullptr;   // potrf: [B][ceil(n/16)] panel flags; Lanczos: exchange granules (invsqrt_coop_words)
    unsigned long long* epoch = nullptr;   // host-side launch counter (tags)
    int* redo = nullptr;                   // [B] slot must be recomputed by the one-workgroup kernel (set on a time-out, cleared by the fall-back)
    int* timeouts = nullptr;               // [1] time-outs since the handle was created
    int share = 1;                         // cluster launches of this handle that may be in flight at once (multi-stream schedule): each gets 1/share of the device
    bool usable() const { return flags && epoch && redo && timeouts; }
};
int coop_max_workgroups();                 // per current device: its CU count (one 150 KB-LDS workgroup per CU)
// bounded wait of a cluster member for its partners in ticks of the 100 MHz wall clock (default 1 s; MPOPIS_COOP_WAIT_US) and the test hook
// MPOPIS_COOP_TEST_DROP=1: the last workgroup of every cluster leaves at once, i.e. every cluster times out and is redone by the fall-back
unsigned long long coop_wait_ticks();
int coop_test_drop();

// kernels_linalg.hip
size_t potrf_coop_flag_words(int B, int n);
// panel (nullable, n <= kPanelRows): second copy of the factor in the staging layout of the fused sampler (potrf_panel_doubles(n) per slot)
constexpr int kPanelRows = 128;
size_t potrf_panel_doubles(int n);
// The kernel launch_potrf picks, as a pure function of the launch's shape (the launcher switches on it; tools/kbench_dense.hip writes it into its
// result so that a test written for one form fails when a threshold moves).  G, S, coop_lds: cooperative form only (workgroups per matrix, panels
// per ownership block, dynamic LDS of one workgroup).  MPOPIS_POTRF_REG / _G / _S and MPOPIS_COOP_MAX_WG are read once per process.
enum PotrfKernel { POTRF_LDS = 0, POTRF_REG = 1, POTRF_COOP = 2 /* followed by the one-workgroup kernel on the slots marked in redo */, POTRF_GLOBAL = 3 };
struct PotrfForm { PotrfKernel kernel = POTRF_GLOBAL; int G = 0, S = 0; size_t coop_lds = 0; };
PotrfForm potrf_form(int B, int n, bool coop_usable, int share = 1);
void launch_potrf(const double* A, size_t Astride, double* L, int B, int n, const double* scale, int* status, int* active, hipStream_t s,
                  const CoopCtx& coop = CoopCtx(), double* panel = nullptr, size_t pstride = 0);
void launch_chol_solve_gvec(const double* L, size_t Lstride, const double* Uorig, SlotVal gamma, double* g, int B, int n, const int* active, hipStream_t s,
                            const double* inv_scale2 = nullptr);      // L = chol(Σ) while the proposal is MvNormal(s²Σ) (:cmamppi): g = (s²Σ)^-1 γU = Σ^-1 γU / s²
void launch_gvec_from_inv(const double* Sinv, const double* Uorig, SlotVal gamma, double* g, int B, int n, hipStream_t s);
// :nesmppi (kernels_nes.hip; kernels_invsqrt.hip for the square root)
void launch_nes_break(const double* cost, int B, int K, int* active, int* status, hipStream_t s);
size_t nes_scatter_workspace_doubles(int B, int cs, int ksplit);
void launch_nes_scatter(const double* E, const double* cost, double* part, double* M, double* g, double* Csum, int B, int cs, int K, int ksplit,
                        const int* active, hipStream_t s);
void launch_nes_potri(const double* L, size_t Lstride, double* X, double* S, int B, int n, const int* active, hipStream_t s);
void launch_nes_update(const double* E, const double* cost, double* part, int ksplit, const double* S, size_t Sstride, double* M, double* T,
                       double* g, double* Csum, const double* Ain, size_t Astride, double* Aout, double* Sig, double* U,
                       int B, int cs, int K, SlotVal a_scale /* -sf / K² */, SlotVal u_scale /* sf / K */, const int* active, hipStream_t s);
void launch_sym_sqrt(const double* A, double* M, double* V, double* out, int* status, int n, hipStream_t s);
// kernels_mfma.hip
void launch_trmm_LZ_mfma(const double* L, size_t Lstride, const double* Z, double* E, int B, int n, int K, const int* active, hipStream_t s,
                         const double* oscale2 = nullptr);      // oscale2[b] (nullable): E = sqrt(oscale2[b]) L Z
bool sample_trmm_fusable(int n);
bool launch_sample_trmm_fused(const double* L, size_t Lstride, double* E, int B, int n, int K, const uint64_t* seeds, uint32_t slo, uint32_t shi,
                              const int* active, hipStream_t s, const double* rng_tab, const double* panel, size_t pstride, const double* oscale2 = nullptr);
size_t wcov_mfma_workspace_doubles(int B, int cs, int ksplit);
int wcov_max_cs();                         // largest cs the covariance scatter stages (:cemppi, :μΣaismppi, :pmcmppi)
void launch_wcov_mfma(const double* X, const double* w, const int32_t* idx, int m, const double* mu, double* S, double* part,
                      int B, int cs, int K, int ksplit, int sel_batch /* batch the kernel choice goes by: the handle's whole batch when this launch covers one part-chain of it (0: B; -1: compact form, see mpopis_handle::wcov_sel_batch) */,
                      double den, double ridge, const int* active, hipStream_t s,
                      const double* rscale = nullptr, double* mu_out = nullptr, double* u_add = nullptr, const double* wsum = nullptr,
                      const double* cost = nullptr, unsigned long long* cmin = nullptr, double neg_inv_lambda = 0.0, const double* mu_shift = nullptr);
bool wcov_weights_from_cost_ok(int cs, int K, int ksplit);
// which partial kernel launch_wcov_mfma runs (pair list with 64- / 16-column chunks, the 8-wave row form, the 8-wave tall form), whether it stages the
// fourth-moment rows (sq), the ones row (aug: the pass also yields μ) and the weights from the costs; MPOPIS_WCOV_ROWS is read once per process
enum WcovPartial { WCOV_PAIR64 = 0, WCOV_PAIR16 = 1, WCOV_ROWS = 2, WCOV_TALL = 3 };
struct WcovForm { WcovPartial partial; bool sq, aug, from_cost; };
int wcov_rows_env();
WcovForm wcov_form(int cs, int K, int m, int ksplit, int batch /* > 0, or -1: compact form */, bool has_rscale, bool has_idx, bool wants_mean, bool has_cost);
bool wcov_mfma_can_emit_mean(int cs);
void launch_inv_sd(const double* S, double* rs, int B, int cs, const int* active, hipStream_t s);
void launch_common_shrink(double* S, int B, int cs, int m, int oas, double ridge, const int* active, hipStream_t s);
void launch_fill_f64(double* p, double v, size_t n, hipStream_t s);
void launch_ss_shrink(double* S, const double* Q, double* rs_ws, int B, int cs, int m, double ridge, const int* active, hipStream_t s);
void launch_gather_cols(const double* X, const int32_t* idx, double* Xout, int B, int cs, int K, const int* active, hipStream_t s, double* shift = nullptr);
void launch_gather_mean(const double* X, const int32_t* idx, const double* cw, double* mu, int B, int cs, int K, int m, int divide,
                        const int* active, hipStream_t s);


void launch_gather_mean_strided(const double* X, const int32_t* idx, const double* cw, double* out, size_t out_stride, int B, int cs, int K, int m,
                                const int* active, hipStream_t s);

// kernels_ce.hip: the whole CE proposal update (elite mean, Σ_est covariance + ridge, pol.U += μ′) in one launch for small elite sets
bool ce_cov_small_ok(int cs, int m, int est);
bool ce_sort_fusable(int K);
void launch_ce_cov_small(const double* E, int32_t* order, double* mu, double* S, double* Ucur, int B, int cs, int K, int m, int est, double ridge,
                         int* active, hipStream_t s, const double* cost = nullptr /* non-null (K <= 256): also sortperm(cost) -> order and the elite early break */);
// engine_ais.hip: the same update for any elite set, as the sequence gather-mean, scatter (twice for :ss / :lw), shrinkage, and -- in a call of its
// own, which the handle times apart -- pol.U += μ′ (d_gvec is free as rs there: γ's row is rebuilt per iteration)
void launch_ce_cov_general(const double* E, const int32_t* order, double* mu, double* Sig, double* tmpS, double* rs, double* part,
                           int B, int cs, int K, int m_elite, int ksplit, int sel_batch, int est, double ridge, const int* active, hipStream_t s);
void launch_add_active(const double* x, double* y, int B, int n, const int* active, hipStream_t s);      // y[b] += x[b] for active slots

// kernels_select.hip
void launch_sortperm(const double* cost, int32_t* order, int B, int K, int m_elite, int* active, hipStream_t s,
                     double* skey = nullptr, int* done = nullptr);   // + elite early break; skey [B][K] / done [B] (zeroed): workspace of the chip-wide rank sort
void launch_alias_build(const double* w, double* accept, int32_t* alias, int B, int K, const int* active, hipStream_t s, int* need_ws = nullptr,
                        int32_t* stack_ws = nullptr /* B x 2K ints, needed when K > alias_lds_max_K() */);
int alias_lds_max_K();
// The kernel each launcher picks, as pure functions of the launch's shape (the launchers call them; tools/kbench_select.hip prints them so that a
// test written for one form fails when a threshold moves instead of silently testing another form).
//   have_ws: skey and done both given.  multi_enabled / par_enabled: MPOPIS_SORT_MULTI / MPOPIS_ALIAS_PAR (default 1), read once per process.
enum SortForm { SORT_RANK = 0, SORT_LDS = 1, SORT_BITONIC4 = 2, SORT_BITONIC8 = 3, SORT_RANK_MULTI = 4, SORT_RANK_BIG = 5 };
enum AliasForm { ALIAS_SEQ_LDS = 0, ALIAS_SEQ_GLOBAL = 1, ALIAS_PAR_THEN_SEQ_LDS = 2 };
bool sortperm_multi_enabled();
bool alias_par_enabled();
SortForm sortperm_form(int B, int K, bool have_ws, bool multi_enabled);
AliasForm alias_build_form(int K, bool have_need_ws, bool par_enabled);
void launch_alias_sample(const double* accept, const int32_t* alias, const int32_t* di, size_t di_stride, const double* du,
                         int32_t* out, int32_t* log, size_t log_stride, int B, int K, const int* active, hipStream_t s);

// kernels_plan.hip (mpopis_get_plan): the top samples of a weight row in the order "weight descending, index ascending" (top <= min(K, MPOPIS_PLAN_MAX_TOP);
// idx / wsel [B][top]), then controls [B][cs] = Uin + wn and the noise block Eplan [B][cs][top + 1]: column 0 = wn, column j = E[:, idx[j-1]] + (Ucur - Uin)
// active (nullable, [B]): slots with active == 0 write nothing
void launch_plan_select(const double* w, int B, int K, int top, int32_t* idx, double* wsel, hipStream_t s, const int* active = nullptr);
void launch_plan_assemble(const double* E, const double* Ucur, const double* Uin, const double* wn, const int32_t* idx, int B, int cs, int K, int top,
                          double* controls, double* Eplan, hipStream_t s, const int* active = nullptr);

// kernels_trace.hip (mpopis_run_trials_traced): the per-step record of the closed loop, written straight into the ABI's
// slot-major arrays (S = num_steps + 1 entries per slot; any pointer may be null), and the reordering of the step-major plan buffers for the copy-out
struct TraceStepOut { double *states, *rewards, *dist, *beta; int32_t *iters, *within; };
// states[b][0] = x[b] for every slot
void launch_trace_start(const double* x, double* states, int B, int ss, int S, hipStream_t s);
// Slots whose step counter cnt[b * cnt_stride] equals step + 1 -- those that were alive during MPC step `step` -- record states[b][step + 1] = x[b],
// rewards / iters [b][step], and within / dist / beta [b][step] of x[b] as mpopis_env_query computes them (car env; other envs: within = 1)
void launch_trace_step(int env_kind, int ncars, int ss, const Track& tk, const Track* slot_tk, const double* x, const double* reward, const int* iters,
                       const double* cnt, int cnt_stride, int step, int S, const TraceStepOut& out, int B, hipStream_t s);
// out[b][j][0..per) = in[j][b][0..per) for j < J, b < B; elem_bytes 4 or 8
void launch_trace_reorder(const void* in, void* out, int B, int J, size_t per, int elem_bytes, hipStream_t s);

// kernels_cma.hip
// kernels_invsqrt.hip: y = A^-1/2 b (Lanczos + quadrature) and fro = tr(A^-1) = scale * ||L^-1||_F^2 with L = chol(scale * A)
constexpr size_t kInvsqrtPadDoubles = 512;
size_t invsqrt_workspace_doubles(int B, int n, int regions_per_slot = 1);
int invsqrt_coop_groups(int B, int n, int share = 1);      // workgroups per matrix the cooperative Lanczos would use for this batch (1: not cooperative)
int invsqrt_max_n();
size_t trtri_dinv_doubles(int B, int n);      // workspace: the inverses of the diagonal 16 x 16 blocks, [B][ceil(n/16)][256]
size_t lanczos_prep_doubles(int B);           // workspace: per slot fro, spectrum bounds, 64 quadrature nodes (left by launch_trtri_fro for launch_lanczos_invsqrt)
void launch_trtri_fro(const double* L, size_t Lstride, double* part, int B, int n, const int* active, hipStream_t s, double* dinv, bool hiprio = true,
                      const double* A = nullptr, const double* scale = nullptr, double* prep = nullptr, unsigned long long* sync2 = nullptr);
void launch_lanczos_invsqrt(const double* A, const double* prep, const double* bvec, size_t bstride,
                            double* V, double* y, double* fro, int* msteps, int B, int n, int* status, const int* active, hipStream_t s,
                            int regions_per_slot = 1, const CoopCtx& coop = CoopCtx());
size_t invsqrt_coop_words(int B, int n);

void launch_cma_begin(double* scal, double* vec, double* sig2, SlotVal sigma0, int cs, int B, hipStream_t s);
void launch_cma_paths(const double* Cdw, const double* fro, const double* E, const int32_t* order, const double* ws, double* Ucur, double* scal, double* vec,
                      double* sig2, int B, int cs, int K, int n_iter, const double* consts7, int m_elite, const int* active, hipStream_t s);
void launch_cma_sigma_update(double* Sig, const double* scal, const double* vec, int B, int cs, const double* consts7, int m_elite,
                             const int* active, hipStream_t s);

}  // namespace mpopis
