// engine_handle.h -- the opaque handle behind include/mpopis.h (see engine.h for the HBM layout).
#pragma once
#include "engine.h"
#include <algorithm>
#include <functional>

struct mpopis_handle {
    mpopis_config cfg{};
    int B = 0, K = 0, T = 0, as = 0, ss = 0, cs = 0, N = 1;
    double gamma = 0.0;
    hipStream_t stream = nullptr;
    // Extra streams.  Part-chain schedule (auto_parts / mpopis_set_overlap, policy_step_enqueue): the batch as 2..4 part-chains, the latency-bound
    // links of one chain (Cholesky, weights, finish kernels: tens of workgroups on 256 CUs) under the others' throughput kernels.  When the batch
    // runs as one chain the same streams carry side chains: ||L^-1||_F of the CMA update (xstream[0]) and the Z prefetch for cs > 128 (xstream[1])
    static constexpr int kMaxSplit = 4;
    hipStream_t xstream[kMaxSplit - 1] = {nullptr, nullptr, nullptr};          // streams of the 2nd .. 4th part
    bool split_pinned = false;   // MPOPIS_NSPLIT set: the schedule is fixed for the process
    const double* cur_L = nullptr; size_t cur_Lstride = 0;   // the factor the current AIS iteration samples from (shared L0 or per-slot d_L)
    bool cur_L_scaled = false;                               // ... factors σ²Σ′ (:cmamppi from the second iteration on) rather than Σ′
    bool trtri_early = false;    // this iteration's ||L^-1||_F launch already sits on xstream[0] (queued right behind the Cholesky)
    bool fork_recorded = false;  // ev_fork already recorded behind the current iteration's rollout
    bool side_free = false;      // batch not split this step: xstream[0] / ev_fork / ev_join[0] carry the CMA side chain (||L^-1||_F beside sort + elite mean)
    hipEvent_t ev_fork = nullptr, ev_join[kMaxSplit - 1] = {nullptr, nullptr, nullptr}, ev_skew[kMaxSplit - 1] = {nullptr, nullptr, nullptr};
    int nsplit = 1;                                                            // parts the batch is split into when split_auto is off
    bool split_auto = true;                                                    // default schedule (one stream); false: nsplit parts (mpopis_set_overlap)
    mpopis::EnvDesc env{};
    mpopis::CustomEnv custom;              // MPOPIS_ENV_CUSTOM: the caller's code object (env.custom points here); unloaded in mpopis_destroy
    std::vector<double> custom_reset;      // ... and the state mpopis_reset restores (ss doubles)
    std::string err;
    // Device memory the handle owns (freed in mpopis_destroy).  A per-slot buffer -- [B_full][per_slot] elements of T -- is declared ONCE, by the
    // slot_alloc call that allocates it (the table in create_handle and the lazy sites beside their first use): that call is the record of its
    // layout and what shift_slots moves it by.  shared_alloc: one buffer for the whole batch, never moved.  slot_view: a pointer into someone
    // else's allocation that moves with the slots (null while unused).  All zero-filled on `stream`; a pointer already set is left alone, so
    // a lazy site just calls them again.  The registry holds addresses of members: a handle is neither copied nor moved.
    std::vector<void*> allocs;
    struct SlotBuf { void* member; size_t bytes_per_slot; };
    std::vector<SlotBuf> slot_bufs;
    int dev_alloc(void** p, size_t bytes);                     // engine_api.hip; sets err
    template <class T> int shared_alloc(T*& p, size_t n) {
        void* q = nullptr;
        if (!p && dev_alloc(&q, std::max<size_t>(n, 1) * sizeof(T)) == 0) p = (T*)q;
        return p ? MPOPIS_OK : MPOPIS_ERR_HIP;
    }
    template <class T> void slot_view(T*& p, size_t per_slot) { slot_bufs.push_back({&p, per_slot * sizeof(T)}); }
    template <class T> int slot_alloc(T*& p, size_t per_slot, size_t pad = 0) {
        if (p) return MPOPIS_OK;
        if (shared_alloc(p, (size_t)B_full * per_slot + pad)) return MPOPIS_ERR_HIP;
        slot_view(p, per_slot);
        return MPOPIS_OK;
    }
    mpopis_handle() = default; mpopis_handle(const mpopis_handle&) = delete; mpopis_handle& operator=(const mpopis_handle&) = delete;
    // resident env + policy state
    double *d_x = nullptr, *d_xext = nullptr, *d_U = nullptr, *d_Ucur = nullptr, *d_Uin = nullptr;
    int *d_t = nullptr, *d_done = nullptr;
    // proposal
    double* d_dscale0 = nullptr;                  // sqrt(diag) of the shared pol.Σ
    double *d_Sig = nullptr, *d_L = nullptr, *d_tmpS = nullptr, *d_dscale = nullptr;
    double* d_Lp = nullptr;                       // the factors once more in the fused sampler's staging layout (potrf_panel_doubles(cs) per matrix; cs <= 128)
    bool sigma_diag = false;                      // pol.Σ diagonal (per-slot Σ: in every slot); d_dscale then holds each slot's sqrt(diag)
    // pol.Σ, its factor, the factor's sampler panel and, for :nesmppi, A0 = sqrt(pol.Σ) and Σ0^-1.  S0 is the set IN FORCE: the shared buffers
    // (S0sh, stride 0) until the first mpopis_set_Sigma_slots, then the [B] copies (S0sl, allocated by that call; strides cs² and the panel size),
    // moved with the slot views by the strides below.  mpopis_set_Sigma switches back to the shared set.
    struct Sigma0Set { double *Sigma = nullptr, *L = nullptr, *Lp = nullptr, *nesA = nullptr, *nesS = nullptr; };
    Sigma0Set S0, S0sh, S0sl;
    size_t S0stride = 0, P0stride = 0;
    // Per-slot λ, α, λ_ais, σ (mpopis_set_slot_hyper).  sl_host: the four arrays in force ([4][B], empty = the config's scalars in every slot);
    // the device arrays hold what the kernels consume, formed on the host like the scalars they replace: -1/λ_b, -1/λ_ais,b (-1/λ_b under :imppi),
    // γ_b, σ_b, and for :nesmppi -sf_b/K² and sf_b/K.  Null while the handle runs on the scalars; moved with the slot views.
    std::vector<double> sl_host;
    double* sl_buf = nullptr;                     // one allocation of 6 B doubles behind the six views
    double *d_sl_nil = nullptr, *d_sl_nil_ais = nullptr, *d_sl_gamma = nullptr, *d_sl_sigma = nullptr, *d_sl_nes_a = nullptr, *d_sl_nes_u = nullptr;
    bool sl_any_gamma = false;
    bool slot_hyper() const { return d_sl_nil != nullptr; }
    bool use_gvec() const { return slot_hyper() ? sl_any_gamma : gamma != 0.0; }      // γ U' Σ^-1 E enters the cost in some slot
    // what the launchers consume: the config's scalar paired with the per-slot array of the same meaning (null: the scalar in every slot)
    mpopis::SlotVal sv_nil() const { return {-1 / cfg.lambda, d_sl_nil}; }
    mpopis::SlotVal sv_nil_ais() const { return {-1 / (cfg.policy == MPOPIS_POL_IMPPI ? cfg.lambda : cfg.lambda_ais), d_sl_nil_ais}; }      // :362 / :647,:712
    mpopis::SlotVal sv_gamma() const { return {gamma, d_sl_gamma}; }
    mpopis::SlotVal sv_sigma() const { return {cfg.cma_sigma, d_sl_sigma}; }
    mpopis::SlotVal sv_nes_a() const { return {-cfg.cma_sigma / ((double)K * K), d_sl_nes_a}; }
    mpopis::SlotVal sv_nes_u() const { return {cfg.cma_sigma / K, d_sl_nes_u}; }
    // Per-slot env (mpopis_set_env_params_slots / mpopis_set_tracks).  One [B] array of ready-made parameter structs -- the one of the handle's env
    // kind -- and one of track descriptors, each allocated by the first call of its setter and moved with the slot views; the tracks themselves
    // are shared buffers the descriptors point into.  *_on: the array is IN FORCE (off again after mpopis_set_env_params / mpopis_set_track).
    // On a car handle with exactly one of the two in force the other array holds B copies of the shared value (sync_slot_env, called by the four
    // setters): the rollout kernels' per-slot form reads both.
    mpopis::CarParams* d_car_sl = nullptr; mpopis::McParams* d_mc_sl = nullptr; mpopis::CpParams* d_cp_sl = nullptr;
    mpopis::Track* d_track_sl = nullptr;
    bool env_params_slots_on = false, track_slots_on = false;
    size_t track_sl_lds_all = 0, track_sl_lds_ring = 0;          // track_lds_bytes of the largest per-slot track (rollout_form goes by it)
    // A fleet (mpopis_set_env_params_cars, multi-car handles): [B][num_cars] structs, allocated by the first call and moved
    // with the slot views.  fleet_on excludes env_params_slots_on (each setter ends the other; mpopis_set_env_params ends both).  While it is in
    // force the track array is passed as well (sync_slot_env fills it with copies of the shared descriptor when no per-slot tracks are set) and
    // the per-slot car array is not: the rollout reads cars[] and track[], the small kernels cars[] behind a test of the pointer.
    mpopis::CarParams* d_cars_sl = nullptr;
    bool fleet_on = false;
    mpopis::SlotEnv slot_env() const {
        mpopis::SlotEnv se;
        const bool car_any = env.kind == MPOPIS_ENV_CAR && (env_params_slots_on || track_slots_on || fleet_on);
        if (env_params_slots_on || (car_any && !fleet_on)) { se.car = d_car_sl; se.mc = d_mc_sl; se.cp = d_cp_sl; }
        if (track_slots_on || car_any) { se.track = d_track_sl; se.lds_all = track_sl_lds_all; se.lds_ring = track_sl_lds_ring; }
        if (fleet_on) se.cars = d_cars_sl;
        return se;
    }
    const mpopis::Track* slot_tracks() const { return slot_env().track; }
    // Scenarios (mpopis_set_scenarios): scen_M > 0 model parameter vectors per slot that the ROLLOUTS of a policy step run
    // under, one launch of the per-slot form each; the real env keeps slot_env().  Layout [scen_cap][B_full] ready-made structs of the handle's env
    // kind and [scen_cap][B_full][K] costs: scenario m is the plane m * B_full slots behind the pointer, which is that of the handle's first slot in
    // plane 0 and moves with the slot views like any [B_full][...] buffer -- so a launch addresses its plane exactly as a plain launch addresses
    // d_car_sl / d_cost.  scen_cap: planes allocated (grows with M; the old buffers stay owned until mpopis_destroy).  On a car handle d_track_sl is
    // kept valid while the mode is on (sync_slot_env fills it with copies of the shared descriptor when no per-slot tracks are set).
    int scen_M = 0, scen_cap = 0, risk_kind = MPOPIS_RISK_TAIL_MEAN, risk_tail = 0;
    double risk_theta = 0.0;
    mpopis::CarParams* d_scen_car = nullptr; mpopis::McParams* d_scen_mc = nullptr; mpopis::CpParams* d_scen_cp = nullptr;
    double* d_scen_cost = nullptr;
    mpopis::SlotEnv scenario_env(int m) const {                // what the rollouts of scenario m read: its parameters, the handle's tracks
        mpopis::SlotEnv se;
        const size_t o = (size_t)m * B_full;
        if (d_scen_car) se.car = d_scen_car + o;
        if (d_scen_mc) se.mc = d_scen_mc + o;
        if (d_scen_cp) se.cp = d_scen_cp + o;
        if (env.kind == MPOPIS_ENV_CAR) { se.track = d_track_sl; se.lds_all = track_sl_lds_all; se.lds_ring = track_sl_lds_ring; }
        return se;
    }
    int sync_slot_env();                                       // engine_api.hip; sets err
    bool fold_weights_cfg = false;                // what weights_in_moments is while λ_ais is the config's scalar
    // samples / costs / weights
    double *d_Z = nullptr, *d_E = nullptr, *d_Zin = nullptr, *d_cost = nullptr, *d_w = nullptr;
    unsigned long long* d_cmin = nullptr;   // [B] running minimum cost of the last rollout launch (cost_key), when the AIS reweighting is folded into the moments kernel
    bool weights_in_moments = false;        // :μΣaismppi on a car env with a shape that allows it (engine_api.hip, create)
    double* d_wsum = nullptr;          // [B] Σ_k w_k of the last k_weights launch of the AIS loop
    double *d_wn = nullptr, *d_mu = nullptr, *d_gvec = nullptr, *d_control = nullptr, *d_reward = nullptr, *d_traj = nullptr;
    int *d_status = nullptr, *d_active = nullptr, *d_iters = nullptr;
    unsigned long long* d_iters_acc = nullptr;   // per slot: AIS iterations executed by the policy steps BEFORE the last one (k_step_begin folds iters in before clearing it)
    uint64_t* d_seeds = nullptr;
    double* d_rng_tab = nullptr;            // Box-Muller tables (philox.h), filled at creation
    int noise_kind = MPOPIS_NOISE_PHILOX;   // how the device draws the proposal's normals (mpopis_set_noise_kind)
    // elite selection / resampling
    int32_t *d_order = nullptr, *d_resi = nullptr, *d_alias = nullptr, *d_residx_log = nullptr, *d_resi_in = nullptr;
    double *d_resu = nullptr, *d_accept = nullptr, *d_resu_in = nullptr;
    // moments workspace
    double* d_part = nullptr; int ksplit = 1;
    // CMA (src/mppi_mpopi_policies.jl:513-525 constants; :536-545 per-call state)
    int m_elite = 0;
    double cma_consts[7] = {0, 0, 0, 0, 0, 0, 0};    // mu_eff, cσ, dσ, cΣ, c1, cμ, E
    std::vector<double> cma_ws_host;
    double *d_cma_scal = nullptr, *d_cma_vec = nullptr, *d_sig2 = nullptr, *d_cma_ws = nullptr;
    double* d_tri_dinv = nullptr;                                                          // [B][ceil(cs/16)][256] diagonal-block inverses of L (k_trtri_diag)
    double *d_lanV = nullptr, *d_Cdw = nullptr, *d_fro_part = nullptr, *d_fro = nullptr, *d_lan_prep = nullptr;   // Σ^-½ δw and tr(Σ^-1) (kernels_invsqrt.hip)
    unsigned long long* d_coop_flags = nullptr; unsigned long long coop_epoch = 0;         // cooperative Cholesky (cs > 128): panel flags [B][ceil(cs/16)], launch counter
    unsigned long long* d_lan_x = nullptr; int lan_regions = 1;                            // cooperative Lanczos: exchange granules, basis spill regions per slot
    int *d_potrf_redo = nullptr, *d_lan_redo = nullptr, *d_coop_timeouts = nullptr;         // cooperative kernels that gave up (CoopCtx, engine.h)
    int* h_coop_timeouts = nullptr; bool coop_disabled = false;                            // pinned mirror of the counter; set after the first time-out
    int coop_share = 1;                                                                    // multi-stream schedule: that many cluster launches may be in flight at once
    mpopis::CoopCtx potrf_coop() { mpopis::CoopCtx c; if (!coop_disabled) { c.flags = d_coop_flags; c.epoch = &coop_epoch; c.redo = d_potrf_redo; c.timeouts = d_coop_timeouts; c.share = coop_share; } return c; }
    mpopis::CoopCtx lan_coop() { mpopis::CoopCtx c; if (!coop_disabled) { c.flags = d_lan_x; c.epoch = &coop_epoch; c.redo = d_lan_redo; c.timeouts = d_coop_timeouts; c.share = coop_share; } return c; }
    int32_t* d_alias_stack = nullptr;                                                      // :pmcmppi with K beyond the LDS-resident alias construction: the two stacks (B x 2K ints)
    int* d_alias_need = nullptr;                                                           // :pmcmppi: slots whose alias table the parallel construction could not certify
    int* d_lan_m = nullptr;                                                                // Lanczos steps taken per slot (diagnostic)
    unsigned long long* d_tri_cnt = nullptr;                                               // [B][2]: arrival counter of a slot's trace workgroups (the last one prepares the Lanczos run) and their ||Σ||_inf; zero between launches
    // :nesmppi (A0 = sqrt(pol.Σ) and Σ0^-1 live in S0): per slot Σ^-1 of the iteration, A′ (ping-pong), M / G, the scatter's g, C, partials
    double *d_nesS = nullptr, *d_nesA[2] = {nullptr, nullptr}, *d_nesM = nullptr, *d_nesg = nullptr, *d_nesC = nullptr, *d_nespart = nullptr;
    double *d_qdist = nullptr, *d_qbeta = nullptr; int* d_qwithin = nullptr;
    // Level-3 harness
    double* d_hs = nullptr; int* d_alive = nullptr; const int* alive_gate = nullptr; bool status_sticky = false;
    double* d_actlog = nullptr; ptrdiff_t actlog_stride = 0;   // run_trials' action log of the current call ([B][num_steps + 1][as]) and its slot stride
    // mpopis_run_trials_traced: the trace of the current call, ONE allocation that lives as long as d_actlog does; every
    // pointer is that of the handle's first slot and moves with the slot views (shift_slots), null while not asked for.  The step fields have
    // the ABI's slot-major layout ([B][S + 1][ss], [B][S], [B][S][ncars]).  The plan fields are step-major -- [nplans][B_full][per slot], so that
    // the plan kernels and the rollout write a step's slice in place with their own strides: entry j of a part starts j * B_full slots further
    // on -- and are reordered into `stage` at the copy-out; E is the noise block of ONE step ([B][cs][top + 1]: a part's steps follow each other
    // on its stream).
    struct TraceBufs {
        void* base = nullptr;
        int plan_every = 0, top = 0, nplans = 0, S = 0, ncars = 1;
        mpopis::TraceStepOut step{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        double *E = nullptr, *controls = nullptr, *traj = nullptr, *cost = nullptr, *w = nullptr; int32_t* idx = nullptr;
        void* stage = nullptr;
    } trace;
    int trace_reserve(const mpopis_trace& tr, int num_steps);  // engine_harness.hip; sets err
    void trace_plan(int j);                                    // plan j of the current part's slots, between its policy step and its env step
    int trace_download(const mpopis_trace& tr);
    double noise_sx = 0.0, noise_sy = 0.0, noise_spsi = 0.0;   // simulate_car_racing state noise (car_example.jl:224-236)
    // RCCL communicator for the summary gather (engine_comm.hip); world == 1 needs none
    void* comm = nullptr; int comm_rank = 0, comm_world = 1;
    // bookkeeping
    uint64_t mpc_step = 0;
    std::vector<int> h_status;
    double* h_pin = nullptr;          // pinned staging for the small per-step outputs (control, iters)
    // mpopis_policy_call mailbox: ONE pinned, device-mapped, coherent host block.  The first kernel of the call reads (x, U, t, done) straight
    // from it, the last kernel writes (control, rolled U, status, iters, cooperative time-outs) straight into it: no copy commands, one wait.
    // doubles: in_x[B*ss] in_U[B*cs] out_control[B*as] out_U[B*cs]; then ints: in_t[B] in_done[B] out_status[B] out_iters[B] out_coop[1]
    double* h_call = nullptr; double* d_call = nullptr;   // host pointer / the same block as the device sees it
    double wait_est_ms = 0.0;                             // how long the last synchronous per-step wait took (0: unknown): long steps block instead of spinning
    unsigned call_seq = 0;                                // sequence number the last k_call_out publishes (the host may spin on it; wraps)
    // timing
    bool timing = false, ev_open = false; int timing_mask = ~0;
    // MPOPIS_DEBUG_LAUNCH=1: after every kernel class of a policy step, hipGetLastError + stream sync, so that a failing
    // launch / faulting kernel is reported with the class it belongs to (release runs check once per call)
    bool debug_launch = false; int cur_class = 0; std::string launch_err;
    std::vector<hipEvent_t> events; std::vector<int> ev_slot; int ev_used = 0;

    // mpopis_get_plan: the read-out of the last policy step (kernels_plan.hip).  plan_ok: that step succeeded and no entry point has written to the
    // handle since -- set at the end of a successful mpopis_policy_step / mpopis_policy_call, cleared by plan_drop at the top of every entry point
    // that is no getter (plan_lost: its name, plan_stepped: a policy step has been asked for at all -- for the refusal's message).  The buffers are
    // ONE allocation of the whole batch, made at the first call and replaced when a call asks for a larger top; no slot views (the call runs on
    // the unsplit batch only).
    bool plan_ok = false, plan_stepped = false; const char* plan_lost = "";
    void plan_drop(const char* by) { plan_ok = false; plan_lost = by; }
    void plan_step_begins(const char* by) { plan_drop(by); plan_stepped = true; }
    struct PlanBufs {
        void* base = nullptr; int cap_top = -1;
        double *controls = nullptr, *E = nullptr, *traj = nullptr, *cost = nullptr, *w = nullptr; int32_t* idx = nullptr;
    } plan;
    int plan_reserve(int top);                                 // engine_api.hip; sets err
    bool plan_rollout(int Kp, hipError_t* custom_err);         // the plan's Kp = top + 1 control sequences from the step's start state into plan.traj / plan.cost

    void time_begin(int slot);
    void time_end();
    void prepare_state();
    mpopis::RolloutArgs rollout_base() const;                  // what every rollout of the handle shares: env, shape, start state, per-slot env
    void rollout(const double* Ucur, const double* Uorig, const double* gvec, const int* act, int* iters = nullptr, int iter_n = 0);
    int B_full = 0;                                       // cfg.batch (B is narrowed to a part's slots while a part-chain is enqueued)
    // What the scatter kernel's form goes by (launch_wcov_mfma): the whole batch -- or -1 = "the compact form" for shapes whose DEFAULT schedule is
    // part-chains: the row form's 8-wave workgroups take a CU's whole LDS (136 KB), which a lone stream does not mind (74 vs 86 us at 64 trials) and
    // concurrent chains do (no rollout / sampler workgroup fits beside one: the 64-trial step 5.64 instead of 5.35 ms).  A function of the shape
    // only, never of the schedule actually running, so that a slot's bits do not depend on mpopis_set_overlap.
    int wcov_sel_batch() const { return auto_parts() > 1 ? -1 : B_full; }
    // The part-chain streams must sit on DIFFERENT hardware queues: HIP deals its (by default four) queues to streams in creation order, whatever else
    // the process has created before, and two chains that share a queue serialise (the same 64-trial step 6.8 instead of 5.3 ms when torch had
    // initialised the device first).  Checked once, at the first multi-part step, with a 200-us spin kernel per stream (verify_part_streams); streams
    // that share a queue with an earlier one are replaced, and max_parts says how many independent ones there are.
    bool part_streams_checked = false;
    int max_parts = kMaxSplit;
    std::vector<hipStream_t> rejected_streams;            // (kept until the handle goes: destroying one would hand its queue to the next candidate)
    void verify_part_streams();
    int auto_parts() const;                               // part-chains of the default schedule for this handle's shape
    int policy_step_enqueue(bool injected);               // one MPC step of the whole batch: chains_fork + chains_step + chains_join
    // Part-chains that outlive a step (engine_api.hip): fork the parts once, enqueue step after step on each part's own stream, join when the host
    // needs the whole batch again.  chain_np: parts of the open set (0: none open); chain_fresh: no step enqueued since the fork.
    int chain_np = 0; bool chain_fresh = false;
    void chains_fork();
    int chains_step(bool injected, const std::function<void()>& tail = {});
    void chains_join();
    int step_enqueue_view(bool injected, hipEvent_t wait_first, hipEvent_t record_after_first_sampler);
    void shift_slots(ptrdiff_t db);                           // move every per-slot device pointer by db slots (slot views)
    // the checks and messages several entry points share
    bool track_missing() { if (env.kind != MPOPIS_ENV_CAR || env.track.P != 0 || track_slots_on) return false; err = "track not set"; return true; }
    int report_status(int st) {                               // the message that goes with the worst per-slot status of a call; returns st
        if (st == MPOPIS_ERR_NOT_PD) err = "PosDefException: proposal covariance is not positive definite";
        else if (st == MPOPIS_ERR_ACTION) err = "Action is not in action space (non-finite control/cost)";
        else if (st == MPOPIS_ERR_NUMERIC) err = "cmamppi: Σ^-0.5 δw could not be formed (non-finite covariance, trace or δw)";
        return st;
    }
    int ais_update(int n, bool injected);
    int run_trials(int num_steps, int laps, double* records, double* actions, const mpopis_trace* tr = nullptr);
    void init_cma_constants();
    void cma_begin();
    const double* cma_sigma2();
};

namespace mpopis {
// Error precedence when several slots (or several kernels of one slot) failed in one call: HIP (-4) > ACTION (-3) > NOT_PD (-2) > NUMERIC (-5),
// i.e. the numeric minimum among the codes of ABI version 1, which the newer MPOPIS_ERR_NUMERIC never hides (include/mpopis.h).
// (status_rank lives in engine.h: the device-side writers merge by the same rule, status_raise)
inline int worse_status(int a, int b) { return status_rank(b) > status_rank(a) ? b : a; }
void launch_scale_rows(double* Z, const double* dsc, int B, int cs, int K, hipStream_t s);
inline void launch_mppi_Z_in(const double* src, double* dst, int B, int T, int K, int as, hipStream_t s) { launch_transpose_in(src, dst, B * T, as, K, s); }
inline void launch_mppi_E_out(const double* src, double* dst, int B, int T, int K, int as, hipStream_t s) { launch_transpose_out(src, nullptr, nullptr, dst, B * T, as, K, s); }
}
