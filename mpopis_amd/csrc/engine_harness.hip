// engine_harness.hip -- Level 3: the closed-loop trial harness, resident on the device.
//   simulate_car_racing trial loop   src/examples/car_example.jl:170-326
//   simulate_mountaincar trial loop  src/examples/mountaincar_example.jl:125-180
//   simulate_cartpole trial loop     src/examples/cartpole_example.jl:110-160
// All B trial slots advance together: policy step -> real env step -> bookkeeping, with no host
// round trip per MPC step (the host only polls the alive flags every few steps to stop early).
// A slot that terminates (laps done, > 10 track violations, > 50 β violations, MountainCar done, or
// cnt > num_steps) is frozen: its `alive` flag gates every kernel of later steps.
#include "engine.h"
#include "engine_handle.h"
#include <math.h>
#include <algorithm>

using namespace mpopis;

namespace mpopis {

__global__ void k_zero_status(int* st, int B) { const int b = blockIdx.x * 64 + threadIdx.x; if (b < B) st[b] = 0; }

}  // namespace mpopis

// ---- mpopis_run_trials_traced -----------------------------------------------------------------------------------------
// The trace of one call, carved out of one allocation (each part 16-byte aligned) and zero-filled on the stream: only what the caller asks for,
// plus what producing it needs (the plan's noise block and controls, which k_plan_assemble always writes; the sample indices when top > 0).
int mpopis_handle::trace_reserve(const mpopis_trace& tr, int num_steps) {
    TraceBufs t;
    t.plan_every = tr.plan_every; t.top = tr.top; t.S = num_steps + 1;
    t.nplans = tr.plan_every > 0 ? num_steps / tr.plan_every + 1 : 0;
    t.ncars = env.kind == MPOPIS_ENV_CAR ? std::max(1, env.ncars) : 1;
    const size_t Bn = (size_t)B_full, S = (size_t)t.S, W = (size_t)t.top + 1, J = (size_t)t.nplans, top = (size_t)t.top;
    auto up = [](size_t bytes) { return (bytes + 15) & ~(size_t)15; };
    const bool want_roll = J && (tr.plan_traj || tr.plan_cost);
    const size_t n_states = tr.states ? up(8 * Bn * (S + 1) * ss) : 0, n_rew = tr.rewards ? up(8 * Bn * S) : 0, n_it = tr.iters ? up(4 * Bn * S) : 0,
                 n_win = tr.within ? up(4 * Bn * S) : 0, n_dist = tr.dist ? up(8 * Bn * S * t.ncars) : 0, n_beta = tr.beta ? up(8 * Bn * S * t.ncars) : 0;
    const size_t n_E = J ? up(8 * Bn * cs * W) : 0, n_ctl = up(8 * J * Bn * cs), n_traj = want_roll ? up(8 * J * Bn * W * ss * T) : 0,
                 n_cost = want_roll ? up(8 * J * Bn * W) : 0, n_w = up(8 * J * Bn * top), n_idx = up(4 * J * Bn * top);
    // the copy-out reorders one plan field at a time into `stage`: as large as the largest field that is downloaded
    size_t n_stage = 0;
    if (tr.plan_controls) n_stage = std::max(n_stage, n_ctl);
    if (tr.plan_traj) n_stage = std::max(n_stage, n_traj);
    if (tr.plan_cost) n_stage = std::max(n_stage, n_cost);
    if (tr.plan_weights) n_stage = std::max(n_stage, n_w);
    if (tr.plan_idx0) n_stage = std::max(n_stage, n_idx);
    const size_t bytes = std::max<size_t>(16, n_states + n_rew + n_it + n_win + n_dist + n_beta + n_E + n_ctl + n_traj + n_cost + n_w + n_idx + n_stage);
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        err = "mpopis_run_trials_traced: hipMalloc of the trace buffers failed (" + std::to_string(bytes) + " bytes)";
        return MPOPIS_ERR_HIP;
    }
    char* c = (char*)p;
    auto take = [&c](size_t n) { char* q = n ? c : nullptr; c += n; return q; };
    t.base = p;
    t.step.states = (double*)take(n_states); t.step.rewards = (double*)take(n_rew); t.step.iters = (int32_t*)take(n_it);
    t.step.within = (int32_t*)take(n_win); t.step.dist = (double*)take(n_dist); t.step.beta = (double*)take(n_beta);
    t.E = (double*)take(n_E); t.controls = (double*)take(n_ctl); t.traj = (double*)take(n_traj); t.cost = (double*)take(n_cost);
    t.w = (double*)take(n_w); t.idx = (int32_t*)take(n_idx); t.stage = take(n_stage);
    trace = t;
    if (hipMemsetAsync(p, 0, bytes, stream) != hipSuccess) { err = "mpopis_run_trials_traced: clearing the trace buffers failed"; return MPOPIS_ERR_HIP; }
    return MPOPIS_OK;
}

// Plan j of the current part's slots, enqueued between the part's policy step and its env step: the launches of mpopis_get_plan with the part's
// own d_w / d_E / d_Ucur / d_Uin / d_wn and start state (d_x, and the d_xext its policy step extended: launch_env_step has not yet run), writing
// step j's slice of the trace in place.  active = d_alive: a frozen slot's stale weights and noise write nothing.
void mpopis_handle::trace_plan(int j) {
    const TraceBufs& t = trace;
    const size_t W = (size_t)t.top + 1, jb = (size_t)j * B_full;
    int32_t* idx = t.top ? t.idx + jb * t.top : nullptr;
    launch_plan_select(d_w, B, K, t.top, idx, t.top ? t.w + jb * t.top : nullptr, stream, d_alive);
    launch_plan_assemble(d_E, d_Ucur, d_Uin, d_wn, idx, B, cs, K, t.top, t.controls + jb * cs, t.E, stream, d_alive);
    if (!t.traj) return;
    RolloutArgs a = rollout_base();
    a.K = (int)W; a.Ucur = d_Uin; a.Uorig = d_Uin; a.E = t.E;
    a.cost = t.cost + jb * W; a.traj = t.traj + jb * W * ss * T; a.active = d_alive;
    hipError_t custom_err = hipSuccess;
    if (!launch_rollout(a, stream, &custom_err) && launch_err.empty())
        launch_err = env.kind == MPOPIS_ENV_CUSTOM ? std::string("mpopis_run_trials_traced: launching the custom env's rollout kernel failed: ") + hipGetErrorString(custom_err)
                                                   : std::string("mpopis_run_trials_traced: no rollout kernel for this env");
}

// The one download, at the end of the call (the stream then holds the joined batch): the step fields as they are, each plan field reordered from
// step-major to the ABI's slot-major layout on the device and copied from there.
int mpopis_handle::trace_download(const mpopis_trace& tr) {
    const TraceBufs& t = trace;
    const size_t Bn = (size_t)B, S = (size_t)t.S, W = (size_t)t.top + 1, top = (size_t)t.top;
    bool ok = true;
    auto get = [&](void* host, const void* dev, size_t bytes) { if (host && bytes) ok &= hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess; };
    get(tr.states, t.step.states, 8 * Bn * (S + 1) * ss); get(tr.rewards, t.step.rewards, 8 * Bn * S); get(tr.iters, t.step.iters, 4 * Bn * S);
    get(tr.within, t.step.within, 4 * Bn * S); get(tr.dist, t.step.dist, 8 * Bn * S * t.ncars); get(tr.beta, t.step.beta, 8 * Bn * S * t.ncars);
    auto get_plan = [&](void* host, const void* dev, size_t per, int elem) {
        if (!host || !per || !t.nplans) return;
        launch_trace_reorder(dev, t.stage, B, t.nplans, per, elem, stream);
        get(host, t.stage, (size_t)elem * Bn * t.nplans * per);
    };
    get_plan(tr.plan_controls, t.controls, (size_t)cs, 8); get_plan(tr.plan_traj, t.traj, W * ss * T, 8); get_plan(tr.plan_cost, t.cost, W, 8);
    get_plan(tr.plan_weights, t.w, top, 8); get_plan(tr.plan_idx0, t.idx, top, 4);
    if (!ok) { err = "mpopis_run_trials_traced: copying the trace out failed"; return MPOPIS_ERR_HIP; }
    return MPOPIS_OK;
}

int mpopis_handle::run_trials(int num_steps, int laps, double* records, double* actions, const mpopis_trace* tr) {
    if (track_missing()) return MPOPIS_ERR_ARG;
    if (num_steps < 0 || laps < 0 || laps > 4) { err = "need num_steps >= 0 and 0 <= laps <= 4"; return MPOPIS_ERR_ARG; }
    if (tr) {
        const int top_max = std::min(K, MPOPIS_PLAN_MAX_TOP);
        const bool plan_ptr = tr->plan_controls || tr->plan_traj || tr->plan_cost || tr->plan_idx0 || tr->plan_weights;
        std::string bad;
        if (tr->plan_every < 0) bad = "plan_every must be >= 0, got " + std::to_string(tr->plan_every);
        else if (tr->top < 0 || tr->top > top_max) bad = "top must be 0.." + std::to_string(top_max) + " (min(K, MPOPIS_PLAN_MAX_TOP)), got " + std::to_string(tr->top);
        else if (tr->plan_every == 0 && tr->top > 0) bad = "top > 0 needs plan_every > 0";
        else if (tr->plan_every == 0 && plan_ptr) bad = "a plan array needs plan_every > 0";
        if (!bad.empty()) { err = "mpopis_run_trials_traced: " + bad; return MPOPIS_ERR_ARG; }
    }
    if (hipSetDevice(cfg.device) != hipSuccess) { err = "hipSetDevice failed"; return MPOPIS_ERR_HIP; }
    if (slot_alloc(d_hs, kH_N) || slot_alloc(d_alive, 1)) { err = "hipMalloc failed"; return MPOPIS_ERR_HIP; }
    // (the trace is a member for the length of this call, like d_actlog below)
    struct TraceGuard { mpopis_handle* h; ~TraceGuard() { if (h->trace.base) (void)hipFree(h->trace.base); h->trace = TraceBufs{}; } } trace_guard{this};
    if (tr) {
        if (const int rc = trace_reserve(*tr, num_steps)) return rc;
        if (trace.step.states) launch_trace_start(d_x, trace.step.states, B, ss, trace.S, stream);
    }
    // (d_actlog is a member for the length of this call: the part-chains log through their slot views of it)
    struct ActlogGuard { mpopis_handle* h; ~ActlogGuard() { if (h->d_actlog) (void)hipFree(h->d_actlog); h->d_actlog = nullptr; h->actlog_stride = 0; } } actlog_guard{this};
    if (actions) {
        if (hipMalloc((void**)&d_actlog, sizeof(double) * (size_t)B * (num_steps + 1) * as) != hipSuccess) { d_actlog = nullptr; err = "hipMalloc failed"; return MPOPIS_ERR_HIP; }
        actlog_stride = (ptrdiff_t)(num_steps + 1) * as;
        (void)hipMemsetAsync(d_actlog, 0, sizeof(double) * (size_t)B * (num_steps + 1) * as, stream);
    }
    launch_harness_init(d_hs, d_alive, B, stream);
    hipLaunchKernelGGL(k_zero_status, dim3((B + 63) / 64), dim3(64), 0, stream, d_status, B);
    mpc_step = 0;
    status_sticky = true;                              // errors of any MPC step survive to the end of the call
    std::vector<int> h_alive(B, 1);
    int worst = 0;
    const bool noisy = noise_sx != 0.0 || noise_sy != 0.0 || noise_spsi != 0.0;
    for (int s = 0; s <= num_steps; ++s) {
        // The part-chains stay forked between the host's looks at the batch (every eighth step): a part's env step and bookkeeping follow its policy
        // step on its own stream, on its own slots, and its next policy step follows them there.
        if (!chain_np) chains_fork();
        alive_gate = d_alive;
        int rc = chains_step(false, [&] {                       // (runs once per part, with B / stream / the slot pointers narrowed to that part)
            if (trace.plan_every > 0 && s % trace.plan_every == 0) trace_plan(s / trace.plan_every);      // before the env step overwrites d_x
            const hipError_t e = launch_env_step(env, d_x, d_t, d_done, d_control, d_reward, d_status, d_alive, B, stream, slot_env());
            if (e != hipSuccess && launch_err.empty()) launch_err = std::string("env step: launching the custom env's kernel failed: ") + hipGetErrorString(e);
            launch_harness_update(env, d_x, d_done, d_reward, d_iters, d_hs, d_alive, d_control, d_actlog, s, num_steps, laps, K, B,
                                  StateNoise{noise_sx, noise_sy, noise_spsi, noisy ? d_seeds : (const uint64_t*)nullptr, d_rng_tab}, slot_env(), stream);
            const TraceStepOut& ts = trace.step;
            if (ts.states || ts.rewards || ts.iters || ts.within || ts.dist || ts.beta)
                launch_trace_step(env.kind, env.ncars, ss, env.track, slot_tracks(), d_x, d_reward, d_iters, d_hs + kH_cnt, kH_N, s, trace.S,
                                              trace.step, B, stream);
        });
        alive_gate = nullptr;
        if (rc) { chains_join(); status_sticky = false; return rc; }
        // error status is sticky per call of policy_step_enqueue (it clears d_status): fold it into the host view now and then
        if ((s & 7) == 7 || s == num_steps) {
            chains_join();
            (void)hipMemcpyAsync(h_alive.data(), d_alive, sizeof(int) * B, hipMemcpyDeviceToHost, stream);
            (void)hipMemcpyAsync(h_status.data(), d_status, sizeof(int) * B, hipMemcpyDeviceToHost, stream);
            if (h_coop_timeouts && !coop_disabled) (void)hipMemcpyAsync(h_coop_timeouts, d_coop_timeouts, sizeof(int), hipMemcpyDeviceToHost, stream);
            if (hipStreamSynchronize(stream) != hipSuccess) { err = "stream sync failed"; return MPOPIS_ERR_HIP; }
            if (h_coop_timeouts && *h_coop_timeouts > 0) coop_disabled = true;   // a cluster gave up (and was redone): stop using clusters, also within this call
            for (int b = 0; b < B; ++b) worst = mpopis::worse_status(worst, h_status[b]);
            bool any = false;
            for (int b = 0; b < B; ++b) any |= h_alive[b] != 0;
            if (!any || worst) break;
        }
    }
    status_sticky = false;
    std::vector<double> hs((size_t)B * kH_N);
    if (hipMemcpyAsync(hs.data(), d_hs, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, stream) != hipSuccess) { err = "copy failed"; return MPOPIS_ERR_HIP; }
    if (actions) (void)hipMemcpyAsync(actions, d_actlog, sizeof(double) * (size_t)B * (num_steps + 1) * as, hipMemcpyDeviceToHost, stream);
    if (tr) { if (const int rc = trace_download(*tr)) return rc; }
    if (hipStreamSynchronize(stream) != hipSuccess) { err = "stream sync failed"; return MPOPIS_ERR_HIP; }
    for (int b = 0; b < B; ++b) {                      // car_example.jl:287-302
        const double* h = hs.data() + (size_t)b * kH_N;
        double* r = records + (size_t)b * MPOPIS_RECORD_LEN;
        const double cnt = h[kH_cnt];
        r[0] = h[kH_rew]; r[1] = cnt - 1; r[2] = h[kH_rew] / (cnt - 1);
        r[3] = h[kH_lap0]; r[4] = h[kH_lap1]; r[5] = h[kH_lap2]; r[6] = h[kH_lap3];
        const bool car = env.kind == MPOPIS_ENV_CAR;
        r[7] = car && cnt > 0 ? h[kH_vmean] / cnt : 0.0; r[8] = car ? h[kH_vmax] : 0.0;
        r[9] = car && cnt > 0 ? h[kH_bmean] / cnt : 0.0; r[10] = car ? h[kH_bmax] : 0.0;
        r[11] = h[kH_beta]; r[12] = h[kH_trk]; r[13] = h[kH_crash]; r[14] = h[kH_rollouts]; r[15] = (double)worst;
    }
    return report_status(worst);
}
