// engine_api.hip -- handle, device buffers, launch sequences and the C ABI of include/mpopis.h.
//
// One handle = B resident independent trials (env + policy pairs).  Every policy step is a fixed
// sequence of kernel launches on the handle's stream; data-dependent control flow of the
// reference (CE/CMA early break :459-461,:567-569, PosDefException) is turned into per-slot
// `active` predicates evaluated on the device, so a step never needs a host round trip.
#include "engine.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include <vector>

using namespace mpopis;

static std::string g_create_error;

#define HIPCHK(h, expr)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            char buf_[512];                                                                     \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            if (h) (h)->err = buf_; else g_create_error = buf_;                                 \
            return MPOPIS_ERR_HIP;                                                              \
        }                                                                                       \
    } while (0)

#include "engine_handle.h"
#include "philox.h"
#include <chrono>
#include <atomic>

// ---- tiny utility kernels -----------------------------------------------------------------------
__global__ void k_fill_i32(int* p, int v, size_t n) { size_t i = blockIdx.x * (size_t)256 + threadIdx.x; if (i < n) p[i] = v; }
__global__ void k_copy_f64(const double* s, double* d, size_t n) { size_t i = blockIdx.x * (size_t)256 + threadIdx.x; if (i < n) d[i] = s[i]; }
__global__ void k_bcast_f64(const double* s, double* d, size_t n, int B) {     // d[b][i] = s[i]
    size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) for (int b = 0; b < B; ++b) d[(size_t)b * n + i] = s[i];
}

__global__ void k_scaled_copy_f64(const double* s, size_t sstride, const double* scale, double* d, size_t n) {   // d[b][i] = scale[b]*s[b][i]
    const int b = blockIdx.y; const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) d[(size_t)b * n + i] = (scale ? scale[b] : 1.0) * s[(size_t)b * sstride + i];
}

// mpopis_policy_call: the hand-over kernels between the pinned mailbox (device-mapped host memory) and the resident buffers.
struct CallBox { double *x, *U, *control, *Uout; int *t, *done, *status, *iters, *coop; volatile int* seq; };
static CallBox call_box(double* base, int B, int ss, int cs, int as) {
    CallBox m;
    m.x = base; m.U = m.x + (size_t)B * ss; m.control = m.U + (size_t)B * cs; m.Uout = m.control + (size_t)B * as;
    m.t = (int*)(m.Uout + (size_t)B * cs); m.done = m.t + B; m.status = m.done + B; m.iters = m.status + B; m.coop = m.iters + B; m.seq = m.coop + 1;
    return m;
}
static size_t call_box_bytes(int B, int ss, int cs, int as) { return sizeof(double) * ((size_t)B * (ss + 2 * cs + as)) + sizeof(int) * ((size_t)4 * B + 4); }
__global__ void k_call_in(CallBox m, double* x, double* U, int* t, int* done, int nx, int nu, int B, int flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if ((flags & 1) && i < nx) x[i] = m.x[i];
    if ((flags & 2) && i < nu) U[i] = m.U[i];
    if (i < B) { if (flags & 4) t[i] = m.t[i]; if (flags & 8) done[i] = m.done[i]; }
}
// ONE workgroup: every thread stores its share and fences at system scope, the workgroup meets, then thread 0 publishes the call's sequence
// number -- the host may spin on that word instead of going through the runtime's completion signal.
__global__ void k_call_out(CallBox m, const double* control, const double* U, const int* status, const int* iters, const int* coop, int nc, int nu, int B, int seq) {
    for (int i = threadIdx.x; i < nc; i += 256) m.control[i] = control[i];
    for (int i = threadIdx.x; i < nu; i += 256) m.Uout[i] = U[i];
    for (int i = threadIdx.x; i < B; i += 256) { m.status[i] = status[i]; m.iters[i] = iters[i]; }
    if (threadIdx.x == 0) *m.coop = coop ? *coop : 0;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) { *m.seq = seq; __threadfence_system(); }
}

static void fill_i32(int* p, int v, size_t n, hipStream_t s) { hipLaunchKernelGGL(k_fill_i32, dim3((n + 255) / 256), dim3(256), 0, s, p, v, n); }
static void copy_f64(const double* s_, double* d, size_t n, hipStream_t s) { hipLaunchKernelGGL(k_copy_f64, dim3((n + 255) / 256), dim3(256), 0, s, s_, d, n); }

// the one place the handle's buffers come from (shared_alloc / slot_alloc, engine_handle.h): zero-filled on the stream, owned until mpopis_destroy
int mpopis_handle::dev_alloc(void** p, size_t bytes) {
    HIPCHK(this, hipMalloc(p, bytes));
    allocs.push_back(*p);
    HIPCHK(this, hipMemsetAsync(*p, 0, bytes, stream));
    return 0;
}

// a setup call that replaces what queued work may still read: wait for everything the handle has queued, on the part-chain streams too
static int quiesce(mpopis_handle* h) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (auto st : h->xstream) if (st) HIPCHK(h, hipStreamSynchronize(st));
    return MPOPIS_OK;
}

static const char* kClassNames[] = {"rollout", "sample", "potrf", "reweight", "moments", "select", "other"};

void mpopis_handle::time_begin(int slot) {
    cur_class = slot;
    ev_open = timing && (timing_mask & (1 << slot)) && ev_used + 2 <= (int)events.size();
    if (!ev_open) return;
    (void)hipEventRecord(events[ev_used], stream);
    ev_slot.push_back(slot);
}
void mpopis_handle::time_end() {
    if (debug_launch && launch_err.empty()) {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) launch_err = std::string("kernel class '") + kClassNames[cur_class] + "': " + hipGetErrorString(e);
    }
    if (!ev_open) return;
    (void)hipEventRecord(events[ev_used + 1], stream);
    ev_used += 2;
    ev_open = false;
}

// Host wait for the handle's stream.  A synchronous pol(env) of one trial is 0.2-2 ms of GPU work; hipStreamSynchronize's blocking wake-up
// adds 20-50 us to that, so poll the stream for the first 3 ms (one host thread spinning, as a CPU implementation of the call would) and
// only then block.
static hipError_t wait_stream(hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(3)) break;
    }
    return hipStreamSynchronize(s);
}
// The per-MPC-step waits (mpopis_policy_step / mpopis_policy_call) know how long the previous step took: the spin only pays for sub-millisecond
// steps (C2 0.15 ms, where the blocking wake-up is a quarter of the call); a handle whose last wait exceeded kSpinWorthMs (C3 1.8 ms, C4 5-25 ms, the
// 64-trial batches) blocks right away instead of burning a host core for 3 ms first -- the 20-50 us wake-up is then below 3 % of the step.
constexpr double kSpinWorthMs = 1.0;
static bool wait_should_spin(const mpopis_handle* h) { return h->wait_est_ms <= kSpinWorthMs; }
static void wait_note(mpopis_handle* h, std::chrono::steady_clock::time_point t0) {
    h->wait_est_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
static hipError_t wait_step(mpopis_handle* h) {
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = wait_should_spin(h) ? wait_stream(h->stream) : hipStreamSynchronize(h->stream);
    wait_note(h, t0);
    return e;
}

static int fold_status(mpopis_handle* h, const int* per_slot) {
    int st = 0;
    for (int b = 0; b < h->B; ++b) st = mpopis::worse_status(st, per_slot[b]);
    return h->report_status(st);
}

static int sync_status(mpopis_handle* h) {
    HIPCHK(h, hipMemcpyAsync(h->h_status.data(), h->d_status, sizeof(int) * h->B, hipMemcpyDeviceToHost, h->stream));
    if (h->h_coop_timeouts && !h->coop_disabled) HIPCHK(h, hipMemcpyAsync(h->h_coop_timeouts, h->d_coop_timeouts, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_step(h));
    // a cluster gave up waiting for a partner (its slot was recomputed by the one-workgroup kernel in the same step, so the results are
    // complete): this device cannot keep the clusters co-resident right now -- stop using them for this handle instead of paying the wait again
    if (h->h_coop_timeouts && *h->h_coop_timeouts > 0) h->coop_disabled = true;
    return fold_status(h, h->h_status.data());
}

// ---- ABI ---------------------------------------------------------------------------------------
extern "C" {

int mpopis_abi_version(void) { return MPOPIS_ABI_VERSION; }

const char* mpopis_last_error(const mpopis_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

static void default_car_params(double* p) {      // src/envs/car_racing.jl:68-93
    const double d2r = M_PI / 180.0;
    const double v[20] = {2000.0, 3764.0, 0.3, 1.53, 1.23, 241.0, 25.1, 150000.0, 280000.0, 0.9, 0.9, 18.0 * d2r, 90.0 * d2r,
                          7200.0, 22500.0, 0.6, 0.0, 45.0 * d2r, 0.1, 0.01};
    memcpy(p, v, sizeof v);
}
static void default_mc_params(double* p) {       // RL.jl MountainCarEnvParams, continuous=true
    const double v[8] = {-1.2, 0.6, 0.07, 0.45, 0.0, 0.0015, 0.0025, 200.0};
    memcpy(p, v, sizeof v);
}

static void default_cp_params(double* p) {       // RL.jl CartPoleEnvParams
    const double v[11] = {9.8, 1.0, 0.1, 1.1, 0.5, 0.05, 10.0, 0.02, 12.0 * 2.0 * M_PI / 360.0, 2.4, 200.0};
    memcpy(p, v, sizeof v);
}

// The checks every create call makes before it touches the device: policy, shape, and the per-policy limits on cs = as * H.
static int check_policy_config(const mpopis_config* cfg, int as) {
    if (cfg->policy < MPOPIS_POL_MPPI || cfg->policy > MPOPIS_POL_NESMPPI) { g_create_error = "No policy_type of that kind"; return MPOPIS_ERR_ARG; }
    if (cfg->num_samples < 1 || cfg->horizon < 1 || cfg->batch < 1) { g_create_error = "num_samples, horizon, batch must be >= 1"; return MPOPIS_ERR_ARG; }
    if (cfg->policy == MPOPIS_POL_NESMPPI) {
        // K = 1: maximum(abs.(diff(cost))) of an empty diff throws in the reference (src/mppi_mpopi_policies.jl:868)
        if (cfg->num_samples < 2) { g_create_error = "nesmppi: num_samples must be >= 2 (the early-break test takes diff(cost))"; return MPOPIS_ERR_ARG; }
        if ((long long)as * cfg->horizon > 512) { g_create_error = "nesmppi: control space too large (cs <= 512, the range of the dense Σ′ scatter)"; return MPOPIS_ERR_ARG; }
        if (!std::isfinite(cfg->cma_sigma)) { g_create_error = "nesmppi: step_factor (cma_sigma) must be finite"; return MPOPIS_ERR_ARG; }
    }
    if (cfg->policy == MPOPIS_POL_CMAMPPI && (long long)as * cfg->horizon > invsqrt_max_n()) { g_create_error = "cmamppi: control space too large for the on-chip Σ^-0.5 δw kernel"; return MPOPIS_ERR_ARG; }
    if ((cfg->policy == MPOPIS_POL_CEMPPI || cfg->policy == MPOPIS_POL_MUSIGMAAISMPPI || cfg->policy == MPOPIS_POL_PMCMPPI) &&
        (long long)as * cfg->horizon > wcov_max_cs()) {
        static const std::string msg = "control space too large for the covariance scatter of :cemppi / :μΣaismppi / :pmcmppi (cs <= " + std::to_string(wcov_max_cs()) + ")";
        g_create_error = msg; return MPOPIS_ERR_ARG;
    }
    return MPOPIS_OK;
}

static int create_handle(const mpopis_config* cfg, int as, int ss, mpopis_handle** out);
// a create call that fails half-way (hipStreamCreate under many handles is a realistic one) must not leak the handle and what it already owns
static int fail_create(mpopis_handle* h, int code, const std::string& msg) { g_create_error = msg; mpopis_destroy(h); return code; }

// hipModuleLoadData takes no length: a buffer whose own tables point past nbytes would be read beyond the caller's memory.  Little-endian ELF64
// (the section header table and, through it, every section must lie inside) or a clang offload bundle (every entry must; an ELF entry is checked too).
static bool code_object_complete(const unsigned char* p, uint64_t n) {
    auto rd = [p](uint64_t off, int bytes) { uint64_t v = 0; for (int i = bytes - 1; i >= 0; --i) v = (v << 8) | p[off + i]; return v; };
    auto inside = [n](uint64_t off, uint64_t len) { return off <= n && len <= n - off; };
    if (n >= 64 && memcmp(p, "\x7f" "ELF", 4) == 0) {
        const uint64_t shoff = rd(0x28, 8), shentsize = rd(0x3A, 2), shnum = rd(0x3C, 2);
        if (shnum == 0) return true;
        if (shentsize < 64 || !inside(shoff, shentsize * shnum)) return false;
        for (uint64_t i = 0; i < shnum; ++i) {
            const uint64_t sh = shoff + i * shentsize;
            if (rd(sh + 4, 4) != 8 /* SHT_NOBITS occupies no file bytes */ && !inside(rd(sh + 0x18, 8), rd(sh + 0x20, 8))) return false;
        }
        return true;
    }
    uint64_t pos = 24;                                                         // behind the magic: entry count, then {offset, size, triple length, triple} per entry
    if (!inside(pos, 8)) return false;
    const uint64_t entries = rd(pos, 8); pos += 8;
    for (uint64_t i = 0; i < entries; ++i) {
        if (!inside(pos, 24)) return false;
        const uint64_t off = rd(pos, 8), size = rd(pos + 8, 8), tl = rd(pos + 16, 8);
        pos += 24;
        if (!inside(pos, tl) || !inside(off, size)) return false;
        pos += tl;
        if (size >= 64 && memcmp(p + off, "\x7f" "ELF", 4) == 0 && !code_object_complete(p + off, size)) return false;
    }
    return true;
}

int mpopis_create(const mpopis_config* cfg, mpopis_handle** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return MPOPIS_ERR_ARG; }
    *out = nullptr;
    const bool car = cfg->env_kind == MPOPIS_ENV_CAR;
    if (cfg->env_kind == MPOPIS_ENV_CUSTOM) { g_create_error = "env kind MPOPIS_ENV_CUSTOM needs a code object: create the handle with mpopis_create_custom"; return MPOPIS_ERR_ARG; }
    if (!(car || cfg->env_kind == MPOPIS_ENV_MOUNTAINCAR || cfg->env_kind == MPOPIS_ENV_CARTPOLE)) { g_create_error = "unknown env kind"; return MPOPIS_ERR_ARG; }
    if (car && (cfg->num_cars < 1 || cfg->num_cars > kMaxCars)) { g_create_error = "num_cars must be 1..8"; return MPOPIS_ERR_ARG; }
    static_assert(kMaxCars == 8, "the message above names the bound");
    const int as = car ? 2 * cfg->num_cars : 1;
    if (const int rc = check_policy_config(cfg, as)) return rc;
    return create_handle(cfg, as, car ? 8 * cfg->num_cars : (cfg->env_kind == MPOPIS_ENV_CARTPOLE ? 4 : 2), out);
}

// A handle on a caller-supplied env (include/mpopis_env.h).  Every argument check comes before the first HIP call.
int mpopis_create_custom(const mpopis_config* cfg_in, const void* code_object, uint64_t nbytes, int32_t state_size, int32_t action_size, int32_t nparams,
                         const double* reset_state, mpopis_handle** out) {
    if (!cfg_in || !code_object || !out) { g_create_error = "null argument"; return MPOPIS_ERR_ARG; }
    *out = nullptr;
    static const char kElf[4] = {0x7f, 'E', 'L', 'F'}, kBundle[] = "__CLANG_OFFLOAD_BUNDLE__";
    if (nbytes < 64) { g_create_error = "mpopis_create_custom: code object too small (nbytes < 64)"; return MPOPIS_ERR_ARG; }
    if (memcmp(code_object, kElf, 4) != 0 && memcmp(code_object, kBundle, sizeof kBundle - 1) != 0) {
        g_create_error = "mpopis_create_custom: not a code object (neither an ELF nor a clang offload bundle: bad magic)"; return MPOPIS_ERR_ARG;
    }
    if (!code_object_complete((const unsigned char*)code_object, nbytes)) {
        g_create_error = "mpopis_create_custom: the code object is truncated (its own tables reach past nbytes)"; return MPOPIS_ERR_ARG;
    }
    if (state_size < 1 || state_size > MPOPIS_ENV_MAX_STATE) { g_create_error = "mpopis_create_custom: state_size must be 1..64"; return MPOPIS_ERR_ARG; }
    if (action_size < 1 || action_size > kMaxAs) { g_create_error = "mpopis_create_custom: action_size must be 1..16"; return MPOPIS_ERR_ARG; }
    if (nparams < 0 || nparams > MPOPIS_ENV_MAX_PARAMS) { g_create_error = "mpopis_create_custom: nparams must be 0..64"; return MPOPIS_ERR_ARG; }
    static_assert(MPOPIS_ENV_MAX_STATE == 64 && kMaxAs == 16 && MPOPIS_ENV_MAX_PARAMS == 64, "the messages above name the bounds");
    mpopis_config cfg = *cfg_in;
    cfg.env_kind = MPOPIS_ENV_CUSTOM; cfg.num_cars = 0;
    if (const int rc = check_policy_config(&cfg, action_size)) return rc;
    mpopis_handle* h = nullptr;
    if (const int rc = create_handle(&cfg, action_size, state_size, &h)) return rc;
    // the module belongs to the handle (two handles with different code objects coexist); mpopis_destroy unloads it
    hipError_t e = hipModuleLoadData(&h->custom.module, code_object);
    if (e != hipSuccess) { h->custom.module = nullptr; return fail_create(h, MPOPIS_ERR_ARG, std::string("mpopis_create_custom: the code object does not load on this device (hipModuleLoadData: ") + hipGetErrorString(e) + "); build it for gfx950"); }
    hipDeviceptr_t abi_ptr = nullptr; size_t abi_bytes = 0;
    int32_t abi[4] = {0, 0, 0, 0};
    if (hipModuleGetGlobal(&abi_ptr, &abi_bytes, h->custom.module, "mpopis_env_abi") != hipSuccess || abi_bytes != sizeof abi ||
        hipMemcpyDtoH(abi, abi_ptr, sizeof abi) != hipSuccess) {
        (void)hipGetLastError();
        return fail_create(h, MPOPIS_ERR_ARG, "mpopis_create_custom: the code object has no constant mpopis_env_abi (was it built with MPOPIS_DEFINE_ENV of mpopis_env.h?)");
    }
    if (abi[0] != MPOPIS_ENV_SDK_VERSION || abi[1] != state_size || abi[2] != action_size || abi[3] != nparams) {
        char buf[256];
        snprintf(buf, sizeof buf, "mpopis_create_custom: the code object was built with SDK version %d for state_size %d, action_size %d, nparams %d; the call says version %d, %d, %d, %d",
                 abi[0], abi[1], abi[2], abi[3], MPOPIS_ENV_SDK_VERSION, state_size, action_size, nparams);
        return fail_create(h, MPOPIS_ERR_ARG, buf);
    }
    // an env with a table (MPOPIS_DEFINE_ENV_TABLE) says so with a second constant and has four kernels under names of their own
    hipDeviceptr_t tab_ptr = nullptr; size_t tab_bytes = 0;
    int32_t tab_abi[2] = {0, 0};
    if (hipModuleGetGlobal(&tab_ptr, &tab_bytes, h->custom.module, "mpopis_env_table_abi") == hipSuccess) {
        if (tab_bytes != sizeof tab_abi || hipMemcpyDtoH(tab_abi, tab_ptr, sizeof tab_abi) != hipSuccess) {
            (void)hipGetLastError();
            return fail_create(h, MPOPIS_ERR_ARG, "mpopis_create_custom: the code object's constant mpopis_env_table_abi cannot be read (two int32 expected)");
        }
        if (tab_abi[0] != MPOPIS_ENV_TABLE_VERSION || tab_abi[1] < 0 || tab_abi[1] > kEnvTableLdsMaxDoubles) {
            char buf[256];
            snprintf(buf, sizeof buf, "mpopis_create_custom: the code object was built with env table version %d (LDS table limit %d doubles); this library knows version %d and stages at most %d",
                     tab_abi[0], tab_abi[1], MPOPIS_ENV_TABLE_VERSION, kEnvTableLdsMaxDoubles);
            return fail_create(h, MPOPIS_ERR_ARG, buf);
        }
        h->custom.has_table = true;
        h->custom.table_lds_doubles = tab_abi[1];
    } else {
        (void)hipGetLastError();
    }
    struct kernel_name { const char* name; hipFunction_t* fn; };
    const std::vector<kernel_name> kernels = h->custom.has_table
        ? std::vector<kernel_name>{{"mpopis_env_rollout_tab", &h->custom.rollout}, {"mpopis_env_rollout_gtab", &h->custom.rollout_gtab},
                                   {"mpopis_env_step_tab", &h->custom.step}, {"mpopis_env_query_tab", &h->custom.query}}
        : std::vector<kernel_name>{{"mpopis_env_rollout", &h->custom.rollout}, {"mpopis_env_step", &h->custom.step}, {"mpopis_env_query", &h->custom.query}};
    for (const auto& k : kernels)
        if (hipModuleGetFunction(k.fn, h->custom.module, k.name) != hipSuccess) {
            (void)hipGetLastError();
            return fail_create(h, MPOPIS_ERR_ARG, std::string("mpopis_create_custom: the code object has no kernel ") + k.name);
        }
    if (h->shared_alloc(h->custom.d_params, (size_t)nparams)) return fail_create(h, MPOPIS_ERR_HIP, h->err);      // zeros until mpopis_set_env_params
    h->custom.nparams = nparams;
    h->custom_reset.assign((size_t)state_size, 0.0);
    if (reset_state) memcpy(h->custom_reset.data(), reset_state, sizeof(double) * state_size);
    if (mpopis_reset(h) != 0) return fail_create(h, MPOPIS_ERR_HIP, h->err);
    *out = h;
    return MPOPIS_OK;
}

// the part of a create call that runs on the device; as / ss: action and state size of the env
static int create_handle(const mpopis_config* cfg, int as, int ss, mpopis_handle** out) {
    const bool car = cfg->env_kind == MPOPIS_ENV_CAR;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_error = "no HIP device available (the engine has no CPU fallback)"; return MPOPIS_ERR_HIP; }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_error = "bad device ordinal"; return MPOPIS_ERR_ARG; }
    mpopis_handle* h = new mpopis_handle();
    h->cfg = *cfg;
    auto streams_and_events = [&]() -> int {
        HIPCHK(h, hipSetDevice(cfg->device));
        HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        for (int i = 0; i < mpopis_handle::kMaxSplit - 1; ++i) {
            HIPCHK(h, hipStreamCreateWithFlags(&h->xstream[i], hipStreamNonBlocking));
            HIPCHK(h, hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
            HIPCHK(h, hipEventCreateWithFlags(&h->ev_skew[i], hipEventDisableTiming));
        }
        return MPOPIS_OK;
    };
    if (streams_and_events()) return fail_create(h, MPOPIS_ERR_HIP, h->err);
    if (const char* e = getenv("MPOPIS_DEBUG_LAUNCH")) h->debug_launch = atoi(e) != 0;
    if (const char* e = getenv("MPOPIS_NSPLIT")) { h->nsplit = std::max(1, std::min((int)mpopis_handle::kMaxSplit, atoi(e))); h->split_auto = false; h->split_pinned = true; }   // experiments / profiling: pins the schedule, mpopis_set_overlap is then ignored
    h->B = cfg->batch; h->B_full = cfg->batch; h->K = cfg->num_samples; h->T = cfg->horizon;
    h->as = as;
    h->ss = ss;
    h->cs = h->as * h->T;
    h->N = (cfg->policy == MPOPIS_POL_MPPI || cfg->policy == MPOPIS_POL_GMPPI) ? 1 : std::max(1, cfg->ais_its);
    h->gamma = cfg->lambda * (1 - cfg->alpha);
    h->env.kind = cfg->env_kind; h->env.ncars = car ? cfg->num_cars : 0; h->env.ss = h->ss; h->env.as = h->as;
    double p[20];
    default_car_params(p); h->env.car = make_car_params(p);
    default_mc_params(p); h->env.mc = make_mc_params(p);
    default_cp_params(p); h->env.cp = make_cp_params(p);
    for (int i = 0; i < kMaxAs; ++i) { h->env.lo[i] = -1.0; h->env.hi[i] = 1.0; }
    h->env.track = Track{nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr};
    h->env.custom = cfg->env_kind == MPOPIS_ENV_CUSTOM ? &h->custom : nullptr;
    const int B = h->B, K = h->K, cs = h->cs;
    const size_t nn = (size_t)cs * cs, per = (size_t)cs * K;
    h->ksplit = std::max(1, std::min(std::min(32, K / 128), std::max(1, 512 / B)));   // ~2-4 workgroups per CU in the scatter kernel
    if (const char* e = getenv("MPOPIS_KSPLIT")) h->ksplit = std::max(1, std::min(32, atoi(e)));
    // The handle's device buffers: this table is the record of the layout in HBM.  slot(p, n): [B][n] elements, one row per trial slot, moved by
    // shift_slots with exactly this n (the workspace sizes are their helpers' value for ONE slot; every helper is B times that);
    // shared(p, n): n elements for the whole batch.  A new per-slot buffer is one more slot(...) line here (or a slot_alloc where it is first
    // needed) and nothing else.  Matrices are column-major; E / Z are [cs][K] row-major by control row (engine.h).
    int rc = 0;
    auto slot = [&](auto*& p, size_t per_slot, size_t pad = 0) { rc |= h->slot_alloc(p, per_slot, pad); };
    auto shared = [&](auto*& p, size_t n) { rc |= h->shared_alloc(p, n); };
    slot(h->d_x, h->ss); slot(h->d_xext, kMaxCars * kCarExt); slot(h->d_t, 1); slot(h->d_done, 1);          // resident real-env state
    slot(h->d_U, cs); slot(h->d_Ucur, cs); slot(h->d_Uin, cs);                                               // pol.U, its rebinding inside a step, U_orig
    shared(h->S0sh.Sigma, nn); slot(h->d_Sig, nn, kInvsqrtPadDoubles); slot(h->d_L, nn);                     // Σ′ (readable a pad beyond the last slot: kernels_invsqrt.hip), its factor
    shared(h->S0sh.L, nn); slot(h->d_tmpS, nn);
    if (sample_trmm_fusable(cs)) { shared(h->S0sh.Lp, potrf_panel_doubles(cs)); slot(h->d_Lp, potrf_panel_doubles(cs)); }
    slot(h->d_coop_flags, potrf_coop_flag_words(1, cs)); slot(h->d_potrf_redo, 1); slot(h->d_lan_redo, 1); shared(h->d_coop_timeouts, 1);
    slot(h->d_Z, per); slot(h->d_E, per); slot(h->d_cost, K); slot(h->d_w, K);
    slot(h->d_wn, cs); slot(h->d_mu, cs); slot(h->d_gvec, cs);
    slot(h->d_dscale, cs); shared(h->d_dscale0, cs);
    slot(h->d_control, h->as); slot(h->d_reward, 1); slot(h->d_wsum, 1); slot(h->d_cmin, 1);
    slot(h->d_status, 1); slot(h->d_active, 1); slot(h->d_iters, 1); slot(h->d_iters_acc, 1);
    slot(h->d_seeds, 1); shared(h->d_rng_tab, mpopis::kRngTabDoubles);      // philox.h
    slot(h->d_order, K); slot(h->d_resi, K); slot(h->d_resu, K); slot(h->d_accept, K); slot(h->d_alias, K); slot(h->d_alias_need, 1);
    if (cfg->policy == MPOPIS_POL_PMCMPPI && K > alias_lds_max_K()) slot(h->d_alias_stack, 2 * (size_t)K);      // the global-workspace alias construction
    slot(h->d_residx_log, (size_t)std::max(1, h->N - 1) * K);
    slot(h->d_part, wcov_mfma_workspace_doubles(1, cs, h->ksplit));
    {
        static const int env_fold = [] { const char* e = getenv("MPOPIS_FOLD_WEIGHTS"); return e ? atoi(e) : 1; }();      // 0: keep the separate reweighting launch (A/B)
        h->weights_in_moments = env_fold && cfg->policy == MPOPIS_POL_MUSIGMAAISMPPI && cfg->env_kind == MPOPIS_ENV_CAR && wcov_weights_from_cost_ok(cs, K, h->ksplit);
        h->fold_weights_cfg = h->weights_in_moments;
    }
    if (cfg->policy == MPOPIS_POL_CMAMPPI) {
        slot(h->d_cma_scal, 8); slot(h->d_cma_vec, 3 * (size_t)cs); slot(h->d_sig2, 1); shared(h->d_cma_ws, K);
        h->lan_regions = invsqrt_coop_groups(B, cs);
        slot(h->d_lanV, invsqrt_workspace_doubles(1, cs, h->lan_regions)); slot(h->d_lan_x, invsqrt_coop_words(1, cs)); slot(h->d_Cdw, cs);
        slot(h->d_fro_part, (cs + 15) / 16); slot(h->d_tri_dinv, trtri_dinv_doubles(1, cs)); slot(h->d_fro, 1); slot(h->d_lan_m, 1); slot(h->d_lan_prep, lanczos_prep_doubles(1)); slot(h->d_tri_cnt, 2);
    }
    if (cfg->policy == MPOPIS_POL_NESMPPI) {
        shared(h->S0sh.nesA, nn); shared(h->S0sh.nesS, nn); slot(h->d_nesS, nn);
        slot(h->d_nesA[0], nn); slot(h->d_nesA[1], nn); slot(h->d_nesM, nn);
        slot(h->d_nesg, cs); slot(h->d_nesC, 1); slot(h->d_nespart, nes_scatter_workspace_doubles(1, cs, h->ksplit));
    }
    if (cfg->log_trajectories) slot(h->d_traj, (size_t)K * h->T * h->ss);
    h->slot_view(h->alive_gate, 1);                             // run_trials' gate: d_alive for the length of a step, else null
    if (rc) return fail_create(h, MPOPIS_ERR_HIP, h->err);
    h->S0 = h->S0sh;
    launch_rng_tab_init(h->d_rng_tab, h->stream);
    h->h_status.assign(B, 0);
    if (hipHostMalloc((void**)&h->h_pin, sizeof(double) * B * (h->as + 2)) != hipSuccess) h->h_pin = nullptr;
    if (hipHostMalloc((void**)&h->h_call, call_box_bytes(B, h->ss, cs, h->as), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h->d_call, h->h_call, 0) != hipSuccess) { if (h->h_call) (void)hipHostFree(h->h_call); h->h_call = nullptr; h->d_call = nullptr; }
    if (h->h_call) memset(h->h_call, 0, call_box_bytes(B, h->ss, cs, h->as));
    if (hipHostMalloc((void**)&h->h_coop_timeouts, sizeof(int)) != hipSuccess) h->h_coop_timeouts = nullptr; else *h->h_coop_timeouts = 0;
    if (const char* e = getenv("MPOPIS_NO_COOP")) h->coop_disabled = atoi(e) != 0;
    // Σ default = I (cov_mat default [1.0], src/mppi_mpopi_policies.jl:42) ; seeds
    const int n0 = (cfg->policy == MPOPIS_POL_MPPI) ? h->as : cs;
    std::vector<double> eye((size_t)n0 * n0, 0.0);
    for (int i = 0; i < n0; ++i) eye[(size_t)i * n0 + i] = 1.0;
    if (mpopis_set_Sigma(h, eye.data(), n0) != 0) return fail_create(h, MPOPIS_ERR_HIP, h->err);
    if (mpopis_seed(h, cfg->seed) != 0) return fail_create(h, MPOPIS_ERR_HIP, h->err);
    if (mpopis_reset(h) != 0) return fail_create(h, MPOPIS_ERR_HIP, h->err);
    if (cfg->policy == MPOPIS_POL_CMAMPPI) {
        h->init_cma_constants();
        if ((long long)cs * h->m_elite < K) return fail_create(h, MPOPIS_ERR_ARG, "BoundsError: δs[order[ii]] needs cs*m_elite >= K (src/mppi_mpopi_policies.jl:593)");
        if (hipMemcpy(h->d_cma_ws, h->cma_ws_host.data(), sizeof(double) * K, hipMemcpyHostToDevice) != hipSuccess) return fail_create(h, MPOPIS_ERR_HIP, "upload failed");
    }
    if (cfg->policy == MPOPIS_POL_CEMPPI) h->m_elite = (int)nearbyint(K * (1 - cfg->elite_threshold));   // :437
    // (no upper limit on K: beyond K = 8192 the sort is the chunked chip-wide rank sort, beyond 7168 the alias table is built on global arrays --
    // the reference's sortperm / Categorical take any K, :455, :804)
    *out = h;
    return MPOPIS_OK;
}

void mpopis_destroy(mpopis_handle* h) {
    if (!h) return;
    if (h->comm) (void)mpopis_comm_destroy(h);
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto st : h->xstream) if (st) (void)hipStreamSynchronize(st);
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->custom.d_table) (void)hipFree(h->custom.d_table);
    if (h->plan.base) (void)hipFree(h->plan.base);
    if (h->custom.module) (void)hipModuleUnload(h->custom.module);
    if (h->h_pin) (void)hipHostFree(h->h_pin);
    if (h->h_call) (void)hipHostFree(h->h_call);
    if (h->h_coop_timeouts) (void)hipHostFree(h->h_coop_timeouts);
    for (auto e : h->events) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    for (auto st : h->xstream) if (st) (void)hipStreamDestroy(st);
    for (auto st : h->rejected_streams) if (st) (void)hipStreamDestroy(st);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (auto e : h->ev_join) if (e) (void)hipEventDestroy(e);
    for (auto e : h->ev_skew) if (e) (void)hipEventDestroy(e);
    delete h;
}

int mpopis_set_env_params(mpopis_handle* h, const double* p, int32_t n) {
    if (h) h->plan_drop("mpopis_set_env_params");
    if (!h || !p) return MPOPIS_ERR_ARG;
    if (h->env.kind == MPOPIS_ENV_CUSTOM) {
        if (n != h->custom.nparams) { h->err = "custom env expects " + std::to_string(h->custom.nparams) + " parameters"; return MPOPIS_ERR_ARG; }
        HIPCHK(h, hipSetDevice(h->cfg.device));
        HIPCHK(h, hipMemcpyAsync(h->custom.d_params, p, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, wait_stream(h->stream));
    } else if (h->env.kind == MPOPIS_ENV_CAR) {
        if (n != MPOPIS_CAR_NPARAMS) { h->err = "car env expects 20 parameters"; return MPOPIS_ERR_ARG; }
        h->env.car = make_car_params(p);
    } else if (h->env.kind == MPOPIS_ENV_CARTPOLE) {
        if (n != MPOPIS_CARTPOLE_NPARAMS) { h->err = "CartPole expects 11 parameters"; return MPOPIS_ERR_ARG; }
        h->env.cp = make_cp_params(p);
    } else {
        if (n != MPOPIS_MOUNTAINCAR_NPARAMS) { h->err = "MountainCar expects 8 parameters"; return MPOPIS_ERR_ARG; }
        h->env.mc = make_mc_params(p);
    }
    if (h->env_params_slots_on || h->track_slots_on || h->fleet_on) {      // (after mpopis_set_env_params_slots / _cars: back to one shared vector)
        if (const int rc = quiesce(h)) return rc;
        h->env_params_slots_on = false; h->fleet_on = false;
        return h->sync_slot_env();
    }
    return MPOPIS_OK;
}

// Car handles: while exactly one of the per-slot arrays is in force, fill the other with B copies of the shared value (engine_handle.h).  The caller
// has quiesced the handle.  (A shared track that is not set yet gives descriptors with P = 0: track_missing() then refuses the calls that need one.)
int mpopis_handle::sync_slot_env() {
    if (env.kind != MPOPIS_ENV_CAR) return MPOPIS_OK;
    const bool params_on = env_params_slots_on || fleet_on;
    if (track_slots_on ? params_on : !(params_on || scen_M > 0)) return MPOPIS_OK;      // (a scenario handle's rollouts read the track array too)
    const char* msg = "hipMalloc of the per-slot env arrays failed";
    if (track_slots_on) {
        if (slot_alloc(d_car_sl, 1)) { (void)hipGetLastError(); err = msg; return MPOPIS_ERR_HIP; }
        const std::vector<CarParams> host((size_t)B_full, env.car);
        HIPCHK(this, hipMemcpyAsync(d_car_sl, host.data(), sizeof(CarParams) * B_full, hipMemcpyHostToDevice, stream));
    } else {
        if (slot_alloc(d_track_sl, 1)) { (void)hipGetLastError(); err = msg; return MPOPIS_ERR_HIP; }
        const std::vector<Track> host((size_t)B_full, env.track);
        HIPCHK(this, hipMemcpyAsync(d_track_sl, host.data(), sizeof(Track) * B_full, hipMemcpyHostToDevice, stream));
        track_sl_lds_all = track_lds_bytes(env.track.P, env.track.nbrw, true); track_sl_lds_ring = track_lds_bytes(env.track.P, env.track.nbrw, false);
    }
    HIPCHK(this, hipStreamSynchronize(stream));
    return MPOPIS_OK;
}

// One parameter vector per slot.  A setup call: the [B] struct array is written only after everything queued has finished (the rollout kernels read
// it through the constant address space).  Everything is checked and formed on the host first, so a refused call changes nothing.
int mpopis_set_env_params_slots(mpopis_handle* h, const double* p, int32_t n) {
    if (h) h->plan_drop("mpopis_set_env_params_slots");
    if (!h) return MPOPIS_ERR_ARG;
    if (!p) { h->err = "mpopis_set_env_params_slots: p is NULL"; return MPOPIS_ERR_ARG; }
    const int kind = h->env.kind, B = h->B_full;
    if (kind == MPOPIS_ENV_CUSTOM) {
        h->err = "mpopis_set_env_params_slots: not for a custom handle (per-slot data of a custom env goes through mpopis_set_env_table(..., per_slot))";
        return MPOPIS_ERR_ARG;
    }
    const int want = kind == MPOPIS_ENV_CAR ? MPOPIS_CAR_NPARAMS : kind == MPOPIS_ENV_CARTPOLE ? MPOPIS_CARTPOLE_NPARAMS : MPOPIS_MOUNTAINCAR_NPARAMS;
    if (n != want) {
        h->err = "mpopis_set_env_params_slots: this env expects " + std::to_string(want) + " parameters per slot, got n = " + std::to_string(n);
        return MPOPIS_ERR_ARG;
    }
    if (const int rc = quiesce(h)) return rc;
    auto upload = [&](auto*& dst, auto make) -> int {
        std::vector<std::remove_reference_t<decltype(*dst)>> host((size_t)B);
        for (int b = 0; b < B; ++b) host[b] = make(p + (size_t)b * n);
        if (h->slot_alloc(dst, 1)) { (void)hipGetLastError(); h->err = "mpopis_set_env_params_slots: hipMalloc of the per-slot parameter array failed"; return MPOPIS_ERR_HIP; }
        HIPCHK(h, hipMemcpyAsync(dst, host.data(), sizeof(host[0]) * B, hipMemcpyHostToDevice, h->stream));      // (behind the buffer's zero-fill)
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return MPOPIS_OK;
    };
    int rc;
    if (kind == MPOPIS_ENV_CAR) rc = upload(h->d_car_sl, [](const double* q) { return make_car_params(q); });
    else if (kind == MPOPIS_ENV_CARTPOLE) rc = upload(h->d_cp_sl, [](const double* q) { return make_cp_params(q); });
    else rc = upload(h->d_mc_sl, [](const double* q) { return make_mc_params(q); });
    if (rc) return rc;
    const bool was = h->env_params_slots_on, was_fleet = h->fleet_on;
    h->env_params_slots_on = true; h->fleet_on = false;        // (a fleet ends here: one vector per slot again)
    if ((rc = h->sync_slot_env())) { h->env_params_slots_on = was; h->fleet_on = was_fleet; }
    return rc;
}

// One parameter vector per CAR of a multi-car slot: env.envs[c] of the reference's MultiCarRacingEnv owns its params
// (multi-car_racing.jl:23-45).  A setup call like the one above; the [B][num_cars] struct array and the [B] track array the fleet rollout reads
// beside it are both allocated before either is written, so nothing fails past that point but a copy on a quiesced stream.
int mpopis_set_env_params_cars(mpopis_handle* h, const double* p, int32_t n, int32_t per_slot) {
    if (h) h->plan_drop("mpopis_set_env_params_cars");
    if (!h) return MPOPIS_ERR_ARG;
    if (!p) { h->err = "mpopis_set_env_params_cars: p is NULL"; return MPOPIS_ERR_ARG; }
    if (h->env.kind == MPOPIS_ENV_CUSTOM) { h->err = "mpopis_set_env_params_cars: not for a custom handle (a custom env has no cars)"; return MPOPIS_ERR_ARG; }
    if (h->env.kind != MPOPIS_ENV_CAR) { h->err = "mpopis_set_env_params_cars: not a car handle (only MultiCarRacingEnv holds several cars)"; return MPOPIS_ERR_ARG; }
    if (h->scen_M > 0) { h->err = "mpopis_set_env_params_cars: not on a scenario handle (all cars of a slot share the scenario's vector; end the mode with mpopis_set_scenarios(h, 0, ...) first)"; return MPOPIS_ERR_ARG; }
    if (n != MPOPIS_CAR_NPARAMS) { h->err = "mpopis_set_env_params_cars: a car expects 20 parameters, got n = " + std::to_string(n); return MPOPIS_ERR_ARG; }
    const int B = h->B_full, NC = h->env.ncars;
    if (NC == 1) return per_slot ? mpopis_set_env_params_slots(h, p, n) : mpopis_set_env_params(h, p, n);      // one car: the existing forms and kernels
    const int nb = per_slot ? B : 1;
    for (int b = 0; b < nb; ++b)
        for (int c = 1; c < NC; ++c) {
            const double *q0 = p + (size_t)b * NC * n, *q = q0 + (size_t)c * n;
            if (q[18] != q0[18] || q[19] != q0[19]) {          // MultiCarRacingEnv has ONE dt / δt (:26-45)
                h->err = "mpopis_set_env_params_cars: dt / δt of slot " + std::to_string(b) + ", car " + std::to_string(c) + " differ from those of the slot's car 0 (a MultiCarRacingEnv has one dt and one δt for all its cars)";
                return MPOPIS_ERR_ARG;
            }
        }
    if (const int rc = quiesce(h)) return rc;
    std::vector<CarParams> host((size_t)B * NC);
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < NC; ++c) host[(size_t)b * NC + c] = make_car_params(p + ((size_t)(per_slot ? b : 0) * NC + c) * n);
    if (h->slot_alloc(h->d_cars_sl, NC) || h->slot_alloc(h->d_track_sl, 1)) { (void)hipGetLastError(); h->err = "mpopis_set_env_params_cars: hipMalloc of the fleet's parameter array failed"; return MPOPIS_ERR_HIP; }
    HIPCHK(h, hipMemcpyAsync(h->d_cars_sl, host.data(), sizeof(CarParams) * host.size(), hipMemcpyHostToDevice, h->stream));      // (behind the buffer's zero-fill)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const bool was = h->env_params_slots_on, was_fleet = h->fleet_on;
    h->env_params_slots_on = false; h->fleet_on = true;
    const int rc = h->sync_slot_env();
    if (rc) { h->env_params_slots_on = was; h->fleet_on = was_fleet; }
    return rc;
}

// M model parameter vectors per slot for the rollouts of a policy step.  A setup call like mpopis_set_env_params_slots:
// everything is checked and formed on the host first, new buffers (first call, or M beyond what is allocated) are all allocated before the handle
// changes, and the struct planes are written only after everything queued has finished.
int mpopis_set_scenarios(mpopis_handle* h, int32_t M, const double* p, int32_t n, int32_t per_slot) {
    if (h) h->plan_drop("mpopis_set_scenarios");
    if (!h) return MPOPIS_ERR_ARG;
    const int kind = h->env.kind, B = h->B_full;
    if (M < 0 || M > MPOPIS_MAX_SCENARIOS) { h->err = "mpopis_set_scenarios: M must be 0.." + std::to_string(MPOPIS_MAX_SCENARIOS) + ", got " + std::to_string(M); return MPOPIS_ERR_ARG; }
    if (kind == MPOPIS_ENV_CUSTOM) { h->err = "mpopis_set_scenarios: not for a custom handle (its parameters belong to the caller's code object)"; return MPOPIS_ERR_ARG; }
    if (M == 0) {
        if (h->scen_M == 0) return MPOPIS_OK;
        if (const int rc = quiesce(h)) return rc;
        h->scen_M = 0; h->risk_kind = MPOPIS_RISK_TAIL_MEAN; h->risk_tail = 0; h->risk_theta = 0.0;
        return MPOPIS_OK;
    }
    if (!p) { h->err = "mpopis_set_scenarios: p is NULL with M > 0"; return MPOPIS_ERR_ARG; }
    const int want = kind == MPOPIS_ENV_CAR ? MPOPIS_CAR_NPARAMS : kind == MPOPIS_ENV_CARTPOLE ? MPOPIS_CARTPOLE_NPARAMS : MPOPIS_MOUNTAINCAR_NPARAMS;
    if (n != want) {
        h->err = "mpopis_set_scenarios: this env expects " + std::to_string(want) + " parameters per scenario, got n = " + std::to_string(n);
        return MPOPIS_ERR_ARG;
    }
    if (h->d_traj) { h->err = "mpopis_set_scenarios: not on a handle created with log_trajectories (the logger holds one trajectory per sample, a scenario step rolls M)"; return MPOPIS_ERR_ARG; }
    if (h->fleet_on) { h->err = "mpopis_set_scenarios: not on a fleet handle (mpopis_set_env_params_cars in force; all cars of a slot share the scenario's vector)"; return MPOPIS_ERR_ARG; }
    if (const int rc = quiesce(h)) return rc;
    const char* nomem = "mpopis_set_scenarios: hipMalloc of the scenario buffers failed";
    const size_t planes = (size_t)std::max(M, h->scen_cap);
    auto upload = [&](auto*& dst, auto make) -> int {
        using P = std::remove_reference_t<decltype(*dst)>;
        std::vector<P> host((size_t)M * B);
        for (int m = 0; m < M; ++m)
            for (int b = 0; b < B; ++b) host[(size_t)m * B + b] = make(p + ((size_t)(per_slot ? b : 0) * M + m) * n);
        P* par = dst; double* cost = h->d_scen_cost;
        if (M > h->scen_cap) {                                 // both allocated before either replaces what the handle holds
            void *q = nullptr, *c = nullptr;
            if (h->dev_alloc(&q, planes * B * sizeof(P)) || h->dev_alloc(&c, planes * B * h->K * sizeof(double))) { (void)hipGetLastError(); h->err = nomem; return MPOPIS_ERR_HIP; }
            par = (P*)q; cost = (double*)c;
        }
        HIPCHK(h, hipMemcpyAsync(par, host.data(), sizeof(P) * host.size(), hipMemcpyHostToDevice, h->stream));      // (behind the buffer's zero-fill)
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (!h->scen_cap) { h->slot_view(dst, 1); h->slot_view(h->d_scen_cost, (size_t)h->K); }      // (registered once: the members keep their addresses)
        dst = par; h->d_scen_cost = cost; h->scen_cap = (int)planes;
        return MPOPIS_OK;
    };
    int rc;
    if (kind == MPOPIS_ENV_CAR) rc = upload(h->d_scen_car, [](const double* q) { return make_car_params(q); });
    else if (kind == MPOPIS_ENV_CARTPOLE) rc = upload(h->d_scen_cp, [](const double* q) { return make_cp_params(q); });
    else rc = upload(h->d_scen_mc, [](const double* q) { return make_mc_params(q); });
    if (rc) return rc;
    const int was = h->scen_M;
    h->scen_M = M;
    if ((rc = h->sync_slot_env())) { h->scen_M = was; return rc; }
    h->risk_kind = MPOPIS_RISK_TAIL_MEAN; h->risk_tail = M; h->risk_theta = 0.0;
    return MPOPIS_OK;
}

int mpopis_set_risk(mpopis_handle* h, int32_t kind, int32_t tail, double theta) {
    if (h) h->plan_drop("mpopis_set_risk");
    if (!h) return MPOPIS_ERR_ARG;
    const int M = h->scen_M;
    if (M == 0) { h->err = "mpopis_set_risk: no scenarios set (mpopis_set_scenarios first)"; return MPOPIS_ERR_ARG; }
    if (kind == MPOPIS_RISK_TAIL_MEAN) {
        if (tail < 0 || tail > M) { h->err = "mpopis_set_risk: tail must be 0.." + std::to_string(M) + " (0 = all), got " + std::to_string(tail); return MPOPIS_ERR_ARG; }
    } else if (kind == MPOPIS_RISK_ENTROPIC) {
        if (!(theta != 0.0) || !(std::fabs(theta) < INFINITY)) { h->err = "mpopis_set_risk: theta must be finite and non-zero"; return MPOPIS_ERR_ARG; }
    } else { h->err = "mpopis_set_risk: unknown kind " + std::to_string(kind); return MPOPIS_ERR_ARG; }
    if (const int rc = quiesce(h)) return rc;
    h->risk_kind = kind;
    h->risk_tail = kind == MPOPIS_RISK_TAIL_MEAN ? (tail ? tail : M) : M;
    h->risk_theta = kind == MPOPIS_RISK_ENTROPIC ? theta : 0.0;
    return MPOPIS_OK;
}

int mpopis_get_scenarios(mpopis_handle* h, int32_t* M, int32_t* kind, int32_t* tail, double* theta) {
    if (!h) return MPOPIS_ERR_ARG;
    if (M) *M = h->scen_M;
    if (kind) *kind = h->risk_kind;
    if (tail) *tail = h->risk_tail;
    if (theta) *theta = h->risk_theta;
    return MPOPIS_OK;
}

// out[b][m][k] from the planes [m][B_full][K]: one strided copy per scenario
int mpopis_get_scenario_costs(mpopis_handle* h, double* out) {
    if (!h) return MPOPIS_ERR_ARG;
    if (!out) { h->err = "mpopis_get_scenario_costs: out is NULL"; return MPOPIS_ERR_ARG; }
    if (h->scen_M == 0) { h->err = "mpopis_get_scenario_costs: no scenarios set"; return MPOPIS_ERR_ARG; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t B = (size_t)h->B_full, K = (size_t)h->K, M = (size_t)h->scen_M;
    for (size_t m = 0; m < M; ++m)
        HIPCHK(h, hipMemcpy2DAsync(out + m * K, sizeof(double) * M * K, h->d_scen_cost + m * B * K, sizeof(double) * K, sizeof(double) * K, B,
                                   hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    return MPOPIS_OK;
}

// The table of a caller's env (MPOPIS_DEFINE_ENV_TABLE).  A setup call: it waits for everything the handle has queued, on the part-chain streams
// too, before the buffer is written or replaced -- the global-memory rollout kernel reads the table through the constant address space, which
// holds only while nothing writes it under a running kernel.
int mpopis_set_env_table(mpopis_handle* h, const double* data, int64_t n, int32_t per_slot) {
    if (h) h->plan_drop("mpopis_set_env_table");
    if (!h) return MPOPIS_ERR_ARG;
    if (h->env.kind != MPOPIS_ENV_CUSTOM) { h->err = "mpopis_set_env_table: not a custom handle (only an env built with MPOPIS_DEFINE_ENV_TABLE of mpopis_env.h takes a table)"; return MPOPIS_ERR_ARG; }
    if (!h->custom.has_table) { h->err = "mpopis_set_env_table: the handle's code object has no mpopis_env_table_abi (build the env with MPOPIS_DEFINE_ENV_TABLE)"; return MPOPIS_ERR_ARG; }
    if (n < 0 || n > MPOPIS_ENV_MAX_TABLE) { h->err = "mpopis_set_env_table: n must be 0.." + std::to_string(MPOPIS_ENV_MAX_TABLE) + " doubles per slot"; return MPOPIS_ERR_ARG; }
    if (n > 0 && !data) { h->err = "mpopis_set_env_table: data is NULL with n > 0"; return MPOPIS_ERR_ARG; }
    if (const int rc = quiesce(h)) return rc;
    mpopis::CustomEnv& ce = h->custom;
    const size_t total = (size_t)n * (per_slot ? (size_t)h->B_full : 1);
    if (total > ce.table_cap) {
        double* d = nullptr;
        HIPCHK(h, hipMalloc((void**)&d, total * sizeof(double)));
        if (ce.d_table) (void)hipFree(ce.d_table);
        ce.d_table = d; ce.table_cap = total;
    }
    if (total) HIPCHK(h, hipMemcpy(ce.d_table, data, total * sizeof(double), hipMemcpyHostToDevice));
    ce.ntab = (int)n;
    ce.table_stride = per_slot ? n : 0;
    ce.table_view = n ? ce.d_table : nullptr;
    return MPOPIS_OK;
}

// one track to the device: x, y, w, |q|^2, the neighbour tables and the ring table with its certificates (car_dynamics.h: TrackHost decides the
// layout); *out = its descriptor
static int upload_track(mpopis_handle* h, const double* x, const double* y, const double* w, int32_t P, Track* out) {
    const TrackHost th(P, x, y, w);
    double *d = nullptr, *dnd = nullptr, *dring = nullptr; int* dni = nullptr;
    if (h->shared_alloc(d, th.xy.size()) || h->shared_alloc(dnd, th.nd.size()) || h->shared_alloc(dni, th.ni.size()) || h->shared_alloc(dring, th.ring.size())) return MPOPIS_ERR_HIP;
    HIPCHK(h, hipMemcpyAsync(d, th.xy.data(), sizeof(double) * th.xy.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dnd, th.nd.data(), sizeof(double) * th.nd.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dni, th.ni.data(), sizeof(int) * th.ni.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dring, th.ring.data(), sizeof(double) * th.ring.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    *out = th.view(d, dni, dnd, dring);
    return MPOPIS_OK;
}

int mpopis_set_track(mpopis_handle* h, const double* x, const double* y, const double* w, int32_t P) {
    if (h) h->plan_drop("mpopis_set_track");
    if (!h || !x || !y || !w || P < 2 || P > mpopis::kMaxTrackPoints) { if (h) h->err = "bad track (need 2 <= P <= 2048 points)"; return MPOPIS_ERR_ARG; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    Track tk;
    if (const int rc = upload_track(h, x, y, w, P, &tk)) return rc;
    if (h->env_params_slots_on || h->track_slots_on || h->fleet_on || h->scen_M > 0) {      // (after mpopis_set_tracks: back to one shared track)
        if (const int rc = quiesce(h)) return rc;
        h->env.track = tk;
        h->track_slots_on = false;
        return h->sync_slot_env();
    }
    h->env.track = tk;
    return MPOPIS_OK;
}

// ntracks tracks, each uploaded once; slot b's descriptor is a copy of that of track track_of_slot[b].  Like mpopis_set_track, every call uploads
// into fresh buffers that the handle keeps until mpopis_destroy (a launch still queued may read the old ones): ~170 B per track point per call.  A setup call like mpopis_set_env_params_slots;
// the handle changes only once every track is on the device.
int mpopis_set_tracks(mpopis_handle* h, int32_t ntracks, const int32_t* P, const double* x, const double* y, const double* w, const int32_t* track_of_slot) {
    if (h) h->plan_drop("mpopis_set_tracks");
    if (!h) return MPOPIS_ERR_ARG;
    const int B = h->B_full;
    if (h->env.kind != MPOPIS_ENV_CAR) { h->err = "mpopis_set_tracks: not a car handle (only the car env drives on a track)"; return MPOPIS_ERR_ARG; }
    if (!P || !x || !y || !w) { h->err = "mpopis_set_tracks: P, x, y or w is NULL"; return MPOPIS_ERR_ARG; }
    if (ntracks < 1) { h->err = "mpopis_set_tracks: need at least one track"; return MPOPIS_ERR_ARG; }
    if (!track_of_slot && ntracks != B) { h->err = "mpopis_set_tracks: without track_of_slot there must be one track per slot (" + std::to_string(B) + "), got " + std::to_string(ntracks); return MPOPIS_ERR_ARG; }
    for (int i = 0; i < ntracks; ++i)
        if (P[i] < 2 || P[i] > mpopis::kMaxTrackPoints) { h->err = "mpopis_set_tracks: bad track " + std::to_string(i) + " (need 2 <= P <= 2048 points, got " + std::to_string(P[i]) + ")"; return MPOPIS_ERR_ARG; }
    if (track_of_slot)
        for (int b = 0; b < B; ++b)
            if (track_of_slot[b] < 0 || track_of_slot[b] >= ntracks) { h->err = "mpopis_set_tracks: track_of_slot of slot " + std::to_string(b) + " is " + std::to_string(track_of_slot[b]) + " (need 0.." + std::to_string(ntracks - 1) + ")"; return MPOPIS_ERR_ARG; }
    if (const int rc = quiesce(h)) return rc;
    std::vector<Track> tks((size_t)ntracks);
    size_t off = 0, lds_all = 0, lds_ring = 0;
    for (int i = 0; i < ntracks; ++i) {
        if (const int rc = upload_track(h, x + off, y + off, w + off, P[i], &tks[i])) return rc;
        off += (size_t)P[i];
    }
    std::vector<Track> host((size_t)B);
    for (int b = 0; b < B; ++b) host[b] = tks[track_of_slot ? track_of_slot[b] : b];
    slot_tracks_lds(host.data(), host.size(), &lds_all, &lds_ring);
    // both arrays are allocated before either is written: past this point nothing can fail but a copy on a quiesced stream
    if (h->slot_alloc(h->d_track_sl, 1) || h->slot_alloc(h->d_car_sl, 1)) { (void)hipGetLastError(); h->err = "mpopis_set_tracks: hipMalloc of the per-slot env arrays failed"; return MPOPIS_ERR_HIP; }
    HIPCHK(h, hipMemcpyAsync(h->d_track_sl, host.data(), sizeof(Track) * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->track_sl_lds_all = lds_all; h->track_sl_lds_ring = lds_ring;
    h->track_slots_on = true;
    return h->sync_slot_env();
}

int mpopis_set_action_bounds(mpopis_handle* h, const double* lo, const double* hi) {
    if (h) h->plan_drop("mpopis_set_action_bounds");
    if (!h || !lo || !hi) return MPOPIS_ERR_ARG;
    for (int i = 0; i < h->as; ++i) { h->env.lo[i] = lo[i]; h->env.hi[i] = hi[i]; }
    return MPOPIS_OK;
}

int mpopis_reset(mpopis_handle* h) {
    if (h) h->plan_drop("mpopis_reset");
    if (!h) return MPOPIS_ERR_ARG;
    std::vector<double> x((size_t)h->B * h->ss, 0.0);
    for (int b = 0; b < h->B; ++b) {
        double* s = x.data() + (size_t)b * h->ss;
        if (h->env.kind == MPOPIS_ENV_CUSTOM) {
            if (!h->custom_reset.empty()) memcpy(s, h->custom_reset.data(), sizeof(double) * h->ss);      // reset_state of mpopis_create_custom
        } else if (h->env.kind == MPOPIS_ENV_CAR) {
            for (int c = 0; c < h->env.ncars; ++c) {            // car_racing.jl:215-223; multi-car_racing.jl:160-180
                const int ii = c + 1;
                if (ii >= 2) s[8 * c] = (ii % 2 == 0) ? (ii / 2.0 * 5.0) : ((1 - ii) / 2.0 * 5.0);
                s[8 * c + 2] = 90.0 * (M_PI / 180.0);
                s[8 * c + 3] = 10.0;
            }
        } else if (h->env.kind == MPOPIS_ENV_MOUNTAINCAR) { s[0] = -0.5; s[1] = 0.0; }   // reference: x ~ U(-0.6,-0.4) from an unseeded RNG
        // CartPole: reference draws 0.1*rand(4) - 0.05; deterministic centre = all zeros
    }
    std::vector<int> z(h->B, 0);
    const int rc = mpopis_set_state(h, x.data(), z.data(), z.data());
    h->plan_drop("mpopis_reset");
    return rc;
}

int mpopis_set_state(mpopis_handle* h, const double* x, const int32_t* t, const int32_t* done) {
    if (h) h->plan_drop("mpopis_set_state");
    if (!h || !x) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_x, x, sizeof(double) * h->B * h->ss, hipMemcpyHostToDevice, h->stream));
    if (t) HIPCHK(h, hipMemcpyAsync(h->d_t, t, sizeof(int) * h->B, hipMemcpyHostToDevice, h->stream));
    if (done) HIPCHK(h, hipMemcpyAsync(h->d_done, done, sizeof(int) * h->B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    return MPOPIS_OK;
}

int mpopis_get_state(mpopis_handle* h, double* x, int32_t* t, int32_t* done) {
    if (!h) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (x) HIPCHK(h, hipMemcpyAsync(x, h->d_x, sizeof(double) * h->B * h->ss, hipMemcpyDeviceToHost, h->stream));
    if (t) HIPCHK(h, hipMemcpyAsync(t, h->d_t, sizeof(int) * h->B, hipMemcpyDeviceToHost, h->stream));
    if (done) HIPCHK(h, hipMemcpyAsync(done, h->d_done, sizeof(int) * h->B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    return MPOPIS_OK;
}

int mpopis_set_U(mpopis_handle* h, const double* U) {
    if (h) h->plan_drop("mpopis_set_U");
    if (!h || !U) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_U, U, sizeof(double) * h->B * h->cs, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    return MPOPIS_OK;
}
int mpopis_get_U(mpopis_handle* h, double* U) {
    if (!h || !U) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(U, h->d_U, sizeof(double) * h->B * h->cs, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    return MPOPIS_OK;
}

// One routine sets pol.Σ, shared (one matrix for every slot, stride 0) or per slot (B matrices).  Everything is formed in buffers that are scratch
// outside a policy step (d_tmpS: the matrices; d_L / d_Lp: their factors and panels; :nesmppi d_nesA[0] / d_nesA[1]: sqrt(Σ) and Σ^-1, with d_nesM /
// d_nesS under them) and copied into the destination set only when every matrix has passed, so a refused call leaves the handle as it was.
static int set_Sigma0(mpopis_handle* h, const double* Sigma, int32_t n, bool per_slot) {
    const int cs = h->cs, as = h->as, B = h->B_full, M = per_slot ? B : 1;
    const size_t nn = (size_t)cs * cs, pd = sample_trmm_fusable(cs) ? potrf_panel_doubles(cs) : 0;
    const bool nes = h->cfg.policy == MPOPIS_POL_NESMPPI;
    auto of_slot = [per_slot](int b) { return per_slot ? " of slot " + std::to_string(b) : std::string(); };
    if (!((n == cs && h->cfg.policy != MPOPIS_POL_MPPI) || n == as)) { h->err = "Covariance matrix size problem"; return MPOPIS_ERR_ARG; }     // :79
    std::vector<double> full((size_t)M * nn, 0.0), ds((size_t)M * cs, 0.0);
    std::vector<char> slot_diag(M, 1);
    bool diag = true;
    for (int b = 0; b < M; ++b) {
        const double* Sb = Sigma + (size_t)b * n * n;
        double* fb = full.data() + (size_t)b * nn;
        if (n == cs && h->cfg.policy != MPOPIS_POL_MPPI) memcpy(fb, Sb, sizeof(double) * nn);
        else
            for (int t = 0; t < h->T; ++t)
                for (int j = 0; j < as; ++j)
                    for (int i = 0; i < as; ++i) fb[(size_t)(t * as + i) + (size_t)(t * as + j) * cs] = Sb[i + (size_t)j * as];
        for (int j = 0; j < cs && slot_diag[b]; ++j) for (int i = 0; i < cs; ++i) if (i != j && fb[(size_t)i + (size_t)j * cs] != 0.0) { slot_diag[b] = 0; break; }
        if (slot_diag[b])
            for (int i = 0; i < cs; ++i) {
                const double v = fb[(size_t)i * (cs + 1)];
                if (!(v > 0.0)) { h->err = "PosDefException: Sigma" + of_slot(b); return MPOPIS_ERR_NOT_PD; }
                ds[(size_t)b * cs + i] = sqrt(v);
            }
        else diag = false;
    }
    if (const int rc = quiesce(h)) return rc;                  // (the set in force and the scratch are in use by whatever is still queued)
    mpopis_handle::Sigma0Set& dst = per_slot ? h->S0sl : h->S0sh;
    // per-slot Σ: the slots' own buffers, from the first such call on ([B] matrices each; S0 is their slot view, by S0stride / P0stride below).
    // Whatever a failed call did allocate stays with the handle for the next one.
    if (per_slot && (h->shared_alloc(dst.Sigma, B * nn) || h->shared_alloc(dst.L, B * nn) || (pd && h->shared_alloc(dst.Lp, B * pd)) ||
                     (nes && (h->shared_alloc(dst.nesA, B * nn) || h->shared_alloc(dst.nesS, B * nn))))) {
        (void)hipGetLastError();
        h->err = "mpopis_set_Sigma_slots: hipMalloc of the per-slot covariance buffers failed";
        return MPOPIS_ERR_HIP;
    }
    auto read_status = [&]() -> int {
        HIPCHK(h, hipMemcpyAsync(h->h_status.data(), h->d_status, sizeof(int) * M, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
        return MPOPIS_OK;
    };
    // factor once (the reference refactors the same Σ every call, :307)
    HIPCHK(h, hipMemcpyAsync(h->d_tmpS, full.data(), sizeof(double) * M * nn, hipMemcpyHostToDevice, h->stream));
    fill_i32(h->d_status, 0, B, h->stream);
    launch_potrf(h->d_tmpS, nn, h->d_L, M, cs, nullptr, h->d_status, nullptr, h->stream, h->potrf_coop(), pd ? h->d_Lp : nullptr, pd);
    if (int rc = read_status()) return rc;
    for (int b = 0; b < M; ++b)
        if (h->h_status[b] != 0) { h->err = "PosDefException: Sigma" + of_slot(b) + " is not positive definite"; return MPOPIS_ERR_NOT_PD; }
    if (nes) {
        // pol.A = sqrt(pol.Σ) (src/mppi_mpopi_policies.jl:849) and the first iteration's invcov(MvNormal(pol.Σ)) = L0^-T L0^-1, once per pol.Σ.
        // A diagonal matrix: closed form; otherwise the device's symmetric eigen-solve
        std::vector<double> a0(nn);
        for (int b = 0; b < M; ++b) {
            if (slot_diag[b]) {
                std::fill(a0.begin(), a0.end(), 0.0);
                for (int i = 0; i < cs; ++i) a0[(size_t)i * (cs + 1)] = ds[(size_t)b * cs + i];
                HIPCHK(h, hipMemcpy(h->d_nesA[0] + (size_t)b * nn, a0.data(), sizeof(double) * nn, hipMemcpyHostToDevice));
            } else {
                launch_sym_sqrt(h->d_tmpS + (size_t)b * nn, h->d_nesM + (size_t)b * nn, h->d_nesS + (size_t)b * nn, h->d_nesA[0] + (size_t)b * nn, h->d_status + b, cs, h->stream);
            }
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));             // (d_nesM is the eigen-solves' workspace until here)
        launch_nes_potri(h->d_L, nn, h->d_nesM, h->d_nesA[1], M, cs, nullptr, h->stream);
        if (int rc = read_status()) return rc;
        for (int b = 0; b < M; ++b)
            if (h->h_status[b] != 0) {
                h->err = per_slot ? "PosDefException: Sigma" + of_slot(b) + " is not positive definite" : "PosDefException: sqrt(Sigma) has a non-positive eigenvalue";
                return MPOPIS_ERR_NOT_PD;
            }
    }
    copy_f64(h->d_tmpS, dst.Sigma, (size_t)M * nn, h->stream);
    copy_f64(h->d_L, dst.L, (size_t)M * nn, h->stream);
    if (pd) copy_f64(h->d_Lp, dst.Lp, (size_t)M * pd, h->stream);
    if (nes) { copy_f64(h->d_nesA[0], dst.nesA, (size_t)M * nn, h->stream); copy_f64(h->d_nesA[1], dst.nesS, (size_t)M * nn, h->stream); }
    // sqrt(diag) per slot for the diagonal-Σ sampler, once per pol.Σ
    HIPCHK(h, hipMemcpyAsync(per_slot ? h->d_dscale : h->d_dscale0, ds.data(), sizeof(double) * M * cs, hipMemcpyHostToDevice, h->stream));
    if (!per_slot) hipLaunchKernelGGL(k_bcast_f64, dim3((cs + 255) / 256), dim3(256), 0, h->stream, h->d_dscale0, h->d_dscale, (size_t)cs, B);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    h->S0 = dst;
    h->S0stride = per_slot ? nn : 0; h->P0stride = per_slot ? pd : 0; h->sigma_diag = diag;
    return MPOPIS_OK;
}

// MPPI_Policy_Params Σ handling :66-81 : an as x as cov_mat is block-replicated (block_diagm, utils.jl:9-21);
// for :mppi the as x as Σ is kept by the reference, which is the same distribution as the
// block-diagonal cs x cs one used here (Cholesky of a block-diagonal matrix is block-diagonal).
int mpopis_set_Sigma(mpopis_handle* h, const double* Sigma, int32_t n) {
    if (h) h->plan_drop("mpopis_set_Sigma");
    if (!h || !Sigma) return MPOPIS_ERR_ARG;
    return set_Sigma0(h, Sigma, n, false);
}
int mpopis_set_Sigma_slots(mpopis_handle* h, const double* Sigma, int32_t n) {
    if (h) h->plan_drop("mpopis_set_Sigma_slots");
    if (!h || !Sigma) { if (h) h->err = "mpopis_set_Sigma_slots: null argument"; return MPOPIS_ERR_ARG; }
    return set_Sigma0(h, Sigma, n, true);
}

// λ, α, λ_ais, σ per slot.  A setup call (it waits for everything queued); the kernels read what is formed here on the host.
int mpopis_set_slot_hyper(mpopis_handle* h, const double* lambda, const double* alpha, const double* lambda_ais, const double* cma_sigma) {
    if (h) h->plan_drop("mpopis_set_slot_hyper");
    if (!h) return MPOPIS_ERR_ARG;
    const int B = h->B_full, K = h->K;
    if (h->cfg.policy == MPOPIS_POL_NESMPPI && cma_sigma)
        for (int b = 0; b < B; ++b)
            if (!std::isfinite(cma_sigma[b])) { h->err = "nesmppi: step_factor (cma_sigma) must be finite (slot " + std::to_string(b) + ")"; return MPOPIS_ERR_ARG; }
    if (const int rc = quiesce(h)) return rc;
    if (!lambda && !alpha && !lambda_ais && !cma_sigma) {       // back to the config's scalars
        h->sl_host.clear();
        h->d_sl_nil = h->d_sl_nil_ais = h->d_sl_gamma = h->d_sl_sigma = h->d_sl_nes_a = h->d_sl_nes_u = nullptr;
        h->sl_any_gamma = false;
        h->weights_in_moments = h->fold_weights_cfg;
        return MPOPIS_OK;
    }
    if (!h->sl_buf) {                                           // six [B] arrays in one allocation; the pointers the kernels get are its slot views
        if (h->shared_alloc(h->sl_buf, (size_t)6 * B)) { (void)hipGetLastError(); h->err = "mpopis_set_slot_hyper: hipMalloc of the per-slot value arrays failed"; return MPOPIS_ERR_HIP; }
        for (double** v : {&h->d_sl_nil, &h->d_sl_nil_ais, &h->d_sl_gamma, &h->d_sl_sigma, &h->d_sl_nes_a, &h->d_sl_nes_u}) h->slot_view(*v, 1);
    }
    std::vector<double> host((size_t)4 * B), dev((size_t)6 * B);
    bool any_gamma = false;
    for (int b = 0; b < B; ++b) {
        const double lam = lambda ? lambda[b] : h->cfg.lambda, al = alpha ? alpha[b] : h->cfg.alpha;
        const double la = lambda_ais ? lambda_ais[b] : h->cfg.lambda_ais, sg = cma_sigma ? cma_sigma[b] : h->cfg.cma_sigma;
        host[b] = lam; host[(size_t)B + b] = al; host[(size_t)2 * B + b] = la; host[(size_t)3 * B + b] = sg;
        const double gm = lam * (1 - al);
        any_gamma |= gm != 0.0;
        dev[b] = -1 / lam;
        dev[(size_t)B + b] = -1 / (h->cfg.policy == MPOPIS_POL_IMPPI ? lam : la);      // :362 / :647,:712
        dev[(size_t)2 * B + b] = gm;
        dev[(size_t)3 * B + b] = sg;
        dev[(size_t)4 * B + b] = -sg / ((double)K * K);
        dev[(size_t)5 * B + b] = sg / K;
    }
    HIPCHK(h, hipMemcpyAsync(h->sl_buf, dev.data(), sizeof(double) * 6 * B, hipMemcpyHostToDevice, h->stream));      // (behind the buffer's zero-fill)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->sl_host.swap(host);
    h->d_sl_nil = h->sl_buf; h->d_sl_nil_ais = h->sl_buf + B; h->d_sl_gamma = h->sl_buf + 2 * (size_t)B; h->d_sl_sigma = h->sl_buf + 3 * (size_t)B;
    h->d_sl_nes_a = h->sl_buf + 4 * (size_t)B; h->d_sl_nes_u = h->sl_buf + 5 * (size_t)B;
    h->sl_any_gamma = any_gamma;
    // per-slot λ_ais leaves the fused "weights inside the moments kernel" form (its -1/λ_ais is one scalar): the path MPOPIS_FOLD_WEIGHTS=0 selects
    h->weights_in_moments = h->fold_weights_cfg && !lambda_ais;
    return MPOPIS_OK;
}

int mpopis_get_slot_hyper(mpopis_handle* h, double* lambda, double* alpha, double* lambda_ais, double* cma_sigma) {
    if (!h) return MPOPIS_ERR_ARG;
    const int B = h->B_full;
    double* out[4] = {lambda, alpha, lambda_ais, cma_sigma};
    const double cfgv[4] = {h->cfg.lambda, h->cfg.alpha, h->cfg.lambda_ais, h->cfg.cma_sigma};
    for (int i = 0; i < 4; ++i)
        if (out[i]) for (int b = 0; b < B; ++b) out[i][b] = h->sl_host.empty() ? cfgv[i] : h->sl_host[(size_t)i * B + b];
    return MPOPIS_OK;
}

int mpopis_seed(mpopis_handle* h, uint64_t seed) {
    if (h) h->plan_drop("mpopis_seed");
    if (!h) return MPOPIS_ERR_ARG;
    std::vector<uint64_t> s(h->B);
    for (int b = 0; b < h->B; ++b) s[b] = seed + (uint64_t)b + 1;              // seed!(pol, seed + k), car_example.jl:188
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_seeds, s.data(), sizeof(uint64_t) * h->B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    h->mpc_step = 0;
    return MPOPIS_OK;
}

int mpopis_seed_slots(mpopis_handle* h, const uint64_t* seeds) {
    if (h) h->plan_drop("mpopis_seed_slots");
    if (!h || !seeds) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_seeds, seeds, sizeof(uint64_t) * h->B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    h->mpc_step = 0;
    return MPOPIS_OK;
}

// How the device draws the proposal's normals.  A setup call: the kind is read while a step is enqueued, never by a kernel,
// but the call still waits for what is queued so that it orders like the other setters.
int mpopis_set_noise_kind(mpopis_handle* h, int32_t kind) {
    if (h) h->plan_drop("mpopis_set_noise_kind");
    if (!h) return MPOPIS_ERR_ARG;
    if (kind != MPOPIS_NOISE_PHILOX && kind != MPOPIS_NOISE_ANTITHETIC && kind != MPOPIS_NOISE_LHS) {
        h->err = "mpopis_set_noise_kind: unknown noise kind " + std::to_string(kind) + " (0 philox, 1 antithetic, 2 lhs)"; return MPOPIS_ERR_ARG;
    }
    if (kind == MPOPIS_NOISE_LHS && h->K > kStratMaxK) { h->err = "mpopis_set_noise_kind: the Latin-hypercube draw takes K <= 2^20"; return MPOPIS_ERR_ARG; }
    if (const int rc = quiesce(h)) return rc;
    h->noise_kind = kind;
    return MPOPIS_OK;
}

int mpopis_get_noise_kind(mpopis_handle* h, int32_t* kind) {
    if (!h || !kind) return MPOPIS_ERR_ARG;
    *kind = h->noise_kind;
    return MPOPIS_OK;
}

// The normals of (mpc_step, iteration) under the handle's kind and seeds, in the layout of one iteration of mpopis_noise.Z.  Drawn into staging
// buffers of the call's own (allocated and freed here), so nothing a later call reads is written and the RNG position (mpc_step) stays.
int mpopis_draw_normals(mpopis_handle* h, uint32_t mpc_step, int32_t iteration, double* Z) {
    if (!h) return MPOPIS_ERR_ARG;
    if (!Z || iteration < 0) { h->err = "mpopis_draw_normals: Z must not be NULL and iteration must be >= 0"; return MPOPIS_ERR_ARG; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, K = h->K, cs = h->cs, as = h->as;
    const bool mppi = h->cfg.policy == MPOPIS_POL_MPPI;
    const size_t n = (size_t)B * cs * K;
    double* rows = nullptr; double* out = nullptr;
    if (hipMalloc((void**)&rows, sizeof(double) * n) != hipSuccess || hipMalloc((void**)&out, sizeof(double) * n) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(rows);
        h->err = "mpopis_draw_normals: hipMalloc of the staging buffers failed"; return MPOPIS_ERR_HIP;
    }
    if (h->noise_kind == MPOPIS_NOISE_PHILOX) launch_sample_normal(rows, B, cs, K, as, mppi, h->d_seeds, mpc_step, (uint32_t)iteration, nullptr, nullptr, h->stream, h->d_rng_tab);
    else launch_sample_strat(rows, B, cs, K, as, mppi, h->noise_kind, h->d_seeds, mpc_step, (uint32_t)iteration, nullptr, h->stream, h->d_rng_tab);
    if (mppi) launch_mppi_E_out(rows, out, B, h->T, K, as, h->stream);
    else launch_transpose_out(rows, nullptr, nullptr, out, B, cs, K, h->stream);
    hipError_t e = hipMemcpyAsync(Z, out, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = wait_stream(h->stream);
    if (e == hipSuccess) e = hipGetLastError();
    (void)hipFree(rows); (void)hipFree(out);
    HIPCHK(h, e);
    return MPOPIS_OK;
}

int mpopis_get_Sigma(mpopis_handle* h, double* out) {
    if (!h || !out) return MPOPIS_ERR_ARG;
    if (h->cfg.policy == MPOPIS_POL_MPPI) { h->err = "mpopis_get_Sigma: :mppi keeps the as x as pol.Σ (no adaptation)"; return MPOPIS_ERR_ARG; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int pol = h->cfg.policy;
    const size_t nn = (size_t)h->cs * h->cs;
    const bool sigma_fixed = (pol == MPOPIS_POL_GMPPI || pol == MPOPIS_POL_IMPPI || pol == MPOPIS_POL_MUAISMPPI);
    // d_tmpS is scratch outside a policy step
    const double* scale = (pol == MPOPIS_POL_CMAMPPI && h->N > 1) ? h->d_sig2 : nullptr;     // MvNormal(σ²Σ′) :550-554
    hipLaunchKernelGGL(k_scaled_copy_f64, dim3((nn + 255) / 256, h->B), dim3(256), 0, h->stream,
                       sigma_fixed ? h->S0.Sigma : h->d_Sig, sigma_fixed ? h->S0stride : nn, scale, h->d_tmpS, nn);
    HIPCHK(h, hipMemcpyAsync(out, h->d_tmpS, sizeof(double) * h->B * nn, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    return MPOPIS_OK;
}

int mpopis_rollout_costs(mpopis_handle* h, const double* x0, const double* U, const double* U_orig, const double* E,
                         const double* Sigma_inv, double* cost) {
    if (h) h->plan_drop("mpopis_rollout_costs");
    if (!h || !U || !E || !cost) return MPOPIS_ERR_ARG;
    if (h->track_missing()) return MPOPIS_ERR_ARG;
    if (h->use_gvec() && !Sigma_inv) { h->err = "Sigma_inv required when alpha != 1"; return MPOPIS_ERR_ARG; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, K = h->K, cs = h->cs;
    if (x0) HIPCHK(h, hipMemcpyAsync(h->d_x, x0, sizeof(double) * B * h->ss, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_Ucur, U, sizeof(double) * B * cs, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_Uin, U_orig ? U_orig : U, sizeof(double) * B * cs, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_Z, E, sizeof(double) * B * cs * K, hipMemcpyHostToDevice, h->stream));
    launch_transpose_in(h->d_Z, h->d_E, B, cs, K, h->stream);
    const double* gv = nullptr;
    if (h->use_gvec()) {
        HIPCHK(h, hipMemcpyAsync(h->d_tmpS, Sigma_inv, sizeof(double) * cs * cs, hipMemcpyHostToDevice, h->stream));
        launch_gvec_from_inv(h->d_tmpS, h->d_Uin, h->sv_gamma(), h->d_gvec, B, cs, h->stream);
        gv = h->d_gvec;
    }
    fill_i32(h->d_status, 0, B, h->stream);
    h->prepare_state();
    h->rollout(h->d_Ucur, h->d_Uin, gv, nullptr);
    if (!h->launch_err.empty()) { h->err = h->launch_err; h->launch_err.clear(); return MPOPIS_ERR_HIP; }
    HIPCHK(h, hipMemcpyAsync(cost, h->d_cost, sizeof(double) * B * K, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    HIPCHK(h, hipGetLastError());
    return MPOPIS_OK;
}

int mpopis_env_step(mpopis_handle* h, const double* action, double* reward) {
    if (h) h->plan_drop("mpopis_env_step");
    if (!h || !action) return MPOPIS_ERR_ARG;
    if (h->track_missing()) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_control, action, sizeof(double) * h->B * h->as, hipMemcpyHostToDevice, h->stream));
    fill_i32(h->d_status, 0, h->B, h->stream);
    HIPCHK(h, launch_env_step(h->env, h->d_x, h->d_t, h->d_done, h->d_control, h->d_reward, h->d_status, nullptr, h->B, h->stream, h->slot_env()));
    if (reward) HIPCHK(h, hipMemcpyAsync(reward, h->d_reward, sizeof(double) * h->B, hipMemcpyDeviceToHost, h->stream));
    return sync_status(h);
}

int mpopis_env_query(mpopis_handle* h, double* reward, int32_t* within, double* dist, double* beta) {
    if (!h) return MPOPIS_ERR_ARG;
    if (h->track_missing()) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, NC = std::max(1, h->env.ncars);
    if (h->slot_alloc(h->d_qdist, NC) || h->slot_alloc(h->d_qbeta, NC) || h->slot_alloc(h->d_qwithin, 1)) return MPOPIS_ERR_HIP;
    HIPCHK(h, launch_env_query(h->env, h->d_x, h->d_t, h->d_done, h->d_reward, h->d_qwithin, h->d_qdist, h->d_qbeta, B, h->stream, h->slot_env()));
    if (reward) HIPCHK(h, hipMemcpyAsync(reward, h->d_reward, sizeof(double) * B, hipMemcpyDeviceToHost, h->stream));
    if (within) HIPCHK(h, hipMemcpyAsync(within, h->d_qwithin, sizeof(int) * B, hipMemcpyDeviceToHost, h->stream));
    if (dist) HIPCHK(h, hipMemcpyAsync(dist, h->d_qdist, sizeof(double) * B * NC, hipMemcpyDeviceToHost, h->stream));
    if (beta) HIPCHK(h, hipMemcpyAsync(beta, h->d_qbeta, sizeof(double) * B * NC, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    return MPOPIS_OK;
}

int mpopis_get_trajectories(mpopis_handle* h, double* out) {
    if (!h || !out) return MPOPIS_ERR_ARG;
    if (!h->d_traj) { h->err = "log_trajectories was not enabled"; return MPOPIS_ERR_ARG; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(out, h->d_traj, sizeof(double) * h->B * h->K * h->T * h->ss, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    return MPOPIS_OK;
}

// The plan's buffers for every top up to the one asked for, carved out of one allocation (each part 16-byte aligned).  A larger request replaces
// the block; the handle is idle then (the call that used the old one ended with a stream wait).  On failure the old block stays.
int mpopis_handle::plan_reserve(int top) {
    if (top <= plan.cap_top) return MPOPIS_OK;
    const size_t W = (size_t)top + 1, Bn = (size_t)B_full;
    auto up = [](size_t n) { return (n + 1) & ~(size_t)1; };     // doubles, rounded up to 16 bytes
    const size_t n_controls = up(Bn * cs), n_E = up(Bn * cs * W), n_traj = up(Bn * W * ss * T), n_cost = up(Bn * W), n_w = up(Bn * std::max(top, 1));
    const size_t n_idx = up((Bn * std::max(top, 1) + 1) / 2);       // int32 pairs
    const size_t bytes = sizeof(double) * (n_controls + n_E + n_traj + n_cost + n_w + n_idx);
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        err = "mpopis_get_plan: hipMalloc of the plan buffers failed (" + std::to_string(bytes) + " bytes)";
        return MPOPIS_ERR_HIP;
    }
    if (plan.base) (void)hipFree(plan.base);
    plan.base = p; plan.cap_top = top;
    double* d = (double*)p;
    plan.controls = d; d += n_controls;
    plan.E = d; d += n_E;
    plan.traj = d; d += n_traj;
    plan.cost = d; d += n_cost;
    plan.w = d; d += n_w;
    plan.idx = (int32_t*)d;
    HIPCHK(this, hipMemsetAsync(p, 0, bytes, stream));
    return MPOPIS_OK;
}

// The plan of the last policy step and its `top` highest-weight sample rollouts (include/mpopis.h).  A getter: everything it reads -- d_w, d_E,
// d_Ucur, d_Uin, d_wn and the step's start state d_x / d_xext -- is still resident, and it writes the plan's own buffers only.
int mpopis_get_plan(mpopis_handle* h, int32_t top, double* controls, double* traj, double* cost, int32_t* idx0, double* weights) {
    if (!h) return MPOPIS_ERR_ARG;
    if (!h->plan_ok) {
        const std::string by = h->plan_lost;
        if (!h->plan_stepped) h->err = "mpopis_get_plan: no mpopis_policy_step or mpopis_policy_call has run on this handle yet";
        else if (by == "mpopis_policy_step" || by == "mpopis_policy_call") h->err = "mpopis_get_plan: the last policy step returned an error; there is no plan to read";
        else h->err = "mpopis_get_plan: " + by + " has written to the handle since the last policy step; the plan is read before any other call that is no getter";
        return MPOPIS_ERR_ARG;
    }
    const int B = h->B, K = h->K, cs = h->cs;
    if (top < 0 || top > std::min(K, MPOPIS_PLAN_MAX_TOP)) {
        h->err = "mpopis_get_plan: top must be 0.." + std::to_string(std::min(K, MPOPIS_PLAN_MAX_TOP)) + " (min(K, MPOPIS_PLAN_MAX_TOP)), got " + std::to_string(top);
        return MPOPIS_ERR_ARG;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (const int rc = h->plan_reserve(top)) return rc;
    const size_t W = (size_t)top + 1;
    mpopis_handle::PlanBufs& pl = h->plan;
    launch_plan_select(h->d_w, B, K, top, pl.idx, pl.w, h->stream);
    launch_plan_assemble(h->d_E, h->d_Ucur, h->d_Uin, h->d_wn, pl.idx, B, cs, K, top, pl.controls, pl.E, h->stream);
    if (traj || cost) {
        // the extended start states once more, from the d_x the step started from: a step that ran as part-chains left each part's in that part's
        // own view of d_xext (its slot stride is that of kMaxCars cars), not in the whole batch's
        h->prepare_state();
        hipError_t custom_err = hipSuccess;
        if (!h->plan_rollout((int)W, &custom_err)) {
            h->err = h->env.kind == MPOPIS_ENV_CUSTOM ? std::string("mpopis_get_plan: launching the custom env's rollout kernel failed: ") + hipGetErrorString(custom_err)
                                                      : std::string("mpopis_get_plan: no rollout kernel for this env");
            return MPOPIS_ERR_HIP;
        }
    }
    if (controls) HIPCHK(h, hipMemcpyAsync(controls, pl.controls, sizeof(double) * B * cs, hipMemcpyDeviceToHost, h->stream));
    if (traj) HIPCHK(h, hipMemcpyAsync(traj, pl.traj, sizeof(double) * B * W * h->ss * h->T, hipMemcpyDeviceToHost, h->stream));
    if (cost) HIPCHK(h, hipMemcpyAsync(cost, pl.cost, sizeof(double) * B * W, hipMemcpyDeviceToHost, h->stream));
    if (top > 0 && idx0) HIPCHK(h, hipMemcpyAsync(idx0, pl.idx, sizeof(int32_t) * B * top, hipMemcpyDeviceToHost, h->stream));
    if (top > 0 && weights) HIPCHK(h, hipMemcpyAsync(weights, pl.w, sizeof(double) * B * top, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    HIPCHK(h, hipGetLastError());
    return MPOPIS_OK;
}

int mpopis_policy_step(mpopis_handle* h, const mpopis_noise* noise, double* control, double* cost, double* weights,
                       double* E_out, int32_t* resample_idx0, int32_t* iters_run) {
    if (h) h->plan_step_begins("mpopis_policy_step");
    if (!h) return MPOPIS_ERR_ARG;
    if (h->track_missing()) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, K = h->K, cs = h->cs, N = h->N;
    const size_t per = (size_t)cs * K;
    if (noise && noise->Z) {
        if (h->slot_alloc(h->d_Zin, N * per)) return MPOPIS_ERR_HIP;
        HIPCHK(h, hipMemcpyAsync(h->d_Zin, noise->Z, sizeof(double) * B * N * per, hipMemcpyHostToDevice, h->stream));
        if (h->cfg.policy == MPOPIS_POL_PMCMPPI && N > 1) {
            if (!noise->res_i0 || !noise->res_u) { h->err = "pmcmppi with injected noise needs resampling draws"; return MPOPIS_ERR_ARG; }
            if (h->slot_alloc(h->d_resi_in, (size_t)(N - 1) * K) || h->slot_alloc(h->d_resu_in, (size_t)(N - 1) * K)) return MPOPIS_ERR_HIP;
            HIPCHK(h, hipMemcpyAsync(h->d_resi_in, noise->res_i0, sizeof(int32_t) * B * (N - 1) * K, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(h->d_resu_in, noise->res_u, sizeof(double) * B * (N - 1) * K, hipMemcpyHostToDevice, h->stream));
        }
    }
    int rc = h->policy_step_enqueue(noise && noise->Z);
    if (rc) return rc;
    if (control) HIPCHK(h, hipMemcpyAsync(h->h_pin ? h->h_pin : control, h->d_control, sizeof(double) * B * h->as, hipMemcpyDeviceToHost, h->stream));
    if (cost) HIPCHK(h, hipMemcpyAsync(cost, h->d_cost, sizeof(double) * B * K, hipMemcpyDeviceToHost, h->stream));
    if (weights) HIPCHK(h, hipMemcpyAsync(weights, h->d_w, sizeof(double) * B * K, hipMemcpyDeviceToHost, h->stream));
    if (E_out) {
        // E .+= (pol.U - U_orig), returned in the reference layout.  d_Z is free at this point.
        if (h->cfg.policy == MPOPIS_POL_MPPI) {
            // reference E[k,t] (as-vectors, k fastest): element ((t*K+k)*as+a)  <- rows r=t*as+a
            launch_mppi_E_out(h->d_E, h->d_Z, B, h->T, K, h->as, h->stream);
        } else {
            launch_transpose_out(h->d_E, h->d_Ucur, h->d_Uin, h->d_Z, B, cs, K, h->stream);
        }
        HIPCHK(h, hipMemcpyAsync(E_out, h->d_Z, sizeof(double) * B * per, hipMemcpyDeviceToHost, h->stream));
    }
    if (resample_idx0 && N > 1) HIPCHK(h, hipMemcpyAsync(resample_idx0, h->d_residx_log, sizeof(int32_t) * B * (N - 1) * K, hipMemcpyDeviceToHost, h->stream));
    if (iters_run) HIPCHK(h, hipMemcpyAsync(h->h_pin ? (void*)(h->h_pin + (size_t)B * h->as) : (void*)iters_run, h->d_iters, sizeof(int) * B, hipMemcpyDeviceToHost, h->stream));
    rc = sync_status(h);
    if (h->h_pin) {
        if (control) memcpy(control, h->h_pin, sizeof(double) * B * h->as);
        if (iters_run) memcpy(iters_run, h->h_pin + (size_t)B * h->as, sizeof(int) * B);
    }
    HIPCHK(h, hipGetLastError());
    h->plan_ok = rc == MPOPIS_OK;                               // what mpopis_get_plan reads stays resident until the next writing call
    return rc;
}

// control = pol(env) with ONE host wait: the synchronous per-MPC-step call of the reference's harness (src/examples/car_example.jl:203-207,
// mountaincar_example.jl:150-153).  Same results as set_state + set_U + policy_step + get_U (tests/test_gpu_host_api.py); the small inputs and
// outputs travel through the handle's device-mapped mailbox, so the stream carries kernels only.
int mpopis_policy_call(mpopis_handle* h, const double* x, const int32_t* t, const int32_t* done, double* U_inout, const mpopis_noise* noise,
                       double* control, double* cost, double* weights, int32_t* iters_run) {
    if (h) h->plan_step_begins("mpopis_policy_call");
    if (!h) return MPOPIS_ERR_ARG;
    if (!h->h_call || (noise && noise->Z)) {
        // injected noise is a parity-test path (megabytes of host data): plain composition of the four calls
        int rc = 0;
        if (x || t || done) {
            if (!x) { h->err = "mpopis_policy_call: t / done without x"; return MPOPIS_ERR_ARG; }
            if ((rc = mpopis_set_state(h, x, t, done)) != 0) return rc;
        }
        if (U_inout && (rc = mpopis_set_U(h, U_inout)) != 0) return rc;
        rc = mpopis_policy_step(h, noise, control, cost, weights, nullptr, nullptr, iters_run);
        if (U_inout) { const int r2 = mpopis_get_U(h, U_inout); if (!rc) rc = r2; }
        return rc;
    }
    if ((t || done) && !x) { h->err = "mpopis_policy_call: t / done without x"; return MPOPIS_ERR_ARG; }
    if (h->track_missing()) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, K = h->K, cs = h->cs, as = h->as, ss = h->ss;
    const CallBox hb = call_box(h->h_call, B, ss, cs, as), db = call_box(h->d_call, B, ss, cs, as);
    int flags = 0;
    if (x) { memcpy(hb.x, x, sizeof(double) * B * ss); flags |= 1; }
    if (U_inout) { memcpy(hb.U, U_inout, sizeof(double) * B * cs); flags |= 2; }
    if (t) { memcpy(hb.t, t, sizeof(int) * B); flags |= 4; }
    if (done) { memcpy(hb.done, done, sizeof(int) * B); flags |= 8; }
    const int nx = B * ss, nu = B * cs, nmax = std::max(std::max(nx, nu), B);
    if (flags) hipLaunchKernelGGL(k_call_in, dim3((nmax + 255) / 256), dim3(256), 0, h->stream, db, h->d_x, h->d_U, h->d_t, h->d_done, nx, nu, B, flags);
    int rc = h->policy_step_enqueue(false);
    if (rc) return rc;
    const int seq = (int)(++h->call_seq);
    hipLaunchKernelGGL(k_call_out, dim3(1), dim3(256), 0, h->stream, db, h->d_control, h->d_U, h->d_status, h->d_iters,
                       h->coop_disabled ? (const int*)nullptr : h->d_coop_timeouts, B * as, nu, B, seq);
    if (cost) HIPCHK(h, hipMemcpyAsync(cost, h->d_cost, sizeof(double) * B * K, hipMemcpyDeviceToHost, h->stream));
    if (weights) HIPCHK(h, hipMemcpyAsync(weights, h->d_w, sizeof(double) * B * K, hipMemcpyDeviceToHost, h->stream));
    // Host wait.  Without bulk outputs everything the caller gets back sits in the mailbox, published by the sequence word: spin on that word
    // (coherent host memory; the store lands ~1-2 us after the kernel issues it) and leave the stream's completion signal alone -- the next call
    // is ordered behind this one by the stream anyway.  Every ~20 us the stream is queried so that a fault ends the wait; after 3 ms: block.
    // Only when the previous step of this handle was short (wait_should_spin): a long step blocks from the start.
    static const int env_wait = [] { const char* e = getenv("MPOPIS_CALL_WAIT"); return e ? atoi(e) : 1; }();      // 0: runtime wait only (A/B)
    if (env_wait && !cost && !weights && wait_should_spin(h)) {
        const auto t0 = std::chrono::steady_clock::now();
        auto tq = t0;
        for (;;) {
            if (*hb.seq == seq) break;
            const auto now = std::chrono::steady_clock::now();
            if (now - tq > std::chrono::microseconds(20)) {
                tq = now;
                const hipError_t e = hipStreamQuery(h->stream);
                if (e == hipSuccess) break;
                if (e != hipErrorNotReady) HIPCHK(h, e);
                if (now - t0 > std::chrono::milliseconds(3)) { HIPCHK(h, hipStreamSynchronize(h->stream)); break; }
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        wait_note(h, t0);
    } else {
        HIPCHK(h, wait_step(h));
    }
    if (*hb.coop > 0) h->coop_disabled = true;
    if (control) memcpy(control, hb.control, sizeof(double) * B * as);
    if (U_inout) memcpy(U_inout, hb.Uout, sizeof(double) * B * cs);
    if (iters_run) memcpy(iters_run, hb.iters, sizeof(int) * B);
    rc = fold_status(h, hb.status);
    HIPCHK(h, hipGetLastError());
    h->plan_ok = rc == MPOPIS_OK;
    return rc;
}

int mpopis_set_state_noise(mpopis_handle* h, double sigma_x, double sigma_y, double sigma_psi) {
    if (h) h->plan_drop("mpopis_set_state_noise");
    if (!h) return MPOPIS_ERR_ARG;
    if (!(sigma_x >= 0.0 && sigma_y >= 0.0 && sigma_psi >= 0.0)) { h->err = "state noise sigmas must be >= 0"; return MPOPIS_ERR_ARG; }
    h->noise_sx = sigma_x; h->noise_sy = sigma_y; h->noise_spsi = sigma_psi;
    return MPOPIS_OK;
}

int mpopis_run_trials(mpopis_handle* h, int32_t num_steps, int32_t laps, double* records, double* actions) {
    if (h) h->plan_drop("mpopis_run_trials");
    if (!h || !records) return MPOPIS_ERR_ARG;
    return h->run_trials(num_steps, laps, records, actions);
}

int mpopis_run_trials_traced(mpopis_handle* h, int32_t num_steps, int32_t laps, double* records, double* actions, const mpopis_trace* trace) {
    if (h) h->plan_drop("mpopis_run_trials_traced");
    if (!h || !records) return MPOPIS_ERR_ARG;
    return h->run_trials(num_steps, laps, records, actions, trace);
}

int mpopis_set_overlap(mpopis_handle* h, int32_t on) {
    if (h) h->plan_drop("mpopis_set_overlap");
    if (!h) return MPOPIS_ERR_ARG;
    if (h->split_pinned) return MPOPIS_OK;
    if (on <= 0) { h->nsplit = 1; h->split_auto = true; return MPOPIS_OK; }                   // the default: the engine picks (auto_parts)
    h->nsplit = std::min((int)mpopis_handle::kMaxSplit, (int)on);                            // 1: one stream; 2..4: that many parts
    h->split_auto = false;
    return MPOPIS_OK;
}

int mpopis_timing_enable(mpopis_handle* h, int32_t on) {
    if (h) h->plan_drop("mpopis_timing_enable");
    if (!h) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (on && h->events.empty()) {
        h->events.resize(2 * 8192);
        // timing events carry no system-scope fence: a default event makes the queue write back / invalidate the caches at every record, which
        // costs the kernels around it (measured in the bench's timed region: two records per rollout launch, ~1 % of the step)
        for (auto& e : h->events) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    }
    h->timing = on != 0;
    h->timing_mask = (on == 1 || on == 0) ? ~0 : (on >> 1);     // 1: every class; otherwise bit (class + 1) selects a class
    return MPOPIS_OK;
}
int mpopis_timing_reset(mpopis_handle* h) { if (h) h->plan_drop("mpopis_timing_reset"); if (!h) return MPOPIS_ERR_ARG; h->ev_used = 0; h->ev_slot.clear(); return MPOPIS_OK; }
int mpopis_timing_read(mpopis_handle* h, char* names, int32_t names_cap, double* ms_total, int64_t* launches, int32_t* n) {
    if (!h || !n) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, wait_stream(h->stream));
    const char* const* kNames = kClassNames;
    const int nslots = 7;
    std::vector<double> ms(nslots, 0.0); std::vector<int64_t> cnt(nslots, 0);
    for (size_t i = 0; i < h->ev_slot.size(); ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, h->events[2 * i], h->events[2 * i + 1]) == hipSuccess) { ms[h->ev_slot[i]] += t; cnt[h->ev_slot[i]]++; }
    }
    std::string nm;
    const int m = std::min<int>(*n, nslots);
    for (int i = 0; i < m; ++i) { if (i) nm += ";"; nm += kNames[i]; if (ms_total) ms_total[i] = ms[i]; if (launches) launches[i] = cnt[i]; }
    if (names && names_cap > 0) { strncpy(names, nm.c_str(), names_cap - 1); names[names_cap - 1] = 0; }
    *n = m;
    return MPOPIS_OK;
}

int mpopis_bench_policy_steps(mpopis_handle* h, int32_t steps, double* ms, double* rollouts) {
    if (h) h->plan_drop("mpopis_bench_policy_steps");
    if (!h || steps < 0) return MPOPIS_ERR_ARG;
    if (h->track_missing()) return MPOPIS_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
    // rollouts EXECUTED, not B * N * K: a CE / CMA iteration loop may break early (src/mppi_mpopi_policies.jl:458-461, :567-569).  k_step_begin folds
    // every step's per-slot iteration count into d_iters_acc before clearing it; the last step's is still in d_iters when the region ends.
    HIPCHK(h, hipMemsetAsync(h->d_iters_acc, 0, sizeof(unsigned long long) * h->B, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_iters, 0, sizeof(int) * h->B, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    HIPCHK(h, hipEventRecord(e0, h->stream));
    h->chains_fork();                                           // the parts are forked once and joined once: a part's steps follow each other on its stream
    for (int s = 0; s < steps; ++s) {
        int rc = h->chains_step(false);
        if (rc) { h->chains_join(); return rc; }
    }
    h->chains_join();
    HIPCHK(h, hipEventRecord(e1, h->stream));
    HIPCHK(h, hipEventSynchronize(e1));
    float t = 0.f;
    HIPCHK(h, hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t;
    if (rollouts) {
        std::vector<unsigned long long> acc(h->B); std::vector<int> last(h->B);
        HIPCHK(h, hipMemcpy(acc.data(), h->d_iters_acc, sizeof(unsigned long long) * h->B, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(last.data(), h->d_iters, sizeof(int) * h->B, hipMemcpyDeviceToHost));
        double its = 0.0;
        for (int b = 0; b < h->B; ++b) its += (double)acc[b] + (double)last[b];
        *rollouts = its * h->K;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    int rc = sync_status(h);
    HIPCHK(h, hipGetLastError());
    return rc;
}

}  // extern "C"

// ---- launch sequences -----------------------------------------------------------------------------
void mpopis_handle::prepare_state() {
    if (env.kind == MPOPIS_ENV_CAR) launch_extend_state(d_x, d_xext, B, env.ncars, stream, env.track, slot_tracks());
}

RolloutArgs mpopis_handle::rollout_base() const {
    RolloutArgs a;
    a.env = env; a.B = B; a.K = 0; a.T = T; a.cs = cs;
    a.x0 = d_x; a.x0ext = d_xext; a.t0 = d_t; a.done0 = d_done;
    a.Ucur = a.Uorig = a.E = a.gvec = nullptr; a.cost = a.traj = nullptr;
    a.active = nullptr; a.iters = nullptr; a.iter_n = 0; a.cmin = nullptr; a.status = nullptr;
    a.senv = scen_M > 0 ? scenario_env(0) : slot_env();      // (scenario 0 = the nominal model: what the plan read-outs roll under)
    return a;
}

// The read-out's rollout: nominal controls U_orig, noise block plan.E, no control cost, every slot, nothing of the step's own outputs touched.
// Not a launch of a policy step: outside the timing classes.
bool mpopis_handle::plan_rollout(int Kp, hipError_t* custom_err) {
    RolloutArgs a = rollout_base();
    a.K = Kp; a.Ucur = d_Uin; a.Uorig = d_Uin; a.E = plan.E;
    a.cost = plan.cost; a.traj = plan.traj;
    return launch_rollout(a, stream, custom_err);
}

void mpopis_handle::rollout(const double* Ucur, const double* Uorig, const double* gvec, const int* act, int* iters, int iter_n) {
    RolloutArgs a = rollout_base();
    a.K = K; a.Ucur = Ucur; a.Uorig = Uorig; a.E = d_E; a.gvec = gvec;
    a.cost = d_cost; a.traj = d_traj; a.active = act; a.iters = iters; a.iter_n = iter_n;
    a.cmin = weights_in_moments ? d_cmin : nullptr; a.status = weights_in_moments ? d_status : nullptr;
    a.share = coop_share;
    time_begin(0);
    hipError_t custom_err = hipSuccess;
    if (scen_M > 0) {
        // One launch of the per-slot form per scenario, serial on the part's stream, each into its own cost plane and none of them touching
        // cmin / status; then the risk kernel forms the K costs the step sees and does the epilogue's cmin / status work on those.
        unsigned long long* cmin = a.cmin; int* status = a.status;
        a.cmin = nullptr; a.status = nullptr; a.traj = nullptr;
        const size_t plane = (size_t)B_full * K;
        bool ok = true;
        for (int m = 0; m < scen_M && ok; ++m) {
            a.senv = scenario_env(m); a.cost = d_scen_cost + m * plane;
            ok = launch_rollout(a, stream, &custom_err);
        }
        ok = ok && launch_risk(d_scen_cost, plane, scen_M, d_cost, B, K, risk_kind, risk_tail, risk_theta, act, cmin, status, stream);
        if (!ok && launch_err.empty()) launch_err = "rollout: no kernel for this env under scenarios (num_cars " + std::to_string(env.ncars) + ")";
        time_end();
        return;
    }
    if (!launch_rollout(a, stream, &custom_err) && launch_err.empty())
        launch_err = env.kind == MPOPIS_ENV_CUSTOM ? std::string("rollout: launching the custom env's kernel failed: ") + hipGetErrorString(custom_err)
                                                   : "rollout: no kernel for this env (num_cars " + std::to_string(env.ncars) + ")";
    time_end();
}

// calculate_trajectory_costs(pol, env) for the configured policy + functor tail.  `injected`: noise
// staged in d_Zin / d_resi_in / d_resu_in, else device Philox streams (mpc_step, iteration).
// Slot views: every per-slot buffer is laid out [B][...], so "slots [b0, b0 + nb)" is the same handle with its pointers moved.
// The registry (slot_bufs: every slot_alloc / slot_view, with the extent it was declared with) does the moving; named here are only the views whose
// stride changes at run time, each next to the variable that holds it.
void mpopis_handle::shift_slots(ptrdiff_t db) {
    for (const SlotBuf& sb : slot_bufs) {
        char* q; memcpy(&q, sb.member, sizeof q);               // (the member is a T* of some T: read and written as bytes)
        if (q) { q += db * (ptrdiff_t)sb.bytes_per_slot; memcpy(sb.member, &q, sizeof q); }
    }
    auto mv = [db](auto*& p, ptrdiff_t stride) { if (p) p += db * stride; };
    mv(S0.Sigma, (ptrdiff_t)S0stride); mv(S0.L, (ptrdiff_t)S0stride); mv(S0.Lp, (ptrdiff_t)P0stride); mv(S0.nesA, (ptrdiff_t)S0stride); mv(S0.nesS, (ptrdiff_t)S0stride);   // per-slot pol.Σ (stride 0: shared)
    mv(custom.table_view, (ptrdiff_t)custom.table_stride);                     // a custom env's per-slot tables (stride 0: one shared table)
    mv(d_actlog, actlog_stride);                                               // run_trials' action log of the current call
    if (trace.base) {                                                          // ... and its trace
        const ptrdiff_t S = trace.S, W = trace.top + 1;
        mv(trace.step.states, (S + 1) * ss); mv(trace.step.rewards, S); mv(trace.step.iters, S); mv(trace.step.within, S);
        mv(trace.step.dist, S * trace.ncars); mv(trace.step.beta, S * trace.ncars);
        mv(trace.E, (ptrdiff_t)cs * W); mv(trace.controls, (ptrdiff_t)cs); mv(trace.traj, W * ss * T); mv(trace.cost, W);
        mv(trace.w, (ptrdiff_t)trace.top); mv(trace.idx, (ptrdiff_t)trace.top);
    }
}

// pol(env) for all slots.  With >= 2 slots the batch may be split into parts that run as independent chains on
// their own streams, each started one sampler later than the previous: while one part sits in a latency-bound link of its chain
// (Cholesky: nb workgroups on 256 CUs; weights; the scatter's finish), the other half's rollout / sampler fills the chip.
// Per-slot results are bit-identical to the single-stream order (every kernel is slot-independent and deterministic).
// How many part-chains the default schedule uses.  The chain of one AIS iteration (weights -> moments -> Cholesky -> sampler -> rollout) is
// serial per trial, some links are latency-bound (Cholesky: B workgroups on 256 CUs; sort; alias table; finish kernels), and a rollout launch
// that exactly fills the wave slots (64 K=4096-trials = 4096 waves on 4096 slots) leaves them emptying one by one at its tail.  Split into 2-4
// skewed part-chains on their own streams, one part's latency-bound links and launch tails run under another part's throughput kernels.
// Bit-identical per slot (every kernel is slot-independent and deterministic: tests/test_gpu_baseline_shapes.py).  The table is the
// measured optimum (tools/split_sweep.py, one box, K = 4096 and 1024, 16..256 trials, ms per step at 1 / 2 / 3 / 4 parts), by rollout WAVES
// in the batch (B x ceil(K / 64) for one car):
//   :μΣaismppi  32 trials 3.37 / 4.07 / 3.80 / 4.24   48: 4.67 / 4.72 / 4.02 / 4.36   64: 5.79 / 5.70 / 5.43 / 5.19   96: 8.30 / 8.03 / 7.81 / 7.83   128: 10.7 all
//               (48 / 64 / 96 re-measured with the chains persisting across the steps of a call, see chains_fork; with a join after every step the same box gave
//                4.67 / 4.80 / 4.12 / 4.48, 5.78 / 5.75 / 5.57 / 5.28 and 8.30 / 8.12 / 7.93 / 7.95: every multi-part schedule gains, the ranking does not move)
//   :cemppi     32: 5.45 / 5.26 / 5.04 / 5.12        48: 7.02 / 6.09 / 5.51 / 5.56   64: 8.78 / 7.79 / 6.94 / 6.66   128: 15.4 / 13.9 / 13.2 / 12.9
//   :pmcmppi    32: 4.69 / 5.46 / 4.71 / 5.28        48: 6.34 / 5.47 / 5.41 / 5.38   64: 7.93 / 6.95 / 6.78 / 6.77   128: 14.7 / 13.3 / 12.8 / 12.6
//   :μaismppi   16: 2.30 / 2.04 / 2.29 / 2.44        32: 3.16 / 2.80 / 2.93 / 3.17   64: 4.96 / 4.37 / 4.57 / 4.49   128: 9.27 / 8.55 / 8.91 / 8.91
//   :gmppi      no gain at any size (one iteration: nothing to hide)
// Below ~2000 waves every kernel of the chain is latency-bound and splitting only adds launches (and takes the two-wave rollout kernels
// out of their regime).  :cmamppi with cs > 128 at >= 48 slots: the per-slot Cholesky / Lanczos kernels (one workgroup per slot: 64 of 256
// CUs busy for ~540 us per iteration) go under the other parts' rollouts: C4 at 64 trials 28.6 -> 26.9 ms (32 trials: no gain).
// mpopis_set_overlap(h, 1..4) overrides (1 = one stream: what a per-kernel profile wants).
int mpopis_handle::auto_parts() const {
    const int pol = cfg.policy;
    const int B = B_full;                                                     // (the member B is a part's slot count while a part-chain is enqueued)
    if (pol == MPOPIS_POL_CMAMPPI) return (cs > 128 && B >= 48) ? 4 : 1;
    if (N <= 1 || cs > 128 || env.kind != MPOPIS_ENV_CAR) return 1;           // one iteration / shapes outside the sweep: one stream
    const long long waves = (long long)B * ((K + 63) / 64);
    int np = 1;
    if (pol == MPOPIS_POL_MUAISMPPI || pol == MPOPIS_POL_IMPPI) np = waves >= 1024 ? 2 : 1;
    else if (pol == MPOPIS_POL_CEMPPI) np = waves >= 4096 ? 4 : (waves >= 2048 ? 3 : 1);
    else if (pol == MPOPIS_POL_PMCMPPI) np = waves >= 3072 ? 4 : 1;
    else if (pol == MPOPIS_POL_MUSIGMAAISMPPI) np = waves >= 4096 ? 4 : (waves >= 3072 ? 3 : 1);
    return std::min(np, B);
}

// spin for `ticks` of the 100 MHz real-time counter (one wave) and leave the kernel's own [start, end] on that clock in ts[0..1]
__global__ void k_spin_ticks(unsigned long long ticks, unsigned long long* ts) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
    if (threadIdx.x == 0) { ts[0] = t0; ts[1] = __builtin_amdgcn_s_memrealtime(); }
}

void mpopis_handle::verify_part_streams() {
    part_streams_checked = true;
    static const int env_check = [] { const char* e = getenv("MPOPIS_STREAM_CHECK"); return e ? atoi(e) : 1; }();
    if (!env_check) return;
    constexpr double kSpinUs = 200.0;
    // Do one spin kernel per stream run at the same time?  Decided on the DEVICE's clock -- every kernel records its own [start, end] and the
    // intervals must pairwise overlap by more than half a spin -- not on host wall time (until round 5: one host measurement against 1.6 spins, which
    // a descheduled host thread or a busy GPU turns into a false "serialised": extra streams for the handle's lifetime and possibly max_parts = 1).
    // Three probes, majority.
    unsigned long long* d_ts = nullptr;
    if (hipMalloc((void**)&d_ts, sizeof(unsigned long long) * 2 * (kMaxSplit + 1)) != hipSuccess) { (void)hipGetLastError(); return; }
    auto probe = [&](const std::vector<hipStream_t>& ss) {
        for (auto s_ : ss) (void)hipStreamSynchronize(s_);
        for (size_t i = 0; i < ss.size(); ++i) hipLaunchKernelGGL(k_spin_ticks, dim3(1), dim3(64), 0, ss[i], (unsigned long long)(kSpinUs * 100.0), d_ts + 2 * i);
        for (auto s_ : ss) (void)hipStreamSynchronize(s_);
        std::vector<unsigned long long> ts(2 * ss.size());
        if (hipMemcpy(ts.data(), d_ts, sizeof(unsigned long long) * ts.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
        const long long need = (long long)(0.5 * kSpinUs * 100.0);
        for (size_t i = 0; i < ss.size(); ++i)
            for (size_t j = i + 1; j < ss.size(); ++j) {
                const long long lo = (long long)std::max(ts[2 * i], ts[2 * j]), hi = (long long)std::min(ts[2 * i + 1], ts[2 * j + 1]);
                if (hi - lo < need) return false;
            }
        return true;
    };
    auto concurrent = [&](const std::vector<hipStream_t>& ss) {
        int yes = 0;
        for (int r = 0; r < 3 && yes < 2 && r - yes < 2; ++r) yes += probe(ss) ? 1 : 0;
        return yes >= 2;
    };
    { std::vector<hipStream_t> warm{stream}; (void)concurrent(warm); }   // (first launch of the kernel: code object load)
    std::vector<hipStream_t> chosen{stream};
    int next_x = 0, created = 0;
    while ((int)chosen.size() < kMaxSplit && created < 12) {
        hipStream_t c = nullptr;
        if (next_x < kMaxSplit - 1) c = xstream[next_x++];                 // the streams the handle was created with first
        else { if (hipStreamCreateWithFlags(&c, hipStreamNonBlocking) != hipSuccess) break; ++created; }
        std::vector<hipStream_t> trial = chosen; trial.push_back(c);
        if (concurrent(trial)) chosen.push_back(c); else rejected_streams.push_back(c);
    }
    // the chosen ones first (part-chains), then rejected ones as fillers: side chains (||L^-1||_F, Z prefetch) only need A stream
    size_t r = 0;
    for (int i = 0; i < kMaxSplit - 1; ++i) {
        if (i + 1 < (int)chosen.size()) xstream[i] = chosen[i + 1];
        else if (r < rejected_streams.size()) { xstream[i] = rejected_streams[r]; rejected_streams.erase(rejected_streams.begin() + r); }
    }
    max_parts = std::max(1, (int)chosen.size());
    (void)hipFree(d_ts);
    (void)hipGetLastError();
}

// Part-chains outlive an MPC step.  Part p's step s + 1 needs nothing but part p's step s (every per-slot buffer is a shift_slots view, every shared
// one is read-only), so a call that enqueues several steps -- mpopis_bench_policy_steps, run_trials -- forks the parts once (chains_fork), enqueues
// step after step on each part's own stream (chains_step) and joins when the host next needs the whole batch (chains_join).  Joining after every step
// drained the chip once per step: the last chain's final rollout alone at one wave per SIMD, then the latency-bound tail (weights, mean, finalize) and
// head (step_begin, Σ0 broadcast) of the step with nothing beside them, and two cross-stream waits in between.
// Skew: part p starts a step when part p-1 has left that step's first sampler.  MPOPIS_CHAIN_SKEW=1 keeps that one-directional edge at every step
// (the default), 0 only at the first step after a fork (chains without any cross-edge may drift into phase: four parts in the same kernel is the
// one-stream schedule); MPOPIS_CHAIN_JOIN=1 joins and re-forks after every step (the schedule before; A/B runs).  Numbers: DESIGN.md section 6.
void mpopis_handle::chains_fork() {
    int np = split_auto ? auto_parts() : std::min(nsplit, B);
    if (np >= 2 && !part_streams_checked) verify_part_streams();
    chain_np = std::max(1, std::min(np, max_parts));
    chain_fresh = true;
    if (chain_np < 2) return;
    (void)hipEventRecord(ev_fork, stream);                      // the other streams start after everything already queued on the main stream
    for (int p = 1; p < chain_np; ++p) (void)hipStreamWaitEvent(xstream[p - 1], ev_fork, 0);
}

void mpopis_handle::chains_join() {
    for (int p = 1; p < chain_np; ++p) {                        // later work on the main stream sees every part
        (void)hipEventRecord(ev_join[p - 1], xstream[p - 1]);
        (void)hipStreamWaitEvent(stream, ev_join[p - 1], 0);
    }
    chain_np = 0;
}

// one MPC step of every part of the open chain set; `tail` (nullable) is enqueued behind each part's step on that part's stream, with the handle
// narrowed to that part's slots
int mpopis_handle::chains_step(bool injected, const std::function<void()>& tail) {
    static const int env_skew = [] { const char* e = getenv("MPOPIS_CHAIN_SKEW"); return e ? atoi(e) : 1; }();
    static const int env_join = [] { const char* e = getenv("MPOPIS_CHAIN_JOIN"); return e ? atoi(e) : 0; }();
    const int B0 = B, np = chain_np;
    int rc = 0;
    if (np < 2) {
        side_free = (xstream[0] != nullptr);
        rc = step_enqueue_view(injected, nullptr, nullptr);
        side_free = false;
        if (!rc && tail) tail();
    } else {
        const bool skew = chain_fresh || env_skew;
        hipStream_t main_stream = stream;
        coop_share = np;                                        // up to np cluster launches in flight at once: each may take 1/np of the device
        int b0 = 0;
        for (int p = 0; p < np; ++p) {
            const int nbp = B0 / np + (p < B0 % np ? 1 : 0);
            if (p > 0) stream = xstream[p - 1];
            B = nbp;
            // part p starts when part p-1 has entered its first rollout (one sampler later) and tells part p+1 when it gets there itself
            const int r = step_enqueue_view(injected, skew && p > 0 ? ev_skew[p - 1] : nullptr, skew && p + 1 < np ? ev_skew[p] : nullptr);
            if (!rc) rc = r;
            if (!r && tail) tail();
            shift_slots(nbp); b0 += nbp;
        }
        shift_slots(-b0); B = B0; stream = main_stream; coop_share = 1;
    }
    chain_fresh = false;
    mpc_step += 1;
    if (env_join && np >= 2) { chains_join(); chains_fork(); }
    if (!rc && !launch_err.empty()) { err = launch_err; launch_err.clear(); return MPOPIS_ERR_HIP; }
    return rc;
}

// a single-step call: fork and join per call
int mpopis_handle::policy_step_enqueue(bool injected) {
    chains_fork();
    const int rc = chains_step(injected);
    chains_join();
    return rc;
}

int mpopis_handle::step_enqueue_view(bool injected, hipEvent_t wait_first, hipEvent_t record_after_first_sampler) {
    const int pol = cfg.policy;
    if (wait_first) (void)hipStreamWaitEvent(stream, wait_first, 0);
    const size_t nn = (size_t)cs * cs, per = (size_t)cs * K;
    const bool sigma_fixed = (pol == MPOPIS_POL_MPPI || pol == MPOPIS_POL_GMPPI || pol == MPOPIS_POL_IMPPI || pol == MPOPIS_POL_MUAISMPPI);
    // status / active / iters reset, U_orig = pol.U (d_Uin keeps U_orig; d_Ucur is the rebinding pol.U inside the loop), extended start states
    launch_step_begin(status_sticky ? nullptr : d_status, d_active, alive_gate, d_iters, d_U, d_Uin, d_Ucur, B, cs,
                      env.kind == MPOPIS_ENV_CAR ? d_x : nullptr, d_xext, env.ncars, stream, weights_in_moments ? d_cmin : nullptr, env.track, d_iters_acc, slot_tracks());
    if (!sigma_fixed) {                                                                                                          // Σ′ = pol.Σ
        if (S0stride) copy_f64(S0.Sigma, d_Sig, (size_t)B * nn, stream);                                                         // (each slot's own)
        else hipLaunchKernelGGL(k_bcast_f64, dim3((nn + 255) / 256), dim3(256), 0, stream, S0.Sigma, d_Sig, nn, B);
    }
    if (pol == MPOPIS_POL_CMAMPPI) cma_begin();
    // Shapes the fused sampler does not cover (cs > 128: Z goes through memory anyway) with device RNG, a dense proposal from iteration 2 on
    // and the handle's other streams free: prefetch Z on a side stream (see below).  For fusable shapes the prefetch was measured and LOSES
    // (C5, 64 trials: 6.72 vs 6.45 ms per step: the drawing then competes with the moments kernel instead of filling the MFMA bubbles of
    // the fused kernel); MPOPIS_ZPREFETCH=2 forces it for such A/B runs, 0 disables it.
    static const int env_zpre = [] { const char* e = getenv("MPOPIS_ZPREFETCH"); return e ? atoi(e) : 1; }();
    // (the fork and the wait are two packets of ~6 us each on the main stream: below ~4 M normals per draw -- one or two C4 trials, an 8-12 us kernel -- drawing in line is
    // shorter: 4.20 -> 4.165 ms per C4 step at one trial, 4.55 -> 4.525 at two, neutral at four, +1 % at eight)
    // (the antithetic and Latin-hypercube draws are generated in line: no prefetch, no fused form -- they end in the kernels an injected step runs)
    const bool strat = !injected && noise_kind != MPOPIS_NOISE_PHILOX;
    const bool z_prefetch_ok = env_zpre && (env_zpre == 2 || (!sample_trmm_fusable(cs) && (size_t)B * cs * K >= (size_t)4000000)) && side_free && xstream[1] && !injected && !strat &&
                               pol != MPOPIS_POL_MPPI && pol != MPOPIS_POL_PMCMPPI /* d_Z holds E[:, idx] there */ && !(sigma_diag && sigma_fixed) && N > 1;
    bool z_prefetched = false;
    for (int n = 1; n <= N; ++n) {
        // ---- P = MvNormal(Σ′): Cholesky; Σ_inv only through gvec --------------------------------
        const double* Lp; size_t Lstride; const double* dsc = nullptr;
        const bool first_diag = sigma_diag && (sigma_fixed || n == 1);
        // :cmamppi draws from MvNormal(σ²Σ′) (:550-554).  In the first iteration Σ′ = pol.Σ and chol(σ²Σ′) = σ chol(pol.Σ): the shared factor of pol.Σ
        // is used like for every other policy and the step size scales the sampler's output (osc2) -- one Cholesky less per MPC step (160 us at
        // cs = 300).  From the second iteration on σ²Σ′ itself is factored, like the reference does: Σ′ drifts towards indefiniteness there
        // (:598 adds negative-weight terms) and whether a last pivot of relative size 1e-16 comes out positive decides between PosDefException now and
        // a numerically singular factor one iteration later -- factoring the unscaled Σ′ flipped exactly that in test_cma_posdef_error_matches_reference_behaviour.
        const bool cma_scaled = pol == MPOPIS_POL_CMAMPPI && N > 1;
        const double* osc2 = (cma_scaled && n == 1) ? cma_sigma2() : nullptr;
        const bool own_factor = !(sigma_fixed || n == 1);      // this iteration factors its own Σ′ (else: the factor of pol.Σ, shared or per slot)
        if (!own_factor) { Lp = S0.L; Lstride = S0stride; }
        else {
            time_begin(2);
            launch_potrf(d_Sig, nn, d_L, B, cs, cma_scaled ? cma_sigma2() : nullptr, d_status, d_active, stream, potrf_coop(), d_Lp, potrf_panel_doubles(cs));
            time_end();
            Lp = d_L; Lstride = nn;
        }
        cur_L = Lp; cur_Lstride = Lstride; cur_L_scaled = cma_scaled && n > 1;
        if (use_gvec()) launch_chol_solve_gvec(Lp, Lstride, d_Uin, sv_gamma(), d_gvec, B, cs, d_active, stream, osc2);
        // ---- E = rand(rng, P, K) ----------------------------------------------------------------
        time_begin(1);
        if (first_diag && !(pol == MPOPIS_POL_CMAMPPI)) dsc = d_dscale;        // sqrt(diag Σ) per slot, written by mpopis_set_Sigma
        double* Zdst = dsc ? d_E : d_Z;
        bool fused = false;
        if (injected) {
            // B x N x (cs x K col-major) -> rows; source slot stride N*per
            if (pol == MPOPIS_POL_MPPI) launch_mppi_Z_in(d_Zin, Zdst, B, T, K, as, stream);       // N == 1
            else launch_transpose_in(d_Zin + (size_t)(n - 1) * per, Zdst, B, cs, K, stream, (size_t)N * per);
            if (dsc) launch_scale_rows(Zdst, dsc, B, cs, K, stream);
        } else if (strat) {
            launch_sample_strat(Zdst, B, cs, K, as, pol == MPOPIS_POL_MPPI, noise_kind, d_seeds, (uint32_t)mpc_step, (uint32_t)(n - 1), d_active, stream, d_rng_tab);
            if (dsc) launch_scale_rows(Zdst, dsc, B, cs, K, stream);
        } else if (z_prefetched) {
            // this iteration's standard normals were drawn on the side stream while the previous iteration's reweighting / moments / Cholesky
            // kernels (a few workgroups each) left the chip idle: only the matrix product is left on the critical path
            (void)hipStreamWaitEvent(stream, ev_skew[1], 0);
            z_prefetched = false;
        } else if (!dsc && pol != MPOPIS_POL_MPPI) {
            // dense proposal: draw inside the unwhitening kernel when the shape allows it (no Z round trip through HBM)
            fused = launch_sample_trmm_fused(Lp, Lstride, d_E, B, cs, K, d_seeds, (uint32_t)mpc_step, (uint32_t)(n - 1), d_active, stream, d_rng_tab,
                                             own_factor ? d_Lp : S0.Lp, own_factor ? potrf_panel_doubles(cs) : P0stride, osc2);
            if (!fused) launch_sample_normal(Zdst, B, cs, K, as, 0, d_seeds, (uint32_t)mpc_step, (uint32_t)(n - 1), dsc, d_active, stream, d_rng_tab);
        } else {
            launch_sample_normal(Zdst, B, cs, K, as, pol == MPOPIS_POL_MPPI, d_seeds, (uint32_t)mpc_step, (uint32_t)(n - 1), dsc, d_active, stream, d_rng_tab);
        }
        if (!dsc && !fused) launch_trmm_LZ_mfma(Lp, Lstride, d_Z, d_E, B, cs, K, d_active, stream, osc2);
        time_end();
        // (queued BEHIND the sampler / L.Z launch of this iteration: the event record that forks the side chain costs the main stream ~6-10 us, and there it
        // sits under the L.Z kernel instead of between the Cholesky and L.Z on the critical path; the trace still has ~200 us of slack before the Lanczos kernel needs it)
        {
            // :cmamppi: tr(Σ^-1) (= ||L^-1||_F², times σ² when L factors σ²Σ) of THIS iteration's update needs only the factor this iteration samples from -- start it now on the free
            // second stream (low wave priority: it shares the chip with the sampler and the rollout, which at small batches leave most CUs idle), so
            // that the Lanczos kernel of the update never waits for it.  It used to start behind the rollout, beside the sort, and part of it stayed on
            // the critical path: C4 6.56 -> 5.98 ms per step at one trial, 8.25 -> 7.70 at 8, 11.2 -> 10.8 at 16, neutral from 32 on
            // (MPOPIS_TRTRI_EARLY=0 restores the old placement for A/B runs).
            static const int env_early = [] { const char* e = getenv("MPOPIS_TRTRI_EARLY"); return e ? atoi(e) : 1; }();
            trtri_early = false;
            if (env_early && pol == MPOPIS_POL_CMAMPPI && side_free && n < N) {
                (void)hipEventRecord(ev_skew[2], stream);
                (void)hipStreamWaitEvent(xstream[0], ev_skew[2], 0);
                launch_trtri_fro(Lp, Lstride, d_fro_part, B, cs, nullptr, xstream[0], d_tri_dinv, false, d_Sig, cur_L_scaled ? d_sig2 : nullptr, d_lan_prep, d_tri_cnt);   // + the Lanczos run's spectrum bounds / quadrature nodes (Σ and σ² do not change before the update consumes them)
                (void)hipEventRecord(ev_join[0], xstream[0]);
                trtri_early = true;
            }
        }
        if (n == 1 && record_after_first_sampler) (void)hipEventRecord(record_after_first_sampler, stream);   // the next part starts when this one enters its first rollout
        // ---- trajectory_cost = simulate_model(pol, env, E, Σ_inv, U_orig) -------------------------
        rollout(d_Ucur, d_Uin, use_gvec() ? d_gvec : nullptr, d_active, d_iters, n);   // also records iters_run = n for the active slots
        fork_recorded = false;
        if (z_prefetch_ok && n < N) {
            // Z of iteration n+1 depends on nothing but (seed, MPC step, iteration): draw it now, beside the latency-bound kernels that follow
            (void)hipEventRecord(ev_fork, stream);                      // one fork point behind the rollout for both side chains (an event
            fork_recorded = true;                                       // record on the main stream costs ~6 us of its critical path)
            (void)hipStreamWaitEvent(xstream[1], ev_fork, 0);
            // (no `active` predicate: the main stream's sort may clear active[b] concurrently; Z of a slot that stops is simply not consumed)
            launch_sample_normal(d_Z, B, cs, K, as, 0, d_seeds, (uint32_t)mpc_step, (uint32_t)n, nullptr, nullptr, xstream[1], d_rng_tab);
            (void)hipEventRecord(ev_skew[1], xstream[1]);
            z_prefetched = true;
        }
        // ---- adapt (μ, Σ′) ----------------------------------------------------------------------
        if (n < N) {
            int rc = ais_update(n, injected);
            if (rc) return rc;
        }
    }
    // weights = compute_weights(IT(λ), cost); weighted_noise = Σ_k w_k (E_k + (pol.U - U_orig)); roll
    time_begin(3);
    launch_weights(d_cost, d_w, B, K, sv_nil(), alive_gate, d_status, stream);
    launch_wmean(d_E, d_w, d_Ucur, d_Uin, d_wn, B, cs, K, 0, alive_gate, stream);
    launch_finalize_env(d_wn, d_U, d_control, B, cs, as, T, env, stream);
    time_end();
    return MPOPIS_OK;
}
