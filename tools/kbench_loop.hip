// kbench_loop.hip -- runs the launchers of the closed loop's other half -- launch_env_step / launch_env_query (kernels_reweight.hip), launch_harness_init /
// launch_harness_update (kernels_harness.hip), launch_trace_start / _step / _reorder (kernels_trace.hip), launch_plan_select / _assemble
// (kernels_plan.hip) -- on the launches of a case file and writes the raw device outputs back to a file (dev / test tool, not shipped).  It holds no
// reference arithmetic: tests/test_gpu_loop_harness.py writes the case, reads the result and compares with tests/helpers/loop_cases.py.  It calls
// only launchers of engine.h; the device Track is car_dynamics.h's TrackHost, as mpopis_set_track uploads it (kbench_dev.h: dtrack).
// build: tools/build_kbench.sh loop       run: tools/kbench_loop_bin <case file> <result file>
//
// case file (little endian; written by tests/helpers/loop_cases.py):
//   int64  hdr[2] = { magic 'LOPCASE1', n_launches }
//   per launch: int64 lh[5] = { op, B, n_ipar, n_dpar, n_arrays }; int64 ipar[n_ipar]; double dpar[n_dpar];
//               n_arrays x { int64 type (0 f64, 1 i32, 2 u64), int64 count; data }      in the fixed order of the op, count 0 = "not given" (nullptr)
// result file:
//   int64  hdr[3] = { magic 'LOPRES01', guard, n_launches }
//   per launch: int64 rh[2] = { op, n_arrays }; n_arrays x { int64 type, int64 count; data }   (count includes the guard entries; 0: no such buffer)
// Every output buffer is filled with the byte 0xA5 first and carries `guard` extra entries, so the test sees what the launches left untouched.
//
// The env of ops STEP and LOOP: ipar[0..2] = { kind (MPOPIS_ENV_*), ncars, P } and arrays 0..8 =
//   params (20 car / 8 mountaincar / 11 cartpole), tx, ty, tw, lo, hi, slot_params [B][20], slot_P (i32 [B]), slot_xyw (per slot: P_b x, P_b y, P_b w)
//   (slot_params / slot_P + slot_xyw given: the SlotEnv's per-slot car parameters / tracks)
// op 0 STEP     ipar { kind, ncars, P, reward, within, dist, beta, qreward (1: the launch gets this buffer), skip_step (1: launch_env_query only) }
//               arrays 9..: x [B][ss], t, done, action [B][as], status (before; not given: null), alive (not given: null)
//               launch_env_step, then launch_env_query -> x, t, done, reward, status, qreward, within, dist, beta
// op 1 LOOP     ipar { kind, ncars, P, nS (steps run, <= num_steps + 1), num_steps, laps, K, noise, env_step, actlog, trace mask (1 states, 2 rewards, 4 iters,
//               8 within, 16 dist, 32 beta), query, ss (simple envs, scripted, no query: the state size the launches are given instead of the env's own --
//               the harness and trace kernels take it as a plain number; 0: the env's) }      dpar { sx, sy, spsi }
//               arrays 9..: x0 [B][ss], xs [nS][B][ss], reward [nS][B], iters [nS][B], done_env [nS][B], control [nS][B][as], seeds (u64 [B]), alive0
//               launch_harness_init (alive0 given: copied over alive), launch_trace_start; per step s: copy control / iters and, without env_step, x /
//               reward / done_env of step s; with env_step launch_env_step (xs, reward, done_env not given); launch_harness_update; launch_trace_step;
//               with query launch_env_query
//               -> per step [nS][...]: hs, alive, x, reward, q_within, q_dist, q_beta;  at the end: hs, alive, x, actlog, status, t, states, rewards,
//                  iters, within, dist, beta (the trace)
// op 2 PLAN     ipar { K, top, cs }     arrays: w [B][K], E [B][cs][K], Ucur, Uin, wn [B][cs], active (not given: null)
//               launch_plan_select, launch_plan_assemble -> idx, wsel, controls, Eplan
// op 3 REORDER  ipar { J, per, elem_bytes }     arrays: in [J][B][per] (f64 or i32)  -> out [B][J][per]
#include "../mpopis_amd/csrc/engine.h"
#include "../mpopis_amd/csrc/philox.h"      // kRngTabDoubles
#include <algorithm>
#include "kbench_dev.h"
#include <cstdlib>
#include <cmath>
using namespace mpopis;
enum { OP_STEP = 0, OP_LOOP = 1, OP_PLAN = 2, OP_REORDER = 3 };

// EnvDesc and SlotEnv of ops STEP and LOOP from ipar[0..2] and arrays 0..8; 0: fine, 1: HIP error (printed), 2: bad case
static int make_env(const std::vector<long long>& ip, const std::vector<Arr>& A, long long B, EnvDesc* env, SlotEnv* senv) {
    const long long kind = ip[0], ncars = ip[1], P = ip[2];
    const bool car = kind == MPOPIS_ENV_CAR;
    if ((kind != MPOPIS_ENV_CAR && kind != MPOPIS_ENV_MOUNTAINCAR && kind != MPOPIS_ENV_CARTPOLE) ||
        (car && (ncars < 1 || ncars > kMaxCars || P < 3 || P > kMaxTrackPoints)) || (!car && (ncars != 0 || P != 0))) return 2;
    const long long as = car ? 2 * ncars : 1, ss = car ? 8 * ncars : (kind == MPOPIS_ENV_CARTPOLE ? 4 : 2);
    const long long np = car ? kCarNParams : (kind == MPOPIS_ENV_CARTPOLE ? 11 : kMcNParams);
    auto is = [&](int i, long long type, long long count) { return A[i].type == type && A[i].count == count; };
    auto f64 = [&](int i) { return (const double*)A[i].bytes.data(); };
    if (!is(0, 0, np) || !is(4, 0, as) || !is(5, 0, as)) return 2;
    if (car && (!is(1, 0, P) || !is(2, 0, P) || !is(3, 0, P))) return 2;
    if (!car && (A[1].count || A[2].count || A[3].count || A[6].count || A[7].count || A[8].count)) return 2;
    *env = EnvDesc{};
    env->kind = (int)kind; env->ncars = (int)ncars; env->ss = (int)ss; env->as = (int)as; env->custom = nullptr;
    for (int i = 0; i < kMaxAs; ++i) { env->lo[i] = -1.0; env->hi[i] = 1.0; }
    for (int i = 0; i < as; ++i) { env->lo[i] = f64(4)[i]; env->hi[i] = f64(5)[i]; }
    *senv = SlotEnv();
    if (!car) {
        if (kind == MPOPIS_ENV_CARTPOLE) env->cp = make_cp_params(f64(0)); else env->mc = make_mc_params(f64(0));
        return 0;
    }
    env->car = make_car_params(f64(0));
    if (env->car.nsub < 1 || env->car.nsub > 1000) return 2;
    hipError_t e = dtrack(&env->track, TrackHost((int)P, f64(1), f64(2), f64(3)));
    if (e != hipSuccess) { printf("HIP error %s in dtrack\n", hipGetErrorString(e)); return 1; }
    if (A[6].count) {
        if (!is(6, 0, B * kCarNParams)) return 2;
        std::vector<CarParams> cp((size_t)B);
        for (long long b = 0; b < B; ++b) {
            cp[b] = make_car_params(f64(6) + b * kCarNParams);
            if (cp[b].nsub < 1 || cp[b].nsub > 1000) return 2;
        }
        CarParams* d;
        if ((e = dupv(&d, cp)) != hipSuccess) { printf("HIP error %s for the slot parameters\n", hipGetErrorString(e)); return 1; }
        senv->car = d;
    }
    if (A[7].count) {
        if (!is(7, 1, B)) return 2;
        const int* sp = (const int*)A[7].bytes.data();
        long long tot = 0;
        for (long long b = 0; b < B; ++b) { if (sp[b] < 3 || sp[b] > kMaxTrackPoints) return 2; tot += 3ll * sp[b]; }
        if (!is(8, 0, tot)) return 2;
        std::vector<Track> tks((size_t)B);
        const double* q = f64(8);
        for (long long b = 0; b < B; ++b) {
            if ((e = dtrack(&tks[b], TrackHost(sp[b], q, q + sp[b], q + 2 * sp[b]))) != hipSuccess) { printf("HIP error %s in dtrack\n", hipGetErrorString(e)); return 1; }
            q += 3 * sp[b];
        }
        Track* d;
        if ((e = dupv(&d, tks)) != hipSuccess) { printf("HIP error %s for the slot tracks\n", hipGetErrorString(e)); return 1; }
        senv->track = d;
    } else if (A[8].count) return 2;
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi; long long nL = 0;
    if (const char* err = open_case(argv[1], "LOPCASE1", &nL, &fi)) BAD(err);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) BAD("cannot write the result file");
    const long long oh[3] = {magic_word("LOPRES01"), kGuard, nL};
    bool ok = write_arrays(fo, oh, 3, {});
    hipStream_t s; CK(hipStreamCreate(&s));
    for (long long li = 0; li < nL; ++li) {
        Launch L;
        if (const char* err = read_launch(fi, CaseLimits{3, 1, 256, 24, 2, 1ll << 26}, &L)) BAD(err);
        const int op = L.op; const long long B = L.B;
        const std::vector<long long>& ip = L.ip; const std::vector<double>& dp = L.dp; const std::vector<Arr>& A = L.A;
        auto need = [&](int i, long long type, long long count, bool optional) { return L.need(i, type, count, optional); };
        auto host = [&](int i) { return L.host(i); };
        std::vector<Out> outs;
        if (op == OP_STEP || op == OP_LOOP) {
            EnvDesc env; SlotEnv senv;
            const int rc = make_env(ip, A, B, &env, &senv);
            if (rc == 1) return 1;
            if (rc) BAD("bad env");
            long long ss = env.ss;
            const long long as = env.as, nc = std::max(1, env.ncars);
            if (op == OP_LOOP && ip[12]) {
                if (env.kind == MPOPIS_ENV_CAR || ip[8] || ip[11] || ip[12] < 2 || ip[12] > 4096) BAD("ss override out of range");
                ss = ip[12]; env.ss = (int)ss;
            }
            if (op == OP_STEP) {
                const bool skip = ip[8] != 0;
                if (!need(9, 0, B * ss, false) || !need(10, 1, B, false) || !need(11, 1, B, false) || !need(12, 0, B * as, skip) || !need(13, 1, B, true) ||
                    !need(14, 1, B, true)) BAD("wrong array sizes");
                double *d_x, *d_act, *d_rew = nullptr, *d_qrew = nullptr, *d_dist = nullptr, *d_beta = nullptr; int *d_t, *d_done, *d_status = nullptr, *d_alive, *d_within = nullptr;
                CK(dout(&d_x, (size_t)(B * ss), host(9))); CK(dout(&d_t, (size_t)B, host(10))); CK(dout(&d_done, (size_t)B, host(11)));
                CK(dup(&d_act, A[12])); CK(dup(&d_alive, A[14]));
                if (A[13].count) CK(dout(&d_status, (size_t)B, host(13)));
                if (ip[3]) CK(dout(&d_rew, (size_t)B));
                if (ip[4]) CK(dout(&d_within, (size_t)B));
                if (ip[5]) CK(dout(&d_dist, (size_t)(B * nc)));
                if (ip[6]) CK(dout(&d_beta, (size_t)(B * nc)));
                if (ip[7]) CK(dout(&d_qrew, (size_t)B));
                if (!skip) CK(launch_env_step(env, d_x, d_t, d_done, d_act, d_rew, d_status, d_alive, (int)B, s, senv));
                CK(launch_env_query(env, d_x, d_t, d_done, d_qrew, d_within, d_dist, d_beta, (int)B, s, senv));
                outs = {{0, (size_t)(B * ss), d_x}, {1, (size_t)B, d_t}, {1, (size_t)B, d_done}, {0, (size_t)B, d_rew}, {1, (size_t)B, d_status}, {0, (size_t)B, d_qrew},
                        {1, (size_t)B, d_within}, {0, (size_t)(B * nc), d_dist}, {0, (size_t)(B * nc), d_beta}};
            } else {
                const long long nS = ip[3], num_steps = ip[4], laps = ip[5], K = ip[6], noise = ip[7], env_step = ip[8], want_log = ip[9], mask = ip[10], query = ip[11];
                if (nS < 1 || num_steps < 0 || num_steps > 4096 || nS > num_steps + 1 || laps < 0 || laps > 4 || K < 1 || K > (1 << 20) || mask < 0 || mask > 63) BAD("case out of range");
                const bool scripted = !env_step;
                if (!need(9, 0, B * ss, false) || !need(10, 0, nS * B * ss, !scripted) || !need(11, 0, nS * B, !scripted) || !need(12, 1, nS * B, false) ||
                    !need(13, 1, nS * B, !scripted) || !need(14, 0, nS * B * as, false) || !need(15, 2, B, !noise) || !need(16, 1, B, true)) BAD("wrong array sizes");
                if (scripted != (A[10].count != 0) || scripted != (A[11].count != 0) || scripted != (A[13].count != 0)) BAD("scripted arrays and env_step disagree");
                const long long S = num_steps + 1;
                double *d_x, *d_rew, *d_ctl, *d_hs, *d_actlog = nullptr, *d_tab = nullptr; int *d_t, *d_done, *d_iters, *d_alive, *d_status; unsigned long long* d_seeds = nullptr;
                CK(dout(&d_x, (size_t)(B * ss), host(9))); CK(dout(&d_rew, (size_t)B)); CK(dout(&d_ctl, (size_t)(B * as))); CK(dout(&d_hs, (size_t)(B * kH_N)));
                CK(dout(&d_iters, (size_t)B)); CK(dout(&d_alive, (size_t)B));
                std::vector<int> zeros((size_t)B, 0);
                CK(dout(&d_t, (size_t)B, zeros.data())); CK(dout(&d_done, (size_t)B, zeros.data())); CK(dout(&d_status, (size_t)B, zeros.data()));
                if (want_log) CK(dout(&d_actlog, (size_t)(B * S * as)));
                if (noise) {
                    CK(dup(&d_seeds, A[15]));
                    CK(dmalloc((void**)&d_tab, sizeof(double) * kRngTabDoubles));
                    launch_rng_tab_init(d_tab, s);
                }
                TraceStepOut tr{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
                if (mask & 1) CK(dout(&tr.states, (size_t)(B * (S + 1) * ss)));
                if (mask & 2) CK(dout(&tr.rewards, (size_t)(B * S)));
                if (mask & 4) CK(dout(&tr.iters, (size_t)(B * S)));
                if (mask & 8) CK(dout(&tr.within, (size_t)(B * S)));
                if (mask & 16) CK(dout(&tr.dist, (size_t)(B * S * nc)));
                if (mask & 32) CK(dout(&tr.beta, (size_t)(B * S * nc)));
                double *l_hs, *l_x, *l_rew, *q_dist = nullptr, *q_beta = nullptr; int *l_alive, *q_within = nullptr;
                CK(dout(&l_hs, (size_t)(nS * B * kH_N))); CK(dout(&l_x, (size_t)(nS * B * ss))); CK(dout(&l_rew, (size_t)(nS * B))); CK(dout(&l_alive, (size_t)(nS * B)));
                if (query) { CK(dout(&q_within, (size_t)(nS * B))); CK(dout(&q_dist, (size_t)(nS * B * nc))); CK(dout(&q_beta, (size_t)(nS * B * nc))); }
                launch_harness_init(d_hs, d_alive, (int)B, s);
                if (A[16].count) CK(hipMemcpyAsync(d_alive, host(16), sizeof(int) * B, hipMemcpyHostToDevice, s));
                if (tr.states) launch_trace_start(d_x, tr.states, (int)B, (int)ss, (int)S, s);
                const StateNoise nz{dp[0], dp[1], dp[2], noise ? (const uint64_t*)d_seeds : (const uint64_t*)nullptr, d_tab};
                for (long long st = 0; st < nS; ++st) {
                    CK(hipMemcpyAsync(d_ctl, (const double*)host(14) + st * B * as, sizeof(double) * B * as, hipMemcpyHostToDevice, s));
                    CK(hipMemcpyAsync(d_iters, (const int*)host(12) + st * B, sizeof(int) * B, hipMemcpyHostToDevice, s));
                    if (scripted) {
                        CK(hipMemcpyAsync(d_x, (const double*)host(10) + st * B * ss, sizeof(double) * B * ss, hipMemcpyHostToDevice, s));
                        CK(hipMemcpyAsync(d_rew, (const double*)host(11) + st * B, sizeof(double) * B, hipMemcpyHostToDevice, s));
                        CK(hipMemcpyAsync(d_done, (const int*)host(13) + st * B, sizeof(int) * B, hipMemcpyHostToDevice, s));
                    } else CK(launch_env_step(env, d_x, d_t, d_done, d_ctl, d_rew, d_status, d_alive, (int)B, s, senv));
                    launch_harness_update(env, d_x, d_done, d_rew, d_iters, d_hs, d_alive, d_ctl, d_actlog, (int)st, (int)num_steps, (int)laps, (int)K, (int)B, nz, senv, s);
                    if (mask) launch_trace_step(env.kind, env.ncars, (int)ss, env.track, senv.track, d_x, d_rew, d_iters, d_hs + kH_cnt, kH_N, (int)st, (int)S, tr, (int)B, s);
                    if (query) CK(launch_env_query(env, d_x, d_t, d_done, nullptr, q_within + st * B, q_dist + st * B * nc, q_beta + st * B * nc, (int)B, s, senv));
                    CK(hipMemcpyAsync(l_hs + st * B * kH_N, d_hs, sizeof(double) * B * kH_N, hipMemcpyDeviceToDevice, s));
                    CK(hipMemcpyAsync(l_x + st * B * ss, d_x, sizeof(double) * B * ss, hipMemcpyDeviceToDevice, s));
                    CK(hipMemcpyAsync(l_rew + st * B, d_rew, sizeof(double) * B, hipMemcpyDeviceToDevice, s));
                    CK(hipMemcpyAsync(l_alive + st * B, d_alive, sizeof(int) * B, hipMemcpyDeviceToDevice, s));
                    CK(hipStreamSynchronize(s));                            // (one step at a time: a fault is reported at the step that caused it)
                }
                outs = {{0, (size_t)(nS * B * kH_N), l_hs}, {1, (size_t)(nS * B), l_alive}, {0, (size_t)(nS * B * ss), l_x}, {0, (size_t)(nS * B), l_rew},
                        {1, (size_t)(nS * B), q_within}, {0, (size_t)(nS * B * nc), q_dist}, {0, (size_t)(nS * B * nc), q_beta},
                        {0, (size_t)(B * kH_N), d_hs}, {1, (size_t)B, d_alive}, {0, (size_t)(B * ss), d_x}, {0, (size_t)(B * S * as), d_actlog}, {1, (size_t)B, d_status}, {1, (size_t)B, d_t},
                        {0, (size_t)(B * (S + 1) * ss), tr.states}, {0, (size_t)(B * S), tr.rewards}, {1, (size_t)(B * S), tr.iters}, {1, (size_t)(B * S), tr.within},
                        {0, (size_t)(B * S * nc), tr.dist}, {0, (size_t)(B * S * nc), tr.beta}};
            }
        } else if (op == OP_PLAN) {
            const long long K = ip[0], top = ip[1], cs = ip[2];
            if (K < 1 || K > 8192 || top < 1 || top > K || top > MPOPIS_PLAN_MAX_TOP || cs < 1 || cs > 1024) BAD("case out of range");
            if (!need(0, 0, B * K, false) || !need(1, 0, B * cs * K, false) || !need(2, 0, B * cs, false) || !need(3, 0, B * cs, false) || !need(4, 0, B * cs, false) ||
                !need(5, 1, B, true)) BAD("wrong array sizes");
            double *d_w, *d_E, *d_Ucur, *d_Uin, *d_wn, *d_wsel, *d_ctl, *d_Ep; int *d_active; int32_t* d_idx;
            CK(dup(&d_w, A[0])); CK(dup(&d_E, A[1])); CK(dup(&d_Ucur, A[2])); CK(dup(&d_Uin, A[3])); CK(dup(&d_wn, A[4])); CK(dup(&d_active, A[5]));
            CK(dout(&d_idx, (size_t)(B * top))); CK(dout(&d_wsel, (size_t)(B * top))); CK(dout(&d_ctl, (size_t)(B * cs))); CK(dout(&d_Ep, (size_t)(B * cs * (top + 1))));
            launch_plan_select(d_w, (int)B, (int)K, (int)top, d_idx, d_wsel, s, d_active);
            launch_plan_assemble(d_E, d_Ucur, d_Uin, d_wn, d_idx, (int)B, (int)cs, (int)K, (int)top, d_ctl, d_Ep, s, d_active);
            outs = {{1, (size_t)(B * top), d_idx}, {0, (size_t)(B * top), d_wsel}, {0, (size_t)(B * cs), d_ctl}, {0, (size_t)(B * cs * (top + 1)), d_Ep}};
        } else {
            const long long J = ip[0], per = ip[1], elem = ip[2];
            if (J < 1 || J > 64 || per < 1 || per > 65536 || (elem != 4 && elem != 8)) BAD("case out of range");
            if (!need(0, elem == 4 ? 1 : 0, J * B * per, false)) BAD("wrong array sizes");
            void* d_in; CK(dup(&d_in, A[0]));
            if (elem == 4) {
                int32_t* d_out; CK(dout(&d_out, (size_t)(J * B * per)));
                launch_trace_reorder(d_in, d_out, (int)B, (int)J, (size_t)per, 4, s);
                outs = {{1, (size_t)(J * B * per), d_out}};
            } else {
                double* d_out; CK(dout(&d_out, (size_t)(J * B * per)));
                launch_trace_reorder(d_in, d_out, (int)B, (int)J, (size_t)per, 8, s);
                outs = {{0, (size_t)(J * B * per), d_out}};
            }
        }
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        const long long rh[2] = {op, (long long)outs.size()};
        if (const int rc = write_back(fo, rh, 2, outs)) return rc;
        CK(dfree_all());
    }
    if (const char* err = close_case(fi)) BAD(err);
    if (!ok || fclose(fo) != 0) BAD("write failed");
    printf("launches %lld\n", nL);
    return 0;
}
