// kbench_rollout.hip -- runs the rollout launcher (launch_rollout: every body of kernels_rollout.hip, with the start state made by launch_extend_state or
// launch_step_begin) or the step-begin launcher alone on the launches of a case file and writes the raw device outputs back to a file (dev / test
// tool, not shipped).  It holds no reference arithmetic: tests/test_gpu_rollout_harness.py writes the case, reads the result and compares with the
// oracle, NumPy longdouble and exact invariants.  It calls only launchers of engine.h; the launches of one file share the process and therefore the
// settings read once per process (MPOPIS_ROLLOUT_DUO, MPOPIS_COOP_MAX_WG).
// build: tools/build_kbench.sh rollout       run: tools/kbench_rollout_bin <case file> <result file>
//
// case file (little endian; written by tests/helpers/rollout_cases.py):
//   int64  hdr[2] = { magic 'ROLCASE1', n_launches }
//   per launch: int64 lh[5] = { op, B, n_ipar, n_dpar, n_arrays }; int64 ipar[n_ipar]; double dpar[n_dpar];
//               n_arrays x { int64 type (0 f64, 1 i32, 2 u64), int64 count; data }      in the fixed order of the op, count 0 = "not given" (nullptr)
// result file:
//   int64  hdr[3] = { magic 'ROLRES01', guard, n_launches }
//   per launch: int64 rh[6] = { op, body, log, tlds, dynamic LDS bytes, n_arrays }  (rollout_form's value; zeros for BEGIN);
//               n_arrays x { int64 type, int64 count; data }     (count includes the guard entries; 0: the launch was not given this buffer)
// Every output buffer is filled with the byte 0xA5 first and carries `guard` extra entries, so the test sees what the launch left untouched.
//
// op 0 ROLLOUT  ipar { kind (MPOPIS_ENV_*), ncars, K, T, P, iter_n, share, want_traj, want_iters, begin (0 launch_extend_state, 1 launch_step_begin) }
//               arrays: active, params (20 car / 8 mountaincar / 11 cartpole), tx, ty, tw, lo, hi, x0, t0, done0, Ucur, Uorig, E [B][cs][K], gvec,
//                       cmin (u64: the value before the launch; not given: no cmin), status (i32: the value before the launch; not given: none)
//               -> cost, traj, cmin, status, iters, xext
// op 1 BEGIN    ipar { ncars, cs, P }
//               arrays: alive, status (before), iters (before), iters_acc (before), U, x [B][ncars][8], tx, ty, tw, cmin (before)
//               -> status, active, iters, iters_acc, Uin, Ucur, cmin, xext (launch_step_begin), xext (launch_extend_state on the same x)
#include "../mpopis_amd/csrc/engine.h"
#include "kbench_dev.h"
#include <cstdlib>
#include <cmath>
using namespace mpopis;
enum { OP_ROLLOUT = 0, OP_BEGIN = 1 };

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi; long long nL = 0;
    if (const char* err = open_case(argv[1], "ROLCASE1", &nL, &fi)) BAD(err);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) BAD("cannot write the result file");
    const long long oh[3] = {magic_word("ROLRES01"), kGuard, nL};
    bool ok = write_arrays(fo, oh, 3, {});
    hipStream_t s; CK(hipStreamCreate(&s));
    for (long long li = 0; li < nL; ++li) {
        Launch L;
        if (const char* err = read_launch(fi, CaseLimits{1, 1, 8, 16, 2}, &L)) BAD(err);
        const int op = L.op; const long long B = L.B;
        const std::vector<long long>& ip = L.ip; const std::vector<double>& dp = L.dp; const std::vector<Arr>& A = L.A;
        auto need = [&](int i, long long type, long long count, bool optional) { return L.need(i, type, count, optional); };
        auto f64 = [&](int i) { return L.f64(i); };
        long long form[4] = {0, 0, 0, 0};
        std::vector<Out> outs;
        if (op == OP_ROLLOUT) {
            const long long kind = ip[0], ncars = ip[1], K = ip[2], T = ip[3], P = ip[4], iter_n = ip[5], share = ip[6], want_traj = ip[7], want_iters = ip[8], begin = ip[9];
            const bool car = kind == MPOPIS_ENV_CAR;
            if ((kind != MPOPIS_ENV_CAR && kind != MPOPIS_ENV_MOUNTAINCAR && kind != MPOPIS_ENV_CARTPOLE) || K < 1 || K > 8192 || T < 1 || T > 64 || share < 1 || share > 64 ||
                (car && (ncars < 1 || ncars > kMaxCars || P < 3 || P > kMaxTrackPoints)) || (!car && (ncars != 0 || P != 0))) BAD("case out of range");
            const long long as = car ? 2 * ncars : 1, ss = car ? 8 * ncars : (kind == MPOPIS_ENV_CARTPOLE ? 4 : 2), cs = as * T;
            const long long np = car ? kCarNParams : (kind == MPOPIS_ENV_CARTPOLE ? 11 : kMcNParams);
            if (!need(0, 1, B, true) || !need(1, 0, np, false) || !need(2, 0, P, !car) || !need(3, 0, P, !car) || !need(4, 0, P, !car) || !need(5, 0, as, false) ||
                !need(6, 0, as, false) || !need(7, 0, B * ss, false) || !need(8, 1, B, true) || !need(9, 1, B, true) || !need(10, 0, B * cs, false) ||
                !need(11, 0, B * cs, false) || !need(12, 0, B * cs * K, false) || !need(13, 0, B * cs, true) || !need(14, 2, B, true) || !need(15, 1, B, true)) BAD("wrong array sizes");
            RolloutArgs a{};
            a.env.kind = (int)kind; a.env.ncars = (int)ncars; a.env.ss = (int)ss; a.env.as = (int)as; a.env.custom = nullptr;
            if (car) {
                a.env.car = make_car_params(f64(1));
                if (a.env.car.nsub < 1 || a.env.car.nsub > 1000) BAD("sub-step count out of range");
                CK(dtrack(&a.env.track, TrackHost((int)P, f64(2), f64(3), f64(4))));
            } else if (kind == MPOPIS_ENV_CARTPOLE) a.env.cp = make_cp_params(f64(1));
            else a.env.mc = make_mc_params(f64(1));
            for (int i = 0; i < as; ++i) { a.env.lo[i] = f64(5)[i]; a.env.hi[i] = f64(6)[i]; }
            double *d_x, *d_U, *d_Uo, *d_E, *d_g, *d_cost, *d_traj = nullptr, *d_xext = nullptr; int *d_active, *d_t0, *d_done0, *d_status = nullptr, *d_iters = nullptr; unsigned long long* d_cmin = nullptr;
            CK(dup(&d_active, A[0])); CK(dup(&d_x, A[7])); CK(dup(&d_t0, A[8])); CK(dup(&d_done0, A[9])); CK(dup(&d_U, A[10])); CK(dup(&d_Uo, A[11])); CK(dup(&d_E, A[12])); CK(dup(&d_g, A[13]));
            CK(dout(&d_cost, (size_t)(B * K)));
            if (want_traj) CK(dout(&d_traj, (size_t)(B * K * ss * T)));
            if (A[14].count) CK(dout(&d_cmin, (size_t)B, &A[14]));
            if (A[15].count) CK(dout(&d_status, (size_t)B, &A[15]));
            if (want_iters) CK(dout(&d_iters, (size_t)B));
            if (car) {
                CK(dout(&d_xext, (size_t)(B * ncars * kCarExt)));
                if (begin) {                                               // the start state as policy_step makes it; the step-begin's own outputs are op BEGIN's business
                    int *w_active, *w_iters; double *w_Uin, *w_Ucur;
                    CK(dout(&w_active, (size_t)B)); CK(dout(&w_iters, (size_t)B)); CK(dout(&w_Uin, (size_t)(B * cs))); CK(dout(&w_Ucur, (size_t)(B * cs)));
                    launch_step_begin(nullptr, w_active, nullptr, w_iters, d_U, w_Uin, w_Ucur, (int)B, (int)cs, d_x, d_xext, (int)ncars, s, nullptr, a.env.track);
                } else launch_extend_state(d_x, d_xext, (int)B, (int)ncars, s, a.env.track);
            }
            a.B = (int)B; a.K = (int)K; a.T = (int)T; a.cs = (int)cs;
            a.x0 = car ? nullptr : d_x; a.x0ext = d_xext; a.t0 = d_t0; a.done0 = d_done0; a.Ucur = d_U; a.Uorig = d_Uo; a.E = d_E; a.gvec = d_g;
            a.cost = d_cost; a.traj = d_traj; a.active = d_active; a.iters = d_iters; a.iter_n = (int)iter_n; a.cmin = d_cmin; a.status = d_status; a.share = (int)share;
            const RolloutForm f = rollout_form(a);
            form[0] = (long long)f.body; form[1] = f.log; form[2] = f.tlds; form[3] = (long long)f.lds;
            if (!launch_rollout(a, s)) BAD("no rollout kernel for this case");
            outs = {{0, (size_t)(B * K), d_cost}, {0, (size_t)(B * K * ss * T), d_traj}, {2, (size_t)B, d_cmin}, {1, (size_t)B, d_status}, {1, (size_t)B, d_iters},
                    {0, (size_t)(B * ncars * kCarExt), d_xext}};
        } else {
            const long long ncars = ip[0], cs = ip[1], P = ip[2];
            const bool have_x = A[5].count != 0;
            if (ncars < 0 || ncars > kMaxCars || cs < 1 || cs > 4096 || P < 0 || P > kMaxTrackPoints || (have_x && (ncars < 1 || P < 1))) BAD("case out of range");
            if (!need(0, 1, B, true) || !need(1, 1, B, true) || !need(2, 1, B, false) || !need(3, 2, B, true) || !need(4, 0, B * cs, false) || !need(5, 0, B * ncars * 8, true) ||
                !need(6, 0, P, false) || !need(7, 0, P, false) || !need(8, 0, P, false) || !need(9, 2, B, true)) BAD("wrong array sizes");
            Track tk{nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr};
            if (P > 0) CK(dtrack(&tk, TrackHost((int)P, f64(6), f64(7), f64(8))));
            int *d_alive, *d_status = nullptr, *d_active, *d_iters; unsigned long long *d_acc = nullptr, *d_cmin = nullptr; double *d_U, *d_x, *d_Uin, *d_Ucur, *d_xext = nullptr, *d_xref = nullptr;
            CK(dup(&d_alive, A[0])); CK(dup(&d_U, A[4])); CK(dup(&d_x, A[5]));
            if (A[1].count) CK(dout(&d_status, (size_t)B, &A[1]));
            CK(dout(&d_active, (size_t)B)); CK(dout(&d_iters, (size_t)B, &A[2]));
            if (A[3].count) CK(dout(&d_acc, (size_t)B, &A[3]));
            if (A[9].count) CK(dout(&d_cmin, (size_t)B, &A[9]));
            CK(dout(&d_Uin, (size_t)(B * cs))); CK(dout(&d_Ucur, (size_t)(B * cs)));
            if (ncars > 0) { CK(dout(&d_xext, (size_t)(B * ncars * kCarExt))); if (have_x) CK(dout(&d_xref, (size_t)(B * ncars * kCarExt))); }
            launch_step_begin(d_status, d_active, d_alive, d_iters, d_U, d_Uin, d_Ucur, (int)B, (int)cs, d_x, d_xext, (int)ncars, s, d_cmin, tk, d_acc);
            if (have_x) launch_extend_state(d_x, d_xref, (int)B, (int)ncars, s, tk);
            outs = {{1, (size_t)B, d_status}, {1, (size_t)B, d_active}, {1, (size_t)B, d_iters}, {2, (size_t)B, d_acc}, {0, (size_t)(B * cs), d_Uin}, {0, (size_t)(B * cs), d_Ucur},
                    {2, (size_t)B, d_cmin}, {0, (size_t)(B * ncars * kCarExt), d_xext}, {0, (size_t)(B * ncars * kCarExt), d_xref}};
        }
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        const long long rh[6] = {op, form[0], form[1], form[2], form[3], (long long)outs.size()};
        if (const int rc = write_back(fo, rh, 6, outs)) return rc;
        CK(dfree_all());
    }
    if (const char* err = close_case(fi)) BAD(err);
    if (!ok || fclose(fo) != 0) BAD("write failed");
    printf("launches %lld\n", nL);
    return 0;
}
