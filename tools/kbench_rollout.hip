// kbench_rollout.hip -- runs the rollout launcher (launch_rollout: every body of kernels_rollout.hip, its per-slot-env twins of kernels_rollout_slots.hip and
// the fleet body of kernels_rollout_fleet.hip, with the start state made by launch_extend_state or launch_step_begin) or the step-begin launcher alone on the launches of a case file and writes the raw device outputs back to a file (dev / test
// tool, not shipped).  It holds no reference arithmetic: tests/test_gpu_rollout_harness.py writes the case, reads the result and compares with the
// oracle, NumPy longdouble and exact invariants (the per-slot ops: tests/test_gpu_rollout_slots_harness.py).  It calls only launchers of engine.h; the launches of one file share the process and therefore the
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
// The per-slot ops carry a track table: track_P (i32 [ntracks], the point counts), tx / ty / tw (the tracks' points, concatenated in that order) and
// track_of_slot (i32 [B]).  Every distinct track is uploaded once (dtrack); slot b's descriptor is a copy of that of track track_of_slot[b], and the [B]
// descriptor array is what the launchers get as SlotEnv::track / slot_tk.  The SlotEnv is the one a handle forms (engine_handle.h: slot_env()): a car
// launch sets car + track, a fleet cars + track with car null, a simple env mc or cp alone; lds_all / lds_ring come from slot_tracks_lds (engine.h),
// which mpopis_set_tracks calls too.  The shared EnvDesc holds the parameters of slot 0 (fleet: of its car 0) and the first track of the table.
// op 2 ROLLOUT_SLOTS  ipar { kind, ncars, K, T, ntracks (0 for the simple envs), iter_n, share, want_traj, want_iters, begin, fleet (1: params per car) }
//               arrays 0..15 as op ROLLOUT with params [B][np] (fleet: [B][ncars][20]) and tx / ty / tw concatenated; 16: track_P, 17: track_of_slot
//               the start state by launch_extend_state / launch_step_begin with slot_tk      -> as op ROLLOUT
// op 3 BEGIN_SLOTS    ipar { ncars, cs, ntracks }
//               arrays 0..9 as op BEGIN with tx / ty / tw concatenated (x is required); 10: track_P, 11: track_of_slot      -> as op BEGIN, both launchers with slot_tk
#include "../mpopis_amd/csrc/engine.h"
#include "kbench_dev.h"
#include <cstdlib>
#include <cmath>
using namespace mpopis;
enum { OP_ROLLOUT = 0, OP_BEGIN = 1, OP_ROLLOUT_SLOTS = 2, OP_BEGIN_SLOTS = 3 };

// the track table of the per-slot ops (arrays iP: track_P, ix .. ix + 2: tx, ty, tw, itos: track_of_slot) -> the [B] descriptors on the host and on the
// device; 0: fine, 1: HIP error (printed), 2: bad case
static int make_slot_tracks(const Launch& L, int iP, int ix, int itos, long long ntracks, int minP, std::vector<Track>* host, Track** dev) {
    const long long B = L.B;
    if (ntracks < 1 || ntracks > 64 || !L.need(iP, 1, ntracks, false) || !L.need(itos, 1, B, false)) return 2;
    const int *P = (const int*)L.host(iP), *tos = (const int*)L.host(itos);
    long long tot = 0;
    for (long long i = 0; i < ntracks; ++i) { if (P[i] < minP || P[i] > kMaxTrackPoints) return 2; tot += P[i]; }
    for (long long b = 0; b < B; ++b) if (tos[b] < 0 || tos[b] >= ntracks) return 2;
    if (!L.need(ix, 0, tot, false) || !L.need(ix + 1, 0, tot, false) || !L.need(ix + 2, 0, tot, false)) return 2;
    std::vector<Track> tks((size_t)ntracks);
    hipError_t e;
    for (long long i = 0, off = 0; i < ntracks; off += P[i], ++i)
        if ((e = dtrack(&tks[i], TrackHost(P[i], L.f64(ix) + off, L.f64(ix + 1) + off, L.f64(ix + 2) + off))) != hipSuccess) { printf("HIP error %s in dtrack\n", hipGetErrorString(e)); return 1; }
    host->resize((size_t)B);
    for (long long b = 0; b < B; ++b) (*host)[b] = tks[tos[b]];
    if ((e = dupv(dev, *host)) != hipSuccess) { printf("HIP error %s for the slot tracks\n", hipGetErrorString(e)); return 1; }
    return 0;
}

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
        if (const char* err = read_launch(fi, CaseLimits{3, 1, 8, 18, 2}, &L)) BAD(err);
        const int op = L.op; const long long B = L.B;
        const std::vector<long long>& ip = L.ip; const std::vector<double>& dp = L.dp; const std::vector<Arr>& A = L.A;
        auto need = [&](int i, long long type, long long count, bool optional) { return L.need(i, type, count, optional); };
        auto f64 = [&](int i) { return L.f64(i); };
        long long form[4] = {0, 0, 0, 0};
        std::vector<Out> outs;
        if (op == OP_ROLLOUT || op == OP_ROLLOUT_SLOTS) {
            const bool slots = op == OP_ROLLOUT_SLOTS;
            const long long kind = ip[0], ncars = ip[1], K = ip[2], T = ip[3], P = ip[4] /* slots: the number of tracks */, iter_n = ip[5], share = ip[6], want_traj = ip[7], want_iters = ip[8], begin = ip[9];
            const bool car = kind == MPOPIS_ENV_CAR, fleet = slots && ip[10] != 0;
            if ((kind != MPOPIS_ENV_CAR && kind != MPOPIS_ENV_MOUNTAINCAR && kind != MPOPIS_ENV_CARTPOLE) || K < 1 || K > 8192 || T < 1 || T > 64 || share < 1 || share > 64 ||
                (car && (ncars < 1 || ncars > kMaxCars || (!slots && (P < 3 || P > kMaxTrackPoints)))) || (!car && (ncars != 0 || P != 0)) || (fleet && (!car || ncars < 2))) BAD("case out of range");
            const long long as = car ? 2 * ncars : 1, ss = car ? 8 * ncars : (kind == MPOPIS_ENV_CARTPOLE ? 4 : 2), cs = as * T;
            const long long np1 = car ? kCarNParams : (kind == MPOPIS_ENV_CARTPOLE ? 11 : kMcNParams), np = slots ? B * (fleet ? ncars : 1) * np1 : np1;
            std::vector<Track> slot_tk; Track* d_slot_tk = nullptr;
            if (slots && car) {
                const int rc = make_slot_tracks(L, 16, 2, 17, P, 3, &slot_tk, &d_slot_tk);
                if (rc == 1) return 1;
                if (rc) BAD("bad track table");
            } else if (A[16].count || A[17].count || (slots && (A[2].count || A[3].count || A[4].count))) BAD("wrong array sizes");
            if (!need(0, 1, B, true) || !need(1, 0, np, false) || (!slots && (!need(2, 0, P, !car) || !need(3, 0, P, !car) || !need(4, 0, P, !car))) || !need(5, 0, as, false) ||
                !need(6, 0, as, false) || !need(7, 0, B * ss, false) || !need(8, 1, B, true) || !need(9, 1, B, true) || !need(10, 0, B * cs, false) ||
                !need(11, 0, B * cs, false) || !need(12, 0, B * cs * K, false) || !need(13, 0, B * cs, true) || !need(14, 2, B, true) || !need(15, 1, B, true)) BAD("wrong array sizes");
            RolloutArgs a{};
            a.env.kind = (int)kind; a.env.ncars = (int)ncars; a.env.ss = (int)ss; a.env.as = (int)as; a.env.custom = nullptr;
            if (car) {
                a.env.car = make_car_params(f64(1));
                if (a.env.car.nsub < 1 || a.env.car.nsub > 1000) BAD("sub-step count out of range");
                if (!slots) CK(dtrack(&a.env.track, TrackHost((int)P, f64(2), f64(3), f64(4))));
            } else if (kind == MPOPIS_ENV_CARTPOLE) a.env.cp = make_cp_params(f64(1));
            else a.env.mc = make_mc_params(f64(1));
            if (slots && car) {                                            // the SlotEnv of a handle after mpopis_set_tracks + mpopis_set_env_params_slots / _cars
                const int* P_of = (const int*)L.host(16);
                CK(dtrack(&a.env.track, TrackHost(P_of[0], f64(2), f64(3), f64(4))));
                std::vector<CarParams> cp((size_t)(np / np1));
                for (size_t i = 0; i < cp.size(); ++i) {
                    cp[i] = make_car_params(f64(1) + i * kCarNParams);
                    if (cp[i].nsub < 1 || cp[i].nsub > 1000) BAD("sub-step count out of range");
                }
                CarParams* d_cp; CK(dupv(&d_cp, cp));
                if (fleet) a.senv.cars = d_cp; else a.senv.car = d_cp;
                a.senv.track = d_slot_tk;
                slot_tracks_lds(slot_tk.data(), slot_tk.size(), &a.senv.lds_all, &a.senv.lds_ring);
            } else if (slots && kind == MPOPIS_ENV_CARTPOLE) {
                std::vector<CpParams> cp((size_t)B);
                for (long long b = 0; b < B; ++b) cp[b] = make_cp_params(f64(1) + b * np1);
                CpParams* d_cp; CK(dupv(&d_cp, cp)); a.senv.cp = d_cp;
            } else if (slots) {
                std::vector<McParams> mc((size_t)B);
                for (long long b = 0; b < B; ++b) mc[b] = make_mc_params(f64(1) + b * np1);
                McParams* d_mc; CK(dupv(&d_mc, mc)); a.senv.mc = d_mc;
            }
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
                    launch_step_begin(nullptr, w_active, nullptr, w_iters, d_U, w_Uin, w_Ucur, (int)B, (int)cs, d_x, d_xext, (int)ncars, s, nullptr, a.env.track, nullptr, d_slot_tk);
                } else launch_extend_state(d_x, d_xext, (int)B, (int)ncars, s, a.env.track, d_slot_tk);
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
            const bool slots = op == OP_BEGIN_SLOTS;
            const long long ncars = ip[0], cs = ip[1], P = ip[2] /* slots: the number of tracks */;
            const bool have_x = A[5].count != 0;
            if (ncars < 0 || ncars > kMaxCars || cs < 1 || cs > 4096 || P < 0 || (!slots && P > kMaxTrackPoints) || (have_x && (ncars < 1 || P < 1)) || (slots && !have_x)) BAD("case out of range");
            if (!need(0, 1, B, true) || !need(1, 1, B, true) || !need(2, 1, B, false) || !need(3, 2, B, true) || !need(4, 0, B * cs, false) || !need(5, 0, B * ncars * 8, true) ||
                (!slots && (!need(6, 0, P, false) || !need(7, 0, P, false) || !need(8, 0, P, false) || A[10].count || A[11].count)) || !need(9, 2, B, true)) BAD("wrong array sizes");
            Track tk{nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr};
            std::vector<Track> slot_tk; Track* d_slot_tk = nullptr;
            if (slots) {
                const int rc = make_slot_tracks(L, 10, 6, 11, P, 1, &slot_tk, &d_slot_tk);
                if (rc == 1) return 1;
                if (rc) BAD("bad track table");
                CK(dtrack(&tk, TrackHost(((const int*)L.host(10))[0], f64(6), f64(7), f64(8))));
            } else if (P > 0) CK(dtrack(&tk, TrackHost((int)P, f64(6), f64(7), f64(8))));
            int *d_alive, *d_status = nullptr, *d_active, *d_iters; unsigned long long *d_acc = nullptr, *d_cmin = nullptr; double *d_U, *d_x, *d_Uin, *d_Ucur, *d_xext = nullptr, *d_xref = nullptr;
            CK(dup(&d_alive, A[0])); CK(dup(&d_U, A[4])); CK(dup(&d_x, A[5]));
            if (A[1].count) CK(dout(&d_status, (size_t)B, &A[1]));
            CK(dout(&d_active, (size_t)B)); CK(dout(&d_iters, (size_t)B, &A[2]));
            if (A[3].count) CK(dout(&d_acc, (size_t)B, &A[3]));
            if (A[9].count) CK(dout(&d_cmin, (size_t)B, &A[9]));
            CK(dout(&d_Uin, (size_t)(B * cs))); CK(dout(&d_Ucur, (size_t)(B * cs)));
            if (ncars > 0) { CK(dout(&d_xext, (size_t)(B * ncars * kCarExt))); if (have_x) CK(dout(&d_xref, (size_t)(B * ncars * kCarExt))); }
            launch_step_begin(d_status, d_active, d_alive, d_iters, d_U, d_Uin, d_Ucur, (int)B, (int)cs, d_x, d_xext, (int)ncars, s, d_cmin, tk, d_acc, d_slot_tk);
            if (have_x) launch_extend_state(d_x, d_xref, (int)B, (int)ncars, s, tk, d_slot_tk);
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
