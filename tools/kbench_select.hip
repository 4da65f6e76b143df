// kbench_select.hip -- runs ONE launch of a selection kernel (sort + elite early break, alias table, alias draw, softmax weights, the CE kernel's
// fused sort) on the inputs of a case file and writes the raw device outputs back to a file (dev / test tool, not shipped).
// It holds no reference arithmetic: tests/test_gpu_select_harness.py writes the case, reads the result and compares with the oracle and NumPy.
// build: tools/build_kbench.sh select       run: tools/kbench_select_bin <case file> <result file>
//
// case file (little endian; layout shared with tests/helpers/select_cases.py):
//   int64  hdr[8]  = { magic 'SELCASE1', op, B, K, m_elite, flags, di_stride, log_stride }      flags bit 0: run WITHOUT the workspaces (nullptr)
//   double par[2]  = { lambda, lambda_odd }         flags bit 1 (op 3): per-slot λ -- even slots weigh with lambda, odd slots with lambda_odd
//   int32  active[B], status0[B]            (status0: what status[] holds before the launch; the test poisons the inactive slot's entry itself)
//   op 0 sort / 4 CE sort: double cost[B K]
//   op 1 alias build:      double w[B K]
//   op 2 alias sample:     double accept[B K], du[B di_stride]; int32 alias[B K], di[B di_stride]
//   op 3 weights:          double cost[B K]
// result file:
//   int64  hdr[4]  = { magic 'SELRES01', form, guard, 0 }       form: the enum of engine.h the launcher's own choice function returned (op 2: 0, op 4: 100)
//   op 0 / 4: int32 order[B K + guard], active[B], done[B]
//   op 1:     double accept[B K + guard]; int32 alias[B K + guard], need[B]
//   op 2:     int32 out[B K + guard], log[B log_stride + guard]
//   op 3:     double w[B K + guard], wsum[B]; int32 status[B]
// Every output buffer is filled with the byte 0xA5 first (and carries `guard` extra entries), so the test sees what the launch left untouched.
#include "../mpopis_amd/csrc/engine.h"
#include "kbench_dev.h"
#include <cstdlib>
#include <cmath>
using namespace mpopis;
static const long long kMagicIn = 0x31455341434c4553ll, kMagicOut = 0x31305345524c4553ll;       // "SELCASE1", "SELRES01"
enum { OP_SORT = 0, OP_ALIAS_BUILD = 1, OP_ALIAS_SAMPLE = 2, OP_WEIGHTS = 3, OP_CE_SORT = 4 };


int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hdr; std::vector<double> par; std::vector<int> active, status0;
    if (!rd(fi, hdr, 8) || hdr[0] != kMagicIn) { printf("bad case header\n"); return 2; }
    const int op = (int)hdr[1]; const long long B = hdr[2], K = hdr[3], m_elite = hdr[4], flags = hdr[5], di_stride = hdr[6], log_stride = hdr[7];
    if (B < 1 || B > 64 || K < 1 || K > (1 << 20) || m_elite < 0 || m_elite > K || op < 0 || op > 4) { printf("case out of range\n"); return 2; }
    const bool no_ws = flags & 1, lam_per_slot = flags & 2;
    const size_t BK = (size_t)B * K;
    if (!rd(fi, par, 2) || !rd(fi, active, B) || !rd(fi, status0, B)) { printf("short case file\n"); return 2; }
    std::vector<double> f0, f1; std::vector<int32_t> i0, i1;
    bool ok = true;
    if (op == OP_ALIAS_SAMPLE) {
        if (di_stride < K || log_stride < K || di_stride > 4 * K + 64 || log_stride > 4 * K + 64) { printf("bad strides\n"); return 2; }
        ok = rd(fi, f0, BK) && rd(fi, f1, (size_t)B * di_stride) && rd(fi, i0, BK) && rd(fi, i1, (size_t)B * di_stride);
    } else ok = rd(fi, f0, BK);
    if (!ok || fgetc(fi) != EOF) { printf("case file has the wrong length\n"); return 2; }
    fclose(fi);

    hipStream_t s; CK(hipStreamCreate(&s));
    int* d_active; CK(dupload(&d_active, active));
    long long form = 0;
    std::vector<double> of0, of1; std::vector<int32_t> oi0, oi1, oi2;
    if (op == OP_SORT || op == OP_CE_SORT) {
        double* d_cost; int32_t* d_order; CK(dupload(&d_cost, f0)); CK(dpoison(&d_order, BK + kGuard));
        // workspace as the engine gives it (engine_ais.hip): skey = a [B][K] double buffer with whatever the last alias table left in it, done = B zeroed ints
        double* d_skey = nullptr; int* d_done = nullptr;
        CK(dpoison(&d_skey, BK)); CK(hipMalloc(&d_done, B * 4)); CK(hipMemset(d_done, 0, B * 4));
        if (op == OP_SORT) {
            form = sortperm_form((int)B, (int)K, !no_ws, sortperm_multi_enabled());
            launch_sortperm(d_cost, d_order, (int)B, (int)K, (int)m_elite, d_active, s, no_ws ? nullptr : d_skey, no_ws ? nullptr : d_done);
        } else {
            const int cs = 4, est = MPOPIS_SIGMA_EST_MLE;
            if (!ce_sort_fusable((int)K) || m_elite > K || !ce_cov_small_ok(cs, (int)m_elite, est)) { printf("the CE kernel does not take this case\n"); return 2; }
            double *d_E, *d_mu, *d_S, *d_U;
            CK(hipMalloc(&d_E, BK * cs * 8)); CK(hipMemset(d_E, 0, BK * cs * 8));
            CK(dpoison(&d_mu, (size_t)B * cs)); CK(dpoison(&d_S, (size_t)B * cs * cs)); CK(hipMalloc(&d_U, B * cs * 8)); CK(hipMemset(d_U, 0, B * cs * 8));
            form = 100;
            launch_ce_cov_small(d_E, d_order, d_mu, d_S, d_U, (int)B, cs, (int)K, (int)m_elite, est, 10e-9, d_active, s, d_cost);
        }
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(oi0, d_order, BK + kGuard)); CK(dfetch(oi1, d_active, B)); CK(dfetch(oi2, d_done, B));
    } else if (op == OP_ALIAS_BUILD) {
        double *d_w, *d_accept; int32_t *d_alias, *d_stack = nullptr; int* d_need;
        CK(dupload(&d_w, f0)); CK(dpoison(&d_accept, BK + kGuard)); CK(dpoison(&d_alias, BK + kGuard)); CK(dpoison(&d_need, B));
        if (K > alias_lds_max_K()) CK(dpoison(&d_stack, BK * 2));                  // engine_api.hip: the two stacks of the global-workspace construction
        form = alias_build_form((int)K, !no_ws, alias_par_enabled());
        launch_alias_build(d_w, d_accept, d_alias, (int)B, (int)K, d_active, s, no_ws ? nullptr : d_need, d_stack);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_accept, BK + kGuard)); CK(dfetch(oi0, d_alias, BK + kGuard)); CK(dfetch(oi1, d_need, B));
    } else if (op == OP_ALIAS_SAMPLE) {
        // the draw kernel indexes with alias[] and di[]: only a table the host has validated gets near it
        for (size_t e = 0; e < BK; ++e) if (!std::isfinite(f0[e]) || i0[e] < 0 || i0[e] >= K) { printf("invalid table entry %zu\n", e); return 3; }
        for (size_t e = 0; e < i1.size(); ++e) if (i1[e] < 0 || i1[e] >= K) { printf("invalid draw index %zu\n", e); return 3; }
        double *d_accept, *d_du; int32_t *d_alias, *d_di, *d_out, *d_log;
        CK(dupload(&d_accept, f0)); CK(dupload(&d_du, f1)); CK(dupload(&d_alias, i0)); CK(dupload(&d_di, i1));
        CK(dpoison(&d_out, BK + kGuard)); CK(dpoison(&d_log, (size_t)B * log_stride + kGuard));
        launch_alias_sample(d_accept, d_alias, d_di, (size_t)di_stride, d_du, d_out, d_log, (size_t)log_stride, (int)B, (int)K, d_active, s);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(oi0, d_out, BK + kGuard)); CK(dfetch(oi1, d_log, (size_t)B * log_stride + kGuard));
    } else {
        double *d_cost, *d_w, *d_wsum; int* d_status;
        CK(dupload(&d_cost, f0)); CK(dpoison(&d_w, BK + kGuard)); CK(dpoison(&d_wsum, B)); CK(dupload(&d_status, status0));
        form = weights_form((int)K);
        SlotVal nil{-1 / par[0], nullptr};
        if (lam_per_slot) {
            std::vector<double> nil_b(B);
            for (long long b = 0; b < B; ++b) nil_b[b] = -1 / par[b & 1];
            double* d_nil; CK(dupload(&d_nil, nil_b));
            nil.per_slot = d_nil;
        }
        launch_weights(d_cost, d_w, (int)B, (int)K, nil, d_active, d_status, s, d_wsum);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_w, BK + kGuard)); CK(dfetch(of1, d_wsum, B)); CK(dfetch(oi0, d_status, B));
    }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { printf("cannot write %s\n", argv[2]); return 2; }
    const std::vector<long long> oh = {kMagicOut, form, kGuard, 0};
    if (!wr(fo, oh) || !wr(fo, of0) || !wr(fo, of1) || !wr(fo, oi0) || !wr(fo, oi1) || !wr(fo, oi2) || fclose(fo) != 0) { printf("write failed\n"); return 2; }
    printf("op %d B %lld K %lld form %lld\n", op, B, K, form);
    return 0;
}
