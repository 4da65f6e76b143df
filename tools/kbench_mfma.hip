// kbench_mfma.hip -- runs ONE op of the matrix-core half of the AIS loop (the sampler E = L Z in its generic and fused Philox forms, the covariance
// scatter in every partial-kernel form with its finish kernel, the shrinkage kernels, both CE updates, the gather / mean helpers) on the inputs of a
// case file and writes the raw device outputs back to a file (dev / test tool, not shipped).  It holds no reference arithmetic:
// tests/test_gpu_mfma_harness.py writes the case, reads the result and compares with NumPy longdouble and the oracle.
// build: tools/build_kbench.sh mfma       run: tools/kbench_mfma_bin <case file> <result file>
//
// case file (little endian; written by tests/helpers/mfma_cases.py):
//   int64  hdr[6] = { magic 'MFMCASE1', op, B, n_ipar, n_dpar, n_arrays }
//   int64  ipar[n_ipar]; double dpar[n_dpar]
//   n_arrays x { int64 type (0 f64, 1 i32, 2 u64), int64 count; data }      in the fixed order of the op, count 0 = "not given" (nullptr)
// result file:
//   int64  hdr[4] = { magic 'MFMRES01', form, guard, n_arrays }; n_arrays x { int64 type, int64 count; data }     (count includes the guard entries)
// Every output buffer is filled with the byte 0xA5 first and carries `guard` extra entries, so the test sees what the launch left untouched; the
// K-split partial workspace of the scatter is filled with NaN, so a partial the finish kernel reads but no workgroup wrote shows in Σ′.
//
// op 0 TRMM        ipar { n, K, Lstride (0 or n n) }            arrays: active, L, Z, oscale2           -> E
// op 1 FUSED       ipar { n, K, shared, slo, shi }              arrays: active, A, seeds, oscale2       -> L, panel, E; form = the launcher's return value
// op 2 TWOKERNEL   like FUSED: launch_potrf, launch_sample_normal, launch_trmm_LZ_mfma                  -> L, Z, E
// op 3 WCOV        ipar { cs, K, m, ksplit, sel_batch, want_mu_out }    dpar { den, ridge, -1/λ }
//                  arrays: active, X, w, wsum, idx, mu, rscale, cost, mu_shift, u0 (given: u_add starts there)
//                  -> S, mu_out, u_add, cmin (u64: the slot minimum in engine.h's cost_key encoding before the launch, whatever the launch left after),
//                     part (the K-split partial workspace as the partial kernel left it, no guard: NaN wherever nothing was written)
//                  form = partial | sq << 8 | aug << 9 | from_cost << 10      (wcov_form)
// op 4 SHRINK      ipar { cs, m, kind (0 rblw, 1 oas, 2 ss, 3 lw) }  dpar { ridge }   arrays: active, S, Q      -> S, rs
// op 5 CE_SMALL    ipar { cs, K, m, est, ksplit }  dpar { ridge }    arrays: active, E, order, U                -> mu, S, U
// op 6 CE_GENERAL  the same through launch_ce_cov_general + launch_add_active, as mpopis_handle::ais_update runs them
// op 7 GATHER      ipar { cs, K, m, sub (0 gather_cols, 1 gather_cols + shift, 2 gather_mean, 3 wmean), normalize }
//                  arrays: active, X, idx, w, shiftA, shiftB                                             -> Xout, shift, mu
#include "../mpopis_amd/csrc/engine.h"
#include "../mpopis_amd/csrc/philox.h"
#include "kbench_dev.h"
#include <cstdlib>
#include <cmath>
using namespace mpopis;
enum { OP_TRMM = 0, OP_FUSED = 1, OP_TWOKERNEL = 2, OP_WCOV = 3, OP_SHRINK = 4, OP_CE_SMALL = 5, OP_CE_GENERAL = 6, OP_GATHER = 7 };

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi; Launch L;
    const char* err = open_case(argv[1], "MFMCASE1", nullptr, &fi);
    if (!err) err = read_launch(fi, CaseLimits{7, 1, 8, 16, 2, 1ll << 28, 0}, &L);
    if (!err) err = close_case(fi);
    if (err) BAD(err);
    const int op = L.op; const long long B = L.B, nD = L.nD;
    const std::vector<long long>& ip = L.ip; const std::vector<double>& dp = L.dp; const std::vector<Arr>& A = L.A;
    auto need = [&](int i, long long type, long long count, bool optional) { return L.need(i, type, count, optional); };
    if (!need(0, 1, B, false)) BAD("active[B] missing");

    hipStream_t s; CK(hipStreamCreate(&s));
    int* d_active; CK(dup(&d_active, A[0]));
    long long form = 0;
    std::vector<Out> outs;
    if (op == OP_TRMM) {
        const long long n = ip[0], K = ip[1], Ls = ip[2];
        if (n < 1 || n > 800 || K < 1 || K > 8192 || (Ls != 0 && Ls != n * n)) BAD("case out of range");
        if (!need(1, 0, (Ls ? B : 1) * n * n, false) || !need(2, 0, B * n * K, false) || !need(3, 0, B, true)) BAD("wrong array sizes");
        double *d_L, *d_Z, *d_osc, *d_E;
        CK(dup(&d_L, A[1])); CK(dup(&d_Z, A[2])); CK(dup(&d_osc, A[3])); CK(dout(&d_E, (size_t)(B * n * K)));
        launch_trmm_LZ_mfma(d_L, (size_t)Ls, d_Z, d_E, (int)B, (int)n, (int)K, d_active, s, d_osc);
        outs = {{0, (size_t)(B * n * K), d_E}};
    } else if (op == OP_FUSED || op == OP_TWOKERNEL) {
        const long long n = ip[0], K = ip[1], shared = ip[2];
        const uint32_t slo = (uint32_t)ip[3], shi = (uint32_t)ip[4];
        if (n < 1 || n > 144 || K < 1 || K > 8192) BAD("case out of range");
        const long long nL = shared ? 1 : B;
        if (!need(1, 0, nL * n * n, false) || !need(2, 2, B, false) || !need(3, 0, B, true)) BAD("wrong array sizes");
        const size_t pd = potrf_panel_doubles((int)n);
        double *d_A, *d_osc, *d_L, *d_panel, *d_E, *d_tab; uint64_t* d_seeds; int* d_status;
        CK(dup(&d_A, A[1])); CK(dup(&d_seeds, A[2])); CK(dup(&d_osc, A[3]));
        CK(dout(&d_L, (size_t)(nL * n * n))); CK(dout(&d_panel, (size_t)nL * pd)); CK(dout(&d_E, (size_t)(B * n * K)));
        CK(dfill(&d_tab, (size_t)kRngTabDoubles, 0)); CK(dfill(&d_status, (size_t)B, 0));
        launch_rng_tab_init(d_tab, s);
        // the factor as the engine makes it: per slot with the slots' active flags, or once (B = 1, no flags) for the shared first-iteration factor
        if (shared) launch_potrf(d_A, 0, d_L, 1, (int)n, nullptr, d_status, nullptr, s, CoopCtx(), pd ? d_panel : nullptr, 0);
        else launch_potrf(d_A, (size_t)(n * n), d_L, (int)B, (int)n, nullptr, d_status, d_active, s, CoopCtx(), pd ? d_panel : nullptr, pd);
        const size_t Lstride = shared ? 0 : (size_t)(n * n), pstride = shared ? 0 : pd;
        if (op == OP_FUSED) {
            form = launch_sample_trmm_fused(d_L, Lstride, d_E, (int)B, (int)n, (int)K, d_seeds, slo, shi, d_active, s, d_tab, d_panel, pstride, d_osc) ? 1 : 0;
            outs = {{0, (size_t)(nL * n * n), d_L}, {0, (size_t)nL * pd, d_panel}, {0, (size_t)(B * n * K), d_E}};
        } else {
            double* d_Z; CK(dout(&d_Z, (size_t)(B * n * K)));
            launch_sample_normal(d_Z, (int)B, (int)n, (int)K, 1, 0, d_seeds, slo, shi, nullptr, d_active, s, d_tab);
            launch_trmm_LZ_mfma(d_L, Lstride, d_Z, d_E, (int)B, (int)n, (int)K, d_active, s, d_osc);
            outs = {{0, (size_t)(nL * n * n), d_L}, {0, (size_t)(B * n * K), d_Z}, {0, (size_t)(B * n * K), d_E}};
        }
    } else if (op == OP_WCOV) {
        const long long cs = ip[0], K = ip[1], m = ip[2], ksplit = ip[3], sel_batch = ip[4], want_mu = ip[5];
        if (cs < 1 || cs > wcov_max_cs() || K < 1 || K > 8192 || m < 1 || m > K || ksplit < 1 || ksplit > 64) BAD("case out of range");
        if (!need(1, 0, B * cs * K, false) || !need(2, 0, B * K, true) || !need(3, 0, B, true) || !need(4, 1, B * K, true) || !need(5, 0, B * cs, true) ||
            !need(6, 0, B * cs, true) || !need(7, 0, B * K, true) || !need(8, 0, B * cs, true) || !need(9, 0, B * cs, true)) BAD("wrong array sizes");
        if (A[4].count) { const int32_t* ix = (const int32_t*)A[4].bytes.data(); for (long long e = 0; e < B * K; ++e) if (ix[e] < 0 || ix[e] >= K) BAD("invalid column index"); }
        if (!A[4].count && m != K) BAD("m < K needs idx");
        if (!A[5].count && !want_mu) BAD("neither mu nor mu_out");
        double *d_X, *d_w, *d_wsum, *d_mu, *d_rs, *d_cost, *d_shift, *d_S, *d_muo, *d_u, *d_part; int32_t* d_idx; unsigned long long* d_cmin;
        CK(dup(&d_X, A[1])); CK(dup(&d_w, A[2])); CK(dup(&d_wsum, A[3])); CK(dup(&d_idx, A[4])); CK(dup(&d_mu, A[5])); CK(dup(&d_rs, A[6]));
        CK(dup(&d_cost, A[7])); CK(dup(&d_shift, A[8]));
        CK(dout(&d_S, (size_t)(B * cs * cs))); CK(dout(&d_muo, (size_t)(B * cs))); CK(dout(&d_u, (size_t)(B * cs), &A[9]));
        CK(dfill(&d_part, wcov_mfma_workspace_doubles((int)B, (int)cs, (int)ksplit), 0xFF));             // NaN
        std::vector<unsigned long long> cmin(B, ~0ull);
        if (A[7].count) {
            const double* c = (const double*)A[7].bytes.data();
            for (long long b = 0; b < B; ++b) for (long long k = 0; k < K; ++k) { const unsigned long long key = cost_key(c[b * K + k]); if (key < cmin[b]) cmin[b] = key; }
        }
        CK(hipMalloc(&d_cmin, B * 8)); CK(hipMemcpy(d_cmin, cmin.data(), B * 8, hipMemcpyHostToDevice));
        const WcovForm f = wcov_form((int)cs, (int)K, (int)m, (int)ksplit, sel_batch == 0 ? (int)B : (int)sel_batch, d_rs != nullptr, d_idx != nullptr, want_mu != 0, d_cost != nullptr);
        form = (long long)f.partial | (f.sq ? 1 << 8 : 0) | (f.aug ? 1 << 9 : 0) | (f.from_cost ? 1 << 10 : 0);
        if (!f.aug && !d_mu) BAD("this shape has no ones row: the case must give mu");
        launch_wcov_mfma(d_X, d_w, d_idx, (int)m, d_mu, d_S, d_part, (int)B, (int)cs, (int)K, (int)ksplit, (int)sel_batch, dp[0], dp[1], d_active, s, d_rs,
                         want_mu ? d_muo : nullptr, (want_mu && A[9].count) ? d_u : nullptr, d_wsum, d_cost, d_cost ? d_cmin : nullptr, dp[2], d_shift);
        outs = {{0, (size_t)(B * cs * cs), d_S}, {0, (size_t)(B * cs), d_muo}, {0, (size_t)(B * cs), d_u}, {2, (size_t)B, d_cmin, false},
                {0, wcov_mfma_workspace_doubles((int)B, (int)cs, (int)ksplit), d_part, false}};
    } else if (op == OP_SHRINK) {
        const long long cs = ip[0], m = ip[1], kind = ip[2];
        if (cs < 1 || cs > 800 || m < 2 || kind < 0 || kind > 3) BAD("case out of range");
        if (!need(1, 0, B * cs * cs, false) || !need(2, 0, B * cs * cs, kind < 2)) BAD("wrong array sizes");
        double *d_S, *d_Q, *d_rs;
        CK(dout(&d_S, (size_t)(B * cs * cs), &A[1])); CK(dup(&d_Q, A[2])); CK(dout(&d_rs, (size_t)(B * cs)));
        if (kind < 2) launch_common_shrink(d_S, (int)B, (int)cs, (int)m, kind == 1, dp[0], d_active, s);
        else {
            if (kind == 2) launch_inv_sd(d_S, d_rs, (int)B, (int)cs, d_active, s);
            else launch_fill_f64(d_rs, 1.0, (size_t)(B * cs), s);
            launch_ss_shrink(d_S, d_Q, d_rs, (int)B, (int)cs, (int)m, dp[0], d_active, s);
        }
        outs = {{0, (size_t)(B * cs * cs), d_S}, {0, (size_t)(B * cs), d_rs}};
    } else if (op == OP_CE_SMALL || op == OP_CE_GENERAL) {
        const long long cs = ip[0], K = ip[1], m = ip[2], est = ip[3], ksplit = ip[4];
        if (cs < 1 || cs > wcov_max_cs() || K < 1 || K > 8192 || m < 2 || m > K || est < 0 || est > 4 || ksplit < 1 || ksplit > 64) BAD("case out of range");
        if (!need(1, 0, B * cs * K, false) || !need(2, 1, B * K, false) || !need(3, 0, B * cs, false)) BAD("wrong array sizes");
        { const int32_t* ix = (const int32_t*)A[2].bytes.data(); for (long long e = 0; e < B * K; ++e) if (ix[e] < 0 || ix[e] >= K) BAD("invalid column index"); }
        double *d_E, *d_mu, *d_S, *d_U; int32_t* d_order;
        CK(dup(&d_E, A[1])); CK(dup(&d_order, A[2])); CK(dout(&d_mu, (size_t)(B * cs))); CK(dout(&d_S, (size_t)(B * cs * cs))); CK(dout(&d_U, (size_t)(B * cs), &A[3]));
        if (op == OP_CE_SMALL) {
            if (!ce_cov_small_ok((int)cs, (int)m, (int)est)) BAD("the CE kernel does not take this case");
            form = 100;
            launch_ce_cov_small(d_E, d_order, d_mu, d_S, d_U, (int)B, (int)cs, (int)K, (int)m, (int)est, dp[0], d_active, s, nullptr);
        } else {
            double *d_tmpS, *d_rs, *d_part;
            CK(dfill(&d_tmpS, (size_t)(B * cs * cs), kPoison)); CK(dfill(&d_rs, (size_t)(B * cs), kPoison));
            CK(dfill(&d_part, wcov_mfma_workspace_doubles((int)B, (int)cs, (int)ksplit), 0xFF));
            form = (long long)wcov_form((int)cs, (int)K, (int)m, (int)ksplit, (int)B, false, true, false, false).partial;
            launch_ce_cov_general(d_E, d_order, d_mu, d_S, d_tmpS, d_rs, d_part, (int)B, (int)cs, (int)K, (int)m, (int)ksplit, 0, (int)est, dp[0], d_active, s);
            launch_add_active(d_mu, d_U, (int)B, (int)cs, d_active, s);
        }
        outs = {{0, (size_t)(B * cs), d_mu}, {0, (size_t)(B * cs * cs), d_S}, {0, (size_t)(B * cs), d_U}};
    } else {
        const long long cs = ip[0], K = ip[1], m = ip[2], sub = ip[3], normalize = ip[4];
        if (cs < 1 || cs > 800 || K < 1 || K > 8192 || m < 1 || m > K || sub < 0 || sub > 3) BAD("case out of range");
        if (!need(1, 0, B * cs * K, false) || !need(2, 1, B * K, sub == 3) || !need(3, 0, B * K, sub != 3) || !need(4, 0, B * cs, true) || !need(5, 0, B * cs, true) ||
            (A[4].count != 0) != (A[5].count != 0)) BAD("wrong array sizes");
        if (A[2].count) { const int32_t* ix = (const int32_t*)A[2].bytes.data(); for (long long e = 0; e < B * K; ++e) if (ix[e] < 0 || ix[e] >= K) BAD("invalid column index"); }
        double *d_X, *d_w, *d_sa, *d_sb, *d_Xo, *d_shift, *d_mu; int32_t* d_idx;
        CK(dup(&d_X, A[1])); CK(dup(&d_idx, A[2])); CK(dup(&d_w, A[3])); CK(dup(&d_sa, A[4])); CK(dup(&d_sb, A[5]));
        CK(dout(&d_Xo, (size_t)(B * cs * K))); CK(dout(&d_shift, (size_t)(B * cs))); CK(dout(&d_mu, (size_t)(B * cs)));
        if (sub <= 1) launch_gather_cols(d_X, d_idx, d_Xo, (int)B, (int)cs, (int)K, d_active, s, sub ? d_shift : nullptr);
        else if (sub == 2) launch_gather_mean(d_X, d_idx, nullptr, d_mu, (int)B, (int)cs, (int)K, (int)m, 1, d_active, s);
        else launch_wmean(d_X, d_w, d_sa, d_sb, d_mu, (int)B, (int)cs, (int)K, (int)normalize, d_active, s);
        outs = {{0, (size_t)(B * cs * K), d_Xo}, {0, (size_t)(B * cs), d_shift}, {0, (size_t)(B * cs), d_mu}};
    }
    CK(hipGetLastError()); CK(hipStreamSynchronize(s));
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) BAD("cannot write the result file");
    const long long oh[4] = {magic_word("MFMRES01"), form, kGuard, (long long)outs.size()};
    if (const int rc = write_back(fo, oh, 4, outs)) return rc;
    if (fclose(fo) != 0) BAD("write failed");
    printf("op %d B %lld form %lld\n", op, B, form);
    return 0;
}
