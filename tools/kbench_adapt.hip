// kbench_adapt.hip -- runs ONE op of the two adaptation steps (kernels_nes.hip: early break, signed scatter, Σ^-1 from the factor, the whole
// update; kernels_cma.hip: begin, paths, Σ update) on the inputs of a case file and writes the raw device outputs back to a file (dev / test
// tool, not shipped).  It holds no reference arithmetic: tests/test_gpu_adapt_harness.py writes the case, reads the result and compares with
// NumPy longdouble.  Only launchers declared in engine.h are called (k_nes_gemm is reached through POTRI and the four products of UPDATE).
// build: tools/build_kbench.sh adapt       run: tools/kbench_adapt_bin <case file> <result file>
//
// case file (little endian; written by tests/helpers/adapt_cases.py):
//   int64  hdr[6] = { magic 'ADPCASE1', op, B, n_ipar, n_dpar, n_arrays }
//   int64  ipar[n_ipar]; double dpar[n_dpar]
//   n_arrays x { int64 type (0 f64, 1 i32), int64 count; data }      in the fixed order of the op, count 0 = "not given" (nullptr)
// result file:
//   int64  hdr[4] = { magic 'ADPRES01', 0, guard, n_arrays }; n_arrays x { int64 type, int64 count; data }     (count includes the guard entries)
// Every output buffer is filled with the byte 0xA5 first (in/out buffers: then the case's values) and carries `guard` extra entries, so the
// test sees what the launch left untouched; the K-split partial workspace of the scatter is filled with NaN, so a partial the finish kernel
// reads but no workgroup wrote shows in M, g or C.  array 0 is always active[B]; `use_active` 0 passes nullptr where the launcher allows it.
//
// op 0 BREAK      ipar { K }                                       arrays: active, cost, status                   -> active, status
// op 1 SCATTER    ipar { cs, K, ksplit }                           arrays: active, E, cost                        -> M, g, Csum
// op 2 POTRI      ipar { n, Lstride (0 or n n), use_active }       arrays: active, L                              -> X, S
// op 3 UPDATE     ipar { cs, K, ksplit, Sstride, Astride }  dpar { a_scale, u_scale }
//                 arrays: active, E, cost, S, Ain, U, a_scale_b (given: per slot), u_scale_b                     -> T, M (= G), g, Csum, Aout, Sig, U
// op 4 CMA_BEGIN  ipar { cs }  dpar { sigma0 }                     arrays: active (unused), sigma0_b (given: per slot) -> scal, vec, sig2
// op 5 CMA_PATHS  ipar { cs, K, n_iter, m_elite, use_active }  dpar consts7
//                 arrays: active, Cdw, fro, E, order, ws, Ucur, scal, vec                                         -> Ucur, scal, vec, sig2
// op 6 CMA_SIGMA  ipar { cs, m_elite, use_active }  dpar consts7   arrays: active, Sig, scal, vec                 -> Sig
#include "../mpopis_amd/csrc/engine.h"
#include "kbench_dev.h"
#include <cstdlib>
#include <cmath>
using namespace mpopis;
enum { OP_BREAK = 0, OP_SCATTER = 1, OP_POTRI = 2, OP_UPDATE = 3, OP_CMA_BEGIN = 4, OP_CMA_PATHS = 5, OP_CMA_SIGMA = 6 };

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi; Launch L;
    const char* err = open_case(argv[1], "ADPCASE1", nullptr, &fi);
    if (!err) err = read_launch(fi, CaseLimits{6, 1, 8, 16, 1, 1ll << 28, 0}, &L);
    if (!err) err = close_case(fi);
    if (err) BAD(err);
    const int op = L.op; const long long B = L.B, nD = L.nD;
    const std::vector<long long>& ip = L.ip; const std::vector<double>& dp = L.dp; const std::vector<Arr>& A = L.A;
    auto need = [&](int i, long long type, long long count, bool optional) { return L.need(i, type, count, optional); };
    if (!need(0, 1, B, false)) BAD("active[B] missing");

    hipStream_t s; CK(hipStreamCreate(&s));
    int* d_active; CK(dup(&d_active, A[0]));
    std::vector<Out> outs;
    if (op == OP_BREAK) {
        const long long K = ip[0];
        if (K < 1 || K > 8192) BAD("case out of range");
        if (!need(1, 0, B * K, false) || !need(2, 1, B, false)) BAD("wrong array sizes");
        double* d_cost; int *d_act, *d_status;
        CK(dup(&d_cost, A[1])); CK(dout(&d_act, (size_t)B, &A[0])); CK(dout(&d_status, (size_t)B, &A[2]));
        launch_nes_break(d_cost, (int)B, (int)K, d_act, d_status, s);
        outs = {{1, (size_t)B, d_act}, {1, (size_t)B, d_status}};
    } else if (op == OP_SCATTER || op == OP_UPDATE) {
        const long long cs = ip[0], K = ip[1], ksplit = ip[2], nn = cs * cs;
        if (cs < 1 || cs > 512 || K < 1 || K > 8192 || ksplit < 1 || ksplit > 64) BAD("case out of range");
        if (!need(1, 0, B * cs * K, false) || !need(2, 0, B * K, false)) BAD("wrong array sizes");
        double *d_E, *d_cost, *d_part, *d_M, *d_g, *d_C;
        CK(dup(&d_E, A[1])); CK(dup(&d_cost, A[2]));
        CK(dfill(&d_part, nes_scatter_workspace_doubles((int)B, (int)cs, (int)ksplit), 0xFF));             // NaN
        CK(dout(&d_M, (size_t)(B * nn))); CK(dout(&d_g, (size_t)(B * cs))); CK(dout(&d_C, (size_t)B));
        if (op == OP_SCATTER) {
            launch_nes_scatter(d_E, d_cost, d_part, d_M, d_g, d_C, (int)B, (int)cs, (int)K, (int)ksplit, d_active, s);
            outs = {{0, (size_t)(B * nn), d_M}, {0, (size_t)(B * cs), d_g}, {0, (size_t)B, d_C}};
        } else {
            const long long Ss = ip[3], As = ip[4];
            if ((Ss != 0 && Ss != nn) || (As != 0 && As != nn)) BAD("case out of range");
            if (!need(3, 0, (Ss ? B : 1) * nn, false) || !need(4, 0, (As ? B : 1) * nn, false) || !need(5, 0, B * cs, false) || !need(6, 0, B, true) ||
                !need(7, 0, B, true)) BAD("wrong array sizes");
            double *d_S, *d_Ain, *d_as, *d_us, *d_T, *d_Aout, *d_Sig, *d_U;
            CK(dup(&d_S, A[3])); CK(dup(&d_Ain, A[4])); CK(dup(&d_as, A[6])); CK(dup(&d_us, A[7]));
            CK(dout(&d_T, (size_t)(B * nn))); CK(dout(&d_Aout, (size_t)(B * nn))); CK(dout(&d_Sig, (size_t)(B * nn))); CK(dout(&d_U, (size_t)(B * cs), &A[5]));
            launch_nes_update(d_E, d_cost, d_part, (int)ksplit, d_S, (size_t)Ss, d_M, d_T, d_g, d_C, d_Ain, (size_t)As, d_Aout, d_Sig, d_U, (int)B, (int)cs, (int)K,
                              SlotVal{dp[0], d_as}, SlotVal{dp[1], d_us}, d_active, s);
            outs = {{0, (size_t)(B * nn), d_T}, {0, (size_t)(B * nn), d_M}, {0, (size_t)(B * cs), d_g}, {0, (size_t)B, d_C}, {0, (size_t)(B * nn), d_Aout},
                    {0, (size_t)(B * nn), d_Sig}, {0, (size_t)(B * cs), d_U}};
        }
    } else if (op == OP_POTRI) {
        const long long n = ip[0], Ls = ip[1], use_active = ip[2];
        if (n < 1 || n > 800 || (Ls != 0 && Ls != n * n)) BAD("case out of range");
        if (!need(1, 0, (Ls ? B : 1) * n * n, false)) BAD("wrong array sizes");
        double *d_L, *d_X, *d_S;
        CK(dup(&d_L, A[1])); CK(dout(&d_X, (size_t)(B * n * n))); CK(dout(&d_S, (size_t)(B * n * n)));
        launch_nes_potri(d_L, (size_t)Ls, d_X, d_S, (int)B, (int)n, use_active ? d_active : nullptr, s);
        outs = {{0, (size_t)(B * n * n), d_X}, {0, (size_t)(B * n * n), d_S}};
    } else if (op == OP_CMA_BEGIN) {
        const long long cs = ip[0];
        if (cs < 1 || cs > 800) BAD("case out of range");
        if (!need(1, 0, B, true)) BAD("wrong array sizes");
        double *d_s0, *d_scal, *d_vec, *d_sig2;
        CK(dup(&d_s0, A[1])); CK(dout(&d_scal, (size_t)(B * 8))); CK(dout(&d_vec, (size_t)(B * 3 * cs))); CK(dout(&d_sig2, (size_t)B));
        launch_cma_begin(d_scal, d_vec, d_sig2, SlotVal{dp[0], d_s0}, (int)cs, (int)B, s);
        outs = {{0, (size_t)(B * 8), d_scal}, {0, (size_t)(B * 3 * cs), d_vec}, {0, (size_t)B, d_sig2}};
    } else if (op == OP_CMA_PATHS) {
        const long long cs = ip[0], K = ip[1], n_iter = ip[2], m_elite = ip[3], use_active = ip[4];
        if (cs < 1 || cs > 800 || K < 1 || K > 8192 || n_iter < 1 || n_iter > 64 || m_elite < 1 || m_elite > K || cs * m_elite < K || nD != 7) BAD("case out of range");
        if (!need(1, 0, B * cs, false) || !need(2, 0, B, false) || !need(3, 0, B * cs * K, false) || !need(4, 1, B * K, false) || !need(5, 0, K, false) ||
            !need(6, 0, B * cs, false) || !need(7, 0, B * 8, false) || !need(8, 0, B * 3 * cs, false)) BAD("wrong array sizes");
        { const int32_t* ix = (const int32_t*)A[4].bytes.data(); for (long long e = 0; e < B * K; ++e) if (ix[e] < 0 || ix[e] >= K) BAD("invalid column index"); }
        double *d_Cdw, *d_fro, *d_E, *d_ws, *d_U, *d_scal, *d_vec, *d_sig2; int32_t* d_order;
        CK(dup(&d_Cdw, A[1])); CK(dup(&d_fro, A[2])); CK(dup(&d_E, A[3])); CK(dup(&d_order, A[4])); CK(dup(&d_ws, A[5]));
        CK(dout(&d_U, (size_t)(B * cs), &A[6])); CK(dout(&d_scal, (size_t)(B * 8), &A[7])); CK(dout(&d_vec, (size_t)(B * 3 * cs), &A[8])); CK(dout(&d_sig2, (size_t)B));
        launch_cma_paths(d_Cdw, d_fro, d_E, d_order, d_ws, d_U, d_scal, d_vec, d_sig2, (int)B, (int)cs, (int)K, (int)n_iter, dp.data(), (int)m_elite,
                         use_active ? d_active : nullptr, s);
        outs = {{0, (size_t)(B * cs), d_U}, {0, (size_t)(B * 8), d_scal}, {0, (size_t)(B * 3 * cs), d_vec}, {0, (size_t)B, d_sig2}};
    } else {
        const long long cs = ip[0], m_elite = ip[1], use_active = ip[2];
        if (cs < 1 || cs > 800 || nD != 7) BAD("case out of range");
        if (!need(1, 0, B * cs * cs, false) || !need(2, 0, B * 8, false) || !need(3, 0, B * 3 * cs, false)) BAD("wrong array sizes");
        double *d_Sig, *d_scal, *d_vec;
        CK(dout(&d_Sig, (size_t)(B * cs * cs), &A[1])); CK(dup(&d_scal, A[2])); CK(dup(&d_vec, A[3]));
        launch_cma_sigma_update(d_Sig, d_scal, d_vec, (int)B, (int)cs, dp.data(), (int)m_elite, use_active ? d_active : nullptr, s);
        outs = {{0, (size_t)(B * cs * cs), d_Sig}};
    }
    CK(hipGetLastError()); CK(hipStreamSynchronize(s));
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) BAD("cannot write the result file");
    const long long oh[4] = {magic_word("ADPRES01"), 0, kGuard, (long long)outs.size()};
    if (const int rc = write_back(fo, oh, 4, outs)) return rc;
    if (fclose(fo) != 0) BAD("write failed");
    printf("op %d B %lld\n", op, B);
    return 0;
}
