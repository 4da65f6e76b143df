// kbench_dense.hip -- runs ONE op of the dense linear algebra (kernels_linalg.hip: the four Cholesky kernels behind launch_potrf, the two g-row
// launchers; kernels_invsqrt.hip: the triangular-inverse trace with the Lanczos preparation, the Lanczos / Jacobi inverse square root, the symmetric
// square root) on the inputs of a case file and writes the raw device outputs back to a file (dev / test tool, not shipped; kbench_linalg.hip stays the
// timing tool).  It holds no reference arithmetic: tests/test_gpu_dense_harness.py writes the case, reads the result and compares with NumPy longdouble.
// Only launchers declared in engine.h are called.
// build: tools/build_kbench.sh dense       run: tools/kbench_dense_bin <case file> <result file>
//
// case file (little endian; written by tests/helpers/dense_cases.py):
//   int64  hdr[6] = { magic 'DNSCASE1', op, B, n_ipar, n_dpar, n_arrays }
//   int64  ipar[n_ipar]; double dpar[n_dpar]
//   n_arrays x { int64 type (0 f64, 1 i32, 2 u64), int64 count; data }      in the fixed order of the op, count 0 = "not given" (nullptr)
// result file:
//   int64  hdr[4] = { magic 'DNSRES01', form, guard, n_arrays }; n_arrays x { int64 type, int64 count; data }     (count includes the guard entries)
//   form = potrf_form(...).kernel | G << 8 | (workgroups per matrix of the Lanczos launch) << 16          (ops that launch neither: 0)
// Every output buffer is filled with the byte 0xA5 first (in/out buffers: then the case's values) and carries `guard` extra entries, so the test sees
// what the launch left untouched; workspaces are filled with NaN.  array 0 is always active[B]; `use_active` 0 passes nullptr.
//
// op 0 POTRF    ipar { n, Astride (0 or n n), use_active, use_coop, want_panel }       arrays: active, A, scale (given: per slot), status
//                                                                                       -> L, panel, status, active
// op 1 SOLVE    ipar { n, Lstride (0 or n n), use_active }  dpar { gamma }             arrays: active, L, U, gamma_b (given: per slot), inv_scale2 -> g
// op 2 GVEC     ipar { n }  dpar { gamma }                                             arrays: active (unused), Sinv, U, gamma_b           -> g
// op 3 TRTRI    ipar { n, Lstride, use_active, hiprio, launches (1 or 2) }             arrays: active, L, A (given: with prep), scale
//                                                                                       -> part, prep, part2, prep2, sync2   (the second launch reuses sync2)
// op 4 INVSQRT  ipar { n, use_active, use_coop, regions (0: 1, 1: invsqrt_coop_groups), bstride, boff }
//               arrays: active, A, scale, bbuf [boff + (B - 1) bstride + n ...], status -> L, part, prep, y, fro, msteps, status, active
// op 5 SYM_SQRT ipar { n }  (B = 1)                                                    arrays: active (unused), A, status                  -> out, status
#include "../mpopis_amd/csrc/engine.h"
#include "kbench_dev.h"
#include <cstdlib>
#include <cmath>
using namespace mpopis;
enum { OP_POTRF = 0, OP_SOLVE = 1, OP_GVEC = 2, OP_TRTRI = 3, OP_INVSQRT = 4, OP_SYM_SQRT = 5 };

// the cooperative kernels' workspace, as the handle allocates it (zero-initialised once)
struct Coop {
    unsigned long long* flags = nullptr; unsigned long long epoch = 0; int* redo = nullptr;
    CoopCtx ctx;
    hipError_t init(size_t words, int B) {
        hipError_t e = dfill(&flags, words, 0);
        if (e == hipSuccess) e = dfill(&redo, (size_t)B + 1, 0);
        ctx.flags = flags; ctx.epoch = &epoch; ctx.redo = redo; ctx.timeouts = redo + B;
        return e;
    }
};

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi; Launch L;
    const char* err = open_case(argv[1], "DNSCASE1", nullptr, &fi);
    if (!err) err = read_launch(fi, CaseLimits{5, 1, 8, 16, 2, 1ll << 28, 1}, &L);
    if (!err) err = close_case(fi);
    if (err) BAD(err);
    const int op = L.op; const long long B = L.B, nD = L.nD;
    const std::vector<long long>& ip = L.ip; const std::vector<double>& dp = L.dp; const std::vector<Arr>& A = L.A;
    auto need = [&](int i, long long type, long long count, bool optional) { return L.need(i, type, count, optional); };
    if (!need(0, 1, B, false)) BAD("active[B] missing");
    const long long n = ip[0], nn = n * n;
    if (n < 1 || n > 512 || n > invsqrt_max_n()) BAD("case out of range");

    hipStream_t s; CK(hipStreamCreate(&s));
    long long form = 0;
    std::vector<Out> outs;
    if (op == OP_POTRF) {
        const long long As = ip[1], use_active = ip[2], use_coop = ip[3], want_panel = ip[4];
        if (As != 0 && As != nn) BAD("case out of range");
        if (!need(1, 0, (As ? B : 1) * nn, false) || !need(2, 0, B, true) || !need(3, 1, B, false)) BAD("wrong array sizes");
        const size_t pd = want_panel ? potrf_panel_doubles((int)n) : 0;
        double *d_A, *d_sc, *d_L, *d_P; int *d_st, *d_act;
        CK(dup(&d_A, A[1])); CK(dup(&d_sc, A[2]));
        CK(dout(&d_L, (size_t)(B * nn))); CK(dout(&d_P, (size_t)B * pd)); CK(dout(&d_st, (size_t)B, &A[3])); CK(dout(&d_act, (size_t)B, &A[0]));
        Coop pc;
        if (use_coop) CK(pc.init(potrf_coop_flag_words((int)B, (int)n), (int)B));
        const PotrfForm f = potrf_form((int)B, (int)n, pc.ctx.usable(), pc.ctx.share);
        form = (long long)f.kernel | ((long long)f.G << 8);
        launch_potrf(d_A, (size_t)As, d_L, (int)B, (int)n, d_sc, d_st, use_active ? d_act : nullptr, s, pc.ctx, pd ? d_P : nullptr, pd);
        outs = {{0, (size_t)(B * nn), d_L}, {0, (size_t)B * pd, d_P}, {1, (size_t)B, d_st}, {1, (size_t)B, d_act}};
    } else if (op == OP_SOLVE) {
        const long long Ls = ip[1], use_active = ip[2];
        if (Ls != 0 && Ls != nn) BAD("case out of range");
        if (!need(1, 0, (Ls ? B : 1) * nn, false) || !need(2, 0, B * n, false) || !need(3, 0, B, true) || !need(4, 0, B, true)) BAD("wrong array sizes");
        double *d_L, *d_U, *d_gam, *d_isc, *d_g; int* d_act;
        CK(dup(&d_L, A[1])); CK(dup(&d_U, A[2])); CK(dup(&d_gam, A[3])); CK(dup(&d_isc, A[4])); CK(dup(&d_act, A[0]));
        CK(dout(&d_g, (size_t)(B * n)));
        launch_chol_solve_gvec(d_L, (size_t)Ls, d_U, SlotVal{dp[0], d_gam}, d_g, (int)B, (int)n, use_active ? d_act : nullptr, s, d_isc);
        outs = {{0, (size_t)(B * n), d_g}};
    } else if (op == OP_GVEC) {
        if (!need(1, 0, nn, false) || !need(2, 0, B * n, false) || !need(3, 0, B, true)) BAD("wrong array sizes");
        double *d_S, *d_U, *d_gam, *d_g;
        CK(dup(&d_S, A[1])); CK(dup(&d_U, A[2])); CK(dup(&d_gam, A[3])); CK(dout(&d_g, (size_t)(B * n)));
        launch_gvec_from_inv(d_S, d_U, SlotVal{dp[0], d_gam}, d_g, (int)B, (int)n, s);
        outs = {{0, (size_t)(B * n), d_g}};
    } else if (op == OP_TRTRI) {
        const long long Ls = ip[1], use_active = ip[2], hiprio = ip[3], launches = ip[4], nb = (n + 15) / 16;
        if ((Ls != 0 && Ls != nn) || launches < 1 || launches > 2) BAD("case out of range");
        if (!need(1, 0, (Ls ? B : 1) * nn, false) || !need(2, 0, B * nn, true) || !need(3, 0, B, true) || (A[3].count && !A[2].count)) BAD("wrong array sizes");
        const bool with_prep = A[2].count != 0;
        const size_t np = with_prep ? lanczos_prep_doubles((int)B) : 0;
        double *d_L, *d_A, *d_sc, *d_dinv, *d_part[2], *d_prep[2]; int* d_act; unsigned long long* d_sync;
        CK(dup(&d_L, A[1])); CK(dup(&d_A, A[2], kInvsqrtPadDoubles)); CK(dup(&d_sc, A[3])); CK(dup(&d_act, A[0]));
        CK(dfill(&d_dinv, trtri_dinv_doubles((int)B, (int)n), 0xFF));
        CK(hipMalloc(&d_sync, (size_t)(2 * B + kGuard) * 8)); CK(hipMemset(d_sync, kPoison, (size_t)(2 * B + kGuard) * 8)); CK(hipMemset(d_sync, 0, (size_t)(2 * B) * 8));
        for (int l = 0; l < 2; ++l) { CK(dout(&d_part[l], (size_t)(B * nb))); CK(dout(&d_prep[l], np)); }
        for (int l = 0; l < launches; ++l)
            launch_trtri_fro(d_L, (size_t)Ls, d_part[l], (int)B, (int)n, use_active ? d_act : nullptr, s, d_dinv, hiprio != 0, d_A, d_sc,
                             with_prep ? d_prep[l] : nullptr, with_prep ? d_sync : nullptr);
        outs = {{0, (size_t)(B * nb), d_part[0]}, {0, np, d_prep[0]}, {0, (size_t)(B * nb), d_part[1]}, {0, np, d_prep[1]}, {2, (size_t)(2 * B), d_sync}};
    } else if (op == OP_INVSQRT) {
        const long long use_active = ip[1], use_coop = ip[2], regions_sel = ip[3], bstride = ip[4], boff = ip[5], nb = (n + 15) / 16;
        if (bstride < n || bstride > 4 * n || boff < 0 || boff + n > bstride) BAD("case out of range");
        if (!need(1, 0, B * nn, false) || !need(2, 0, B, true) || !need(3, 0, B * bstride, false) || !need(4, 1, B, false)) BAD("wrong array sizes");
        const int regions = regions_sel ? invsqrt_coop_groups((int)B, (int)n) : 1;
        double *d_A, *d_sc, *d_b, *d_L, *d_part, *d_prep, *d_dinv, *d_V, *d_y, *d_fro; int *d_st, *d_act, *d_m; unsigned long long* d_sync;
        CK(dup(&d_A, A[1], kInvsqrtPadDoubles)); CK(dup(&d_sc, A[2])); CK(dup(&d_b, A[3]));
        CK(dout(&d_L, (size_t)(B * nn))); CK(dout(&d_part, (size_t)(B * nb))); CK(dout(&d_prep, lanczos_prep_doubles((int)B)));
        CK(dout(&d_y, (size_t)(B * n))); CK(dout(&d_fro, (size_t)B)); CK(dout(&d_m, (size_t)B)); CK(dout(&d_st, (size_t)B, &A[4])); CK(dout(&d_act, (size_t)B, &A[0]));
        CK(dfill(&d_dinv, trtri_dinv_doubles((int)B, (int)n), 0xFF)); CK(dfill(&d_V, invsqrt_workspace_doubles((int)B, (int)n, regions), 0xFF));
        CK(dfill(&d_sync, (size_t)(2 * B), 0));
        Coop pc, lc;
        if (use_coop) { CK(pc.init(potrf_coop_flag_words((int)B, (int)n), (int)B)); CK(lc.init(invsqrt_coop_words((int)B, (int)n), (int)B)); }
        const PotrfForm f = potrf_form((int)B, (int)n, pc.ctx.usable(), pc.ctx.share);
        const int lanG = lc.ctx.usable() ? std::min(invsqrt_coop_groups((int)B, (int)n, lc.ctx.share), regions) : 1;
        form = (long long)f.kernel | ((long long)f.G << 8) | ((long long)lanG << 16);
        int* act = use_active ? d_act : nullptr;
        launch_potrf(d_A, (size_t)nn, d_L, (int)B, (int)n, d_sc, d_st, act, s, pc.ctx);
        launch_trtri_fro(d_L, (size_t)nn, d_part, (int)B, (int)n, act, s, d_dinv, true, d_A, d_sc, d_prep, d_sync);
        launch_lanczos_invsqrt(d_A, d_prep, d_b + boff, (size_t)bstride, d_V, d_y, d_fro, d_m, (int)B, (int)n, d_st, act, s, regions, lc.ctx);
        outs = {{0, (size_t)(B * nn), d_L}, {0, (size_t)(B * nb), d_part}, {0, lanczos_prep_doubles((int)B), d_prep}, {0, (size_t)(B * n), d_y}, {0, (size_t)B, d_fro},
                {1, (size_t)B, d_m}, {1, (size_t)B, d_st}, {1, (size_t)B, d_act}};
    } else {
        if (B != 1 || !need(1, 0, nn, false) || !need(2, 1, 1, false)) BAD("wrong array sizes");
        double *d_A, *d_M, *d_V, *d_out; int* d_st;
        CK(dup(&d_A, A[1])); CK(dfill(&d_M, (size_t)nn, 0xFF)); CK(dfill(&d_V, (size_t)nn, 0xFF)); CK(dout(&d_out, (size_t)nn)); CK(dout(&d_st, (size_t)1, &A[2]));
        launch_sym_sqrt(d_A, d_M, d_V, d_out, d_st, (int)n, s);
        outs = {{0, (size_t)nn, d_out}, {1, (size_t)1, d_st}};
    }
    CK(hipGetLastError()); CK(hipStreamSynchronize(s));
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) BAD("cannot write the result file");
    const long long oh[4] = {magic_word("DNSRES01"), form, kGuard, (long long)outs.size()};
    if (const int rc = write_back(fo, oh, 4, outs)) return rc;
    if (fclose(fo) != 0) BAD("write failed");
    printf("op %d B %lld n %lld form %lld\n", op, B, n, form);
    return 0;
}
