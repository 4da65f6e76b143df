// kbench_sample.hip -- runs ONE launch of a sampling kernel (table fill, the three k_sample_normal* forms, the resampling draws), of the step's read-out
// tail (k_finalize, the two transposes) or of a probe kernel over philox.h (the Philox rounds, box_muller_u32 with the table in LDS or in global
// memory, philox_normal_quad / philox_normal_pair with a 64-bit counter) on the inputs of a case file and writes the raw device outputs back to a
// file (dev / test tool, not shipped).  It holds no reference arithmetic: tests/test_gpu_sample_harness.py writes the case, reads the result and
// compares with the oracle and NumPy.  It calls only launchers declared in engine.h, plus the probe kernels below.
// build: tools/build_kbench.sh sample       run: tools/kbench_sample_bin <case file> <result file>
//
// case file (little endian; layout shared with tests/helpers/sample_cases.py):
//   int64  hdr[16] = { magic 'SMPCASE1', op, B, cs, K, as, T, mppi_order, flags, n, slo, shi, src_stride, src_off, 0, 0 }
//   op 0 TAB:       nothing
//   op 1 WORDS:     uint32 in[6 n]  = n x { c0, c1, c2, c3, k0, k1 }
//   op 2 BOXMULLER: uint32 w[2 n]   = n x { wr, wa }                      flags bit 0: read the table from global memory instead of LDS
//   op 3 NORMALQ:   uint64 in[3 n]  = n x { seed, slo | shi << 32, q }
//   op 4 NORMALS:   uint64 seeds[B]; int32 active[B]; double dscale[B cs] (flags bit 0)       flags bit 1: active = nullptr
//   op 5 DRAWS:     uint64 seeds[B]; int32 active[B]                                          flags bit 1: active = nullptr
//   op 6 FINALIZE:  double lo[16], hi[16], U[B cs], wn[B cs]
//   op 7 T_IN:      double src[n]; the launch reads from src + src_off with src_stride (0: the launcher's default cs K)
//   op 8 T_OUT:     double src[B cs K]; double A[B cs], Bv[B cs] (flags bit 0: the shift pair)
// result file:
//   int64  hdr[4]  = { magic 'SMPRES01', form, guard, 0 }       form: what sample_normal_form returned (op 4), else -1
//   op 0: double tab[kRngTabDoubles + guard]           op 1: uint32 out[4 n + guard]          op 2: double z[2 n + guard]
//   op 3: double z[8 n + guard] = n x { quad(q)[4], pair(2q)[2], pair(2q+1)[2] }              op 4: double Z[B cs K + guard]
//   op 5: double du[B K + guard]; int32 di[B K + guard]
//   op 6: double U[B cs + guard], control[B as + guard], wn[B cs + guard]
//   op 7 / 8: double dst[B cs K + guard]
// Every output buffer is filled with the byte 0xA5 first (and carries `guard` extra entries), so the test sees what the launch left untouched.
#include "../mpopis_amd/csrc/engine.h"
#include "../mpopis_amd/csrc/philox.h"
#include "kbench_dev.h"
#include <cstdlib>
using namespace mpopis;
static const long long kMagicIn = 0x3145534143504d53ll, kMagicOut = 0x3130534552504d53ll;       // "SMPCASE1", "SMPRES01"
enum { OP_TAB = 0, OP_WORDS = 1, OP_BOXMULLER = 2, OP_NORMALQ = 3, OP_NORMALS = 4, OP_DRAWS = 5, OP_FINALIZE = 6, OP_T_IN = 7, OP_T_OUT = 8 };

// ---- probe kernels over philox.h ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_probe_words(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t r[4];
    philox4x32_10(in[6 * i], in[6 * i + 1], in[6 * i + 2], in[6 * i + 3], in[6 * i + 4], in[6 * i + 5], r);
    for (int e = 0; e < 4; ++e) out[4 * i + e] = r[e];
}
// the table staged into LDS as the k_sample_normal* kernels stage it, or read where launch_rng_tab_init left it (k_harness_update's way)
__global__ void __launch_bounds__(256) k_probe_box_muller(const uint32_t* __restrict__ w, double* __restrict__ z, long long n,
                                                          const double* __restrict__ gtab, int from_global) {
    __shared__ double sh_tab[kRngTabDoubles];
    stage_rng_tab(sh_tab, gtab, threadIdx.x, 256);
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double z0, z1;
    if (from_global) box_muller_u32(w[2 * i], w[2 * i + 1], gtab, &z0, &z1);
    else box_muller_u32(w[2 * i], w[2 * i + 1], sh_tab, &z0, &z1);
    z[2 * i] = z0; z[2 * i + 1] = z1;
}
__global__ void __launch_bounds__(256) k_probe_normalq(const uint64_t* __restrict__ in, double* __restrict__ z, long long n, const double* __restrict__ gtab) {
    __shared__ double sh_tab[kRngTabDoubles];
    stage_rng_tab(sh_tab, gtab, threadIdx.x, 256);
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t seed = in[3 * i], st = in[3 * i + 1], q = in[3 * i + 2];
    const uint32_t slo = (uint32_t)st, shi = (uint32_t)(st >> 32);
    double o[8];
    philox_normal_quad(seed, slo, shi, q, sh_tab, o);
    philox_normal_pair(seed, slo, shi, 2 * q, sh_tab, &o[4], &o[5]);
    philox_normal_pair(seed, slo, shi, 2 * q + 1, sh_tab, &o[6], &o[7]);
    for (int e = 0; e < 8; ++e) z[8 * i + e] = o[e];
}


int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hdr;
    if (!rd(fi, hdr, 16) || hdr[0] != kMagicIn) { printf("bad case header\n"); return 2; }
    const int op = (int)hdr[1];
    const long long B = hdr[2], cs = hdr[3], K = hdr[4], as = hdr[5], T = hdr[6], mppi_order = hdr[7], flags = hdr[8], n = hdr[9], src_stride = hdr[12], src_off = hdr[13];
    const uint32_t slo = (uint32_t)hdr[10], shi = (uint32_t)hdr[11];
    // every launch below indexes with these alone: B slots of cs rows of K samples, cs = as T wherever a kernel splits a row index
    if (op < 0 || op > OP_T_OUT || B < 1 || B > 64 || cs < 1 || cs > 4096 || K < 1 || K > (1 << 20) || as < 1 || as > kMaxAs || T < 1 || n < 0 || n > (1 << 22) ||
        B * cs * K > (1ll << 24) || hdr[10] < 0 || hdr[10] > 0xffffffffll || hdr[11] < 0 || hdr[11] > 0xffffffffll || (mppi_order != 0 && mppi_order != 1)) {
        printf("case out of range\n"); return 2;
    }
    if ((op == OP_FINALIZE || (op == OP_NORMALS && mppi_order)) && cs != as * T) { printf("cs != as T\n"); return 2; }
    const size_t BC = (size_t)B * cs, BCK = BC * K, BK = (size_t)B * K;
    const bool flag0 = flags & 1, no_active = flags & 2;
    std::vector<uint32_t> u32; std::vector<uint64_t> u64; std::vector<int> active; std::vector<double> f0, f1, f2, f3;
    bool ok = true;
    size_t stride = 0;
    if (op == OP_WORDS) ok = rd(fi, u32, (size_t)6 * n);
    else if (op == OP_BOXMULLER) ok = rd(fi, u32, (size_t)2 * n);
    else if (op == OP_NORMALQ) ok = rd(fi, u64, (size_t)3 * n);
    else if (op == OP_NORMALS) ok = rd(fi, u64, B) && rd(fi, active, B) && (!flag0 || rd(fi, f0, BC));
    else if (op == OP_DRAWS) ok = rd(fi, u64, B) && rd(fi, active, B);
    else if (op == OP_FINALIZE) ok = rd(fi, f0, kMaxAs) && rd(fi, f1, kMaxAs) && rd(fi, f2, BC) && rd(fi, f3, BC);
    else if (op == OP_T_IN) {
        stride = src_stride ? (size_t)src_stride : (size_t)cs * K;
        if (src_stride < 0 || src_off < 0 || (src_stride && src_stride < cs * K) || (size_t)src_off + (size_t)(B - 1) * stride + (size_t)cs * K > (size_t)n) { printf("bad stride\n"); return 2; }
        ok = rd(fi, f0, (size_t)n);
    } else if (op == OP_T_OUT) ok = rd(fi, f0, BCK) && (!flag0 || (rd(fi, f1, BC) && rd(fi, f2, BC)));
    if (!ok || fgetc(fi) != EOF) { printf("case file has the wrong length\n"); return 2; }
    fclose(fi);
    if ((op == OP_WORDS || op == OP_BOXMULLER || op == OP_NORMALQ) && n < 1) { printf("empty case\n"); return 2; }

    hipStream_t s; CK(hipStreamCreate(&s));
    long long form = -1;
    std::vector<double> of0, of1, of2; std::vector<uint32_t> ou; std::vector<int32_t> oi;
    double* d_tab = nullptr;
    if (op == OP_TAB) CK(dpoison(&d_tab, (size_t)kRngTabDoubles + kGuard));
    else if (op >= OP_BOXMULLER && op <= OP_NORMALS) { CK(dpoison(&d_tab, (size_t)kRngTabDoubles)); launch_rng_tab_init(d_tab, s); CK(hipGetLastError()); CK(hipStreamSynchronize(s)); }
    const unsigned nblk = (unsigned)((n + 255) / 256);
    if (op == OP_TAB) {
        launch_rng_tab_init(d_tab, s);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_tab, (size_t)kRngTabDoubles + kGuard));
    } else if (op == OP_WORDS) {
        uint32_t *d_in, *d_out; CK(dupload(&d_in, u32)); CK(dpoison(&d_out, (size_t)4 * n + kGuard));
        hipLaunchKernelGGL(k_probe_words, dim3(nblk), dim3(256), 0, s, d_in, d_out, n);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(ou, d_out, (size_t)4 * n + kGuard));
    } else if (op == OP_BOXMULLER) {
        uint32_t* d_in; double* d_z; CK(dupload(&d_in, u32)); CK(dpoison(&d_z, (size_t)2 * n + kGuard));
        hipLaunchKernelGGL(k_probe_box_muller, dim3(nblk), dim3(256), 0, s, d_in, d_z, n, d_tab, flag0 ? 1 : 0);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_z, (size_t)2 * n + kGuard));
    } else if (op == OP_NORMALQ) {
        uint64_t* d_in; double* d_z; CK(dupload(&d_in, u64)); CK(dpoison(&d_z, (size_t)8 * n + kGuard));
        hipLaunchKernelGGL(k_probe_normalq, dim3(nblk), dim3(256), 0, s, d_in, d_z, n, d_tab);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_z, (size_t)8 * n + kGuard));
    } else if (op == OP_NORMALS) {
        uint64_t* d_seeds; int* d_active; double *d_Z, *d_dscale = nullptr;
        CK(dupload(&d_seeds, u64)); CK(dupload(&d_active, active)); CK(dpoison(&d_Z, BCK + kGuard));
        if (flag0) CK(dupload(&d_dscale, f0));
        form = sample_normal_form((int)cs, (int)as, (int)mppi_order);
        launch_sample_normal(d_Z, (int)B, (int)cs, (int)K, (int)as, (int)mppi_order, d_seeds, slo, shi, d_dscale, no_active ? nullptr : d_active, s, d_tab);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_Z, BCK + kGuard));
    } else if (op == OP_DRAWS) {
        uint64_t* d_seeds; int* d_active; int32_t* d_di; double* d_du;
        CK(dupload(&d_seeds, u64)); CK(dupload(&d_active, active)); CK(dpoison(&d_di, BK + kGuard)); CK(dpoison(&d_du, BK + kGuard));
        launch_sample_resample_draws(d_di, d_du, (int)B, (int)K, d_seeds, slo, shi, no_active ? nullptr : d_active, s);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_du, BK + kGuard)); CK(dfetch(oi, d_di, BK + kGuard));
    } else if (op == OP_FINALIZE) {
        EnvDesc env{};                                                           // k_finalize reads lo / hi alone
        for (int i = 0; i < kMaxAs; ++i) { env.lo[i] = f0[i]; env.hi[i] = f1[i]; }
        double *d_U, *d_wn, *d_control;
        CK(dupload(&d_U, f2, kGuard)); CK(dupload(&d_wn, f3, kGuard)); CK(dpoison(&d_control, (size_t)B * as + kGuard));
        launch_finalize_env(d_wn, d_U, d_control, (int)B, (int)cs, (int)as, (int)T, env, s);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_U, BC + kGuard)); CK(dfetch(of1, d_control, (size_t)B * as + kGuard)); CK(dfetch(of2, d_wn, BC + kGuard));
    } else if (op == OP_T_IN) {
        double *d_src, *d_dst; CK(dupload(&d_src, f0)); CK(dpoison(&d_dst, BCK + kGuard));
        if (src_stride) launch_transpose_in(d_src + src_off, d_dst, (int)B, (int)cs, (int)K, s, (size_t)src_stride);
        else launch_transpose_in(d_src + src_off, d_dst, (int)B, (int)cs, (int)K, s);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_dst, BCK + kGuard));
    } else {
        double *d_src, *d_dst, *d_A = nullptr, *d_Bv = nullptr; CK(dupload(&d_src, f0)); CK(dpoison(&d_dst, BCK + kGuard));
        if (flag0) { CK(dupload(&d_A, f1)); CK(dupload(&d_Bv, f2)); }
        launch_transpose_out(d_src, d_A, d_Bv, d_dst, (int)B, (int)cs, (int)K, s);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        CK(dfetch(of0, d_dst, BCK + kGuard));
    }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { printf("cannot write %s\n", argv[2]); return 2; }
    const std::vector<long long> oh = {kMagicOut, form, kGuard, 0};
    if (!wr(fo, oh) || !wr(fo, of0) || !wr(fo, of1) || !wr(fo, of2) || !wr(fo, ou) || !wr(fo, oi) || fclose(fo) != 0) { printf("write failed\n"); return 2; }
    printf("op %d B %lld cs %lld K %lld n %lld form %lld\n", op, B, cs, K, n, form);
    return 0;
}
