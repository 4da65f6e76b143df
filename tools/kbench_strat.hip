// kbench_strat.hip -- runs ONE launch of the antithetic / Latin-hypercube generator (kernels_strat.hip) or of a probe kernel over strat.h (the keyed
// permutation alone, the jitter words, the inverse normal CDF on given inputs) on the inputs of a case file and writes the raw device output back
// to a file (dev / test tool, not shipped).  It holds no reference arithmetic: tests/test_gpu_strat_harness.py writes the case, reads the result
// and compares with NumPy and mpmath (tests/helpers/strat_cases.py).  It calls only launchers declared in engine.h, plus the probe kernels below.
// build: tools/build_kbench.sh strat       run: tools/kbench_strat_bin <case file> <result file>
//
// case file (tools/kbench_io.h, single launch): magic 'STRCASE1', { op, B, n_ipar, n_dpar, n_arrays }, ipar, arrays; array 0 is always active[B]
//   op 0 PERM    ipar { cs, K, step, iter }                                  arrays: active, seeds u64[B]      -> j   i32[B cs K]  (pi_r(k))
//   op 1 JITTER  ipar { cs, K, step, iter }                                  arrays: active, seeds             -> x   i32[B cs K]  (the words' bits)
//   op 2 PHIINV  ipar { K, n }  (B = 1)                                      arrays: active, j i32[n], x i32[n] -> z  f64[n]
//   op 3 GEN     ipar { cs, K, as, mppi_order, kind, step, iter, use_active } arrays: active, seeds             -> Z   f64[B cs K]
//                kind 0 runs launch_sample_normal (no row scales): what the antithetic draw's first half must equal bit for bit
// result file: int64 hdr[4] = { magic 'STRRES01', 0, guard, 1 }, then the one array { type, count; data } (count includes the guard entries)
// The output buffer is filled with the byte 0xA5 first and carries `guard` extra entries; rows of inactive slots must come back as they were.
#include "../mpopis_amd/csrc/engine.h"
#include "../mpopis_amd/csrc/strat.h"
#include "kbench_dev.h"
#include <cstdlib>
using namespace mpopis;
enum { OP_PERM = 0, OP_JITTER = 1, OP_PHIINV = 2, OP_GEN = 3 };

// one thread per (slot, row, sample), like the generator
__global__ void __launch_bounds__(256) k_probe_rows(int32_t* __restrict__ out, int cs, int K, int half, int jitter, const uint64_t* seeds, uint32_t step, uint32_t iter,
                                                    const int* active) {
    const int b = blockIdx.z, r = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (!active[b] || k >= K) return;
    uint32_t v;
    if (jitter) v = strat_jitter_word(seeds[b], step, iter, (uint32_t)r, (uint32_t)k);
    else {
        uint32_t key[4];
        strat_round_keys(seeds[b], step, iter, (uint32_t)r, key);
        v = strat_perm((uint32_t)k, (uint32_t)K, half, key);
    }
    out[((size_t)b * cs + r) * K + k] = (int32_t)v;
}
__global__ void __launch_bounds__(256) k_probe_phi_inv(const int32_t* __restrict__ j, const int32_t* __restrict__ x, double* __restrict__ z, long long n, int K,
                                                       const double* __restrict__ gtab) {
    __shared__ double sh_tab[kRngTabDoubles];
    stage_rng_tab(sh_tab, gtab, threadIdx.x, 256);
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    z[i] = strat_phi_inv((uint32_t)j[i], (uint32_t)x[i], (uint32_t)K, sh_tab);
}

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi; Launch L;
    const char* err = open_case(argv[1], "STRCASE1", nullptr, &fi);
    if (!err) err = read_launch(fi, CaseLimits{3, 1, 3, 3, 2, 1ll << 22, 2}, &L);
    if (!err) err = close_case(fi);
    if (err) BAD(err);
    const int op = L.op; const long long B = L.B;
    const std::vector<long long>& ip = L.ip; const std::vector<Arr>& A = L.A;
    if (!L.need(0, 1, B, false)) BAD("active[B] missing");

    hipStream_t s; CK(hipStreamCreate(&s));
    int* d_active; CK(dup(&d_active, A[0]));
    std::vector<Out> outs;
    if (op == OP_PHIINV) {
        const long long K = ip[0], n = ip[1];
        if (B != 1 || K < 1 || K > kStratMaxK || n < 1 || n > (1 << 22)) BAD("case out of range");
        if (!L.need(1, 1, n, false) || !L.need(2, 1, n, false)) BAD("wrong array sizes");
        { const int32_t* jj = (const int32_t*)L.host(1); for (long long e = 0; e < n; ++e) if (jj[e] < 0 || jj[e] >= K) BAD("stratum out of range"); }
        int32_t *d_j, *d_x; double *d_z, *d_tab;
        CK(dup(&d_j, A[1])); CK(dup(&d_x, A[2])); CK(dout(&d_z, (size_t)n));
        CK(dpoison(&d_tab, (size_t)kRngTabDoubles)); launch_rng_tab_init(d_tab, s); CK(hipGetLastError()); CK(hipStreamSynchronize(s));
        hipLaunchKernelGGL(k_probe_phi_inv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_j, d_x, d_z, n, (int)K, d_tab);
        outs = {{0, (size_t)n, d_z}};
    } else {
        // every launch below indexes with these alone: B slots of cs rows of K samples, cs = as T where a row index is split
        const long long cs = ip[0], K = ip[1];
        const bool gen = op == OP_GEN;
        const long long as = gen ? ip[2] : 1, mppi_order = gen ? ip[3] : 0, kind = gen ? ip[4] : MPOPIS_NOISE_LHS, step = ip[gen ? 5 : 2], iter = ip[gen ? 6 : 3];
        const long long use_active = gen ? ip[7] : 1;
        if (cs < 1 || cs > 4096 || K < 1 || K > kStratMaxK || B * cs * K > (1ll << 22) || as < 1 || as > kMaxAs || cs % as != 0 || (mppi_order != 0 && mppi_order != 1) ||
            kind < MPOPIS_NOISE_PHILOX || kind > MPOPIS_NOISE_LHS || step < 0 || step > 0xffffffffll || iter < 0 || iter >= (1 << 28)) BAD("case out of range");
        if (!L.need(1, 2, B, false)) BAD("seeds[B] missing");
        const size_t n = (size_t)(B * cs * K);
        uint64_t* d_seeds; CK(dup(&d_seeds, A[1]));
        if (!gen) {
            int32_t* d_out; CK(dout(&d_out, n));
            hipLaunchKernelGGL(k_probe_rows, dim3((unsigned)((K + 255) / 256), (unsigned)cs, (unsigned)B), dim3(256), 0, s, d_out, (int)cs, (int)K, strat_half_bits((int)K),
                               op == OP_JITTER ? 1 : 0, d_seeds, (uint32_t)step, (uint32_t)iter, d_active);
            outs = {{1, n, d_out}};
        } else {
            double *d_Z, *d_tab; CK(dout(&d_Z, n));
            CK(dpoison(&d_tab, (size_t)kRngTabDoubles)); launch_rng_tab_init(d_tab, s); CK(hipGetLastError()); CK(hipStreamSynchronize(s));
            const int* act = use_active ? d_active : nullptr;
            if (kind == MPOPIS_NOISE_PHILOX) launch_sample_normal(d_Z, (int)B, (int)cs, (int)K, (int)as, (int)mppi_order, d_seeds, (uint32_t)step, (uint32_t)iter, nullptr, act, s, d_tab);
            else launch_sample_strat(d_Z, (int)B, (int)cs, (int)K, (int)as, (int)mppi_order, (int)kind, d_seeds, (uint32_t)step, (uint32_t)iter, act, s, d_tab);
            outs = {{0, n, d_Z}};
        }
    }
    CK(hipGetLastError()); CK(hipStreamSynchronize(s));
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) BAD("cannot write the result file");
    const long long oh[4] = {magic_word("STRRES01"), 0, kGuard, (long long)outs.size()};
    if (const int rc = write_back(fo, oh, 4, outs)) return rc;
    if (fclose(fo) != 0) BAD("write failed");
    printf("op %d B %lld\n", op, B);
    return 0;
}
