// kernels_strat.hip -- the proposal's standard normals by antithetic pairs or Latin-hypercube strata: the generator the
// step loop launches where it launches launch_sample_normal when the handle's noise kind is not MPOPIS_NOISE_PHILOX.  It writes plain standard
// normals Z[b][r][k] (K fastest); scaling by sqrt(diag Σ) or the product with the Cholesky factor follow as separate launches, as for injected noise.
#include "engine.h"
#include "strat.h"

namespace mpopis {

// One thread per (slot b, Z row r, sample k); consecutive threads hold consecutive k, so a wave stores 64 consecutive doubles.
//   antithetic: column k < h = ceil(K / 2) is the normal k_sample_normal draws for (r, k) (same Philox call, same Box-Muller, in the order the
//               policy draws in: lin = k cs + r, or (t K + k) as + a under :mppi); column k >= h is minus column k - h.
//   LHS:        row r's sample k falls in stratum j = pi_r(k) with jitter word x; Z = Phi^-1((j + xi) / K) (strat.h).  r = t as + a in both orders,
//               so the draw does not depend on the order.  The four round keys of a row are computed once per workgroup.
__global__ void __launch_bounds__(256) k_sample_strat(double* __restrict__ Z, int cs, int K, int as, int mppi_order, int kind, int half,
                                                      const uint64_t* seeds, uint32_t step, uint32_t iter, const int* active, const double* __restrict__ rng_tab) {
    const int b = blockIdx.z;
    if (active && !active[b]) return;
    __shared__ double sh_tab[kRngTabDoubles];
    __shared__ uint32_t sh_key[4];
    stage_rng_tab(sh_tab, rng_tab, threadIdx.x, 256);
    const int r = blockIdx.y;
    const uint64_t seed = seeds[b];
    if (kind == MPOPIS_NOISE_LHS && threadIdx.x == 0) {
        uint32_t key[4];
        strat_round_keys(seed, step, iter, (uint32_t)r, key);
        for (int i = 0; i < 4; ++i) sh_key[i] = key[i];
    }
    __syncthreads();
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double z;
    if (kind == MPOPIS_NOISE_LHS) {
        const uint32_t key[4] = {sh_key[0], sh_key[1], sh_key[2], sh_key[3]};
        const uint32_t j = strat_perm((uint32_t)k, (uint32_t)K, half, key);
        z = strat_phi_inv(j, strat_jitter_word(seed, step, iter, (uint32_t)r, (uint32_t)k), (uint32_t)K, sh_tab);
    } else {
        const int h = (K + 1) / 2, k0 = k < h ? k : k - h;
        uint64_t lin;
        if (mppi_order) { const int t = r / as, a = r - t * as; lin = ((uint64_t)t * K + k0) * as + a; }
        else lin = (uint64_t)k0 * cs + r;
        double z0, z1;
        philox_normal_pair(seed, step, iter, lin >> 1, sh_tab, &z0, &z1);
        z = (lin & 1) ? z1 : z0;
        if (k >= h) z = -z;
    }
    Z[((size_t)b * cs + r) * K + k] = z;
}

void launch_sample_strat(double* Z, int B, int cs, int K, int as, int mppi_order, int kind, const uint64_t* seeds, uint32_t step, uint32_t iter,
                         const int* active, hipStream_t s, const double* rng_tab) {
    hipLaunchKernelGGL(k_sample_strat, dim3((K + 255) / 256, cs, B), dim3(256), 0, s, Z, cs, K, as, mppi_order, kind, strat_half_bits(K), seeds, step, iter, active, rng_tab);
}

}  // namespace mpopis
