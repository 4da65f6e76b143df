// strat.h -- the two variance-reduced draws of the proposal, device side: the keyed permutation and the jitter word of the
// Latin-hypercube draw, and the inverse normal CDF that turns a stratum into a normal.  Shared by kernels_strat.hip and the probe kernels of
// tools/kbench_strat.hip; tests/helpers/strat_cases.py restates the integer part bit for bit and the floating-point part operation by operation.
#pragma once
#include "philox.h"

namespace mpopis {

// Philox streams of the new draws: counter = (c0, c1, MPC step, tag | AIS iteration), key = the slot's seed.  The tags in use elsewhere are the
// plain iteration index (the normals), 0x80000000 | n (resampling) and 0x40000000 (state noise); iterations stay far below 2^28.
constexpr uint32_t kStratTagKeys = 0x10000000u;      // c0 = Z row r, c1 = 0: the four round keys of pi_r
constexpr uint32_t kStratTagJitter = 0x20000000u;    // c0 = sample k, c1 = Z row r: word 0 is the jitter word x
// (K <= kStratMaxK = 2^20 of engine.h: j 2^33 + 2 x + 1 must stay below 2^53 in strat_phi_inv)

// half the width of the Feistel domain: the bits of K - 1, rounded up to an even count, halved.  Domain 4^half in [K, 4 K) for K >= 2.
__host__ __device__ inline int strat_half_bits(int K) {
    int nb = 0;
    for (unsigned v = (unsigned)(K - 1); v; v >>= 1) ++nb;
    return nb < 1 ? 1 : (nb + 1) / 2;
}
__device__ __forceinline__ void strat_round_keys(uint64_t seed, uint32_t step, uint32_t iter, uint32_t r, uint32_t* key) {
    philox4x32_10(r, 0u, step, kStratTagKeys | iter, (uint32_t)seed, (uint32_t)(seed >> 32), key);
}
__device__ __forceinline__ uint32_t strat_jitter_word(uint64_t seed, uint32_t step, uint32_t iter, uint32_t r, uint32_t k) {
    uint32_t w[4];
    philox4x32_10(k, r, step, kStratTagJitter | iter, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    return w[0];
}
// round function: `half` bits of a multiply-xorshift hash of (right half, round key)
__device__ __forceinline__ uint32_t strat_round(uint32_t x, uint32_t key, int half) {
    uint32_t t = (x ^ key) * 0x9E3779B1u;
    t ^= t >> 15; t *= 0x85EBCA6Bu; t ^= t >> 13;
    return t >> (32 - half);
}
// pi_r(k): four balanced Feistel rounds over 2 half bits, walked until the image falls below K.  A permutation of the domain restricted to
// [0, K) by cycle walking is a permutation of [0, K); the walk returns below K after at most (domain - K + 1) steps, which bounds the loop
// (expected: domain / K < 4 steps).  The only lane-divergent loop of the generator.
__device__ __forceinline__ uint32_t strat_perm(uint32_t k, uint32_t K, int half, const uint32_t* key) {
    if (K == 1) return 0;
    const uint32_t mask = (1u << half) - 1u, dom = 1u << (2 * half);
    uint32_t y = k;
    for (uint32_t walk = 0; walk < dom; ++walk) {
        uint32_t L = y >> half, R = y & mask;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const uint32_t t = L ^ strat_round(R, key[i], half); L = R; R = t; }
        y = (L << half) | R;
        if (y < K) break;
    }
    return y;
}

// sqrt of a positive normal-range number, <= 1 ulp: the iteration of box_muller_u32 (philox.h)
__device__ __forceinline__ double strat_sqrt(double v) {
    const double y = __builtin_amdgcn_rsq(v);
    double g = v * y, h = 0.5 * y;
    const double rr = fma(-h, g, 0.5);
    g = fma(g, rr, g); h = fma(h, rr, h);
    return fma(fma(-g, g, v), h, g);
}

// Z = Phi^-1((j + xi) / K), xi = (x + 0.5) 2^-32, for stratum j < K <= 2^20 and jitter word x.  Evaluated from the SMALL side: a stratum in the
// upper half (or the upper half of the middle stratum of an odd K) is mirrored to (K - 1 - j, ~x) -- 1 - xi is exactly (~x + 0.5) 2^-32 -- and
// the sign flipped, so that mirrored inputs give exact negatives and the upper tail keeps the digits of the lower one.
//   p = (j 2^33 + 2 x + 1) 2^-33 / K in (0, 1/2]: the numerator is an integer below 2^53 (exact), the division rounds once.
//   p > exp(-2):  y = p - 1/2, w = y + y (y^2 P0(y^2) / Q0(y^2)), |Z| = -w sqrt(2 pi)
//   else:         t = sqrt(-2 log p), t0 = t - log(t) / t, |Z| = t0 - (1/t) P(1/t) / Q(1/t), (P, Q) = (P1, Q1) for t < 8, else (P2, Q2)
// The rational approximations are those of ndtri() of the Cephes Math Library (S. L. Moshier; coefficients highest degree first, as published).
// log is log_unit of philox.h (table in LDS, every term of its error documented there), sqrt is strat_sqrt: no device-library function is involved.
// The error bound, term by term, is phi_inv_bound of tests/helpers/strat_cases.py.
__device__ __forceinline__ double strat_horner(double x, const double* c, int n) {
    double s = c[0];
#pragma unroll
    for (int i = 1; i < n; ++i) s = fma(s, x, c[i]);
    return s;
}
__device__ __forceinline__ double strat_phi_inv(uint32_t j, uint32_t x, uint32_t K, const double* __restrict__ tab) {
    const double P0[5] = {-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1, 1.39312609387279679503E1, -1.23916583867381258016E0};
    const double Q0[9] = {1.00000000000000000000E0, 1.95448858338141759834E0, 4.67627912898881538453E0, 8.63602421390890590575E1, -2.25462687854119370527E2,
                          2.00260212380060660359E2, -8.20372256168333339912E1, 1.59056225126211695515E1, -1.18331621121330003142E0};
    const double P1[9] = {4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1, 4.40805073893200834700E1, 1.46849561928858024014E1,
                          2.18663306850790267539E0, -1.40256079171354495875E-1, -3.50424626827848203418E-2, -8.57456785154685413611E-4};
    const double Q1[9] = {1.00000000000000000000E0, 1.57799883256466749731E1, 4.53907635128879210584E1, 4.13172038254672030440E1, 1.50425385692907503408E1,
                          2.50464946208309415979E0, -1.42182922854787788574E-1, -3.80806407691578277194E-2, -9.33259480895457427372E-4};
    const double P2[9] = {3.23774891776946035970E0, 6.91522889068984211695E0, 3.93881025292474443415E0, 1.33303460815807542389E0, 2.01485389549179081538E-1,
                          1.23716634817820021358E-2, 3.01581553508235416007E-4, 2.65806974686737550832E-6, 6.23974539184983293730E-9};
    const double Q2[9] = {1.00000000000000000000E0, 6.02427039364742014255E0, 3.67983563856160859403E0, 1.37702099489081330271E0, 2.16236993594496635890E-1,
                          1.34204006088543189037E-2, 3.28014464682127739104E-4, 2.89247864745380683936E-6, 6.79019408009981274425E-9};
    const uint32_t twice = 2u * j + 1u;
    const bool flip = twice > K || (twice == K && x >= 0x80000000u);
    const uint32_t js = flip ? K - 1u - j : j, xs = flip ? ~x : x;
    const double num = (double)(((uint64_t)js << 33) | (((uint64_t)xs << 1) | 1ull));
    const double p = (num * 0x1p-33) / (double)K;
    double mag;
    if (p > 0.13533528323661269189) {
        const double y = p - 0.5, y2 = y * y;
        const double q = (y2 * strat_horner(y2, P0, 5)) / strat_horner(y2, Q0, 9);
        mag = -(fma(y, q, y) * 2.50662827463100050242E0);
    } else {
        const double t = strat_sqrt(-2.0 * log_unit(p, tab));
        const double t0 = t - log_unit(t, tab) / t;
        const double z = 1.0 / t;
        const double t1 = t < 8.0 ? (z * strat_horner(z, P1, 9)) / strat_horner(z, Q1, 9) : (z * strat_horner(z, P2, 9)) / strat_horner(z, Q2, 9);
        mag = t0 - t1;
    }
    return flip ? mag : -mag;
}

}  // namespace mpopis
