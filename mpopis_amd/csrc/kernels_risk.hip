// kernels_risk.hip -- the risk aggregate of a scenario handle (mpopis_set_scenarios / mpopis_set_risk).
//
// After the M scenario launches of one rollout the costs lie in M planes [B_full][K] (plane m starts m * pstride doubles after plane 0, slot b of
// the launch at b * K inside a plane, exactly where a plain rollout writes cost).  One thread per (slot, sample) loads its M costs -- every load
// coalesced along k --, forms J and writes cost[b * K + k]; then what rollout_epilogue does for a handle whose reweighting is folded into the
// moments kernel: the running minimum of the slot's costs as a cost_key (wave reduce, one atomicMin per wave) and MPOPIS_ERR_ACTION in the
// slot's status for a non-finite J.
//
// The M costs stay in registers: the kernel is a template over M and every loop over them is fully unrolled, so no index into c[] is a run-time
// value (a run-time index would put the array into scratch).  tail and the kind are wave-uniform run-time values that only predicate.
#include "engine.h"

namespace mpopis {

// Mean of the `tail` largest of c[0..M): an odd-even transposition sort into descending order (M passes of compare-exchange, all indices
// compile-time; a plain comparison and swap, so the bits of every input survive), then the first `tail` entries summed from the largest down.
template <int M>
__device__ __forceinline__ double risk_tail_mean(double (&c)[M], int tail) {
#pragma unroll
    for (int p = 0; p < M; ++p) {
#pragma unroll
        for (int i = (p & 1); i + 1 < M; i += 2) {
            const double a = c[i], b = c[i + 1];
            const bool sw = a < b;
            c[i] = sw ? b : a; c[i + 1] = sw ? a : b;
        }
    }
    if (tail == 1) return c[0];
    double s = c[0];
#pragma unroll
    for (int i = 1; i < M; ++i) if (i < tail) s += c[i];
    return s / (double)tail;
}

// c* + log(mean exp(theta (c - c*))) / theta with c* the extreme the sign of theta selects (every exponent <= 0: no overflow; the term of c* is 1)
template <int M>
__device__ __forceinline__ double risk_entropic(const double (&c)[M], double theta) {
    double cs = c[0];
#pragma unroll
    for (int i = 1; i < M; ++i) cs = theta > 0 ? (c[i] > cs ? c[i] : cs) : (c[i] < cs ? c[i] : cs);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) s += exp(theta * (c[i] - cs));
    return cs + log(s / (double)M) / theta;
}

template <int M>
__global__ void __launch_bounds__(256) k_risk(const double* __restrict__ sc, size_t pstride, double* __restrict__ cost, int K, int kind, int tail,
                                              double theta, const int* __restrict__ active, unsigned long long* __restrict__ cmin, int* __restrict__ status) {
    const int b = blockIdx.y;
    if (active && active[b] == 0) return;
    const int k = blockIdx.x * 256 + threadIdx.x;
    const bool valid = k < K;
    double J = 0.0;
    if (valid) {
        double c[M];
        const double* p = sc + (size_t)b * K + k;
#pragma unroll
        for (int m = 0; m < M; ++m) c[m] = p[(size_t)m * pstride];
        // the non-finite inputs, summed under IEEE rules: NaN if one is NaN or both infinities occur, else the infinity
        double bad = 0.0; bool any_bad = false, any_nan = false;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            if (!(fabs(c[m]) < INFINITY)) { bad += c[m]; any_bad = true; }
            any_nan |= c[m] != c[m];
        }
        if (kind == MPOPIS_RISK_ENTROPIC) J = any_bad ? bad : risk_entropic<M>(c, theta);
        else J = any_nan ? bad : risk_tail_mean<M>(c, tail);
        cost[(size_t)b * K + k] = J;
    }
    if (cmin) {
        unsigned long long key = valid ? cost_key(J) : ~0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(key, o, 64); key = (t < key) ? t : key; }
        if ((threadIdx.x & 63) == 0) atomicMin(&cmin[b], key);
    }
    if (status && valid && !(fabs(J) < INFINITY)) status_raise(&status[b], MPOPIS_ERR_ACTION);
}

template <int M>
static void risk_go(const double* sc, size_t pstride, double* cost, int B, int K, int kind, int tail, double theta, const int* active,
                    unsigned long long* cmin, int* status, hipStream_t s) {
    hipLaunchKernelGGL(k_risk<M>, dim3((K + 255) / 256, B), dim3(256), 0, s, sc, pstride, cost, K, kind, tail, theta, active, cmin, status);
}

bool launch_risk(const double* sc, size_t pstride, int M, double* cost, int B, int K, int kind, int tail, double theta, const int* active,
                 unsigned long long* cmin, int* status, hipStream_t s) {
    if (B <= 0 || K <= 0) return true;
    switch (M) {
#define MPOPIS_RISK_CASE(m) case m: risk_go<m>(sc, pstride, cost, B, K, kind, tail, theta, active, cmin, status, s); return true;
        MPOPIS_RISK_CASE(1) MPOPIS_RISK_CASE(2) MPOPIS_RISK_CASE(3) MPOPIS_RISK_CASE(4) MPOPIS_RISK_CASE(5) MPOPIS_RISK_CASE(6)
        MPOPIS_RISK_CASE(7) MPOPIS_RISK_CASE(8) MPOPIS_RISK_CASE(9) MPOPIS_RISK_CASE(10) MPOPIS_RISK_CASE(11) MPOPIS_RISK_CASE(12)
        MPOPIS_RISK_CASE(13) MPOPIS_RISK_CASE(14) MPOPIS_RISK_CASE(15) MPOPIS_RISK_CASE(16)
#undef MPOPIS_RISK_CASE
    }
    return false;
}

}  // namespace mpopis
