// kernels_plan.hip -- the read-out behind mpopis_get_plan: which samples of the last step carry the most weight, and the
// control sequences of the plan and of those samples as one [B][cs][top + 1] noise block that the rollout kernels take as they take E.
// Nothing here runs during a policy step.  mpopis_run_trials_traced launches the same kernels between a policy step and its env step, on the part's
// slots, with active = the harness' alive flags.
#include "engine.h"

namespace mpopis {

// A sample's place in the order "weight descending, then index ascending" as one key that is compared high to low: the weight's raw bit pattern
// (weights are finite and >= +0, so the pattern orders like the number) and K - index.  The larger key comes first.  lo = 0 is no sample's.
struct PlanKey { unsigned long long bits; unsigned lo; };
__device__ __forceinline__ bool plan_key_less(const PlanKey& a, const PlanKey& b) { return a.bits < b.bits || (a.bits == b.bits && a.lo < b.lo); }

// One workgroup per slot, any K, top <= MPOPIS_PLAN_MAX_TOP <= K: idx[b][j], wsel[b][j] for j < top.  Round j: every lane scans its strided share of
// the row for the largest key strictly below the one round j - 1 took, the lanes of a wave reduce by shuffles, the waves through one LDS row
// (two rows in turn: one barrier per round).  No scratch, no marking of taken samples, no atomics: equal weights cost nothing extra.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_plan_select(const double* __restrict__ w, int K, int top, int32_t* __restrict__ idx, double* __restrict__ wsel,
                                                       const int* __restrict__ active) {
    MPOPIS_HI_PRIO();
    if (active && !active[blockIdx.x]) return;                                 // (the traced closed loop: a frozen slot's stale weights stay out of the trace)
    constexpr int NW = BLOCK / 64;
    __shared__ unsigned long long sh_bits[2][NW];
    __shared__ unsigned sh_lo[2][NW];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long* wb = reinterpret_cast<const unsigned long long*>(w) + (size_t)b * K;
    PlanKey prev{~0ull, ~0u};
    for (int j = 0; j < top; ++j) {
        PlanKey best{0ull, 0u};
        for (int k = threadIdx.x; k < K; k += BLOCK) {
            const PlanKey c{wb[k], (unsigned)(K - k)};
            if (plan_key_less(c, prev) && plan_key_less(best, c)) best = c;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const PlanKey t{(unsigned long long)__shfl_xor((long long)best.bits, o, 64), (unsigned)__shfl_xor((int)best.lo, o, 64)};
            if (plan_key_less(best, t)) best = t;
        }
        if (lane == 0) { sh_bits[j & 1][wave] = best.bits; sh_lo[j & 1][wave] = best.lo; }
        __syncthreads();
        best = PlanKey{sh_bits[j & 1][0], sh_lo[j & 1][0]};
#pragma unroll
        for (int v = 1; v < NW; ++v) {
            const PlanKey t{sh_bits[j & 1][v], sh_lo[j & 1][v]};
            if (plan_key_less(best, t)) best = t;
        }
        prev = best;                                                           // (the same in every lane)
        if (threadIdx.x == 0) {
            // top <= K: every round finds a sample.  Were a weight not a number >= +0 the order would be that of the patterns, never an index out of range.
            const int k = best.lo ? K - (int)best.lo : 0;
            idx[(size_t)b * top + j] = k;
            wsel[(size_t)b * top + j] = w[(size_t)b * K + k];
        }
    }
}

// controls = U_orig + weighted noise (the addition k_finalize performs), and the noise block of the read-out's rollout, whose nominal sequence is
// U_orig: column 0 the weighted noise itself, column j the sample's noise after the final shift, formed like k_transpose_out forms E_out.
__global__ void __launch_bounds__(256) k_plan_assemble(const double* __restrict__ E, const double* __restrict__ Ucur, const double* __restrict__ Uin,
                                                       const double* __restrict__ wn, const int32_t* __restrict__ idx, int cs, int K, int top,
                                                       double* __restrict__ controls, double* __restrict__ Eplan, const int* __restrict__ active) {
    MPOPIS_HI_PRIO();
    const int b = blockIdx.y, W = top + 1;
    if (active && !active[b]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cs * W) return;
    const int r = i / W, j = i - r * W;
    const size_t br = (size_t)b * cs + r;
    double v;
    if (j == 0) {
        v = wn[br];
        controls[br] = Uin[br] + v;
    } else {
        const int k = idx[(size_t)b * top + (j - 1)];
        v = E[br * K + k] + (Ucur[br] - Uin[br]);
    }
    Eplan[br * W + j] = v;
}

void launch_plan_select(const double* w, int B, int K, int top, int32_t* idx, double* wsel, hipStream_t s, const int* active) {
    if (top < 1) return;
    if (K > 1024) hipLaunchKernelGGL(k_plan_select<1024>, dim3(B), dim3(1024), 0, s, w, K, top, idx, wsel, active);
    else hipLaunchKernelGGL(k_plan_select<256>, dim3(B), dim3(256), 0, s, w, K, top, idx, wsel, active);
}

void launch_plan_assemble(const double* E, const double* Ucur, const double* Uin, const double* wn, const int32_t* idx, int B, int cs, int K, int top,
                          double* controls, double* Eplan, hipStream_t s, const int* active) {
    hipLaunchKernelGGL(k_plan_assemble, dim3((cs * (top + 1) + 255) / 256, B), dim3(256), 0, s, E, Ucur, Uin, wn, idx, cs, K, top, controls, Eplan, active);
}

}  // namespace mpopis
