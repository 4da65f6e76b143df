// kernels_trace.hip -- the per-step record behind mpopis_run_trials_traced: where each slot's env stood after every MPC step
// of the closed loop, what the step earned, and the lane / β read-out of that state.  Launched behind k_harness_update on each part's own stream;
// plain vector stores into zero-filled arrays in the ABI's slot-major layout, no atomics, no LDS.
#include "engine.h"

namespace mpopis {

// one wave per slot, lane = state element: states[b][0] = the state the run starts from
__global__ void __launch_bounds__(64) k_trace_start(const double* __restrict__ x, double* __restrict__ states, int ss, int S) {
    const int b = blockIdx.x;
    for (int e = threadIdx.x; e < ss; e += 64) states[(size_t)b * (S + 1) * ss + e] = x[(size_t)b * ss + e];
}

// One wave per slot.  Lane e copies state element e; lane c < ncars reads car c's lane distance and β off the post-noise state with the device
// functions k_env_query uses (within_track, atan2: the same operands, the same bits); lane 0 writes the scalars.  The gate is the step counter
// k_harness_update has just advanced: cnt == step + 1 exactly for the slots that were alive during this step (`alive` itself may already be 0).
__global__ void __launch_bounds__(64) k_trace_step(int env_kind, int ncars, int ss, Track tk, const Track* __restrict__ slot_tk, const double* __restrict__ x,
                                                   const double* __restrict__ reward, const int* __restrict__ iters, const double* __restrict__ cnt,
                                                   int cnt_stride, int step, int S, TraceStepOut out) {
    const int b = blockIdx.x, e = threadIdx.x;
    if (cnt[(size_t)b * cnt_stride] != (double)(step + 1)) return;
    const double* xb = x + (size_t)b * ss;
    const size_t row = (size_t)b * S + step;
    if (out.states) for (int i = e; i < ss; i += 64) out.states[((size_t)b * (S + 1) + step + 1) * ss + i] = xb[i];
    if (e == 0) {
        if (out.rewards) out.rewards[row] = reward[b];
        if (out.iters) out.iters[row] = iters[b];
    }
    if (env_kind != MPOPIS_ENV_CAR) {
        if (e == 0 && out.within) out.within[row] = 1;
        return;
    }
    if (!out.within && !out.dist && !out.beta) return;
    if (slot_tk) tk = slot_tk[b];
    bool outside = false;
    if (e < ncars) {
        const double* s = xb + 8 * e;
        double d;
        outside = !within_track(tk, s[0], s[1], &d, nullptr);
        if (out.dist) out.dist[row * ncars + e] = d;
        if (out.beta) out.beta[row * ncars + e] = atan2(s[4], s[3]);
    }
    const unsigned long long any_outside = __ballot(outside);
    if (e == 0 && out.within) out.within[row] = any_outside == 0;
}

// out[b][j][:] = in[j][b][:]: one workgroup per (j, b) row
template <class T>
__global__ void __launch_bounds__(256) k_trace_reorder(const T* __restrict__ in, T* __restrict__ out, int B, int J, size_t per) {
    const size_t r = blockIdx.x;
    const size_t j = r / B, b = r - j * B;
    const T* src = in + r * per;
    T* dst = out + (b * J + j) * per;
    for (size_t i = threadIdx.x; i < per; i += 256) dst[i] = src[i];
}

void launch_trace_start(const double* x, double* states, int B, int ss, int S, hipStream_t s) {
    hipLaunchKernelGGL(k_trace_start, dim3(B), dim3(64), 0, s, x, states, ss, S);
}

void launch_trace_step(int env_kind, int ncars, int ss, const Track& tk, const Track* slot_tk, const double* x, const double* reward, const int* iters,
                       const double* cnt, int cnt_stride, int step, int S, const TraceStepOut& out, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_trace_step, dim3(B), dim3(64), 0, s, env_kind, ncars, ss, tk, slot_tk, x, reward, iters, cnt, cnt_stride, step, S, out);
}

void launch_trace_reorder(const void* in, void* out, int B, int J, size_t per, int elem_bytes, hipStream_t s) {
    if (B < 1 || J < 1 || per < 1) return;
    const dim3 grid((unsigned)((size_t)B * J));
    if (elem_bytes == 4) hipLaunchKernelGGL(k_trace_reorder<int32_t>, grid, dim3(256), 0, s, (const int32_t*)in, (int32_t*)out, B, J, per);
    else hipLaunchKernelGGL(k_trace_reorder<double>, grid, dim3(256), 0, s, (const double*)in, (double*)out, B, J, per);
}

}  // namespace mpopis
