// kernels_nes.hip -- the adaptation step of :nesmppi (NESMPPI_Policy, src/mppi_mpopi_policies.jl:855-893) between two iterations:
//   early break            max_k |c_{k+1} - c_k| < 10e-3 stops the slot (:868-870; a NaN never breaks)
//   signed scatter         M = Σ_k c_k E_k E_k', g = Σ_k c_k E_k, C = Σ_k c_k   (one pass over E, FP64 MFMA; the costs have either sign)
//   Σ^-1 from the factor   S = L^-T L^-1 of the Cholesky factor the iteration sampled from (invcov(P), :866)
//   dense products         G = S M S - C S ; A′ ← A′ - (sf/K²) A′ G ; Σ′ = A′' A′ ; U ← U - (sf/K) S g   (:872-878)
// All per-slot, predicated on active[b]; every kernel is deterministic, so a slot's bits do not depend on the schedule.
#include "engine.h"

namespace mpopis {

typedef double v4f64 __attribute__((ext_vector_type(4)));

// ---- early break + finiteness ------------------------------------------------------------------
// One workgroup per slot.  Julia's maximum propagates NaN and NaN < 10e-3 is false, so a NaN difference keeps the slot running; a non-finite
// cost is the G-variants' MPOPIS_ERR_ACTION (k_weights reports the same code for the costs the loop ends with), and the slot stops adapting.
__global__ void __launch_bounds__(256) k_nes_break(const double* __restrict__ cost, int K, int* active, int* status) {
    MPOPIS_HI_PRIO();
    const int b = blockIdx.x;
    if (!active[b]) return;
    const double* c = cost + (size_t)b * K;
    double mx = 0.0; int nan = 0, bad = 0;
    for (int k = threadIdx.x; k < K; k += 256) {
        const double v = c[k];
        if (!isfinite(v)) bad = 1;
        if (k + 1 < K) { const double d = fabs(c[k + 1] - v); if (d != d) nan = 1; else mx = fmax(mx, d); }
    }
    __shared__ double smx[4]; __shared__ int sfl[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_xor(mx, o, 64)); nan |= __shfl_xor(nan, o, 64); bad |= __shfl_xor(bad, o, 64); }
    if ((threadIdx.x & 63) == 0) { smx[threadIdx.x >> 6] = mx; sfl[threadIdx.x >> 6] = nan | (bad << 1); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double m = fmax(fmax(smx[0], smx[1]), fmax(smx[2], smx[3]));
        const int f = sfl[0] | sfl[1] | sfl[2] | sfl[3];
        if (f & 2) { status_raise(&status[b], MPOPIS_ERR_ACTION); active[b] = 0; }
        else if (!(f & 1) && m < 10e-3) active[b] = 0;
    }
}
void launch_nes_break(const double* cost, int B, int K, int* active, int* status, hipStream_t s) {
    hipLaunchKernelGGL(k_nes_break, dim3(B), dim3(256), 0, s, cost, K, active, status);
}

// ---- signed cost-weighted scatter ----------------------------------------------------------------
// The rows of E (d_E: [B][cs][K]) plus a ones row at index cs are staged chunk by chunk in LDS (rows_pad = 16 (cs/16 + 1) rows, stride KC+1),
// the chunk's costs beside them.  A wave owns up to kNesPW lower-triangle tile pairs (ta >= tb) and feeds v_mfma_f64_16x16x4 with
// A = c_k x_a (the cost multiplied into the A operand as it is read: one multiply per MFMA, the weight may be negative so the sqrt(w) staging
// of the AIS scatter does not apply) and B = x_b.  Row cs of the result is g, entry (cs, cs) is C.  K is cut into ksplit ranges: partials
// part[b][split][pair][256] are summed in split order by the finish kernel.
constexpr int kNesKC = 32, kNesS = kNesKC + 1, kNesPW = 7, kNesPB = 4 * kNesPW;
__device__ __forceinline__ void nes_decode_pair(int q, int* ta, int* tb) { int a = 0; while (q >= a + 1) { q -= a + 1; ++a; } *ta = a; *tb = q; }
static int nes_nt(int cs) { return cs / 16 + 1; }
size_t nes_scatter_workspace_doubles(int B, int cs, int ksplit) { const int nt = nes_nt(cs); return (size_t)B * ksplit * (nt * (nt + 1) / 2) * 256; }

__global__ void __launch_bounds__(256) k_nes_scatter_partial(const double* __restrict__ X, const double* __restrict__ cost, double* __restrict__ part,
                                                             int cs, int K, int ksplit, int npairs, const int* active) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = blockIdx.z;
    if (!active[b]) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int nt = cs / 16 + 1, rows_pad = nt * 16;
    double* Xs = smem;                                   // [rows_pad][kNesS]
    double* cl = smem + (size_t)rows_pad * kNesS;        // [kNesKC]
    const double* Xb = X + (size_t)b * cs * K;
    const double* cb = cost + (size_t)b * K;
    int pa[kNesPW], pb[kNesPW];
    const int qbase = blockIdx.y * kNesPB + wv * kNesPW;
#pragma unroll
    for (int p = 0; p < kNesPW; ++p) { if (qbase + p < npairs) nes_decode_pair(qbase + p, &pa[p], &pb[p]); else { pa[p] = 0; pb[p] = 0; } }
    v4f64 acc[kNesPW];
#pragma unroll
    for (int p = 0; p < kNesPW; ++p) acc[p] = (v4f64){0.0, 0.0, 0.0, 0.0};
    const int per = ((K + ksplit - 1) / ksplit + kNesKC - 1) / kNesKC * kNesKC;
    const int kbeg = blockIdx.x * per, kend = min(K, kbeg + per);
    const int skk = threadIdx.x % kNesKC, sr0 = threadIdx.x / kNesKC;   // staging: column skk, rows sr0 + 8u
    constexpr int kRowStep = 256 / kNesKC;
    for (int c0 = kbeg; c0 < kend; c0 += kNesKC) {
        const int kq = c0 + skk;
        const bool kin = kq < kend;
        for (int row = sr0; row < rows_pad; row += kRowStep)
            Xs[(size_t)row * kNesS + skk] = !kin ? 0.0 : (row < cs ? Xb[(size_t)row * K + kq] : (row == cs ? 1.0 : 0.0));
        if (threadIdx.x < kNesKC) cl[threadIdx.x] = (c0 + (int)threadIdx.x < kend) ? cb[c0 + threadIdx.x] : 0.0;
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < kNesKC; kk0 += 4) {
            const double cv = cl[kk0 + lk];
#pragma unroll
            for (int p = 0; p < kNesPW; ++p) {
                const double a = Xs[(size_t)(pa[p] * 16 + li) * kNesS + kk0 + lk] * cv;
                const double bb = Xs[(size_t)(pb[p] * 16 + li) * kNesS + kk0 + lk];
                acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[p], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < kNesPW; ++p) {
        if (qbase + p < npairs) {
            double* pp = part + (((size_t)b * ksplit + blockIdx.x) * npairs + qbase + p) * 256 + lane * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) pp[r] = acc[p][r];
        }
    }
}

// M (cs x cs, written symmetric), g = row cs, C = entry (cs, cs).  Grid (npairs, B).
__global__ void __launch_bounds__(256) k_nes_scatter_finish(const double* __restrict__ part, double* __restrict__ M, double* __restrict__ g,
                                                            double* __restrict__ Csum, int cs, int ksplit, int npairs, const int* active) {
    MPOPIS_HI_PRIO();
    const int b = blockIdx.y;
    if (!active[b]) return;
    int ta, tb;
    nes_decode_pair(blockIdx.x, &ta, &tb);
    const int e = threadIdx.x, lane = e >> 2, r = e & 3;
    const int ia = ta * 16 + (lane >> 4) + 4 * r, ib = tb * 16 + (lane & 15);
    if (ia > cs || ib > cs || (ta == tb && ib > ia)) return;
    const double* src = part + ((size_t)b * ksplit * npairs + blockIdx.x) * 256 + e;
    const size_t stride = (size_t)npairs * 256;
    double v = 0.0;
    for (int sp = 0; sp < ksplit; ++sp) v += src[(size_t)sp * stride];
    if (ia < cs) {
        M[(size_t)b * cs * cs + ia + (size_t)ib * cs] = v;
        M[(size_t)b * cs * cs + ib + (size_t)ia * cs] = v;
    } else if (ib < cs) g[(size_t)b * cs + ib] = v;
    else Csum[b] = v;
}

void launch_nes_scatter(const double* E, const double* cost, double* part, double* M, double* g, double* Csum, int B, int cs, int K, int ksplit,
                        const int* active, hipStream_t s) {
    const int nt = nes_nt(cs), npairs = nt * (nt + 1) / 2;
    const size_t lds = ((size_t)nt * 16 * kNesS + kNesKC) * sizeof(double);
    static std::atomic<unsigned long long> seen{0};
    ensure_dyn_lds((const void*)k_nes_scatter_partial, 160 * 1024, seen);
    hipLaunchKernelGGL(k_nes_scatter_partial, dim3(ksplit, (npairs + kNesPB - 1) / kNesPB, B), dim3(256), lds, s, E, cost, part, cs, K, ksplit, npairs, active);
    hipLaunchKernelGGL(k_nes_scatter_finish, dim3(npairs, B), dim3(256), 0, s, part, M, g, Csum, cs, ksplit, npairs, active);
}

// ---- batched cs x cs FP64 MFMA GEMM ---------------------------------------------------------------------
// C[b] = α α_b[b] op(A[b]) op(B[b]) + β β_b[b] D[b], column-major, op = optional transpose; strides 0 share one matrix between slots.
// One wave per 16 x 16 output tile, operands straight from memory (the matrices are L2-resident: 80 KB at cs = 100).  sym: only tiles with
// ti >= tj, the lower triangle written and mirrored, so the result is exactly symmetric (A′'A′ feeds a Cholesky, which needs that).
// C never aliases A, B or D (ping-pong buffers).
struct NesGemm {
    const double* A; size_t sa; int ta;
    const double* Bm; size_t sb; int tb;
    const double* D; size_t sd;
    double* C; size_t sc;
    double alpha; const double* alpha_b; double beta; const double* beta_b;
    int sym;
};
__global__ void __launch_bounds__(256) k_nes_gemm(NesGemm a, int n, const int* active) {
    MPOPIS_HI_PRIO();
    const int b = blockIdx.y;
    if (active && !active[b]) return;
    const int nt = (n + 15) / 16;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= nt * nt) return;
    const int ti = t % nt, tj = t / nt;
    if (a.sym && ti < tj) return;
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const double* A = a.A + (size_t)b * a.sa;
    const double* Bm = a.Bm + (size_t)b * a.sb;
    const int i = ti * 16 + li, j = tj * 16 + li;
    const int ic = min(i, n - 1), jc = min(j, n - 1);
    v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += 4) {
        const int k = k0 + lk, kc = min(k, n - 1);
        double av = a.ta ? A[kc + (size_t)ic * n] : A[ic + (size_t)kc * n];
        double bv = a.tb ? Bm[jc + (size_t)kc * n] : Bm[kc + (size_t)jc * n];
        if (i >= n || k >= n) av = 0.0;
        if (j >= n || k >= n) bv = 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    const double al = a.alpha * (a.alpha_b ? a.alpha_b[b] : 1.0);
    const double be = a.beta * (a.beta_b ? a.beta_b[b] : 1.0);
    double* C = a.C + (size_t)b * a.sc;
    const double* D = a.D ? a.D + (size_t)b * a.sd : nullptr;
    const int col = tj * 16 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = ti * 16 + lk + 4 * r;
        if (row >= n || col >= n) continue;
        double v = al * acc[r];
        if (D) v = fma(be, D[row + (size_t)col * n], v);
        if (a.sym) {
            if (row < col) continue;
            C[row + (size_t)col * n] = v;
            C[col + (size_t)row * n] = v;
        } else C[row + (size_t)col * n] = v;
    }
}
static void nes_gemm(const NesGemm& g, int B, int n, const int* active, hipStream_t s) {
    const int nt = (n + 15) / 16;
    hipLaunchKernelGGL(k_nes_gemm, dim3((nt * nt + 3) / 4, B), dim3(256), 0, s, g, n, active);
}

// ---- Σ^-1 = L^-T L^-1 (potri) ----------------------------------------------------------------------------
// X = L^-1 by forward substitution, one thread per column of X, cpb columns per workgroup held in LDS (row i of the block at i cpb); the
// entries of L are the same for every lane (scalar loads).  Rows above the column are zero, so every lane runs the same loop.
__global__ void __launch_bounds__(64) k_nes_trtri(const double* __restrict__ L, size_t Lstride, double* __restrict__ X, int n, int cpb, const int* active) {
    MPOPIS_HI_PRIO();
    extern __shared__ __attribute__((aligned(16))) double xs[];      // [n][cpb]
    const int b = blockIdx.y;
    if (active && !active[b]) return;
    const double* Lb = L + (size_t)b * Lstride;
    const int jj = threadIdx.x, j = blockIdx.x * cpb + jj;
    const bool own = jj < cpb && j < n;
    for (int i = 0; i < n; ++i) {
        double s0 = (i == j) ? 1.0 : 0.0, s1 = 0.0;
        int k = 0;
        for (; k + 1 < i; k += 2) {
            s0 = fma(-Lb[i + (size_t)k * n], own ? xs[k * cpb + jj] : 0.0, s0);
            s1 = fma(-Lb[i + (size_t)(k + 1) * n], own ? xs[(k + 1) * cpb + jj] : 0.0, s1);
        }
        if (k < i) s0 = fma(-Lb[i + (size_t)k * n], own ? xs[k * cpb + jj] : 0.0, s0);
        if (own) xs[i * cpb + jj] = (s0 + s1) / Lb[i + (size_t)i * n];
    }
    if (!own) return;
    double* Xb = X + (size_t)b * n * n;
    for (int i = 0; i < n; ++i) Xb[i + (size_t)j * n] = xs[i * cpb + jj];
}
static int nes_trtri_cpb(int n) { return std::max(1, std::min(64, (150 * 1024 / 8) / n)); }
// S = L^-T L^-1 for B factors (Lstride 0: one shared factor); X: B x n x n scratch
void launch_nes_potri(const double* L, size_t Lstride, double* X, double* S, int B, int n, const int* active, hipStream_t s) {
    const int cpb = nes_trtri_cpb(n);
    static std::atomic<unsigned long long> seen{0};
    ensure_dyn_lds((const void*)k_nes_trtri, 160 * 1024, seen);
    hipLaunchKernelGGL(k_nes_trtri, dim3((n + cpb - 1) / cpb, B), dim3(64), (size_t)n * cpb * sizeof(double), s, L, Lstride, X, n, cpb, active);
    const size_t nn = (size_t)n * n;
    NesGemm g{X, nn, 1, X, nn, 0, nullptr, 0, S, nn, 1.0, nullptr, 0.0, nullptr, 1};
    nes_gemm(g, B, n, active, s);
}

// ---- U ← U - (sf/K) S g  (Scale = const double*: per-slot step_factor, scale[b] = sf_b / K) -----------------
template <class Scale>
__global__ void __launch_bounds__(256) k_nes_u_update(const double* __restrict__ S, size_t Sstride, const double* __restrict__ g, double* __restrict__ U,
                                                      int n, Scale scale_arg, const int* active) {
    MPOPIS_HI_PRIO();
    const int b = blockIdx.y;
    if (!active[b]) return;
    const double scale = slot_val(scale_arg, b);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* Sb = S + (size_t)b * Sstride;
    const double* gb = g + (size_t)b * n;
    double acc = 0.0;
    for (int j = 0; j < n; ++j) acc = fma(Sb[i + (size_t)j * n], gb[j], acc);
    U[(size_t)b * n + i] -= scale * acc;
}

// The whole update of iteration n < N (after launch_nes_break).  S: Σ^-1 of the iteration (stride 0 at n = 1: Σ0^-1), Ain / Aout: A′ before / after,
// Sig: Σ′ out, T and M: B x cs x cs scratch (M ends holding G).
void launch_nes_update(const double* E, const double* cost, double* part, int ksplit, const double* S, size_t Sstride, double* M, double* T,
                       double* g, double* Csum, const double* Ain, size_t Astride, double* Aout, double* Sig, double* U,
                       int B, int cs, int K, SlotVal a_scale, SlotVal u_scale, const int* active, hipStream_t s) {
    const size_t nn = (size_t)cs * cs;
    launch_nes_scatter(E, cost, part, M, g, Csum, B, cs, K, ksplit, active, s);
    nes_gemm(NesGemm{S, Sstride, 0, M, nn, 0, nullptr, 0, T, nn, 1.0, nullptr, 0.0, nullptr, 0}, B, cs, active, s);            // T = S M
    nes_gemm(NesGemm{T, nn, 0, S, Sstride, 0, S, Sstride, M, nn, 1.0, nullptr, -1.0, Csum, 0}, B, cs, active, s);              // G = T S - C S
    nes_gemm(NesGemm{Ain, Astride, 0, M, nn, 0, Ain, Astride, Aout, nn, a_scale.per_slot ? 1.0 : a_scale.v, a_scale.per_slot, 1.0, nullptr, 0}, B, cs, active, s);   // A′ - (sf/K²) A′ G
    nes_gemm(NesGemm{Aout, nn, 1, Aout, nn, 0, nullptr, 0, Sig, nn, 1.0, nullptr, 0.0, nullptr, 1}, B, cs, active, s);        // Σ′ = A′' A′
    if (u_scale.per_slot) hipLaunchKernelGGL(k_nes_u_update<const double*>, dim3((cs + 255) / 256, B), dim3(256), 0, s, S, Sstride, g, U, cs, u_scale.per_slot, active);
    else hipLaunchKernelGGL(k_nes_u_update<double>, dim3((cs + 255) / 256, B), dim3(256), 0, s, S, Sstride, g, U, cs, u_scale.v, active);
}

}  // namespace mpopis
