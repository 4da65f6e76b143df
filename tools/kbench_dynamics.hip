// kbench_dynamics.hip -- runs the car model of mpopis_amd/csrc/car_dynamics.h AS THE DEVICE COMPILES IT (the rcp / rsq seeds and Newton steps, the inline
// v_min / v_max / v_fma forms, the wave masks of the ring tiers, exec) on the inputs of a case file, one lane per case, and writes the raw device
// outputs back to a file (dev / test tool, not shipped).  It holds no reference arithmetic: tests/test_gpu_dynamics_harness.py writes the case, reads
// the result and compares with long double, the oracle and NumPy.  Header-only: includes car_dynamics.h and links nothing of the library.
// build: tools/build_kbench.sh dynamics       run: tools/kbench_dynamics_bin <case file> <result file>
//
// case file (little endian; layout shared with tests/helpers/dynamics_cases.py):
//   int64  hdr[8] = { magic 'DYNCASE1', op, n, G, P, 0, 0, 0 }        n: lanes (op 0, 2), G: groups (op 1), P: track points (op 2)
//   op 0 primitives: double bnd[2] = { lo, hi } of clampd_u (kernel arguments: wave-uniform); double in[n][14] =
//                    { x, q, angle, cv, clo, chi, sv, sthr, fa, fb, fc, mufz, Ca, fxt }
//   op 1 model step: G times { int64 gh[4] = { PSI, renorm, n_g, 0 }; double p20[20]; double bnd[4] = { lo0, hi0, lo1, hi1 };
//                    double in[n_g][14] = { x, y, psi, Vx, Vy, r, delta, pedal, sp, cp, sd, cd, a0, a1 } }       (sp .. cd as given, not recomputed)
//   op 2 reward:     double p20[20], tx[P], ty[P], tw[P]; double in[n][5] = { px, py, Vx, Vy, anchor }              (anchor: -1 .. P-1, as a double)
// result file:
//   int64  hdr[4] = { magic 'DYNRES01', op, guard, launches }
//   op 0: double out[n][16 + guard entries at the end] = { fast_rcp1(x), fast_rcp(x), fast_sqrt(q), fast_sqrt_rsq(q): s, 1/s, sincos_tiny(angle): sin, cos,
//         clamp_sym(sv, sthr), clampd_u(cv, lo, hi), clampd_v(cv, clo, chi), fma_v(fa, fb, fc), tire_consts(mufz, Ca, fxt): fymax, thr, k2, k3, (untouched) }
//   op 1: per group double out[n_g][12] + guard = the CarState after clampd_u of both actions and ONE car_action_step<PSI>(p, s, a0, a1, renorm)
//   op 2: double out[n][12] + guard = { car_reward(.., &anchor), anchor after it, lane's bit of ring_candidates, its rel, lane's bit of ring5_candidates
//         (0 when P < 5: car_reward does not call it then), its rel, within / dist / anchor of an unanchored within_track, and as raw 64-bit patterns the
//         whole ring_candidates mask, the whole ring5_candidates mask and exec }
// Every output buffer is filled with the byte 0xA5 first and carries `guard` extra entries; every launch has 64-lane workgroups, lanes past n return.
#include "kbench_dev.h"
#include "../mpopis_amd/csrc/car_dynamics.h"
#include <cstdlib>
#include <cmath>
using namespace mpopis;
static const long long kMagicIn = 0x31455341434e5944ll, kMagicOut = 0x31305345524e5944ll;       // "DYNCASE1", "DYNRES01"
enum { OP_PRIMS = 0, OP_STEP = 1, OP_REWARD = 2 };
constexpr int kPrimIn = 14, kPrimOut = 16, kStepIn = 14, kStepOut = 12, kRewIn = 5, kRewOut = 12;

__global__ __launch_bounds__(64) void k_prims(const double* __restrict__ in, double* __restrict__ out, int n, double lo, double hi) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* a = in + (size_t)i * kPrimIn;
    double* o = out + (size_t)i * kPrimOut;
    o[0] = fast_rcp1(a[0]);
    o[1] = fast_rcp(a[0]);
    o[2] = fast_sqrt(a[1]);
    double rs; const double s = fast_sqrt_rsq(a[1], &rs);
    o[3] = s; o[4] = rs;
    double sn, cs; sincos_tiny(a[2], &sn, &cs);
    o[5] = sn; o[6] = cs;
    o[7] = clamp_sym(a[6], a[7]);
    o[8] = clampd_u(a[3], lo, hi);
    o[9] = clampd_v(a[3], a[4], a[5]);
    o[10] = fma_v(a[8], a[9], a[10]);
    const TireK k = tire_consts(a[11], a[12], a[13]);
    o[11] = k.fymax; o[12] = k.thr; o[13] = k.k2; o[14] = k.k3;
}

template <bool PSI>
__global__ __launch_bounds__(64) void k_step(CarParams p, const double* __restrict__ in, double* __restrict__ out, int n, double lo0, double hi0, double lo1, double hi1, int renorm) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* a = in + (size_t)i * kStepIn;
    double* o = out + (size_t)i * kStepOut;
    CarState c;
    c.x = a[0]; c.y = a[1]; c.psi = a[2]; c.Vx = a[3]; c.Vy = a[4]; c.r = a[5]; c.delta = a[6]; c.pedal = a[7];
    c.sp = a[8]; c.cp = a[9]; c.sd = a[10]; c.cd = a[11]; c.near = -1;
    const double a0 = clampd_u(a[12], lo0, hi0), a1 = clampd_u(a[13], lo1, hi1);
    car_action_step<PSI>(p, c, a0, a1, renorm != 0);
    o[0] = c.x; o[1] = c.y; o[2] = c.psi; o[3] = c.Vx; o[4] = c.Vy; o[5] = c.r; o[6] = c.delta; o[7] = c.pedal;
    o[8] = c.sp; o[9] = c.cp; o[10] = c.sd; o[11] = c.cd;
}

__global__ __launch_bounds__(64) void k_reward(CarParams p, Track tk, const double* __restrict__ in, double* __restrict__ out, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* a = in + (size_t)i * kRewIn;
    double* o = out + (size_t)i * kRewOut;
    const double px = a[0], py = a[1], m2x = -2.0 * px, m2y = -2.0 * py;
    const int a_in = (int)a[4];
    int anchor = a_in;
    o[0] = car_reward(p, tk, px, py, a[2], a[3], &anchor);
    o[1] = (double)anchor;
    const int lane = wave_lane();
    int rel3 = 0, rel5 = 0;
    const unsigned long long m3 = ring_candidates(tk.ring, tk.ring_cert, a_in, px, py, m2x, m2y, &rel3);
    unsigned long long m5 = 0ull;
    if (tk.P >= 5) m5 = ring5_candidates(tk.ring, tk.ring_cert + tk.P, a_in, px, py, m2x, m2y, &rel5);
    o[2] = (double)((m3 >> lane) & 1ull); o[3] = (double)rel3;
    o[4] = (double)((m5 >> lane) & 1ull); o[5] = (double)rel5;
    int none = -1; double dist = 0.0;
    const bool w = within_track(tk, px, py, &dist, &none);
    o[6] = w ? 1.0 : 0.0; o[7] = dist; o[8] = (double)none;
    o[9] = __longlong_as_double((long long)m3); o[10] = __longlong_as_double((long long)m5);
    o[11] = __longlong_as_double((long long)__builtin_amdgcn_read_exec());
}

static int blocks(long long n) { return (int)((n + 63) / 64); }

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hdr;
    if (!rd(fi, hdr, 8) || hdr[0] != kMagicIn) { printf("bad case header\n"); return 2; }
    const int op = (int)hdr[1]; const long long n = hdr[2], G = hdr[3], P = hdr[4];
    if (op < 0 || op > 2 || n < 0 || n > (1 << 20) || G < 0 || G > 4096 || P < 0 || P > kMaxTrackPoints) { printf("case out of range\n"); return 2; }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { printf("cannot write %s\n", argv[2]); return 2; }
    long long launches = 0;
    std::vector<std::vector<double>> outs;
    hipStream_t s; CK(hipStreamCreate(&s));
    if (op == OP_PRIMS) {
        std::vector<double> bnd, in;
        if (n < 1 || !rd(fi, bnd, 2) || !rd(fi, in, (size_t)n * kPrimIn) || fgetc(fi) != EOF) { printf("case file has the wrong length\n"); return 2; }
        double *d_in, *d_out; CK(dupload(&d_in, in)); CK(dpoison(&d_out, (size_t)n * kPrimOut + kGuard));
        hipLaunchKernelGGL(k_prims, dim3(blocks(n)), dim3(64), 0, s, d_in, d_out, (int)n, bnd[0], bnd[1]);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s)); ++launches;
        outs.emplace_back(); CK(dfetch(outs.back(), d_out, (size_t)n * kPrimOut + kGuard));
    } else if (op == OP_STEP) {
        if (G < 1) { printf("no groups\n"); return 2; }
        for (long long g = 0; g < G; ++g) {
            std::vector<long long> gh; std::vector<double> p20, bnd, in;
            if (!rd(fi, gh, 4) || gh[2] < 1 || gh[2] > (1 << 20) || !rd(fi, p20, kCarNParams) || !rd(fi, bnd, 4) || !rd(fi, in, (size_t)gh[2] * kStepIn)) { printf("short case file (group %lld)\n", g); return 2; }
            const int ng = (int)gh[2];
            const CarParams p = make_car_params(p20.data());
            if (p.nsub < 1 || p.nsub > 1000) { printf("sub-step count out of range (group %lld)\n", g); return 2; }
            double *d_in, *d_out; CK(dupload(&d_in, in)); CK(dpoison(&d_out, (size_t)ng * kStepOut + kGuard));
            if (gh[0]) hipLaunchKernelGGL(k_step<true>, dim3(blocks(ng)), dim3(64), 0, s, p, d_in, d_out, ng, bnd[0], bnd[1], bnd[2], bnd[3], (int)gh[1]);
            else hipLaunchKernelGGL(k_step<false>, dim3(blocks(ng)), dim3(64), 0, s, p, d_in, d_out, ng, bnd[0], bnd[1], bnd[2], bnd[3], (int)gh[1]);
            CK(hipGetLastError()); CK(hipStreamSynchronize(s)); ++launches;
            outs.emplace_back(); CK(dfetch(outs.back(), d_out, (size_t)ng * kStepOut + kGuard));
            CK(dfree_all());
        }
        if (fgetc(fi) != EOF) { printf("case file has the wrong length\n"); return 2; }
    } else {
        std::vector<double> p20, tx, ty, tw, in;
        if (n < 1 || P < 3 || !rd(fi, p20, kCarNParams) || !rd(fi, tx, P) || !rd(fi, ty, P) || !rd(fi, tw, P) || !rd(fi, in, (size_t)n * kRewIn) || fgetc(fi) != EOF) { printf("case file has the wrong length\n"); return 2; }
        // the kernel indexes the tables with the anchor: only an anchor the host has validated gets near it
        for (long long i = 0; i < n; ++i) { const double a = in[(size_t)i * kRewIn + 4]; if (!(a >= -1.0 && a <= (double)(P - 1)) || a != floor(a)) { printf("invalid anchor in lane %lld\n", i); return 3; } }
        const CarParams p = make_car_params(p20.data());
        Track tk; double *d_in, *d_out;
        CK(dtrack(&tk, TrackHost((int)P, tx.data(), ty.data(), tw.data()))); CK(dupload(&d_in, in)); CK(dpoison(&d_out, (size_t)n * kRewOut + kGuard));
        hipLaunchKernelGGL(k_reward, dim3(blocks(n)), dim3(64), 0, s, p, tk, d_in, d_out, (int)n);
        CK(hipGetLastError()); CK(hipStreamSynchronize(s)); ++launches;
        outs.emplace_back(); CK(dfetch(outs.back(), d_out, (size_t)n * kRewOut + kGuard));
    }
    fclose(fi);
    const std::vector<long long> oh = {kMagicOut, op, kGuard, launches};
    bool ok = wr(fo, oh);
    for (const auto& o : outs) ok = ok && wr(fo, o);
    if (!ok || fclose(fo) != 0) { printf("write failed\n"); return 2; }
    printf("op %d n %lld groups %lld P %lld launches %lld\n", op, n, G, P, launches);
    return 0;
}
