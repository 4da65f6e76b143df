// kbench_risk.hip -- runs ONE launch of the risk kernel (kernels_risk.hip: launch_risk) on the inputs of a case file and writes the raw device
// outputs back to a file (dev / test tool, not shipped).  It holds no reference arithmetic: tests/test_gpu_risk_harness.py writes the case, reads
// the result and compares with mpopis_amd.scenarios.aggregate in NumPy longdouble.
// build: tools/build_kbench.sh risk       run: tools/kbench_risk_bin <case file> <result file> [reps]
// With reps > 0 the same launch is then repeated that many times between two events (after the result is written; cmin / status not reset) and
// `TIME_US <microseconds per launch>` is printed: the kernel's own time for tools/scenario_bench.py.
//
// case file (little endian; written by tests/helpers/risk_cases.py over tests/helpers/harness_io.py):
//   int64  hdr[6] = { magic 'RSKCASE1', op (0), B, n_ipar, n_dpar, n_arrays }
//   int64  ipar[8] = { M, B_full, b0, K, kind, tail, use_active, use_status };  double dpar[1] = { theta }
//   arrays: active [B] i32, sc [M][B_full][K] f64 (the scenario planes of the whole batch), cmin [B] u64 (given: passed, with these values before
//           the launch), status [B] i32 (its values before the launch; passed when use_status)
// The launch covers the B slots b0 .. b0 + B - 1 of the planes, as a slot view of a handle does: sc + b0 K with the plane stride B_full K.
// result file:
//   int64  hdr[4] = { magic 'RSKRES01', 0, guard, 3 }; cost [B][K] f64, cmin [B] u64, status [B] i32     (counts include the guard entries)
// The cost buffer is filled with the byte 0xA5 first and every output carries `guard` extra entries (kbench_dev.h).
#include "../mpopis_amd/csrc/engine.h"
#include "kbench_dev.h"
#include <cstdlib>
using namespace mpopis;

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE* fi; Launch L;
    const char* err = open_case(argv[1], "RSKCASE1", nullptr, &fi);
    if (!err) err = read_launch(fi, CaseLimits{0, 1, 64, 4, 2, 1ll << 24, 8}, &L);
    if (!err) err = close_case(fi);
    if (err) BAD(err);
    const long long B = L.B, M = L.ip[0], Bf = L.ip[1], b0 = L.ip[2], K = L.ip[3], kind = L.ip[4], tail = L.ip[5], use_active = L.ip[6], use_status = L.ip[7];
    if (L.nI != 8 || L.nD != 1 || M < 1 || M > MPOPIS_MAX_SCENARIOS || Bf < B || Bf > 64 || b0 < 0 || b0 + B > Bf || K < 1 || K > 8192 ||
        (kind != MPOPIS_RISK_TAIL_MEAN && kind != MPOPIS_RISK_ENTROPIC) || tail < 1 || tail > M) BAD("case out of range");
    if (!L.need(0, 1, B, false) || !L.need(1, 0, M * Bf * K, false) || !L.need(2, 2, B, true) || !L.need(3, 1, B, false)) BAD("wrong array sizes");

    hipStream_t s; CK(hipStreamCreate(&s));
    int *d_active, *d_status; double *d_sc, *d_cost; unsigned long long* d_cmin = nullptr;
    CK(dup(&d_active, L.A[0])); CK(dup(&d_sc, L.A[1]));
    CK(dout(&d_cost, (size_t)(B * K)));
    if (L.A[2].count) CK(dout(&d_cmin, (size_t)B, &L.A[2]));
    CK(dout(&d_status, (size_t)B, &L.A[3]));
    auto go = [&] {
        return launch_risk(d_sc + b0 * K, (size_t)(Bf * K), (int)M, d_cost, (int)B, (int)K, (int)kind, (int)tail, L.dp[0], use_active ? d_active : nullptr, d_cmin,
                           use_status ? d_status : nullptr, s);
    };
    if (!go()) BAD("no kernel for this M");
    CK(hipGetLastError()); CK(hipStreamSynchronize(s));
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) BAD("cannot write the result file");
    const long long oh[4] = {magic_word("RSKRES01"), 0, kGuard, 3};
    if (const int rc = write_back(fo, oh, 4, {{0, (size_t)(B * K), d_cost}, {2, (size_t)B, d_cmin}, {1, (size_t)B, d_status}})) return rc;
    if (fclose(fo) != 0) BAD("write failed");
    printf("M %lld B %lld of %lld K %lld kind %lld tail %lld\n", M, B, Bf, K, kind, tail);
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    if (reps > 0 && reps <= 100000) {
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        CK(hipEventRecord(e0, s));
        for (int r = 0; r < reps; ++r) go();
        CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
        float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
        printf("TIME_US %.3f\n", 1e3 * ms / reps);
    }
    return 0;
}
