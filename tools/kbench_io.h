// kbench_io.h -- the file side of the kernel harnesses (tools/kbench_<x>.hip): plain C++17, no HIP, so tools/kbench_io_echo.cpp can put the
// reader and the writer through a host compiler and tests/test_harness_io_cpu.py can feed them malformed files without a GPU.
//
// A launch record (little endian; written by tests/helpers/harness_io.py):
//   int64 lh[5] = { op, B, n_ipar, n_dpar, n_arrays }; int64 ipar[n_ipar]; double dpar[n_dpar];
//   n_arrays x { int64 type (0 f64, 1 i32, 2 u64), int64 count; data }      in the fixed order of the op, count 0 = "not given"
// A single-launch case file is { magic, one record } and nothing behind it; a multi-launch one is { magic, n_launches, the records }.
// What a tool writes back is a list of { int64 type, int64 count; data } behind header words of its own (write_arrays).
// The three raw-header tools (select, sample, dynamics) read and write whole vectors with rd / wr instead.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

#define BAD(msg) do { printf("%s (line %d)\n", msg, __LINE__); return 2; } while (0)

struct Arr { long long type = 0, count = 0; std::vector<char> bytes; };
inline size_t tsize(long long t) { return t == 1 ? 4 : 8; }

template <class T> inline bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> inline bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

// what a tool takes: nothing outside these limits gets past read_launch
struct CaseLimits {
    int max_op; long long min_B, max_B; long long max_arrays; long long max_type;
    long long max_count = 1ll << 28; long long min_ipar = 0;
};
struct Launch {
    int op = 0; long long B = 0, nI = 0, nD = 0, nA = 0;
    std::vector<long long> ip; std::vector<double> dp;       // 16 each, zero beyond n_ipar / n_dpar
    std::vector<Arr> A;                                       // max_arrays, count 0 beyond n_arrays
    bool need(int i, long long type, long long count, bool optional) const {
        return (optional && A[i].count == 0) || (A[i].type == type && A[i].count == count);
    }
    const void* host(int i) const { return A[i].bytes.data(); }
    const double* f64(int i) const { return (const double*)A[i].bytes.data(); }
};

// opens a case file and checks its magic; n_launches == nullptr: a single-launch file, else { magic, n_launches } with 1 <= n_launches <= 4096.
// nullptr, or why not
inline const char* open_case(const char* path, const char* magic, long long* n_launches, FILE** f) {
    *f = fopen(path, "rb");
    if (!*f) return "cannot open the case file";
    long long hdr[2] = {0, 0};
    const size_t nh = n_launches ? 2 : 1;
    if (fread(hdr, 8, nh, *f) != nh || memcmp(hdr, magic, 8) != 0 || (n_launches && (hdr[1] < 1 || hdr[1] > 4096))) return "bad case header";
    if (n_launches) *n_launches = hdr[1];
    return nullptr;
}
// one launch record; nullptr, or why it is refused
inline const char* read_launch(FILE* f, const CaseLimits& lim, Launch* L) {
    long long lh[5];
    if (fread(lh, 8, 5, f) != 5) return "short case file";
    L->op = (int)lh[0]; L->B = lh[1]; L->nI = lh[2]; L->nD = lh[3]; L->nA = lh[4];
    if (lh[0] < 0 || lh[0] > lim.max_op || L->B < lim.min_B || L->B > lim.max_B || L->nI < lim.min_ipar || L->nI > 16 || L->nD < 0 || L->nD > 16 || L->nA < 1 ||
        L->nA > lim.max_arrays) return "case out of range";
    L->ip.assign(16, 0); L->dp.assign(16, 0.0);
    if ((L->nI && fread(L->ip.data(), 8, L->nI, f) != (size_t)L->nI) || (L->nD && fread(L->dp.data(), 8, L->nD, f) != (size_t)L->nD)) return "short case file";
    L->A.assign((size_t)lim.max_arrays, Arr());
    for (long long i = 0; i < L->nA; ++i) {
        long long h[2];
        if (fread(h, 8, 2, f) != 2 || h[0] < 0 || h[0] > lim.max_type || h[1] < 0 || h[1] > lim.max_count) return "bad array header";
        Arr& a = L->A[i];
        a.type = h[0]; a.count = h[1]; a.bytes.resize((size_t)h[1] * tsize(h[0]));
        if (h[1] && fread(a.bytes.data(), 1, a.bytes.size(), f) != a.bytes.size()) return "short case file";
    }
    return nullptr;
}
// behind the last record: the end of the file
inline const char* close_case(FILE* f) {
    const bool end = fgetc(f) == EOF;
    fclose(f);
    return end ? nullptr : "case file has the wrong length";
}

struct HostArr { long long type; size_t count; const void* bytes; };
// `nhdr` header words, then every array as { type, count; data }
inline bool write_arrays(FILE* f, const long long* hdr, size_t nhdr, const std::vector<HostArr>& arrays) {
    bool ok = fwrite(hdr, 8, nhdr, f) == nhdr;
    for (const HostArr& a : arrays) {
        const long long ah[2] = {a.type, (long long)a.count};
        const size_t bytes = a.count * tsize(a.type);
        ok = ok && fwrite(ah, 8, 2, f) == 2 && (bytes == 0 || fwrite(a.bytes, 1, bytes, f) == bytes);
    }
    return ok;
}
// the first header word of a result file
inline long long magic_word(const char* magic) { long long w; memcpy(&w, magic, 8); return w; }
