// kbench_dev.h -- the device side of the kernel harnesses (tools/kbench_<x>.hip): what the contract in tools/README.md promises of every output
// buffer lives here.  An output buffer is filled with the byte kPoison first and carries kGuard extra entries behind the ones the launch may
// write, so the test sees what the launch left untouched and what it wrote past the end; the write-back copies every buffer to the result file
// as the device left it.  No reference arithmetic, and no include of engine.h: kbench_dynamics.hip links nothing of the library.
#pragma once
#include <hip/hip_runtime.h>
#include "kbench_io.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
static const int kGuard = 64, kPoison = 0xA5;

// every allocation of the current launch; the multi-launch tools free them after each launch of the file (dfree_all)
inline std::vector<void*> g_allocs;
inline hipError_t dmalloc(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes ? bytes : 8);
    if (e == hipSuccess) g_allocs.push_back(*p);
    return e;
}
inline hipError_t dfree_all() {
    hipError_t e = hipSuccess;
    for (void* p : g_allocs) { const hipError_t f = hipFree(p); if (e == hipSuccess) e = f; }
    g_allocs.clear();
    return e;
}
template <class T> static hipError_t dfill(T** p, size_t n, int byte) {     // workspace of n entries of `byte` (0xFF: NaN)
    hipError_t e = dmalloc((void**)p, (n ? n : 1) * sizeof(T));
    return e != hipSuccess ? e : hipMemset(*p, byte, (n ? n : 1) * sizeof(T));
}
template <class T> static hipError_t dpoison(T** p, size_t n) { return dfill(p, n, kPoison); }
// output buffer of n entries (+ guard), poisoned; init (nullable): its first n entries
template <class T> static hipError_t dout(T** p, size_t n, const void* init = nullptr) {
    hipError_t e = dpoison(p, n + kGuard);
    return (e != hipSuccess || !init || !n) ? e : hipMemcpy(*p, init, n * sizeof(T), hipMemcpyHostToDevice);
}
template <class T> static hipError_t dout(T** p, size_t n, const Arr* init) { return dout(p, n, (init && init->count) ? (const void*)init->bytes.data() : nullptr); }
// input copy (+ `pad` zero entries behind it); nullptr when the array is not given
template <class T> static hipError_t dup(T** p, const Arr& a, size_t pad = 0) {
    *p = nullptr;
    if (!a.count) return hipSuccess;
    const size_t bytes = a.bytes.size() + pad * tsize(a.type);
    hipError_t e = dmalloc((void**)p, bytes);
    if (e == hipSuccess && pad) e = hipMemset(*p, 0, bytes);
    return e != hipSuccess ? e : hipMemcpy(*p, a.bytes.data(), a.bytes.size(), hipMemcpyHostToDevice);
}
// a host vector on the device: v, then `guard` entries of poison
template <class T> static hipError_t dupload(T** p, const std::vector<T>& v, size_t guard = 0) {
    hipError_t e = dpoison(p, v.size() + guard);
    return (e != hipSuccess || v.empty()) ? e : hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}
template <class T> static hipError_t dupv(T** p, const std::vector<T>& v) { return dupload(p, v); }
template <class T> static hipError_t dfetch(std::vector<T>& v, const T* p, size_t n) { v.resize(n); return hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost); }

// the device Track of a host-built one (car_dynamics.h: TrackHost, which mpopis_set_track uploads too): its four buffers, and the view over them
template <class TrackHost, class Track> static hipError_t dtrack(Track* tk, const TrackHost& th) {
    double *d, *dnd, *dring; int* dni;
    hipError_t e;
    if ((e = dupv(&d, th.xy)) != hipSuccess || (e = dupv(&dnd, th.nd)) != hipSuccess || (e = dupv(&dni, th.ni)) != hipSuccess || (e = dupv(&dring, th.ring)) != hipSuccess) return e;
    *tk = th.view(d, dni, dnd, dring);
    return hipSuccess;
}

// one output of a launch: `count` entries of `type` at dev, written with its guard entries unless !guarded (a workspace handed back as it is);
// dev == nullptr: the launch was not given this buffer, written as count 0
struct Out { long long type; size_t count; const void* dev; bool guarded = true; };

// fetches every output and writes { hdr, the arrays } to f; 0, 1 (a HIP error, printed) or 2 (the write failed, printed)
inline int write_back(FILE* f, const long long* hdr, size_t nhdr, const std::vector<Out>& outs) {
    std::vector<std::vector<char>> host(outs.size());
    std::vector<HostArr> arrays;
    for (size_t i = 0; i < outs.size(); ++i) {
        const Out& o = outs[i];
        const size_t cnt = o.dev ? o.count + (o.guarded ? kGuard : 0) : 0;
        host[i].resize(cnt * tsize(o.type));
        if (!host[i].empty()) CK(hipMemcpy(host[i].data(), o.dev, host[i].size(), hipMemcpyDeviceToHost));
        arrays.push_back({o.type, cnt, host[i].data()});
    }
    if (!write_arrays(f, hdr, nhdr, arrays)) BAD("write failed");
    return 0;
}
