// Shared host-side utilities for the saamge_amd HIP library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <stdexcept>
#include <string>
#include <vector>

namespace saamge_amd {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

#define SA_HIP_CHECK(expr)                                                              \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            throw ::saamge_amd::Error(2, std::string(__FILE__) + ":" +                  \
                                             std::to_string(__LINE__) + " " + #expr +   \
                                             " -> " + hipGetErrorString(e_));           \
    } while (0)

// The reference aborts through SA_ASSERT (amg/inc/common.hpp:635-647); we throw and
// translate to an error code at the C ABI.
#define SA_REQUIRE(cond, msg)                                                           \
    do {                                                                                \
        if (!(cond))                                                                    \
            throw ::saamge_amd::Error(1, std::string(__FILE__) + ":" +                  \
                                             std::to_string(__LINE__) + " " + (msg));   \
    } while (0)

// ---- device affinity of helper threads -------------------------------------------------
// HIP's current device is a per-host-thread property and defaults to device 0.  One process
// drives one GPU (rank r on device LOCAL_RANK), so every helper thread that may touch HIP
// (hipMalloc, copies, pinned allocations, launches) adopts the device of the thread that
// spawned it, and the helper streams are kept per device.
inline int current_device() {
    int d = 0;
    SA_HIP_CHECK(hipGetDevice(&d));
    return d;
}
inline void adopt_device(int dev) { SA_HIP_CHECK(hipSetDevice(dev)); }
// non-blocking helper stream number `slot` of the calling thread's current device
hipStream_t side_stream(int slot);

inline bool is_device_ptr(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // clear: plain host memory reports an error
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

}  // namespace saamge_amd
#include "xfer.h"      // the pinned host pool, hvec, and the transfer layer: every host <-> device and device <-> device copy
namespace saamge_amd {

// ---- process-wide diagnostics and the host heap policy (runtime.hip) ----------------------
// Applied once, with the host_heap_pad_mb of the first hierarchy of the process (capi.hip): see Options::host_heap_pad_mb
// and DESIGN.md section 7.0.
void host_heap_policy(int mb);
bool env_timing();      // SAAMGE_AMD_TIMING
bool env_timing_host(); // SAAMGE_AMD_TIMING=host
bool env_serial();      // SAAMGE_AMD_SERIAL: no worker threads in the setup (counter passes)

// ---- device memory: caching allocator behind every DBuf -----------------------------------
// hipMalloc costs 10 us - 1 ms and hipFree additionally waits for the whole device, which stalls the
// host between setup kernels and serialises streams that are meant to overlap.  Freed blocks are kept
// and handed out again: at once to the stream that freed them (stream order makes that safe), to any
// other stream once the event recorded at the free has completed.  The freeing stream is the calling
// thread's `thread_stream()` (set by every API entry and every worker thread); a thread without one
// frees through hipFree as before.  Idle blocks beyond SAAMGE_AMD_POOL_MAX_GB (default 64) are returned
// to the driver, all of them by dev_pool_release() or when a hipMalloc fails.
void set_thread_stream(hipStream_t s);
void unset_thread_stream();      // the thread frees through hipFree again (its stream may be destroyed next)
hipStream_t thread_stream();
bool thread_stream_is_set();
void *dev_alloc(size_t bytes);
void dev_free(void *p) noexcept;
void dev_pool_release();
size_t dev_pool_idle_bytes();
// device bytes the library holds in DBufs right now and their high-water mark since the last reset
void dev_memory_stats(size_t *live, size_t *peak, bool reset_peak);
// requests of the pool that went to the driver since the last reset (hipMalloc calls and their bytes, hipFree of cached blocks)
void dev_pool_counts(long *n_malloc, long *n_free, size_t *malloc_bytes, bool reset);
struct ThreadStreamScope {       // the calling thread's stream for a scope (restored at its end)
    hipStream_t prev;
    bool had;
    explicit ThreadStreamScope(hipStream_t s) : prev(thread_stream()), had(thread_stream_is_set()) { set_thread_stream(s); }
    ~ThreadStreamScope() { if (had) set_thread_stream(prev); else unset_thread_stream(); }
};
// Close the batch of frees `s` is filling NOW (its event is recorded while the stream is certainly alive) -- called
// when a hierarchy is destroyed: its caller may destroy the stream next, and an open batch would later record its
// event on a dead handle.
void dev_pool_close_stream(hipStream_t s);

// RAII device buffer.  What fills and reads it is in xfer.h.
template <class T>
struct DBuf {
    T *p = nullptr;
    size_t n = 0;
    bool owned = true;
    DBuf() {}
    explicit DBuf(size_t n_) { alloc(n_); }
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    DBuf(DBuf &&o) noexcept : p(o.p), n(o.n), owned(o.owned) { o.p = nullptr; o.n = 0; }
    DBuf &operator=(DBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p; n = o.n; owned = o.owned;
            o.p = nullptr; o.n = 0;
        }
        return *this;
    }
    ~DBuf() { release(); }
    void release() {
        if (p && owned) dev_free(p);
        p = nullptr; n = 0; owned = true;
    }
    void alloc(size_t n_) {
        release();
        n = n_;
        if (n) p = (T *)dev_alloc(n * sizeof(T));
    }
    void zero(hipStream_t s = 0) {
        if (n) SA_HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(T), s));
    }
    // a copy of n values at a host OR device pointer, of a host vector; back as a host vector.  All complete on return (xfer.h).
    void assign(const T *src, size_t n_, hipStream_t s = 0) { upload(*this, src, n_, s); }
    template <class V>
    void from_host(const V &v, hipStream_t s = 0) { upload(*this, v, s); }
    hvec<T> to_host(hipStream_t s = 0) const { return fetch_host((const T *)p, n, s); }
    // non-owning view of an existing device pointer
    void view(T *ptr, size_t n_) {
        release();
        p = ptr; n = n_; owned = false;
    }
};

// Row offsets of every CSR / SELL operator are 64-bit: column indices and dimensions are int32 like the
// reference's hypre/MFEM types, but the stored entries of one operator may exceed 2^31 (Q2 elasticity at
// 96^3: 4.2e9) -- the reference splits such an operator over MPI ranks, here one GPU holds it.
typedef int64_t roff_t;

}  // namespace saamge_amd
#include "sell.h"      // struct Sell, SELL_*: the SELL-64 copy of a DCsr
namespace saamge_amd {
// Device CSR matrix.
struct DCsr {
    int nrows = 0, ncols = 0;
    int64_t nnz = 0;
    DBuf<roff_t> rowptr;
    DBuf<int> col;
    DBuf<double> val;
    int lanes_per_row = 8;  // SpMV launch shape, chosen from the average row length
    mutable int max_row = -1;  // longest row (computed on first use by the fused AE assembly)
    Sell sell;  // optional SELL-64 copy for the SpMV family (sell.h)
};

// Row offsets crossing the C ABI (sparse.hip).  In: int32 (the reference's HYPRE_Int; widened on the device)
// or int64 (device pointers viewed in place); host or device pointer either way.  Out: narrowed to int32 for
// the callers of the 32-bit getters (an operator beyond 2^31 entries is an error there).
void import_rowptr(DBuf<roff_t> &dst, const void *src, int bits, size_t n, hipStream_t s);
void export_rowptr32(int *dst_host, const DBuf<roff_t> &src, size_t n, hipStream_t s);

inline int pick_lanes_per_row(int64_t nnz, int nrows) {
    double avg = nrows ? double(nnz) / nrows : 1.0;
    int l = 1;
    while (l < 64 && l * 2 <= avg * 0.75 + 1.0) l *= 2;  // ~ half-full last pass at worst
    return l;
}

inline int div_up(int64_t a, int64_t b) { return int((a + b - 1) / b); }
// the grid of a kernel with one lane per item and 256 lanes per workgroup (one workgroup for no items: the launch stays valid)
inline dim3 grid_flat(long n) { return dim3((unsigned)(n > 256 ? (n + 255) / 256 : 1)); }
// Home slot of `key` in an open-addressing table of `size` slots (a power of two >= 2): the HIGH bits of the multiplicative
// hash.  (Until round 4 the tables took the low bits, which are a permutation of the key's own low bits: the dofs of a box
// of a lexicographically numbered grid -- x + 257 y + 66049 z -- collide in lattices, 4.2 probes per look-up instead of 1.0
// for the 405 dofs of the headline's agglomerates in 1 024 slots.)
__host__ __device__ inline unsigned hash_home(unsigned key, unsigned size) {
    return (key * 2654435761u) >> (__builtin_clz(size) + 1);
}

// ---- optional per-kernel timing (bench.py's roofline leg) -------------------------
struct KernelStat {
    std::string name;
    double ms = 0.0;
    int64_t launches = 0;
    double bytes = 0.0;  // ALGORITHMIC bytes summed over launches (the CSR stream of the reference)
    double flops = 0.0;  // ALGORITHMIC flops summed over launches
    double fmt_bytes = 0.0;  // bytes the kernel has to move IN THE FORMAT IT RUNS (coded SELL slices, tables, vectors); 0: same as bytes
};

struct Profiler {
    bool enabled = false;
    std::vector<KernelStat> stats;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int level_tag = 0;  // Options::debug bit 2: setup kernels of level l > 0 are listed as name@Ll
    KernelStat &get(const std::string &name) {
        for (auto &s : stats)
            if (s.name == name) return s;
        stats.push_back(KernelStat());
        stats.back().name = name;
        return stats.back();
    }
    void begin(hipStream_t s) {
        if (!enabled) return;
        if (!e0) {
            SA_HIP_CHECK(hipEventCreate(&e0));
            SA_HIP_CHECK(hipEventCreate(&e1));
        }
        SA_HIP_CHECK(hipEventRecord(e0, s));
    }
    // count: the applications this one timing covers (a block launch on k columns is listed as k applications under the
    // single-vector label, with the bytes and flops of all of them)
    void end(hipStream_t s, const char *name, double bytes, double flops, double fmt_bytes = 0.0, int count = 1) {
        if (!enabled) return;
        SA_HIP_CHECK(hipEventRecord(e1, s));
        SA_HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        SA_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        KernelStat &k = level_tag > 0 ? get(std::string(name) + "@L" + std::to_string(level_tag)) : get(name);
        k.ms += ms;
        k.launches += count;
        k.bytes += bytes;
        k.flops += flops;
        k.fmt_bytes += fmt_bytes > 0.0 ? fmt_bytes : bytes;
    }
};

Profiler &profiler();

}  // namespace saamge_amd
