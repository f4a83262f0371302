// The transfer layer: every copy between host and device memory, and between device buffers, is one of the functions below
// (common.h includes this file; nothing else in csrc calls the runtime's copy functions, but for the exported
// saamge_amd_memcpy of capi.hip, a primitive with an error convention of its own).  DESIGN.md section 7.0 states the rule.
//
//   host -> device   upload            allocate-or-fill, staged where the rule asks for it, complete on return: the source may die
//                    upload_async      enqueue only: a page-locked hvec, or a source below the staging threshold that outlives the copy
//   device -> host   fetch_host / DBuf::to_host / read_back / read_one   into the library's own memory, complete on return
//                    download          enqueue only, into a page-locked hvec; the caller synchronises
//                    copy_to_caller    into a getter's output (host or device pointer): direct, complete on return
//   device -> device copy_device       enqueue only
//   an argument that may be a host or a device pointer: DevIn (input), DevOut (output, or in/out with `load`)
#pragma once
// (included by common.h, ahead of DBuf)

namespace saamge_amd {

template <class T>
struct DBuf;

// ---- pinned host memory: pooled allocator for the big host-side tables -----------------
// Pageable <-> device copies run at a few GB/s; page-locked ones at PCIe speed.  hipHostMalloc
// itself is slow (it pins pages), so freed blocks are kept in a size-class pool and reused
// by the next level / hierarchy.
void *pinned_alloc(size_t bytes);
void pinned_free(void *p, size_t bytes);
void pinned_pool_release();

template <class T>
struct PinnedAlloc {
    typedef T value_type;
    PinnedAlloc() {}
    template <class U>
    PinnedAlloc(const PinnedAlloc<U> &) {}
    T *allocate(size_t n) { return (T *)pinned_alloc(n * sizeof(T)); }
    void deallocate(T *p, size_t n) { pinned_free((void *)p, n * sizeof(T)); }
    template <class U>
    bool operator==(const PinnedAlloc<U> &) const { return true; }
    template <class U>
    bool operator!=(const PinnedAlloc<U> &) const { return false; }
};
template <class T>
using hvec = std::vector<T, PinnedAlloc<T>>;


// The staging rule.  A pageable source of STAGE_MIN_BYTES or more is copied into a page-locked block of the library's own
// (the pinned pool, never returned to the system while in use) and sent from there: handed over as it is, the runtime
// registers the caller's pages with the GPU for the transfer and keeps the registration cached -- pages that go back to the
// kernel when the source dies (host_heap_policy, runtime.hip).  Smaller sources the runtime copies through its own buffers.
// The pinned pool (runtime.hip) starts at the same number: a smaller request of pinned_alloc is plain malloc, so an hvec
// below it is pageable memory that needs no staging either.
constexpr size_t STAGE_MIN_BYTES = 256u << 10;

namespace xfer_detail {
inline void copy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    SA_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, kind, s));
    SA_HIP_CHECK(hipStreamSynchronize(s));
}
// what the caller knows of a source: nothing (looked up once, here), that it is host memory, or that it is an hvec (page-locked)
enum class Src { unknown, host, pinned };
inline void upload_bytes(void *dst, const void *src, size_t bytes, Src kind, hipStream_t s) {
    if (!bytes) return;
    if (kind != Src::pinned && bytes >= STAGE_MIN_BYTES && (kind == Src::host || !is_device_ptr(src))) {
        void *stage = pinned_alloc(bytes);
        std::memcpy(stage, src, bytes);
        const hipError_t e = hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, s);
        const hipError_t e2 = hipStreamSynchronize(s);
        pinned_free(stage, bytes);
        SA_HIP_CHECK(e);
        SA_HIP_CHECK(e2);
        return;
    }
    copy_sync(dst, src, bytes, kind == Src::unknown ? hipMemcpyDefault : hipMemcpyHostToDevice, s);
}
template <class V>
constexpr bool is_hvec() { return std::is_same<typename V::allocator_type, PinnedAlloc<typename V::value_type>>::value; }
}  // namespace xfer_detail

// ---- host (or device) to device, complete on return ---------------------------------------------------------------------------
// n values from src -- pageable, page-locked or device memory -- into device memory that exists
template <class T>
inline void upload(T *dst, const T *src, size_t n, hipStream_t s) { xfer_detail::upload_bytes(dst, src, n * sizeof(T), xfer_detail::Src::unknown, s); }
// ... into a buffer allocated for them
template <class T>
inline void upload(DBuf<T> &dst, const T *src, size_t n, hipStream_t s) {
    dst.alloc(n);
    upload(dst.p, src, n, s);
}
// ... from a host vector; an hvec is known to be page-locked
template <class T, class V>
inline void upload(DBuf<T> &dst, const V &v, hipStream_t s) {
    static_assert(sizeof(typename V::value_type) == sizeof(T), "upload: element sizes differ");
    dst.alloc(v.size());
    xfer_detail::upload_bytes(dst.p, v.data(), v.size() * sizeof(T), xfer_detail::is_hvec<V>() ? xfer_detail::Src::pinned : xfer_detail::Src::host, s);
}

// ---- host to device, enqueue only: the source must stay as it is until the stream has passed the copy ------------------------
template <class T>
inline void upload_async(T *dst, const hvec<T> &src, size_t n, hipStream_t s) {
    SA_REQUIRE(n <= src.size(), "upload_async: more values than the vector holds");
    if (n) SA_HIP_CHECK(hipMemcpyAsync(dst, src.data(), n * sizeof(T), hipMemcpyHostToDevice, s));
}
// a small table (a few words of launch state); at the staging threshold and above only upload() or an hvec will do
template <class T>
inline void upload_async(T *dst, const T *src, size_t n, hipStream_t s) {
    SA_REQUIRE(n * sizeof(T) < STAGE_MIN_BYTES, "upload_async: a source of the staging threshold or more must be an hvec");
    if (n) SA_HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, s));
}

// ---- device to host, into the library's own memory ---------------------------------------------------------------------------
// Fetch an input array (host or device pointer) to the host (for host-side topology).
template <class T>
inline hvec<T> fetch_host(const T *src, size_t n, hipStream_t s) {
    hvec<T> v(n);
    if (n) xfer_detail::copy_sync(v.data(), src, n * sizeof(T), hipMemcpyDefault, s);
    return v;
}
// n values of device memory into a host vector (resized).  Only enqueues the copy: callers batch several under one
// synchronise of their own.
template <class T>
inline void download(hvec<T> &dst, const T *src, size_t n, hipStream_t s) {
    dst.resize(n);
    if (n) SA_HIP_CHECK(hipMemcpyAsync(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, s));
}
template <class T>
inline void download(hvec<T> &dst, const DBuf<T> &src, size_t n, hipStream_t s) { download(dst, (const T *)src.p, n, s); }
// n values from the device in one transfer (synchronises the stream)
template <class T>
inline void read_back(T *dst, const T *src, size_t n, hipStream_t s) {
    if (n) xfer_detail::copy_sync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, s);
}
// one value from the device (synchronises the stream)
template <class T>
inline T read_one(const T *p, hipStream_t s) {
    T v;
    read_back(&v, p, 1, s);
    return v;
}

// ---- device to the caller's memory: a getter's output, host or device pointer ------------------------------------------------
// Direct (not staged: a getter may move gigabytes, and the pinned pool keeps what it once handed out) and complete on return.
// A null dst is an output the caller did not ask for.
template <class T>
inline void copy_to_caller(T *dst, const T *src, size_t n, hipStream_t s) {
    if (dst && n) xfer_detail::copy_sync(dst, src, n * sizeof(T), hipMemcpyDefault, s);
}
template <class T>
inline void copy_to_caller(T *dst, const DBuf<T> &src, hipStream_t s) { copy_to_caller(dst, (const T *)src.p, src.n, s); }

// ---- device to device, enqueue only (the ranges do not overlap) ---------------------------------------------------------------
template <class T>
inline void copy_device(T *dst, const T *src, size_t n, hipStream_t s) {
    if (n) SA_HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToDevice, s));
}

// ---- an argument that may be a host or a device pointer ------------------------------------------------------------------------
// Input of n values: a device pointer is used where it is, a host array is uploaded once.  buf is the view or the copy.
template <class T>
struct DevIn {
    DBuf<T> buf;
    const T *p = nullptr;
    bool on_device = false;      // the one classification of the pointer
    DevIn() {}
    DevIn(const T *src, size_t n, hipStream_t s) { bind(src, n, s); }
    const T *bind(const T *src, size_t n, hipStream_t s) {
        on_device = is_device_ptr(src);
        if (!src) buf.release();
        else if (on_device) buf.view(const_cast<T *>(src), n);
        else {
            buf.alloc(n);
            xfer_detail::upload_bytes(buf.p, src, n * sizeof(T), xfer_detail::Src::host, s);
        }
        return p = buf.p;
    }
    // for a handle that keeps the array
    DBuf<T> take() { p = nullptr; return std::move(buf); }
};
// Output of n values: the kernels write to p, finish() brings a host array home and returns with the stream idle.
// load: the kernels read or add to what the array holds, so a host array is brought along.
template <class T>
struct DevOut {
    DBuf<T> hold;
    T *p = nullptr, *host = nullptr;
    size_t n = 0;
    hipStream_t s = nullptr;
    bool bound = false;      // finish() of an output that was never bound does nothing
    DevOut() {}
    DevOut(T *dst, size_t n_, hipStream_t s_, bool load) { bind(dst, n_, s_, load); }
    T *bind(T *dst, size_t n_, hipStream_t s_, bool load) {
        n = n_; s = s_; host = nullptr; bound = true;
        if (!dst || is_device_ptr(dst)) return p = dst;
        host = dst;
        hold.alloc(n);
        if (load) xfer_detail::upload_bytes(hold.p, dst, n * sizeof(T), xfer_detail::Src::host, s);
        return p = hold.p;
    }
    void finish() {
        if (!bound) return;
        if (host && n) SA_HIP_CHECK(hipMemcpyAsync(host, hold.p, n * sizeof(T), hipMemcpyDeviceToHost, s));      // (as copy_to_caller)
        SA_HIP_CHECK(hipStreamSynchronize(s));
    }
};

}  // namespace saamge_amd
