// Self-checking program of the transfer layer (csrc/xfer.h): every form of copy, at sizes around the staging threshold, against
// patterns written on the host or by a fill kernel here.  Prints one line per group and "xfer test ok" at the end; exits non-zero
// at the first mismatch with the case and the first differing index.  Every buffer is allocated at its full size and nothing is
// read or written past an end.  Built by csrc/Makefile next to the library:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Isaamge_amd/csrc tests/cxx/xfer_test.hip -Lsaamge_amd -lsaamge_amd
#include <cstdio>
#include <cstdlib>
#include <string>
#include <typeinfo>
#include <vector>

#include "common.h"

using namespace saamge_amd;

namespace {

[[noreturn]] void fail(const std::string &what, long index, double got, double want) {
    std::printf("xfer test FAILED: %s: index %ld: got %.17g, expected %.17g\n", what.c_str(), index, got, want);
    std::exit(1);
}
void expect(bool ok, const std::string &what) {
    if (!ok) fail(what, -1, 0.0, 1.0);
}

// value i of pattern k; fits a signed char
template <class T>
__host__ __device__ inline T pattern(size_t i, int k) { return (T)(int)((i * 7 + (size_t)k * 13) % 101) - (T)50; }
template <class T>
__global__ __launch_bounds__(256) void fill_kernel(size_t n, int k, T *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = pattern<T>(i, k);
}
template <class T>
__global__ __launch_bounds__(256) void add_one_kernel(size_t n, T *io) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) io[i] = io[i] + (T)1;
}
template <class T>
void device_fill(hipStream_t s, size_t n, int k, T *out) {
    if (!n) return;
    hipLaunchKernelGGL(fill_kernel<T>, grid_flat((long)n), dim3(256), 0, s, n, k, out);
    SA_HIP_CHECK(hipGetLastError());
}
template <class T>
void device_add_one(hipStream_t s, size_t n, T *io) {
    if (!n) return;
    hipLaunchKernelGGL(add_one_kernel<T>, grid_flat((long)n), dim3(256), 0, s, n, io);
    SA_HIP_CHECK(hipGetLastError());
}
template <class V>
void host_fill(V &v, int k) {
    for (size_t i = 0; i < v.size(); ++i) v[i] = pattern<typename V::value_type>(i, k);
}
// the host values p[0 .. n) against pattern k (+ add)
template <class T>
void expect_pattern(const std::string &what, const T *p, size_t n, int k, int add = 0) {
    for (size_t i = 0; i < n; ++i)
        if (p[i] != (T)(pattern<T>(i, k) + (T)add)) fail(what, (long)i, (double)p[i], (double)(pattern<T>(i, k) + (T)add));
}
// the device values, read back by the plainest form of the layer (itself checked against the fill kernel in device_to_host)
template <class T>
void expect_device(const std::string &what, hipStream_t s, const T *dev, size_t n, int k, int add = 0) {
    std::vector<T> h(n);
    read_back(h.data(), dev, n, s);
    expect_pattern(what, h.data(), n, k, add);
}

// the sizes in elements: 0, 1, threshold -/0/+ one element, 3 thresholds + 5 elements (no power-of-two class of the pinned pool)
template <class T>
std::vector<size_t> sizes() {
    const size_t t = STAGE_MIN_BYTES / sizeof(T);
    return {0, 1, t - 1, t, t + 1, 3 * t + 5};
}
template <class T>
std::string tag(const char *name, size_t n) { return std::string(name) + " <" + typeid(T).name() + "> n = " + std::to_string(n); }

// ---- sources: pageable vector, hvec and device buffer through every host-to-device form; the source is overwritten after the call
template <class T>
void sources(hipStream_t s) {
    for (size_t n : sizes<T>()) {
        std::vector<T> pageable(n);
        hvec<T> pinned(n);
        DBuf<T> dev(n), dst, into(n);
        // upload(DBuf, vector) and DBuf::from_host
        host_fill(pageable, 1);
        upload(dst, pageable, s);
        host_fill(pageable, 2);
        expect(dst.n == n, tag<T>("upload(DBuf, vector): size", n));
        expect_device(tag<T>("upload(DBuf, vector)", n), s, (const T *)dst.p, n, 1);
        dst.from_host(pageable, s);
        host_fill(pageable, 3);
        expect_device(tag<T>("DBuf::from_host(vector)", n), s, (const T *)dst.p, n, 2);
        host_fill(pinned, 4);
        upload(dst, pinned, s);
        host_fill(pinned, 5);
        expect_device(tag<T>("upload(DBuf, hvec)", n), s, (const T *)dst.p, n, 4);
        // upload(DBuf, pointer) and DBuf::assign: pageable, pinned, device
        upload(dst, (const T *)pageable.data(), n, s);
        host_fill(pageable, 6);
        expect_device(tag<T>("upload(DBuf, pageable pointer)", n), s, (const T *)dst.p, n, 3);
        dst.assign(pinned.data(), n, s);
        host_fill(pinned, 7);
        expect_device(tag<T>("DBuf::assign(pinned pointer)", n), s, (const T *)dst.p, n, 5);
        device_fill(s, n, 8, dev.p);
        upload(dst, (const T *)dev.p, n, s);
        device_fill(s, n, 9, dev.p);
        expect_device(tag<T>("upload(DBuf, device pointer)", n), s, (const T *)dst.p, n, 8);
        // upload into memory that exists: pageable, pinned, device
        upload(into.p, (const T *)pageable.data(), n, s);
        host_fill(pageable, 10);
        expect_device(tag<T>("upload(pointer, pageable pointer)", n), s, (const T *)into.p, n, 6);
        upload(into.p, (const T *)pinned.data(), n, s);
        host_fill(pinned, 11);
        expect_device(tag<T>("upload(pointer, pinned pointer)", n), s, (const T *)into.p, n, 7);
        upload(into.p, (const T *)dev.p, n, s);
        device_fill(s, n, 12, dev.p);
        expect_device(tag<T>("upload(pointer, device pointer)", n), s, (const T *)into.p, n, 9);
        // enqueue only from an hvec of any size: the source changes after the caller's synchronise
        upload_async(into.p, pinned, n, s);
        SA_HIP_CHECK(hipStreamSynchronize(s));
        host_fill(pinned, 13);
        expect_device(tag<T>("upload_async(hvec)", n), s, (const T *)into.p, n, 11);
    }
}

// ---- enqueue-only bounds: a pageable source below the threshold goes through, at and above it the call is refused
template <class T>
void enqueue_bounds(hipStream_t s) {
    for (size_t n : sizes<T>()) {
        std::vector<T> pageable(n);
        DBuf<T> into(n);
        host_fill(pageable, 1);
        device_fill(s, n, 2, into.p);
        bool refused = false;
        try {
            upload_async(into.p, (const T *)pageable.data(), n, s);
        } catch (const Error &) {
            refused = true;
        }
        SA_HIP_CHECK(hipStreamSynchronize(s));
        const bool small = n * sizeof(T) < STAGE_MIN_BYTES;
        expect(refused == !small, tag<T>(small ? "upload_async(pointer) refused a small source" : "upload_async(pointer) took a large source", n));
        expect_device(tag<T>("upload_async(pointer)", n), s, (const T *)into.p, n, small ? 1 : 2);      // a refusal copies nothing
    }
    hvec<T> two(2);
    DBuf<T> into(2);
    bool refused = false;
    try {
        upload_async(into.p, two, 3, s);
    } catch (const Error &) {
        refused = true;
    }
    expect(refused, std::string("upload_async(hvec) took more values than the vector holds"));
}

// ---- device to host: every form against what the fill kernel wrote
template <class T>
void device_to_host(hipStream_t s) {
    for (size_t n : sizes<T>()) {
        DBuf<T> dev(n);
        device_fill(s, n, 1, dev.p);
        const hvec<T> a = dev.to_host(s);
        expect(a.size() == n, tag<T>("DBuf::to_host: size", n));
        expect_pattern(tag<T>("DBuf::to_host", n), a.data(), n, 1);
        const hvec<T> b = fetch_host((const T *)dev.p, n, s);
        expect_pattern(tag<T>("fetch_host(device pointer)", n), b.data(), n, 1);
        std::vector<T> host(n);
        host_fill(host, 2);
        const hvec<T> c = fetch_host((const T *)host.data(), n, s);
        expect_pattern(tag<T>("fetch_host(host pointer)", n), c.data(), n, 2);
        hvec<T> d(3, (T)9);
        download(d, dev, n, s);
        SA_HIP_CHECK(hipStreamSynchronize(s));
        expect(d.size() == n, tag<T>("download(DBuf): size", n));
        expect_pattern(tag<T>("download(DBuf)", n), d.data(), n, 1);
        hvec<T> e;
        download(e, (const T *)dev.p, n, s);
        SA_HIP_CHECK(hipStreamSynchronize(s));
        expect_pattern(tag<T>("download(pointer)", n), e.data(), n, 1);
        std::vector<T> f(n);
        read_back(f.data(), (const T *)dev.p, n, s);
        expect_pattern(tag<T>("read_back", n), f.data(), n, 1);
        if (n) {
            expect(read_one((const T *)dev.p + (n - 1), s) == pattern<T>(n - 1, 1), tag<T>("read_one (last value)", n));
            expect(read_one((const T *)dev.p, s) == pattern<T>(0, 1), tag<T>("read_one (first value)", n));
        }
        // into a caller's memory: host array, device array, an output that was not asked for
        std::vector<T> caller(n);
        host_fill(caller, 3);
        copy_to_caller(caller.data(), (const T *)dev.p, n, s);
        expect_pattern(tag<T>("copy_to_caller(host pointer)", n), caller.data(), n, 1);
        DBuf<T> caller_dev(n);
        device_fill(s, n, 3, caller_dev.p);
        copy_to_caller(caller_dev.p, dev, s);
        expect_device(tag<T>("copy_to_caller(device pointer)", n), s, (const T *)caller_dev.p, n, 1);
        copy_to_caller((T *)nullptr, dev, s);
    }
}

// ---- the wrappers, with a host pointer and with a device pointer
template <class T>
void wrappers(hipStream_t s) {
    {      // a null pointer: no array, nothing on the device
        DevIn<T> in((const T *)nullptr, 0, s);
        expect(in.p == nullptr && !in.on_device, "DevIn(null)");
        in.bind((const T *)nullptr, 5, s);
        expect(in.p == nullptr, "DevIn::bind(null)");
        DevOut<T> out((T *)nullptr, 0, s, true);
        expect(out.p == nullptr, "DevOut(null)");
        out.finish();
        DevOut<T> never;
        never.finish();
    }
    for (size_t n : sizes<T>()) {
        std::vector<T> host(n);
        DBuf<T> dev(n);
        // input
        host_fill(host, 1);
        DevIn<T> in_h(host.data(), n, s);
        host_fill(host, 2);
        expect(!in_h.on_device && in_h.p == in_h.buf.p && (n == 0 || in_h.buf.owned), tag<T>("DevIn(host): a copy", n));
        expect_device(tag<T>("DevIn(host)", n), s, in_h.p, n, 1);
        device_fill(s, n, 3, dev.p);
        DevIn<T> in_d(dev.p, n, s);
        if (n) expect(in_d.on_device && in_d.p == dev.p && !in_d.buf.owned, tag<T>("DevIn(device): used where it is", n));
        DBuf<T> kept = in_d.take();
        expect(kept.p == dev.p && in_d.p == nullptr, tag<T>("DevIn::take", n));
        // output, load false: what the kernel wrote comes home
        host_fill(host, 4);
        DevOut<T> out_h(host.data(), n, s, false);
        if (n) expect(out_h.p != host.data() && out_h.p == out_h.hold.p, tag<T>("DevOut(host): a buffer", n));
        device_fill(s, n, 5, out_h.p);
        out_h.finish();
        expect_pattern(tag<T>("DevOut(host, load false)", n), host.data(), n, 5);
        DevOut<T> out_d(dev.p, n, s, false);
        if (n) expect(out_d.p == dev.p && !out_d.hold.p, tag<T>("DevOut(device): written where it is", n));
        device_fill(s, n, 6, out_d.p);
        out_d.finish();
        expect_device(tag<T>("DevOut(device, load false)", n), s, (const T *)dev.p, n, 6);
        // output, load true: the kernel sees what the array held
        host_fill(host, 7);
        DevOut<T> io_h(host.data(), n, s, true);
        host_fill(host, 8);      // (the load is complete: this is overwritten by finish)
        device_add_one(s, n, io_h.p);
        io_h.finish();
        expect_pattern(tag<T>("DevOut(host, load true)", n), host.data(), n, 7, 1);
        device_fill(s, n, 9, dev.p);
        DevOut<T> io_d(dev.p, n, s, true);
        device_add_one(s, n, io_d.p);
        io_d.finish();
        expect_device(tag<T>("DevOut(device, load true)", n), s, (const T *)dev.p, n, 9, 1);
    }
}

// ---- copy_device between two buffers, and between the two halves of one
template <class T>
void device_copies(hipStream_t s) {
    for (size_t n : sizes<T>()) {
        DBuf<T> a(n), b(n), both(2 * n);
        device_fill(s, n, 1, a.p);
        device_fill(s, n, 2, b.p);
        copy_device(b.p, (const T *)a.p, n, s);
        expect_device(tag<T>("copy_device", n), s, (const T *)b.p, n, 1);
        expect_device(tag<T>("copy_device: the source", n), s, (const T *)a.p, n, 1);
        device_fill(s, n, 3, both.p);
        device_fill(s, n, 4, both.p + n);
        copy_device(both.p + n, (const T *)both.p, n, s);
        expect_device(tag<T>("copy_device (upper half)", n), s, (const T *)both.p + n, n, 3);
        expect_device(tag<T>("copy_device (lower half)", n), s, (const T *)both.p, n, 3);
    }
}

template <class F>
void group(const char *name, F &&f) {
    f();
    std::printf("%s: ok\n", name);
    std::fflush(stdout);
}

}  // namespace

int main() {
    try {
        hipStream_t s;
        SA_HIP_CHECK(hipStreamCreate(&s));
        group("sources", [&] { sources<int>(s); sources<double>(s); sources<signed char>(s); });
        group("enqueue-only bounds", [&] { enqueue_bounds<int>(s); enqueue_bounds<double>(s); enqueue_bounds<signed char>(s); });
        group("device to host", [&] { device_to_host<int>(s); device_to_host<double>(s); device_to_host<signed char>(s); });
        group("wrappers", [&] { wrappers<int>(s); wrappers<double>(s); wrappers<signed char>(s); });
        group("copy_device", [&] { device_copies<int>(s); device_copies<double>(s); device_copies<signed char>(s); });
        SA_HIP_CHECK(hipStreamSynchronize(s));
        pinned_pool_release();      // (every hvec and staging block is idle by now)
        SA_HIP_CHECK(hipStreamDestroy(s));
    } catch (const std::exception &e) {
        std::printf("xfer test FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("xfer test ok\n");
    return 0;
}
