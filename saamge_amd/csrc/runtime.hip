// The process runtime: pinned host pool, caching device allocator, the calling thread's stream, helper streams,
// the diagnostic environment switches, the host heap policy and the kernel profiler (declared in common.h).
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <malloc.h>
#include <map>
#include <mutex>
#include <unordered_map>

namespace saamge_amd {

// ---------------------------------------------------------------------------------------
// pinned host memory pool
// ---------------------------------------------------------------------------------------
namespace {
std::mutex g_pin_mu;
std::multimap<size_t, void *> g_pin_free;
constexpr size_t PIN_MIN = STAGE_MIN_BYTES;      // what is not staged is not pinned either (xfer.h)
size_t pin_class(size_t bytes) {
    size_t c = PIN_MIN;
    while (c < bytes) c <<= 1;
    return c;
}
}  // namespace

void *pinned_alloc(size_t bytes) {
    if (bytes == 0) return nullptr;
    if (bytes < PIN_MIN) return std::malloc(bytes);
    const size_t c = pin_class(bytes);
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pin_free.find(c);
        if (it != g_pin_free.end()) {
            void *p = it->second;
            g_pin_free.erase(it);
            return p;
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, c, hipHostMallocPortable) != hipSuccess || !p) {
        (void)hipGetLastError();
        throw std::bad_alloc();
    }
    return p;
}
void pinned_free(void *p, size_t bytes) {
    if (!p) return;
    if (bytes < PIN_MIN) {
        std::free(p);
        return;
    }
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pin_free.insert(std::make_pair(pin_class(bytes), p));
}
void pinned_pool_release() {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (auto &kv : g_pin_free) (void)hipHostFree(kv.second);
    g_pin_free.clear();
}

// ---------------------------------------------------------------------------------------
// device memory pool (see common.h)
// ---------------------------------------------------------------------------------------
namespace {
// Blocks freed on one stream share an EVENT PER BATCH instead of one each: the frees of a hierarchy teardown
// (hundreds of blocks) used to put hundreds of markers into the stream, and on some processes the first kernel
// after them started 10 - 30 ms late (GPU idle in the kernel trace).  A batch ("epoch") stays open while its
// stream keeps freeing; its event is recorded -- on the freeing stream, after everything submitted to it so far,
// hence after the work that preceded every free of the batch -- when the batch is full or when another stream
// first asks for one of its blocks.  The freeing stream itself reuses its blocks at once, without any event.
struct Epoch {
    hipEvent_t ev = nullptr;
    hipStream_t stream = nullptr;
    int dev = 0;
    int refs = 0;           // idle blocks that belong to the batch
    bool recorded = false;
};
struct IdleBlock {
    void *p;
    Epoch *ep;
};
constexpr int POOL_EPOCH_BLOCKS = 64;
struct DevPool {
    std::mutex mu;
    std::multimap<size_t, IdleBlock> idle;              // by size
    std::unordered_map<void *, size_t> live;            // blocks handed out -> size
    std::vector<hipEvent_t> events;                     // spare events
    std::map<std::pair<int, hipStream_t>, Epoch *> open;   // the batch each (device, stream) is filling
    size_t idle_bytes = 0, max_idle = 0;
    size_t live_bytes = 0, peak_bytes = 0;              // handed out now / high-water mark (dev_memory_stats)
    long n_malloc = 0, n_free = 0;                      // requests that went to the driver (dev_pool_counts)
    size_t malloc_bytes = 0;
    bool enabled = true;
    DevPool() {
        const char *e = std::getenv("SAAMGE_AMD_POOL_MAX_GB");
        const double gb = e ? std::atof(e) : 64.0;
        max_idle = (size_t)(gb * (double)(1ull << 30));
        enabled = gb > 0.0;
    }
};
DevPool &dev_pool() {
    static DevPool *p = new DevPool;      // never destroyed: static DBufs are released after main() returns
    return *p;
}
thread_local hipStream_t tl_stream = nullptr;
thread_local bool tl_stream_set = false;
inline size_t pool_round(size_t bytes) { return bytes <= (1u << 20) ? (bytes + 511) / 512 * 512 : (bytes + 65535) / 65536 * 65536; }
// pool lock held: one block leaves its batch; a recorded batch without blocks gives its event back
void epoch_unref(DevPool &P, Epoch *ep) {
    if (--ep->refs > 0 || !ep->recorded) return;
    P.events.push_back(ep->ev);
    delete ep;
}
// pool lock held: close the batch (record its event now) so that other streams can wait for it
bool epoch_record(DevPool &P, Epoch *ep) {
    if (ep->recorded) return true;
    if (hipEventRecord(ep->ev, ep->stream) != hipSuccess) { (void)hipGetLastError(); return false; }
    ep->recorded = true;
    auto it = P.open.find(std::make_pair(ep->dev, ep->stream));
    if (it != P.open.end() && it->second == ep) P.open.erase(it);
    return true;
}
// pool lock held: hipFree one idle block (hipFree waits for the device: whatever used the block is done)
std::multimap<size_t, IdleBlock>::iterator pool_drop_block(DevPool &P, std::multimap<size_t, IdleBlock>::iterator it) {
    (void)hipFree(it->second.p);
    ++P.n_free;
    Epoch *ep = it->second.ep;
    P.idle_bytes -= it->first;
    it = P.idle.erase(it);
    if (ep->refs == 1 && !ep->recorded) {      // the last block of an open batch: the batch goes with it
        auto o = P.open.find(std::make_pair(ep->dev, ep->stream));
        if (o != P.open.end() && o->second == ep) P.open.erase(o);
        ep->recorded = true;
    }
    epoch_unref(P, ep);
    return it;
}
// hipFree the idle blocks for which keep() is false; pool lock held
template <class F>
void pool_drop(DevPool &P, F keep) {
    for (auto it = P.idle.begin(); it != P.idle.end();) {
        if (keep(it)) { ++it; continue; }
        it = pool_drop_block(P, it);
    }
}
}  // namespace


static int timing_mode() {      // 0 off, 1 SAAMGE_AMD_TIMING set, 2 SAAMGE_AMD_TIMING=host
    static const int v = [] {
        const char *e = std::getenv("SAAMGE_AMD_TIMING");
        return !e ? 0 : (e[0] == 'h' ? 2 : 1);
    }();
    return v;
}
bool env_timing() { return timing_mode() == 1; }
// SAAMGE_AMD_TIMING=host: the phases' host times WITHOUT synchronising the stream at their ends
bool env_timing_host() { return timing_mode() == 2; }
// The setup builds some tens of MB of host tables per hierarchy in std::vectors, copies some of them to and from the device
// (where they are handed over as pageable memory the runtime registers the pages with the GPU for the transfer and keeps such
// registrations cached) and releases them with the hierarchy.  What glibc then does with the memory decides how the NEXT setup starts:
//  * from the heap, with the default trimming: the top of the heap goes back to the kernel at every release and is grown
//    again by the next hierarchy.  Unmapping pages the GPU driver still knows invalidates its registration, and the
//    process's queues are stopped and restored: the first kernel of the next setup starts ~20 ms late (GPU trace: the queue
//    idle with the kernel submitted; 127 -> 150-160 ms per setup in half of the processes -- those in which glibc's sliding
//    mmap threshold had moved the tables onto the heap);
//  * from anonymous mappings of their own (the threshold frozen at its initial 128 KB): mapped and unmapped at recurring
//    addresses under the runtime's registration cache -- measured once: GPU memory access faults;
//  * from a heap that is never trimmed: neither.  That is what this asks for, once per process: blocks up to glibc's
//    maximum of 32 MB from the heap, no trimming, the heap grown in steps of host_heap_pad_mb.
// MPI libraries with registration caches set the same three parameters for the same reason.  DESIGN.md section 7.0.
// The transfers themselves follow one rule (xfer.h): a host source of STAGE_MIN_BYTES or more that is not page-locked is
// staged through the pinned pool by every upload that completes on return; smaller sources, hvecs, device-to-host copies and
// copies into a caller's memory go directly; enqueue-only uploads take an hvec or less than STAGE_MIN_BYTES and nothing else.
// The cause of the faults measured above is not known.
void host_heap_policy(int mb) {
    static std::once_flag once;
    std::call_once(once, [mb] {
        if (mb <= 0) return;
        (void)mallopt(M_MMAP_THRESHOLD, 32 << 20);
        (void)mallopt(M_TRIM_THRESHOLD, 0x7ff00000);
        (void)mallopt(M_TOP_PAD, (int)std::min<long>((long)mb << 20, 0x7ff00000l));
    });
}
bool env_serial() {
    static const bool v = std::getenv("SAAMGE_AMD_SERIAL") != nullptr;
    return v;
}

void set_thread_stream(hipStream_t s) { tl_stream = s; tl_stream_set = true; }
void unset_thread_stream() { tl_stream = nullptr; tl_stream_set = false; }
hipStream_t thread_stream() { return tl_stream; }
bool thread_stream_is_set() { return tl_stream_set; }

void *dev_alloc(size_t bytes) {
    if (bytes == 0) return nullptr;
    DevPool &P = dev_pool();
    const size_t want = pool_round(bytes);
    const int dev = current_device();
    {
        std::lock_guard<std::mutex> lk(P.mu);
        // smallest idle block that fits without wasting more than an eighth; same stream, or idle for certain
        const size_t limit = want + want / 8 + 4096;
        for (auto it = P.idle.lower_bound(want); it != P.idle.end() && it->first <= limit; ++it) {
            Epoch *ep = it->second.ep;
            if (ep->dev != dev) continue;
            const bool same = tl_stream_set && ep->stream == tl_stream;
            if (!same) {
                if (!epoch_record(P, ep)) continue;
                if (hipEventQuery(ep->ev) != hipSuccess) { (void)hipGetLastError(); continue; }
            }
            void *p = it->second.p;
            P.live[p] = it->first;
            P.live_bytes += it->first;
            P.peak_bytes = std::max(P.peak_bytes, P.live_bytes);
            P.idle_bytes -= it->first;
            P.idle.erase(it);
            if (ep->refs == 1 && !ep->recorded) {      // an open batch that has just lost its last block stays open
                --ep->refs;
            } else {
                epoch_unref(P, ep);
            }
            return p;
        }
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {          // out of memory: give the cached blocks back and try once more
        (void)hipGetLastError();
        dev_pool_release();
        e = hipMalloc(&p, want);
    }
    if (e != hipSuccess) throw Error((int)e, std::string("hipMalloc of ") + std::to_string(want) + " bytes failed: " + hipGetErrorString(e));
    std::lock_guard<std::mutex> lk(P.mu);
    P.live[p] = want;
    P.live_bytes += want;
    P.peak_bytes = std::max(P.peak_bytes, P.live_bytes);
    ++P.n_malloc;
    P.malloc_bytes += want;
    return p;
}
void dev_pool_counts(long *n_malloc, long *n_free, size_t *malloc_bytes, bool reset) {
    DevPool &P = dev_pool();
    std::lock_guard<std::mutex> lk(P.mu);
    if (n_malloc) *n_malloc = P.n_malloc;
    if (n_free) *n_free = P.n_free;
    if (malloc_bytes) *malloc_bytes = P.malloc_bytes;
    if (reset) { P.n_malloc = P.n_free = 0; P.malloc_bytes = 0; }
}

void dev_free(void *p) noexcept {
    if (!p) return;
    DevPool &P = dev_pool();
    size_t size = 0;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        auto it = P.live.find(p);
        if (it != P.live.end()) { size = it->second; P.live.erase(it); P.live_bytes -= size; }
    }
    int dev = 0;
    if (!size || !P.enabled || !tl_stream_set || size > P.max_idle || hipGetDevice(&dev) != hipSuccess) {
        (void)hipFree(p);
        return;
    }
    std::lock_guard<std::mutex> lk(P.mu);
    Epoch *&cur = P.open[std::make_pair(dev, tl_stream)];
    if (!cur) {
        hipEvent_t ev = nullptr;
        if (!P.events.empty()) { ev = P.events.back(); P.events.pop_back(); }
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            P.open.erase(std::make_pair(dev, tl_stream));
            (void)hipFree(p);
            return;
        }
        cur = new Epoch;
        cur->ev = ev;
        cur->stream = tl_stream;
        cur->dev = dev;
    }
    Epoch *ep = cur;
    ++ep->refs;
    P.idle.insert(std::make_pair(size, IdleBlock{p, ep}));
    P.idle_bytes += size;
    if (ep->refs >= POOL_EPOCH_BLOCKS) (void)epoch_record(P, ep);     // (full: closed, the next free opens a new one)
    while (P.idle_bytes > P.max_idle && !P.idle.empty())       // over the cap: the largest blocks go back to the driver
        (void)pool_drop_block(P, std::prev(P.idle.end()));
}

void dev_pool_close_stream(hipStream_t s) {
    DevPool &P = dev_pool();
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(P.mu);
    auto it = P.open.find(std::make_pair(dev, s));
    if (it == P.open.end()) return;
    Epoch *ep = it->second;
    if (ep->refs == 0) {                  // an open batch without blocks: it just goes
        P.events.push_back(ep->ev);
        P.open.erase(it);
        delete ep;
        return;
    }
    if (!epoch_record(P, ep)) {           // (cannot record: wait for the stream instead, then the blocks are idle for certain)
        (void)hipStreamSynchronize(s);
        ep->recorded = true;
        P.open.erase(it);
    }
}

void dev_pool_release() {
    DevPool &P = dev_pool();
    std::lock_guard<std::mutex> lk(P.mu);
    pool_drop(P, [](std::multimap<size_t, IdleBlock>::iterator) { return false; });
}

void dev_memory_stats(size_t *live, size_t *peak, bool reset_peak) {
    DevPool &P = dev_pool();
    std::lock_guard<std::mutex> lk(P.mu);
    if (live) *live = P.live_bytes;
    if (peak) *peak = P.peak_bytes;
    if (reset_peak) P.peak_bytes = P.live_bytes;
}

size_t dev_pool_idle_bytes() {
    DevPool &P = dev_pool();
    std::lock_guard<std::mutex> lk(P.mu);
    return P.idle_bytes;
}

hipStream_t side_stream(int slot) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, hipStream_t> streams;
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(mu);
    auto it = streams.find(std::make_pair(dev, slot));
    if (it != streams.end()) return it->second;
    hipStream_t s = nullptr;
    SA_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    streams[std::make_pair(dev, slot)] = s;
    return s;
}

Profiler &profiler() {
    static Profiler p;
    return p;
}

}  // namespace saamge_amd
