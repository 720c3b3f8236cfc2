// api.hip -- C-ABI entry points of libseqwin_hip.so (see include/seqwin_hip.h for the contract and
// the reference interfaces each one replaces), device memory pool, batch upload / synthesis.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <memory>
#include <thread>

#include "device.hpp"

namespace sw {

static thread_local std::string g_last_error;
static thread_local uint64_t g_last_occ_cap = 0;
void set_last_error(const char *msg) { g_last_error = msg ? msg : ""; g_last_occ_cap = 0; }
void note_occ_cap(uint64_t n) { g_last_occ_cap = n; }
uint64_t last_occ_cap_n() { return g_last_occ_cap; }
uint64_t occ_cap()
{
    const char *e = SW_TEST_GETENV("SEQWIN_AMD_OCC_CAP");   // (read per call: a handful of times per build)
    const long long v = e ? atoll(e) : 0;
    return v > 0 && (uint64_t)v < 0xFFFFFFFEull ? (uint64_t)v : 0xFFFFFFFEull;
}
void raise_occ_cap(uint64_t n, const char *what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "more than %s %s on one device (%llu): use more devices (SEQWIN_DEVICES)", occ_cap() == 0xFFFFFFFEull ? "2^32-2" : "SEQWIN_AMD_OCC_CAP",
             what, (unsigned long long)n);
    throw OccCapError(n, buf);
}

// ---- caching allocator, stream-aware -----------------------------------------------------------------
// Blocks go back to the pool while work that uses them may still be queued, so every cached block remembers the stream
// context it was released under (the calling thread's StreamScope): the scope's main stream, and one event per forked
// side stream that was active at that moment (recorded at the release, so it covers exactly the work queued before it).
// A later dev_alloc under main stream T
//   * takes a block released under the same main stream as is (stream order covers the hand-over),
//   * for a block released under a different main stream S records an event on S now (S is in order, so the event
//     covers the block's last use) and lets T wait for it,
//   * lets T wait for the block's side-stream events.
// All waits are hipStreamWaitEvent: device-side ordering, the host never blocks.  Two host threads (or two torch
// streams) driving the same device with different streams therefore never see each other's blocks early, and blocks
// released while an exception unwinds past forked side-stream launches are fenced by those streams' events.
namespace {
struct FreeBlock {
    void *ptr = nullptr;
    hipStream_t main = nullptr;
    std::vector<std::pair<hipStream_t, hipEvent_t>> side;
};
struct Pool {
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, FreeBlock> free_blocks;  // (device, size) -> block
    std::map<void *, std::pair<int, size_t>> live;                 // ptr -> (device, size)
    std::map<int, std::vector<hipEvent_t>> spare_events;             // per device: an event is recorded on streams of the device it
                                                                   // was created on (hipEventRecord rejects it elsewhere: ADVICE r4)
    uint64_t total = 0;
};
Pool &pool()
{
    // intentionally leaked: handles may be released by Python finalizers after static destructors have run
    static Pool *p = new Pool;
    return *p;
}
size_t round_size(size_t b)
{
    if (b < 512) return 512;
    if (b < (1u << 20)) return (b + 511) & ~(size_t)511;
    return (b + ((1u << 20) - 1)) & ~(size_t)((1u << 20) - 1);
}
struct AllocCtx {
    hipStream_t main = nullptr;
    std::vector<hipStream_t> side;
};
thread_local AllocCtx g_alloc_ctx;

hipEvent_t take_event(Pool &p, int dev)   // p.mu held; dev = the calling thread's current device (where a new event is created)
{
    auto &spare = p.spare_events[dev];
    if (!spare.empty()) {
        hipEvent_t e = spare.back();
        spare.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);   // (an event belongs to the device that was current when it was made)
    const hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (cur != dev && cur >= 0) (void)hipSetDevice(cur);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return e;
}
}  // namespace

StreamScope::StreamScope(hipStream_t s) : prev_main(g_alloc_ctx.main), prev_side(std::move(g_alloc_ctx.side))
{
    g_alloc_ctx.main = s;
    g_alloc_ctx.side.clear();
}
StreamScope::~StreamScope()
{
    g_alloc_ctx.main = prev_main;
    g_alloc_ctx.side = std::move(prev_side);
}
void alloc_fork(hipStream_t side)
{
    for (hipStream_t s : g_alloc_ctx.side)
        if (s == side) return;
    g_alloc_ctx.side.push_back(side);
}
void alloc_join(hipStream_t side)
{
    auto &v = g_alloc_ctx.side;
    v.erase(std::remove(v.begin(), v.end(), side), v.end());
}

void release_resident_if_idle();   // (below: drops the parked index of the last sw_build unless a call is using it)

// ---- SEQWIN_AMD_POOL_DEBUG=1 (r06) ---------------------------------------------------------------------
// A debugging mode of the pool for soak runs of the multi-device path: EVERY release waits on the host for the whole device,
// fills the block with a poison pattern and caches it; EVERY reuse of a cached block waits for the device again and checks that
// the poison is intact.  A block written after its release -- by a kernel or copy that was still queued on some stream, of any
// thread -- is reported (stderr + the log callback, counted in sw_pool_debug_violations) with the first damaged offset, and the
// allocation fails.  Stream-order bugs cannot survive the device-wide waits, so: a fault that shows only WITHOUT this mode
// convicts the hand-over; a violation WITH it names a kernel that writes outside its buffers or after its stream was waited for.
namespace {
constexpr uint32_t POOL_POISON = 0xA5C3A5C3u;
std::atomic<uint64_t> g_pool_debug_violations{0}, g_pool_handover_syncs{0};
bool pool_debug()
{
    static const bool on = [] { const char *e = getenv("SEQWIN_AMD_POOL_DEBUG"); return e && atoi(e) != 0; }();
    return on;
}
__global__ void k_pool_check(const uint32_t *p, uint64_t n_words, uint32_t poison, unsigned long long *first_bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride)
        if (p[i] != poison) atomicMin(first_bad, (unsigned long long)i);
}
void pool_debug_poison(void *ptr, size_t sz)
{
    (void)hipDeviceSynchronize();
    if (hipMemsetD32Async((hipDeviceptr_t)ptr, (int)POOL_POISON, sz / 4, nullptr) != hipSuccess) (void)hipGetLastError();
    (void)hipStreamSynchronize(nullptr);
    // test hook: SEQWIN_AMD_FAULT_INJECT=pool writes one word into every 64th released block AFTER it was poisoned -- what a kernel
    // still queued at the release would do -- so that the suite can see the detector detect (tests/test_gpu_parity.py)
    static std::atomic<uint64_t> n_released{0};
    const char *inj = SW_TEST_GETENV("SEQWIN_AMD_FAULT_INJECT");
    if (inj && !strcmp(inj, "pool") && sz >= 4096 && n_released.fetch_add(1) % 64 == 63) {
        const uint32_t stray = 0xDEADBEEFu;
        (void)hipMemcpy((char *)ptr + 1024, &stray, 4, hipMemcpyHostToDevice);
    }
}
void pool_debug_check(void *ptr, size_t sz)   // raises if the block was written after pool_debug_poison
{
    (void)hipDeviceSynchronize();
    unsigned long long *d_bad = nullptr, bad = ~0ull;
    if (hipMalloc((void **)&d_bad, 8) != hipSuccess) { (void)hipGetLastError(); return; }
    (void)hipMemcpy(d_bad, &bad, 8, hipMemcpyHostToDevice);
    const uint64_t n_words = sz / 4;
    hipLaunchKernelGGL(k_pool_check, dim3((unsigned)std::min<uint64_t>((n_words + 255) / 256, 4096)), dim3(256), 0, nullptr, (const uint32_t *)ptr,
                       n_words, POOL_POISON, d_bad);
    (void)hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    if (bad != ~0ull) {
        ++g_pool_debug_violations;
        fprintf(stderr, "[seqwin_amd] POOL_DEBUG: block %p of %zu bytes was written AFTER its release (first damaged byte offset %llu)\n", ptr, sz,
                bad * 4);
        raise(SW_ERR_RUNTIME, "POOL_DEBUG: a cached device block of %zu bytes was written after its release (offset %llu)", sz, bad * 4);
    }
}
}  // namespace
uint64_t pool_debug_violations() { return g_pool_debug_violations.load(); }
uint64_t pool_handover_syncs() { return g_pool_handover_syncs.load(); }

void *dev_alloc(size_t bytes)
{
    Pool &p = pool();
    const size_t sz = round_size(bytes);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const hipStream_t T = g_alloc_ctx.main;
    {
        std::unique_lock<std::mutex> lock(p.mu);
        auto it = p.free_blocks.lower_bound(std::make_pair(dev, sz));
        if (it != p.free_blocks.end() && it->first.first == dev && it->first.second <= sz + sz / 4 + (1u << 20)) {
            FreeBlock blk = std::move(it->second);
            const size_t blk_size = it->first.second;
            p.live[blk.ptr] = it->first;
            p.free_blocks.erase(it);
            bool ok = true;
            if (pool_debug()) {   // (the block was poisoned behind a device-wide wait when it was released: no fence to carry over)
                for (auto &se : blk.side) p.spare_events[dev].push_back(se.second);
                lock.unlock();
                try {
                    pool_debug_check(blk.ptr, blk_size);
                } catch (...) {
                    dev_free(blk.ptr);
                    throw;
                }
                return blk.ptr;
            }
            if (blk.main != T) {
                ++g_pool_handover_syncs;   // (host-side hand-overs of this process: sw_pool_debug_stats; zero in single-stream builds)
                // Released under ANOTHER main stream -- another worker thread of a SEQWIN_DEVICES build, whose queued kernels may
                // still read the block.  Until r05 only T was made to wait for them; but the new owner also touches the block from
                // streams that are not T (the upload ring's DMA into a fresh d_packed, synchronous copies on the NULL stream), and
                // one multi-device fuzz campaign of r05 ended in a GPU memory fault with four processes sharing the card
                // (gpurun_out/r5al; not reproduced).  The hand-over between threads is now ordered on the HOST: the releasing
                // stream's work up to now, and that of its forked streams, has finished before the block is returned.  (Within one
                // thread -- every single-device build -- blk.main == T and nothing changes.)
                hipEvent_t e = take_event(p, dev);
                ok = e && hipEventRecord(e, blk.main) == hipSuccess;
                lock.unlock();
#ifdef SW_POOL_TEST_R04_HANDOVER   // (tests/tools/hip_mock: the hand-over as it was until r05 -- only T waits, on the device -- must
                                   //  show up as a data race in the choreography harness; never defined in a library build)
                if (ok) ok = hipStreamWaitEvent(T, e, 0) == hipSuccess;
                for (auto &se : blk.side)
                    if (ok && se.first != T) ok = hipStreamWaitEvent(T, se.second, 0) == hipSuccess;
#else
                if (ok) ok = hipEventSynchronize(e) == hipSuccess;
                for (auto &se : blk.side)
                    if (ok) ok = hipEventSynchronize(se.second) == hipSuccess;
#endif
                if (!ok) {
                    (void)hipGetLastError();
                    (void)hipDeviceSynchronize();
                }
                lock.lock();
                if (e) p.spare_events[dev].push_back(e);
                for (auto &se : blk.side) p.spare_events[dev].push_back(se.second);
                return blk.ptr;
            }
            for (auto &se : blk.side) {   // (a block's events belong to its device = dev: blocks are keyed by device)
                if (se.first != T && ok) ok = hipStreamWaitEvent(T, se.second, 0) == hipSuccess;
                p.spare_events[dev].push_back(se.second);
            }
            if (!ok) {   // could not order the hand-over on the device: order it on the host
                (void)hipGetLastError();
                lock.unlock();
                (void)hipDeviceSynchronize();
            }
            return blk.ptr;
        }
    }
    void *ptr = nullptr;
    hipError_t e = hipMalloc(&ptr, sz);
    // (r06: with the address -- the bimodal nodes stage is decided by where a process's first large blocks land, NOTES.md)
    if (getenv("SEQWIN_AMD_DEBUG_ALLOC") && sz >= (1ull << 28))
        fprintf(stderr, "[seqwin_amd] hipMalloc %.3f GiB at %p (offset in 2 MiB %llu KiB, in 1 GiB %llu MiB)\n", sz / 1073741824.0, ptr,
                (unsigned long long)(((uintptr_t)ptr >> 10) & 2047), (unsigned long long)(((uintptr_t)ptr >> 20) & 1023));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        dev_pool_trim();  // give cached blocks back and retry once
        e = hipMalloc(&ptr, sz);
    }
    if (e != hipSuccess) {   // the index a finished sw_build left resident is a convenience, not a claim on HBM
        (void)hipGetLastError();
        release_resident_if_idle();
        dev_pool_trim();
        e = hipMalloc(&ptr, sz);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        raise(SW_ERR_DEVICE, "hipMalloc of %zu bytes failed: %s", sz, hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lock(p.mu);
    p.live[ptr] = std::make_pair(dev, sz);
    p.total += sz;
    return ptr;
}

void dev_free(void *ptr)
{
    if (!ptr) return;
    Pool &p = pool();
    std::unique_lock<std::mutex> lock(p.mu);
    auto it = p.live.find(ptr);
    if (it == p.live.end()) return;
    const std::pair<int, size_t> key = it->second;
    p.live.erase(it);
    FreeBlock blk;
    blk.ptr = ptr;
    blk.main = g_alloc_ctx.main;
    bool ok = true;
    const int dev = key.first;                 // (the block's device: the releasing thread works on it, its side streams live there)
    for (hipStream_t s : g_alloc_ctx.side) {   // forked streams that may still use the block: fence them precisely, here
        hipEvent_t e = take_event(p, dev);
        if (!e || hipEventRecord(e, s) != hipSuccess) {
            (void)hipGetLastError();
            if (e) p.spare_events[dev].push_back(e);
            ok = false;
            break;
        }
        blk.side.emplace_back(s, e);
    }
    if (!ok) {   // no fence possible (runtime error state): do not cache the block; hipFree waits for the device
        for (auto &se : blk.side) p.spare_events[dev].push_back(se.second);
        p.total -= key.second;
        lock.unlock();
        (void)hipFree(ptr);
        return;
    }
    if (pool_debug()) {
        lock.unlock();
        pool_debug_poison(ptr, key.second);
        lock.lock();
    }
    p.free_blocks.emplace(key, std::move(blk));
}

void dev_pool_trim()
{
    Pool &p = pool();
    std::vector<std::pair<std::pair<int, size_t>, FreeBlock>> blocks;
    {
        std::lock_guard<std::mutex> lock(p.mu);
        for (auto &kv : p.free_blocks) blocks.emplace_back(kv.first, std::move(kv.second));
        p.free_blocks.clear();
        for (auto &b : blocks) {
            p.total -= b.first.second;
            for (auto &se : b.second.side) p.spare_events[b.first.first].push_back(se.second);
        }
    }
    for (auto &b : blocks) (void)hipFree(b.second.ptr);   // hipFree waits for outstanding work on the block's device
    (void)radix_trim_state();   // the radix passes' look-back state (0.27 GB per (device, stream) after a 745 M-element sort)
}

uint64_t dev_pool_bytes() { return pool().total; }

namespace {

void require_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        raise(SW_ERR_DEVICE,
              "no usable HIP device (hipGetDeviceCount: %s); libseqwin_hip has no CPU fallback",
              e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    }
}

// restores the calling thread's device on every way out of a scope that visits other devices
struct DeviceGuard {
    int home = 0;
    DeviceGuard() { SW_HIP(hipGetDevice(&home)); }
    ~DeviceGuard() { (void)hipSetDevice(home); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// Objects live on the device that was current when they were created; one process (or thread) per GPU is the model.
void require_current_device(int device, const char *what)
{
    int cur = -1;
    SW_HIP(hipGetDevice(&cur));
    if (cur != device)
        raise(SW_ERR_VALUE, "%s lives on device %d but the calling thread's current device is %d (sw_set_device)", what, device,
              cur);
}

// The arrays a caller hands in for results are usually fresh (np.empty): their pages are faulted in by the
// device-to-host copies, one page at a time on one thread.  Touching them from a few threads first takes most of
// that time away (18 -> ~8 ms for 280 MB on the target host).
struct HostSpan {
    void *p;
    size_t n;
    // expand != 0 (download only, r05): the source is a packed form that the copiers expand on the way to p --
    //   EXPAND_NODES: {hash u64, stop - start u32} (12 bytes) -> sw_node with start / stop from a running sum that begins at
    //                 chunk_base[chunk] (one entry per NODES_PER_CHUNK nodes) and zero n_tar / n_neg / penalty;
    //   EXPAND_EDGES: {first u64, second u64, weight u32} (20 bytes) -> sw_edge.
    // n stays the number of SOURCE bytes.
    int expand = 0;
    const uint64_t *chunk_base = nullptr;
};
enum { EXPAND_NODES = 1, EXPAND_EDGES = 2 };
constexpr size_t PACKED_NODE = 12, PACKED_EDGE = 20;
void prefault(const HostSpan *spans, int n_spans)
{
    size_t total = 0;
    for (int i = 0; i < n_spans; ++i) total += spans[i].p ? spans[i].n : 0;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned nt = total >= (32u << 20) ? std::min(8u, hw) : 1u;
    if (nt <= 1) return;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([=] {
            for (int i = 0; i < n_spans; ++i) {
                if (!spans[i].p) continue;
                const size_t lo = spans[i].n * t / nt, hi = spans[i].n * (t + 1) / nt;
                for (size_t o = lo; o < hi; o += 4096) ((volatile char *)spans[i].p)[o] = 0;
            }
        });
    for (auto &x : th) x.join();
}

// ---- pipelined download: result arrays leave the device through pinned slots, several host threads copy them on --------
// A plain hipMemcpy into pageable memory (the caller's numpy arrays) runs at ~24 GB/s on the target host (2.28 GB of
// arrays: 96 ms), bound by the one thread that empties the runtime's staging buffers.  Here the DMA engine fills a ring of
// pinned slots and DOWNLOAD_COPIERS threads copy the slots to their place (and fault the fresh pages in on the way).
struct DownloadRing {
    static constexpr size_t SLOT = 8u << 20;
    static constexpr int SLOTS = 8;
    char *base = nullptr;
    hipEvent_t ev[SLOTS];
    hipStream_t st = nullptr;
    std::mutex in_use;
};
DownloadRing &download_ring(int device)
{
    // intentionally leaked, one per device, made by the first large export (allocating pinned memory costs ~0.25 ms per MiB)
    static std::mutex mu;
    static std::map<int, DownloadRing *> *rings = new std::map<int, DownloadRing *>;
    std::lock_guard<std::mutex> lock(mu);
    auto it = rings->find(device);
    if (it != rings->end()) return *it->second;
    DownloadRing *r = new DownloadRing;
    SW_HIP(hipHostMalloc((void **)&r->base, DownloadRing::SLOT * DownloadRing::SLOTS, hipHostMallocDefault));
    SW_HIP(hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking));
    for (auto &e : r->ev) SW_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    (*rings)[device] = r;
    return *r;
}

// dst[i] (host, pageable) <- src[i] (current device), dst[i].n bytes each.  The device data must be complete (every producing
// stream synchronised) when this is called; it returns when the host arrays are.
// bytes of a slot that a chunk may fill (tests: SEQWIN_AMD_DOWNLOAD_SLOT_KB makes small graphs span many chunks)
size_t download_slot_bytes()
{
    size_t b = DownloadRing::SLOT;
    if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_DOWNLOAD_SLOT_KB")) b = std::min(b, (size_t)std::max(1, atoi(e)) << 10);
    return b;
}
size_t download_pipeline_min()
{
    size_t pipeline_min = 256u << 20;   // below: not worth the ring's one-off 16 ms of pinned allocation
    if (const char *e = SW_TEST_GETENV("SEQWIN_AMD_DOWNLOAD_PIPELINE_MB")) pipeline_min = (size_t)std::max(0, atoi(e)) << 20;   // (tests: 0)
    return pipeline_min;
}
// whether download() of `total` bytes goes through the ring (what a caller that offers packed sources has to know beforehand)
bool download_is_pipelined(size_t total) { return total > 0 && total >= download_pipeline_min() && !SW_TEST_GETENV("SEQWIN_AMD_PLAIN_DOWNLOAD"); }

void download(const HostSpan *dst, const void *const *src, int n_spans)
{
    const size_t pipeline_min = download_pipeline_min();
    size_t total = 0;   // bytes that arrive in the destination arrays (a packed source counts as what it expands to)
    for (int i = 0; i < n_spans; ++i) {
        if (!dst[i].p || !src[i]) continue;
        switch (dst[i].expand) {
        case EXPAND_NODES: total += dst[i].n / PACKED_NODE * sizeof(sw_node); break;
        case EXPAND_EDGES: total += dst[i].n / PACKED_EDGE * sizeof(sw_edge); break;
        default: total += dst[i].n;
        }
    }
    if (total == 0) return;
    for (int i = 0; i < n_spans; ++i)
        if (dst[i].p && src[i] && dst[i].expand && !download_is_pipelined(total))
            raise(SW_ERR_RUNTIME, "download: a packed source outside the pipelined route");   // (a caller's mistake)
    if (total < pipeline_min || SW_TEST_GETENV("SEQWIN_AMD_PLAIN_DOWNLOAD")) {
        prefault(dst, n_spans);
        for (int i = 0; i < n_spans; ++i)
            if (dst[i].p && src[i] && dst[i].n) SW_HIP(hipMemcpy(dst[i].p, src[i], dst[i].n, hipMemcpyDeviceToHost));
        return;
    }
    int dev = 0;
    SW_HIP(hipGetDevice(&dev));
    DownloadRing &ring = download_ring(dev);
    std::lock_guard<std::mutex> hold(ring.in_use);
    struct Chunk {
        char *dst;
        const char *src;
        size_t n;
        int expand;
        uint64_t base;
    };
    std::vector<Chunk> chunks;
    const size_t slot_bytes = download_slot_bytes();
    for (int i = 0; i < n_spans; ++i) {
        if (!dst[i].p || !src[i]) continue;
        if (dst[i].expand) {   // whole packed records per slot
            const size_t rec = dst[i].expand == EXPAND_NODES ? PACKED_NODE : PACKED_EDGE;
            const size_t out = dst[i].expand == EXPAND_NODES ? sizeof(sw_node) : sizeof(sw_edge);
            const size_t per = slot_bytes / rec * rec;
            for (size_t o = 0, c = 0; o < dst[i].n; o += per, ++c)
                chunks.push_back({(char *)dst[i].p + o / rec * out, (const char *)src[i] + o, std::min(per, dst[i].n - o), dst[i].expand,
                                  dst[i].expand == EXPAND_NODES ? dst[i].chunk_base[c] : 0});
            continue;
        }
        for (size_t o = 0; o < dst[i].n; o += slot_bytes)
            chunks.push_back({(char *)dst[i].p + o, (const char *)src[i] + o, std::min(slot_bytes, dst[i].n - o), 0, 0});
    }
    std::mutex mu;
    std::condition_variable cv;
    bool slot_busy[DownloadRing::SLOTS] = {false};
    std::deque<std::pair<int, size_t>> ready;   // (slot, chunk): the copy into the slot has been enqueued
    bool no_more = false;
    std::exception_ptr failure;
    // (measured on the target host, 2.28 GB: 68-74 ms = 31-34 GB/s with 4 ... 16 copiers, against 82-106 ms for one hipMemcpy per
    // array; two streams, a copy kernel writing the slots, and huge pages for the fresh arrays changed nothing: the DMA binds)
    const unsigned n_copiers = std::min(8u, std::max(2u, std::thread::hardware_concurrency()));
    auto copier = [&]() {
        (void)hipSetDevice(dev);
        for (;;) {
            std::pair<int, size_t> job;
            {
                std::unique_lock<std::mutex> lock(mu);
                cv.wait(lock, [&] { return !ready.empty() || no_more; });
                if (ready.empty()) return;
                job = ready.front();
                ready.pop_front();
            }
            const hipError_t e = hipEventSynchronize(ring.ev[job.first]);   // the slot holds the chunk
            const Chunk &c = chunks[job.second];
            if (e == hipSuccess) {
                const char *slot = ring.base + (size_t)job.first * DownloadRing::SLOT;
                if (c.expand == EXPAND_NODES) {
                    uint64_t start = c.base;
                    sw_node nd;
                    nd.n_tar = 0;
                    nd.n_neg = 0;
                    nd.penalty = 0.0;
                    for (size_t r = 0; r < c.n / PACKED_NODE; ++r) {
                        uint32_t cnt;
                        memcpy(&nd.hash, slot + r * PACKED_NODE, 8);
                        memcpy(&cnt, slot + r * PACKED_NODE + 8, 4);
                        nd.start = start;
                        start += cnt;
                        nd.stop = start;
                        memcpy(c.dst + r * sizeof(sw_node), &nd, sizeof(sw_node));
                    }
                } else if (c.expand == EXPAND_EDGES) {
                    for (size_t r = 0; r < c.n / PACKED_EDGE; ++r) {
                        sw_edge e;
                        uint32_t wgt;
                        memcpy(&e, slot + r * PACKED_EDGE, 16);
                        memcpy(&wgt, slot + r * PACKED_EDGE + 16, 4);
                        e.weight = wgt;
                        memcpy(c.dst + r * sizeof(sw_edge), &e, sizeof(sw_edge));
                    }
                } else {
                    memcpy(c.dst, slot, c.n);
                }
            }
            {
                std::lock_guard<std::mutex> lock(mu);
                if (e != hipSuccess && !failure)
                    failure = std::make_exception_ptr(Error(SW_ERR_RUNTIME, std::string("download: ") + hipGetErrorString(e)));
                slot_busy[job.first] = false;
            }
            cv.notify_all();
        }
    };
    std::vector<std::thread> th;
    try {
        for (unsigned t = 0; t < n_copiers; ++t) th.emplace_back(copier);
        for (size_t c = 0; c < chunks.size(); ++c) {
            const int s = (int)(c % DownloadRing::SLOTS);
            {
                std::unique_lock<std::mutex> lock(mu);
                cv.wait(lock, [&] { return !slot_busy[s]; });
                if (failure) break;
                slot_busy[s] = true;
            }
            hipStream_t q = ring.st;
            SW_HIP(hipMemcpyAsync(ring.base + (size_t)s * DownloadRing::SLOT, chunks[c].src, chunks[c].n, hipMemcpyDeviceToHost, q));
            SW_HIP(hipEventRecord(ring.ev[s], q));
            {
                std::lock_guard<std::mutex> lock(mu);
                ready.emplace_back(s, c);
            }
            cv.notify_all();
        }
    } catch (...) {
        std::lock_guard<std::mutex> lock(mu);
        if (!failure) failure = std::current_exception();
    }
    {
        std::lock_guard<std::mutex> lock(mu);
        no_more = true;
    }
    cv.notify_all();
    for (auto &t : th) t.join();
    (void)hipStreamSynchronize(ring.st);   // (nothing of this call is left in the ring's stream)
    if (failure) std::rethrow_exception(failure);
}

// Record tables of a HostBatch -> device.
void upload_tables(sw_batch &b)
{
    HostBatch &h = b.host;
    b.n_records = h.rec_len.size();
    b.d_rec_base.alloc(b.n_records);
    if (b.n_records)
        SW_HIP(hipMemcpy(b.d_rec_base.p, h.rec_base.data(), b.n_records * 8, hipMemcpyHostToDevice));
    std::vector<uint32_t> rec_asm(b.n_records);
    for (uint64_t a = 0; a < h.n_assemblies; ++a)
        for (uint32_t r = h.record_offsets[a]; r < h.record_offsets[a + 1]; ++r) rec_asm[r] = (uint32_t)a;
    b.d_rec_asm.alloc(b.n_records);
    if (b.n_records) SW_HIP(hipMemcpy(b.d_rec_asm.p, rec_asm.data(), b.n_records * 4, hipMemcpyHostToDevice));
}

// Upload a HostBatch whose packed chunks are still on the host; they are released afterwards (the rest of the
// host tables are kept for planning).
void upload_batch(sw_batch &b)
{
    HostBatch &h = b.host;
    b.packed_words = h.packed_words32();
    b.d_packed.alloc(b.packed_words);
    const uint64_t n_words64 = h.chunk_word0.empty() ? 0 : h.chunk_word0.back();
    SW_HIP(hipMemsetAsync(b.d_packed.p + 2 * n_words64, 0, 8 * 4, nullptr));   // the read slack
    for (size_t c = 0; c < h.chunks.size(); ++c)    // every assembly goes straight to its place in the stream
        if (!h.chunks[c].empty())
            SW_HIP(hipMemcpyAsync(b.d_packed.p + 2 * h.chunk_word0[c], h.chunks[c].data(), h.chunks[c].size() * 8,
                                  hipMemcpyHostToDevice, nullptr));
    SW_HIP(hipStreamSynchronize(nullptr));
    std::vector<WordBuf>().swap(h.chunks);
    upload_tables(b);
}

// ---- pipelined upload: packed chunks go to the device while later files are still being parsed ------------
// The ingest thread that owns the sink copies each finished chunk through a small ring of pinned slots
// (a plain memcpy into pinned memory + an asynchronous DMA: ~20 GB/s from one thread on the target host, where
// hipMemcpy from freshly written pageable memory manages ~2-3 GB/s because it pins pages on the fly).
struct PinnedRing {
    static constexpr size_t SLOT = 8u << 20;
    static constexpr int SLOTS = 4;
    char *base = nullptr;
    hipEvent_t ev[SLOTS];
    hipStream_t st = nullptr;
    std::mutex in_use;
    std::vector<hipEvent_t> spare;   // events for copies that do not go through a slot (DeviceSink::in_flight); under in_use
    hipEvent_t take_event()
    {
        if (!spare.empty()) {
            hipEvent_t e = spare.back();
            spare.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        SW_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return e;
    }
};
PinnedRing &pinned_ring(int device)
{
    // intentionally leaked, one per device (allocating pinned memory costs ~0.25 ms per MiB)
    static std::mutex mu;
    static std::map<int, PinnedRing *> *rings = new std::map<int, PinnedRing *>;
    std::lock_guard<std::mutex> lock(mu);
    auto it = rings->find(device);
    if (it != rings->end()) return *it->second;
    PinnedRing *r = new PinnedRing;
    SW_HIP(hipHostMalloc((void **)&r->base, PinnedRing::SLOT * PinnedRing::SLOTS, hipHostMallocDefault));
    SW_HIP(hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking));
    for (auto &e : r->ev) SW_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    (*rings)[device] = r;
    return *r;
}

// r05: the parsers' word buffers are page-locked blocks, so a finished assembly goes to HBM by DMA from where the packer wrote it --
// the sink thread no longer copies every packed word into the ring first (2.6 GB at 20 GB/s = 130 ms of one thread for 2 048
// genomes, the longest serial piece of the ingest; gpurun_out/r5z: with 64 parsers on the 16-CPU quota that thread fell behind
// to 450 ms).  One pool per process, leaked like the rings: slabs of 32 MiB cut into blocks of a multiple of 256 KiB, freed blocks
// handed out best-fit, at most SEQWIN_AMD_PINNED_POOL_MB (default 1024) in total -- beyond that get() declines, the parser
// mallocs and the sink takes the ring for that assembly.  SEQWIN_AMD_PINNED_POOL_MB=0: the ring for everything (r01-r05a).
struct PinnedArena : WordArena {
    static constexpr size_t GRAIN = 256u << 10;
    std::atomic<size_t> SLAB{32u << 20};   // (SEQWIN_AMD_PINNED_SLAB_MB: tests make blocks outgrow it)
    std::mutex mu;        // free list, bump pointer, totals
    std::mutex grow_mu;   // one thread page-locks a new slab at a time (the others wait for it rather than lock more memory)
    std::vector<std::pair<uint64_t *, size_t>> free_blocks;   // (block, capacity in words)
    char *slab = nullptr;
    size_t slab_left = 0;
    size_t total_bytes = 0;
    // (atomic: every ingest re-reads the settings while the sinks of other worker threads consult them -- found by ThreadSanitizer on
    //  the mock runtime, tests/tools/hip_mock, r06)
    std::atomic<size_t> limit_bytes{(size_t)1024 << 20};
    // The parsers are plain threads whose current device is 0: a slab is page-locked from the device of a sink that is at work (the
    // memory is portable, any of them will do) -- never a context on a GPU this process does not use.
    std::atomic<int> grow_device{0};
    // (SEQWIN_AMD_DEBUG_TIMING: what an ingest got from the arena)
    std::atomic<uint64_t> n_served{0}, n_declined_busy{0}, n_declined_limit{0}, n_slabs{0}, lock_us{0};
    void read_limit()   // (per ingest, so that one process can compare settings)
    {
        const char *e = getenv("SEQWIN_AMD_PINNED_POOL_MB"), *sl = SW_TEST_GETENV("SEQWIN_AMD_PINNED_SLAB_MB");
        std::lock_guard<std::mutex> lock(mu);
        limit_bytes = e ? (size_t)std::max(0, atoi(e)) << 20 : (size_t)1024 << 20;
        SLAB = sl ? (size_t)std::max(1, atoi(sl)) << 20 : (size_t)32 << 20;
    }
    // under mu: a block of the free list (best fit) or of the current slab
    uint64_t *take(size_t min_words, size_t bytes, size_t *cap_words)
    {
        size_t best = free_blocks.size();
        for (size_t i = 0; i < free_blocks.size(); ++i)
            if (free_blocks[i].second >= min_words && (best == free_blocks.size() || free_blocks[i].second < free_blocks[best].second)) best = i;
        if (best != free_blocks.size()) {
            const auto blk = free_blocks[best];
            free_blocks[best] = free_blocks.back();
            free_blocks.pop_back();
            *cap_words = blk.second;
            return blk.first;
        }
        if (bytes <= slab_left) {
            uint64_t *p = (uint64_t *)slab;
            slab += bytes;
            slab_left -= bytes;
            *cap_words = bytes / 8;
            return p;
        }
        return nullptr;
    }
    uint64_t *get(size_t min_words, size_t *cap_words) override
    {
        const size_t bytes = (min_words * 8 + GRAIN - 1) / GRAIN * GRAIN;
        {
            std::lock_guard<std::mutex> lock(mu);
            if (uint64_t *p = take(min_words, bytes, cap_words)) { ++n_served; return p; }
        }
        // Page-locking fresh memory costs 2-4 ms per MiB on the target host while the parsers keep its CPUs busy, in 2 MiB calls
        // from many threads as in one 64 MiB call (gpurun_out/r5aa, r5ab: the first streaming ingest of a process took 0.15-0.6 s
        // longer): whole slabs, by one thread at a time, and nobody waits for it -- while a slab is being locked the other parsers
        // get nullptr (malloc + the ring for that assembly, as before r05) and find blocks at their next file.
        std::unique_lock<std::mutex> grow(grow_mu, std::try_to_lock);
        if (!grow.owns_lock()) { ++n_declined_busy; return nullptr; }
        const size_t want = std::max(bytes, SLAB.load());
        {
            std::lock_guard<std::mutex> lock(mu);
            if (uint64_t *p = take(min_words, bytes, cap_words)) { ++n_served; return p; }   // (another thread has grown the pool meanwhile)
            if (total_bytes + want > limit_bytes) { ++n_declined_limit; return nullptr; }
            total_bytes += want;
        }
        void *fresh = nullptr;
        (void)hipSetDevice(grow_device.load());
        const auto t_lock = std::chrono::steady_clock::now();
        const hipError_t lock_err = hipHostMalloc(&fresh, want, hipHostMallocPortable);
        lock_us += (uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_lock).count();
        ++n_slabs;
        ++n_served;
        if (lock_err != hipSuccess) {
            (void)hipGetLastError();
            std::lock_guard<std::mutex> lock(mu);
            total_bytes -= want;
            return nullptr;
        }
        std::lock_guard<std::mutex> lock(mu);
        if (slab_left >= GRAIN) free_blocks.emplace_back((uint64_t *)slab, slab_left / 8);   // the old slab's tail stays usable
        slab = (char *)fresh + bytes;
        slab_left = want - bytes;
        *cap_words = bytes / 8;
        return (uint64_t *)fresh;
    }
    void put(uint64_t *p, size_t cap_words) override
    {
        std::lock_guard<std::mutex> lock(mu);
        free_blocks.emplace_back(p, cap_words);
    }
};
PinnedArena &pinned_arena()
{
    static PinnedArena *a = new PinnedArena;   // leaked on purpose (see pool())
    return *a;
}

struct DeviceSink : ChunkSink {
    sw_batch &b;
    PinnedRing &ring;
    std::unique_lock<std::mutex> hold;
    uint64_t cap32 = 0;     // capacity of b.d_packed in 32-bit words
    uint64_t used32 = 0;    // words written so far (a prefix)
    unsigned next_slot = 0;
    struct InFlight {
        WordBuf words;
        hipEvent_t ev;
    };
    std::deque<InFlight> in_flight;   // page-locked buffers whose copies are on their way, oldest first
    uint64_t n_direct = 0, n_ring = 0;
    static constexpr size_t IN_FLIGHT_MAX = 48;
    DeviceSink(sw_batch &batch, PinnedRing &r) : b(batch), ring(r), hold(r.in_use)
    {
        pinned_arena().read_limit();
        pinned_arena().grow_device.store(batch.device);
    }
    WordArena *arena() override { return pinned_arena().limit_bytes ? &pinned_arena() : nullptr; }
    void reap(bool all)
    {
        while (!in_flight.empty()) {
            InFlight &f = in_flight.front();
            if (all || in_flight.size() >= IN_FLIGHT_MAX) {
                SW_HIP(hipEventSynchronize(f.ev));
            } else {
                const hipError_t q = hipEventQuery(f.ev);
                if (q == hipErrorNotReady) break;
                SW_HIP(q);
            }
            ring.spare.push_back(f.ev);
            in_flight.pop_front();   // (the block goes back to the arena)
        }
    }
    void reserve(uint64_t words32)
    {
        if (words32 <= cap32) return;
        const uint64_t ncap = std::max(words32, cap32 + cap32 / 2);
        DevArray<uint32_t> bigger(ncap);
        SW_HIP(hipStreamSynchronize(ring.st));
        if (used32) SW_HIP(hipMemcpy(bigger.p, b.d_packed.p, used32 * 4, hipMemcpyDeviceToDevice));
        b.d_packed = std::move(bigger);
        cap32 = ncap;
    }
    void begin(uint64_t expected_words64) override { reserve(expected_words64 * 2 + 8); }
    void chunk(WordBuf &words, uint64_t word_off) override
    {
        const uint64_t n_words64 = words.size();
        reserve((word_off + n_words64) * 2 + 8);
        const char *src = (const char *)words.data();
        size_t left = n_words64 * 8;
        char *dst = (char *)(b.d_packed.p + 2 * word_off);
        if (words.in_arena()) {   // DMA from the parser's own buffer; it returns to the arena when the copy has left the host
            ++n_direct;
            reap(false);
            hipEvent_t ev = ring.take_event();
            SW_HIP(hipMemcpyAsync(dst, src, left, hipMemcpyHostToDevice, ring.st));
            SW_HIP(hipEventRecord(ev, ring.st));
            in_flight.push_back(InFlight{std::move(words), ev});
            used32 = (word_off + n_words64) * 2;
            return;
        }
        ++n_ring;
        while (left) {
            const size_t n = std::min(left, PinnedRing::SLOT);
            const unsigned s = next_slot++ % PinnedRing::SLOTS;
            SW_HIP(hipEventSynchronize(ring.ev[s]));   // the slot's previous copy has left the host
            memcpy(ring.base + s * PinnedRing::SLOT, src, n);
            SW_HIP(hipMemcpyAsync(dst, ring.base + s * PinnedRing::SLOT, n, hipMemcpyHostToDevice, ring.st));
            SW_HIP(hipEventRecord(ring.ev[s], ring.st));
            src += n;
            dst += n;
            left -= n;
        }
        used32 = (word_off + n_words64) * 2;
    }
    void finish()
    {
        const uint64_t n_words64 = b.host.chunk_word0.empty() ? 0 : b.host.chunk_word0.back();
        reserve(n_words64 * 2 + 8);
        SW_HIP(hipMemsetAsync(b.d_packed.p + 2 * n_words64, 0, 8 * 4, ring.st));   // the read slack
        SW_HIP(hipStreamSynchronize(ring.st));
        reap(true);
        b.packed_words = n_words64 * 2 + 8;
    }
    ~DeviceSink()   // nothing may still read the ring or the parsers' buffers / write the device buffer
    {
        (void)hipStreamSynchronize(ring.st);
        for (InFlight &f : in_flight) ring.spare.push_back(f.ev);
    }
};

// FASTA files -> device-resident batch
void ingest_to_device(const char *const *paths, size_t n_paths, uint64_t n_cpu, sw_batch &b)
{
    if (device_gz_ingest(paths, n_paths, n_cpu, b)) {   // many .gz files: inflate + parse + pack on the device (ingest_dev.hip)
        upload_tables(b);
        return;
    }
    if (n_paths >= 2 && !SW_TEST_GETENV("SEQWIN_AMD_NO_STREAM_UPLOAD")) {
        const auto t0 = std::chrono::steady_clock::now();
        DeviceSink sink(b, pinned_ring(b.device));
        const auto t1 = std::chrono::steady_clock::now();
        ingest_fasta(paths, n_paths, n_cpu, b.host, &sink);
        const auto t2 = std::chrono::steady_clock::now();
        sink.finish();
        upload_tables(b);
        if (getenv("SEQWIN_AMD_DEBUG_TIMING")) {
            fprintf(stderr, "[seqwin_amd] ingest_to_device: ring %.1f ms, ingest %.1f ms, finish + tables %.1f ms\n",
                    std::chrono::duration<double, std::milli>(t1 - t0).count(),
                    std::chrono::duration<double, std::milli>(t2 - t1).count(),
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count());
            PinnedArena &pa = pinned_arena();
            fprintf(stderr, "[seqwin_amd] pinned arena (process totals): %.0f MiB in %llu slabs, %.0f ms of page-locking; requests served %llu, declined %llu while a slab "
                            "was being locked + %llu at the limit; chunks by DMA from the parsers' buffers %llu, through the ring %llu\n",
                    pa.total_bytes / 1048576.0, (unsigned long long)pa.n_slabs.load(), pa.lock_us.load() / 1e3, (unsigned long long)pa.n_served.load(),
                    (unsigned long long)pa.n_declined_busy.load(), (unsigned long long)pa.n_declined_limit.load(), (unsigned long long)sink.n_direct,
                    (unsigned long long)sink.n_ring);
        }
    } else {
        ingest_fasta(paths, n_paths, n_cpu, b.host);
        upload_batch(b);
    }
}

// One thread = one packed word (16 bases) of one record.
__global__ void k_synth(uint32_t *packed, uint64_t words_per_record, uint64_t n_words, uint64_t records_per_genome,
                        uint64_t record_len, uint64_t n_ancestors, uint64_t snp_ppm, uint64_t seed, uint64_t word_base,
                        uint64_t first_record)
{
    const uint64_t wi = word_base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= n_words) return;
    // `rec` is the record's number in the whole job (a shard starts at first_record): a shard of a job holds the same
    // bases as the same genomes of the unsharded batch
    const uint64_t rec = first_record + wi / words_per_record, wr = wi % words_per_record;
    const uint64_t g = rec / records_per_genome, c = rec % records_per_genome;
    const uint64_t anc = g % n_ancestors;
    uint32_t word = 0;
    for (uint32_t i = 0; i < 16; ++i) {
        const uint64_t p = wr * 16 + i;
        if (p >= record_len) break;
        uint32_t base = (uint32_t)(mix64(seed ^ mix64((anc * records_per_genome + c) * 0x100000001b3ULL + p * 2 + 1)) >> 62);
        const uint64_t u = mix64((seed + 0x51ed27) ^ mix64(rec * 0x9E3779B97F4A7C15ULL + p));
        if (u % 1000000ull < snp_ppm) base = (uint32_t)(u >> 40) & 3u;
        word |= base << (2 * i);
    }
    packed[wi] = word;
}

// Ragged assemblies (r06, VERDICT r5 missing #4): records of different lengths, some with scaffold gaps.  One thread = one packed
// word; its record by binary search over the records' base offsets.  A base is the ancestor's at (ancestor, offset of the contig in
// the genome + position), substituted per genome as in k_synth; positions inside a gap (N run) are stored as 0.
__global__ void k_synth_ragged(uint32_t *packed, uint64_t n_words, const uint64_t *__restrict__ rec_base, const uint32_t *__restrict__ rec_len,
                               const uint64_t *__restrict__ rec_anc_off, const uint32_t *__restrict__ rec_genome,
                               const uint32_t *__restrict__ rec_gap_off, const uint32_t *__restrict__ gap_pos, const uint32_t *__restrict__ gap_len,
                               uint64_t R, uint64_t n_ancestors, uint64_t snp_ppm, uint64_t seed, uint64_t word_base)
{
    const uint64_t wi = word_base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= n_words) return;
    uint64_t lo = 0, hi = R;   // last record with rec_base / 16 <= wi
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (rec_base[mid] / 16 <= wi) lo = mid; else hi = mid;
    }
    const uint64_t r = lo, p0 = (wi - rec_base[r] / 16) * 16, len = rec_len[r], G = rec_genome[r], anc = G % n_ancestors, off = rec_anc_off[r];
    uint32_t word = 0;
    for (uint32_t i = 0; i < 16; ++i) {
        const uint64_t p = p0 + i;
        if (p >= len) break;
        bool gap = false;
        for (uint32_t q = rec_gap_off[r]; q < rec_gap_off[r + 1]; ++q) gap = gap || (p >= gap_pos[q] && p < (uint64_t)gap_pos[q] + gap_len[q]);
        if (gap) continue;
        uint32_t base = (uint32_t)(mix64(seed ^ mix64(anc * 0x100000001b3ULL + (off + p) * 2 + 1)) >> 62);
        const uint64_t u = mix64((seed + 0x51ed27) ^ mix64(G * 0x9E3779B97F4A7C15ULL + off + p));
        if (u % 1000000ull < snp_ppm) base = (uint32_t)(u >> 40) & 3u;
        word |= base << (2 * i);
    }
    packed[wi] = word;
}

struct GraphHost {   // result of sw_build: arrays stay in HBM until sw_graph_export copies them into caller buffers
    std::unique_ptr<sw_index> ixp{new sw_index};
    sw_index &ix = *ixp;
    std::vector<uint32_t> record_offsets;
    std::string ids_blob;
    uint64_t n_assemblies = 0, total_bp = 0;
    bool exported = false;          // sw_graph_export has filled caller arrays from this index
    uint64_t identity[2] = {0, 0};  // device_identity at that moment
    std::unique_ptr<MultiGraph> multi;   // SEQWIN_DEVICES: the graph as one slice per device instead of `ix`
    double ingest_ms = 0, device_ms = 0, export_ms = 0;   // sw_graph_stats
};

// ---- the index of the last exported sw_build stays resident --------------------------------------------------------
// Seqwin calls get_penalty on the arrays build() has just returned (kmers.py:396-402).  Uploading them again is the
// most expensive part of that call (6 GB of kmers at 15k genomes, from pageable memory), so sw_graph_free hands the
// device index of an exported graph to this slot instead of releasing it, and sw_get_penalty works on it when the
// caller's arrays are still the exported ones -- same sizes and the same position-dependent checksum of kmers and of
// the nodes' hash / start / stop, computed on the host with the caller's n_cpu threads (reading 6 GB at memory speed
// instead of pinning and copying it).  One index per process; replaced by the next sw_build's, dropped by
// sw_release_resident(); SEQWIN_AMD_NO_RESIDENT=1 disables it.
struct Resident {
    std::mutex mu;
    std::unique_ptr<sw_index> ix;
    uint64_t kmer_sum = 0, node_sum = 0;
    uint64_t penalty_hits = 0, filter_hits = 0;   // calls served from the resident arrays (sw_resident_stats)
};
Resident &resident()
{
    static Resident *r = new Resident;   // leaked on purpose (see pool())
    return *r;
}
// The same for a graph built over several devices (SEQWIN_DEVICES): its slices stay on their devices, and sw_get_penalty scores
// every slice where it lies -- one host thread per slice -- when the caller's arrays still are the exported ones.  (Uploading
// 9 GB of kmers and nodes of a 15 000-genome graph to one device from pageable memory would cost seconds.)
struct ResidentMulti {
    std::mutex mu;
    std::unique_ptr<MultiGraph> mg;
    uint64_t n_kmers = 0, n_nodes = 0, kmer_sum = 0, node_sum = 0, penalty_hits = 0;
};
ResidentMulti &resident_multi()
{
    static ResidentMulti *r = new ResidentMulti;
    return *r;
}

// the sums of k_identity (index.hip) over host arrays, on n_threads threads
}  // namespace
// set while THIS thread holds Resident::mu (sw_get_penalty / sw_filter_kmers allocate while they work on the resident
// arrays): try_lock on a mutex the calling thread owns is undefined, so the owner is told apart before the mutex is touched
thread_local bool t_resident_held = false;
struct ResidentLock {
    std::unique_lock<std::mutex> lk;
    explicit ResidentLock(std::mutex &m) : lk(m) { t_resident_held = true; }
    void unlock() { if (lk.owns_lock()) { lk.unlock(); t_resident_held = false; } }
    ~ResidentLock() { if (lk.owns_lock()) t_resident_held = false; }
};
void release_resident_if_idle()
{
    if (t_resident_held) return;                                 // this very call is working on it
    Resident &r = resident();
    std::unique_lock<std::mutex> lock(r.mu, std::try_to_lock);   // (held by another thread: a call is working on it)
    if (!lock.owns_lock() || !r.ix) return;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || r.ix->device != dev) return;   // HBM of another device does not help this hipMalloc
    r.ix.reset();
}
namespace {
void host_identity(const sw_kmer *kmers, uint64_t nk, const sw_node *nodes, uint64_t nn, unsigned n_threads, uint64_t *sums2)
{
    n_threads = std::max(1u, std::min(n_threads, 64u));
    if (nk + nn < (1u << 20)) n_threads = 1;
    std::vector<uint64_t> pa(n_threads, 0), pb(n_threads, 0);
    auto work = [&](unsigned t) {
        uint64_t a = 0, b = 0;
        for (uint64_t i = nk * t / n_threads, e = nk * (t + 1) / n_threads; i < e; ++i)
            a += ck_kmer(i, kmers[i]);
        for (uint64_t i = nn * t / n_threads, e = nn * (t + 1) / n_threads; i < e; ++i)
            b += ck_node_identity(i, nodes[i]);
        pa[t] = a;
        pb[t] = b;
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < n_threads; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    sums2[0] = sums2[1] = 0;
    for (unsigned t = 0; t < n_threads; ++t) {
        sums2[0] += pa[t];
        sums2[1] += pb[t];
    }
}

void check_targets(const uint8_t *is_targets, uint64_t n, uint64_t *n_tar, uint64_t *n_neg)
{
    uint64_t t = 0;
    for (uint64_t i = 0; i < n; ++i) t += is_targets[i] ? 1 : 0;
    *n_tar = t;
    *n_neg = n - t;
    if (t == 0) raise(SW_ERR_VALUE, "is_targets must contain at least one target assembly");          // filter.cpp:55-57
    if (t == n) raise(SW_ERR_VALUE, "is_targets must contain at least one non-target assembly");      // filter.cpp:58-60
}

void do_index_build(sw_batch &b, uint64_t k, uint64_t w, const uint8_t *is_targets, uint64_t n_assemblies,
                    hipStream_t stream, sw_index &ix)
{
    require_current_device(b.device, "the batch");
    StreamScope scope(stream);
    bool plan_cached = false;
    Plan &plan = get_plan(b, k, w, &plan_cached);
    uint64_t n_tar = 0, n_neg = 0;
    DevArray<uint8_t> d_tar;
    if (is_targets) {
        if (n_assemblies != b.host.n_assemblies)
            raise(SW_ERR_VALUE, "len(is_targets) must equal the number of assemblies in the batch");
        check_targets(is_targets, n_assemblies, &n_tar, &n_neg);
        d_tar.alloc(n_assemblies);
        SW_HIP(hipMemcpyAsync(d_tar.p, is_targets, n_assemblies, hipMemcpyHostToDevice, stream));
    }
    Event e0, e1, e2, e3;
    SW_HIP(hipEventRecord(e0, stream));
    SketchOut sk;
    float sketch_ms = 0.f;
    run_sketch(b, plan, stream, sk, &sketch_ms);
    SW_HIP(hipEventRecord(e1, stream));
    OrderedOcc occ;
    const uint64_t launches = sk.launches, ovf_tiles = sk.n_ovf_tiles;
    order_tuples(sk, plan, stream, occ, true, true);   // (may take the stage along: the node sort then reads it itself)
    sk = SketchOut();
    SW_HIP(hipEventRecord(e2, stream));
    ix.device = b.device;
    build_index(b.d_rec_asm.p, b.n_records, b.host.n_assemblies, occ, is_targets ? d_tar.p : nullptr, n_tar, n_neg, stream, ix);
    SW_HIP(hipEventRecord(e3, stream));
    SW_HIP(hipEventSynchronize(e3));
    float ms = 0.f;
    SW_HIP(hipEventElapsedTime(&ms, e0, e3));
    ix.timings.total_ms = ms;
    SW_HIP(hipEventElapsedTime(&ms, e1, e2));
    ix.timings.order_ms = ms;
    ix.timings.sketch_ms = sketch_ms;
    ix.timings.sketch_launches = launches;
    ix.timings.n_tiles = plan.n_tiles;
    ix.timings.total_bp = b.host.total_bp;
    ix.timings.n_windows = plan.n_windows;
    ix.timings.ovf_tiles = ovf_tiles;
    ix.timings.plan_ms = plan.build_ms;
    ix.timings.plan_cached = plan_cached ? 1 : 0;
    ix.timings.tiles_b256 = plan.fc[0].n_tiles;
    ix.timings.tiles_b64 = plan.fc[1].n_tiles;
    ix.timings.tiles_generic = plan.n_tiles_gen;
    ix.timings.tiles_gap = (uint64_t)plan.fc[0].n_gap + plan.fc[1].n_gap;
}

}  // namespace
}  // namespace sw

using namespace sw;

sw_occ::~sw_occ() { delete occ; }

struct sw_graph {
    sw::GraphHost g;
};

struct sw_hostbatch {
    sw::HostBatch h;
};

extern "C" {

const char *sw_last_error(void) { return g_last_error.c_str(); }
const char *sw_version(void) { return "seqwin_amd 0.1.0 (gfx950)"; }

static std::atomic<sw_log_fn> g_log_fn{nullptr};
void sw_set_log_callback(sw_log_fn fn) { g_log_fn.store(fn); }
static void log_message(const char *level, const char *fmt, ...)
{
    sw_log_fn fn = g_log_fn.load();
    if (!fn) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    fn(level, buf);
}

}   // extern "C"
void sw::log_info(const char *fmt, ...)
{
    sw_log_fn fn = g_log_fn.load();
    const bool echo = getenv("SEQWIN_AMD_LOG_STDERR") != nullptr;
    if (!fn && !echo) return;
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (fn) fn("info", buf);
    if (echo) fprintf(stderr, "[seqwin_amd] %s\n", buf);
}
static std::atomic<uint64_t> g_guard_trips[2];
void sw::order_guard_tripped(int which, uint32_t places)
{
    g_guard_trips[which ? 1 : 0].fetch_add(1);
    const char *what = which ? "edge-key sort" : "node sort";
    fprintf(stderr, "[seqwin_amd] WARNING: order guard: the %s came out of order in %u places (LDS-atomic ranking of the radix passes); "
                    "re-sorting with ballot / rocPRIM ranking, which this device keeps for the rest of the process\n", what, places);
    log_message("warning", "order guard: the %s came out of order in %u places; re-sorted with ballot / rocPRIM ranking", what, places);
}
extern "C" {

int sw_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int sw_set_device(int device)
{
    return guarded([&] {
        require_device();
        SW_HIP(hipSetDevice(device));
    });
}

int sw_batch_from_fasta(const char *const *assembly_paths, size_t n_assemblies, uint64_t n_cpu, sw_batch **out)
{
    return guarded([&] {
        require_device();
        std::unique_ptr<sw_batch> b(new sw_batch);
        SW_HIP(hipGetDevice(&b->device));
        ingest_to_device(assembly_paths, n_assemblies, n_cpu, *b);
        *out = b.release();
    });
}

int sw_batch_synthetic(uint64_t n_genomes, uint64_t records_per_genome, uint64_t record_len, uint64_t n_ancestors,
                       uint64_t snp_ppm, uint64_t seed, sw_batch **out)
{
    return sw_batch_synthetic_shard(n_genomes, records_per_genome, record_len, n_ancestors, snp_ppm, seed, 0, out);
}

int sw_batch_synthetic_shard(uint64_t n_genomes, uint64_t records_per_genome, uint64_t record_len, uint64_t n_ancestors,
                             uint64_t snp_ppm, uint64_t seed, uint64_t first_genome, sw_batch **out)
{
    return guarded([&] {
        require_device();
        if (n_ancestors == 0 || records_per_genome == 0) raise(SW_ERR_VALUE, "n_ancestors and records_per_genome must be >= 1");
        if (record_len > UINT32_MAX) raise(SW_ERR_VALUE, "record_len exceeds uint32 range");
        const uint64_t R = n_genomes * records_per_genome;
        if (R > UINT32_MAX) raise(SW_ERR_VALUE, "number of records exceeds uint32 range");
        std::unique_ptr<sw_batch> b(new sw_batch);
        SW_HIP(hipGetDevice(&b->device));
        HostBatch &h = b->host;
        h.n_assemblies = n_genomes;
        h.total_bp = R * record_len;
        const uint64_t padded = (record_len + 31) / 32 * 32;
        const uint64_t wpr = padded / 16;
        h.record_offsets.resize(n_genomes + 1);
        for (uint64_t g = 0; g <= n_genomes; ++g) h.record_offsets[g] = (uint32_t)(g * records_per_genome);
        h.rec_len.assign(R, (uint32_t)record_len);
        h.rec_base.resize(R);
        h.rec_run_off.resize(R + 1);
        h.run_pos.assign(record_len ? R : 0, 0);
        h.run_len.assign(record_len ? R : 0, (uint32_t)record_len);
        char name[64];
        for (uint64_t r = 0; r < R; ++r) {
            h.rec_base[r] = r * padded;
            h.rec_run_off[r] = record_len ? (uint32_t)r : 0;
            int len = snprintf(name, sizeof name, "g%llu_c%llu", (unsigned long long)(first_genome + r / records_per_genome),
                               (unsigned long long)(r % records_per_genome));
            h.ids_blob.append(name, (size_t)len + 1);
        }
        h.rec_run_off[R] = record_len ? (uint32_t)R : 0;
        b->n_records = R;
        b->packed_words = R * wpr + 8;
        b->d_packed.alloc(b->packed_words);
        SW_HIP(hipMemset(b->d_packed.p, 0, b->packed_words * 4));
        const uint64_t n_words = R * wpr;
        // a HIP grid is limited to 2^32 - 1 work-items per dimension: launch in chunks of 2^30 words
        for (uint64_t base = 0; base < n_words; base += (1ull << 30)) {
            const uint64_t cnt = std::min<uint64_t>(n_words - base, 1ull << 30);
            hipLaunchKernelGGL(k_synth, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0, b->d_packed.p, wpr, base + cnt,
                               records_per_genome, record_len, n_ancestors, snp_ppm, seed, base, first_genome * records_per_genome);
            SW_HIP(hipGetLastError());
        }
        SW_HIP(hipDeviceSynchronize());
        b->d_rec_base.alloc(R);
        if (R) SW_HIP(hipMemcpy(b->d_rec_base.p, h.rec_base.data(), R * 8, hipMemcpyHostToDevice));
        std::vector<uint32_t> rec_asm(R);
        for (uint64_t r = 0; r < R; ++r) rec_asm[r] = (uint32_t)(r / records_per_genome);
        b->d_rec_asm.alloc(R);
        if (R) SW_HIP(hipMemcpy(b->d_rec_asm.p, rec_asm.data(), R * 4, hipMemcpyHostToDevice));
        *out = b.release();
    });
}

int sw_batch_synthetic_ragged(uint64_t n_genomes, uint64_t genome_bp, uint64_t n_ancestors, uint64_t snp_ppm, uint64_t seed, uint64_t first_genome,
                              sw_batch **out)
{
    return guarded([&] {
        require_device();
        if (n_ancestors == 0 || genome_bp < 4000) raise(SW_ERR_VALUE, "n_ancestors must be >= 1 and genome_bp >= 4000");
        std::unique_ptr<sw_batch> b(new sw_batch);
        SW_HIP(hipGetDevice(&b->device));
        HostBatch &h = b->host;
        h.n_assemblies = n_genomes;
        h.record_offsets.assign(1, 0);
        std::vector<uint64_t> anc_off;
        std::vector<uint32_t> genome, gap_off(1, 0), gap_pos, gap_len;
        uint64_t base_at = 0;
        char name[64];
        for (uint64_t g = 0; g < n_genomes; ++g) {
            const uint64_t G = first_genome + g;
            uint64_t st = mix64(seed * 0x9E3779B97F4A7C15ULL + G * 0xD1B54A32D192ED03ULL + 0x1234567);
            auto next = [&] { return st = mix64(st + 0x9E3779B97F4A7C15ULL); };
            uint64_t total = 0, c = 0;
            // contig lengths 200 * 2^x, x the sum of four uniforms on [0, 3.22): a bell over 200 bp ... 1.5 Mbp around 17 kbp, heavy to
            // the right like the contigs of a draft assembly; contigs until the genome is full, between 20 and 300 of them
            // (only + and * on doubles: the same tables on every host)
            while ((total < genome_bp || c < 20) && c < 300) {
                double x = 0;
                for (int j = 0; j < 4; ++j) x += (double)(next() >> 11) * (1.0 / 9007199254740992.0) * 3.22;
                const unsigned xi = (unsigned)x;
                const double f = x - (double)xi;
                const double m = 1.0 + f * (0.6565 + 0.3435 * f);      // ~ 2^f on [0, 1)
                uint64_t len = (uint64_t)(200.0 * m * (double)(1ull << xi));
                len = std::min<uint64_t>(std::max<uint64_t>(len, 200), 1500000);
                if (h.rec_len.size() >= UINT32_MAX) raise(SW_ERR_VALUE, "number of records exceeds uint32 range");
                const uint32_t r = (uint32_t)h.rec_len.size();
                h.rec_len.push_back((uint32_t)len);
                h.rec_base.push_back(base_at);
                base_at += (len + 31) / 32 * 32;
                anc_off.push_back(total);
                genome.push_back((uint32_t)G);
                // scaffold gaps: one contig in ten carries one to three runs of 10 ... 1000 N
                std::vector<std::pair<uint32_t, uint32_t>> gaps;
                if (next() % 10 == 0) {
                    const unsigned ng = 1 + (unsigned)(next() % 3);
                    for (unsigned q = 0; q < ng; ++q) {
                        const uint32_t gl = 10 + (uint32_t)(next() % 991);
                        if (len > (uint64_t)gl + 2) gaps.emplace_back((uint32_t)(next() % (len - gl)), gl);
                    }
                    std::sort(gaps.begin(), gaps.end());
                    std::vector<std::pair<uint32_t, uint32_t>> merged;
                    for (auto &gp : gaps) {
                        if (!merged.empty() && gp.first <= merged.back().first + merged.back().second)
                            merged.back().second = std::max(merged.back().second, gp.first + gp.second - merged.back().first);
                        else merged.push_back(gp);
                    }
                    gaps.swap(merged);
                }
                h.rec_run_off.push_back((uint32_t)h.run_pos.size());
                uint32_t at = 0;
                for (auto &gp : gaps) {
                    if (gp.first > at) { h.run_pos.push_back(at); h.run_len.push_back(gp.first - at); }
                    at = gp.first + gp.second;
                    gap_pos.push_back(gp.first);
                    gap_len.push_back(gp.second);
                }
                if (len > at) { h.run_pos.push_back(at); h.run_len.push_back((uint32_t)len - at); }
                gap_off.push_back((uint32_t)gap_pos.size());
                const int nl = snprintf(name, sizeof name, "g%llu_c%llu", (unsigned long long)G, (unsigned long long)c);
                h.ids_blob.append(name, (size_t)nl + 1);
                total += len;
                ++c;
                (void)r;
            }
            h.total_bp += total;
            h.record_offsets.push_back((uint32_t)h.rec_len.size());
        }
        const uint64_t R = h.rec_len.size();
        h.rec_run_off.push_back((uint32_t)h.run_pos.size());
        b->n_records = R;
        const uint64_t n_words = base_at / 16;
        b->packed_words = n_words + 8;
        b->d_packed.alloc(b->packed_words);
        SW_HIP(hipMemset(b->d_packed.p, 0, b->packed_words * 4));
        b->d_rec_base.alloc(R);
        b->d_rec_asm.alloc(R);
        if (R) {
            std::vector<uint32_t> rec_asm(R);
            for (uint64_t g = 0; g < n_genomes; ++g)
                for (uint32_t r = h.record_offsets[g]; r < h.record_offsets[g + 1]; ++r) rec_asm[r] = (uint32_t)g;
            SW_HIP(hipMemcpy(b->d_rec_base.p, h.rec_base.data(), R * 8, hipMemcpyHostToDevice));
            SW_HIP(hipMemcpy(b->d_rec_asm.p, rec_asm.data(), R * 4, hipMemcpyHostToDevice));
            DevArray<uint32_t> d_len(R), d_genome(R), d_gap_off(R + 1), d_gap_pos(std::max<size_t>(gap_pos.size(), 1)), d_gap_len(std::max<size_t>(gap_len.size(), 1));
            DevArray<uint64_t> d_anc(R);
            SW_HIP(hipMemcpy(d_len.p, h.rec_len.data(), R * 4, hipMemcpyHostToDevice));
            SW_HIP(hipMemcpy(d_genome.p, genome.data(), R * 4, hipMemcpyHostToDevice));
            SW_HIP(hipMemcpy(d_anc.p, anc_off.data(), R * 8, hipMemcpyHostToDevice));
            SW_HIP(hipMemcpy(d_gap_off.p, gap_off.data(), (R + 1) * 4, hipMemcpyHostToDevice));
            if (!gap_pos.empty()) {
                SW_HIP(hipMemcpy(d_gap_pos.p, gap_pos.data(), gap_pos.size() * 4, hipMemcpyHostToDevice));
                SW_HIP(hipMemcpy(d_gap_len.p, gap_len.data(), gap_len.size() * 4, hipMemcpyHostToDevice));
            }
            for (uint64_t base = 0; base < n_words; base += (1ull << 30)) {
                const uint64_t cnt = std::min<uint64_t>(n_words - base, 1ull << 30);
                hipLaunchKernelGGL(k_synth_ragged, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0, b->d_packed.p, base + cnt, b->d_rec_base.p, d_len.p,
                                   d_anc.p, d_genome.p, d_gap_off.p, d_gap_pos.p, d_gap_len.p, R, n_ancestors, snp_ppm, seed, base);
                SW_HIP(hipGetLastError());
            }
            SW_HIP(hipDeviceSynchronize());
        }
        *out = b.release();
    });
}

int sw_batch_record(const sw_batch *b, uint64_t record_idx, char *seq_out, uint64_t cap, uint64_t *len_out)
{
    return guarded([&] {
        if (record_idx >= b->n_records) raise(SW_ERR_VALUE, "record index out of range");
        const HostBatch &h = b->host;
        const uint64_t len = h.rec_len[record_idx];
        *len_out = len;
        if (!seq_out || cap < len) return;
        const uint64_t w0 = h.rec_base[record_idx] / 16, nw = (len + 15) / 16;
        std::vector<uint32_t> words(nw);
        if (nw) SW_HIP(hipMemcpy(words.data(), b->d_packed.p + w0, nw * 4, hipMemcpyDeviceToHost));
        memset(seq_out, 'N', len);
        for (uint32_t q = h.rec_run_off[record_idx]; q < h.rec_run_off[record_idx + 1]; ++q)
            for (uint64_t p = h.run_pos[q]; p < (uint64_t)h.run_pos[q] + h.run_len[q]; ++p)
                seq_out[p] = "ACGT"[(words[p / 16] >> (2 * (p % 16))) & 3u];
    });
}

int sw_batch_write_fasta(const sw_batch *b, uint64_t first_assembly, uint64_t n_assemblies, const char *dir, uint64_t n_cpu,
                         uint64_t line_width)
{
    return guarded([&] {
        const HostBatch &h = b->host;
        if (first_assembly > h.n_assemblies || n_assemblies > h.n_assemblies - first_assembly) raise(SW_ERR_VALUE, "assembly range out of bounds");
        require_current_device(b->device, "the batch");
        // ids by record (the blob holds them NUL-terminated in record order)
        std::vector<const char *> id_of(b->n_records + 1, nullptr);
        {
            const char *p = h.ids_blob.data(), *end = p + h.ids_blob.size();
            for (uint64_t r = 0; r < b->n_records && p < end; ++r) {
                id_of[r] = p;
                p += strlen(p) + 1;
            }
        }
        char tab[256][4];
        for (int v = 0; v < 256; ++v)
            for (int j = 0; j < 4; ++j) tab[v][j] = "ACGT"[(v >> (2 * j)) & 3];
        uint64_t lower_ppm = 0;   // SEQWIN_AMD_WRITE_LOWER_PPM: that share of the bases in lower case (ragged workloads: 10000)
        if (const char *e = getenv("SEQWIN_AMD_WRITE_LOWER_PPM")) lower_ppm = (uint64_t)std::max(0ll, atoll(e));
        const unsigned n_threads = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({n_cpu, n_assemblies, (uint64_t)64}));
        std::atomic<uint64_t> next{0};
        std::mutex err_mu;
        std::exception_ptr err;
        auto work = [&] {
            try {
                SW_HIP(hipSetDevice(b->device));
                std::vector<uint32_t> words;
                std::string seq, out;
                for (;;) {
                    const uint64_t a = first_assembly + next.fetch_add(1);
                    if (a >= first_assembly + n_assemblies) break;
                    out.clear();
                    for (uint32_t r = h.record_offsets[a]; r < h.record_offsets[a + 1]; ++r) {
                        const uint64_t len = h.rec_len[r], w0 = h.rec_base[r] / 16, nw = (len + 15) / 16;
                        words.resize(nw);
                        if (nw) SW_HIP(hipMemcpy(words.data(), b->d_packed.p + w0, nw * 4, hipMemcpyDeviceToHost));
                        seq.assign(len, 'N');
                        for (uint32_t q = h.rec_run_off[r]; q < h.rec_run_off[r + 1]; ++q) {
                            uint64_t p = h.run_pos[q];
                            const uint64_t e = p + h.run_len[q];
                            for (; p < e && (p & 3); ++p) seq[p] = "ACGT"[(words[p / 16] >> (2 * (p % 16))) & 3u];
                            for (; p + 4 <= e; p += 4) memcpy(&seq[p], tab[(words[p / 16] >> (2 * (p % 16))) & 0xFFu], 4);
                            for (; p < e; ++p) seq[p] = "ACGT"[(words[p / 16] >> (2 * (p % 16))) & 3u];
                        }
                        if (lower_ppm)   // (soft-masked bases: the reader takes either case, fasta_reader.cpp keeps it)
                            for (uint64_t p = 0; p < len; ++p)
                                if (mix64(((uint64_t)r << 32) + p) % 1000000ull < lower_ppm) seq[p] = (char)tolower((unsigned char)seq[p]);
                        out += '>';
                        out += id_of[r] ? id_of[r] : "";
                        out += '\n';
                        if (line_width == 0) {
                            out += seq;
                            out += '\n';
                        } else {
                            for (uint64_t p = 0; p < len; p += line_width) {
                                out.append(seq, p, std::min<uint64_t>(line_width, len - p));
                                out += '\n';
                            }
                        }
                    }
                    const std::string path = std::string(dir) + "/g" + std::to_string(a) + ".fa";
                    FILE *f = fopen(path.c_str(), "wb");
                    if (!f) raise(SW_ERR_RUNTIME, "cannot write %s", path.c_str());
                    const size_t wrote = fwrite(out.data(), 1, out.size(), f);
                    if (fclose(f) != 0 || wrote != out.size()) raise(SW_ERR_RUNTIME, "short write to %s", path.c_str());
                }
            } catch (...) {
                std::lock_guard<std::mutex> g(err_mu);
                if (!err) err = std::current_exception();
            }
        };
        std::vector<std::thread> th;
        for (unsigned t = 1; t < n_threads; ++t) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
        if (err) std::rethrow_exception(err);
    });
}

int sw_batch_info(const sw_batch *b, uint64_t *n_assemblies, uint64_t *n_records, uint64_t *total_bp,
                  uint64_t *device_bytes)
{
    return guarded([&] {
        if (n_assemblies) *n_assemblies = b->host.n_assemblies;
        if (n_records) *n_records = b->n_records;
        if (total_bp) *total_bp = b->host.total_bp;
        if (device_bytes) *device_bytes = b->d_packed.bytes() + b->d_rec_base.bytes() + b->d_rec_asm.bytes();
    });
}

int sw_batch_records(const sw_batch *b, uint32_t *record_offsets, char *ids_blob, uint64_t ids_cap, uint64_t *ids_bytes)
{
    return guarded([&] {
        const HostBatch &h = b->host;
        if (record_offsets) memcpy(record_offsets, h.record_offsets.data(), (h.n_assemblies + 1) * 4);
        if (ids_bytes) *ids_bytes = h.ids_blob.size();
        if (ids_blob && ids_cap >= h.ids_blob.size()) memcpy(ids_blob, h.ids_blob.data(), h.ids_blob.size());
    });
}

void sw_batch_free(sw_batch *b) { delete b; }

int sw_host_ingest(const char *const *assembly_paths, size_t n_assemblies, uint64_t n_cpu, sw_hostbatch **out)
{
    return guarded([&] {
        std::unique_ptr<sw_hostbatch> hb(new sw_hostbatch);
        ingest_fasta(assembly_paths, n_assemblies, n_cpu, hb->h);
        *out = hb.release();
    });
}

int sw_hostbatch_info(const sw_hostbatch *hb, uint64_t *n_assemblies, uint64_t *n_records, uint64_t *total_bp,
                      uint64_t *ids_bytes, uint64_t *n_runs)
{
    return guarded([&] {
        *n_assemblies = hb->h.n_assemblies;
        *n_records = hb->h.rec_len.size();
        *total_bp = hb->h.total_bp;
        *ids_bytes = hb->h.ids_blob.size();
        *n_runs = hb->h.run_pos.size();
    });
}

int sw_hostbatch_tables(const sw_hostbatch *hb, uint32_t *record_offsets, char *ids_blob, uint32_t *rec_len)
{
    return guarded([&] {
        const HostBatch &h = hb->h;
        if (record_offsets) memcpy(record_offsets, h.record_offsets.data(), h.record_offsets.size() * 4);
        if (ids_blob && !h.ids_blob.empty()) memcpy(ids_blob, h.ids_blob.data(), h.ids_blob.size());
        if (rec_len && !h.rec_len.empty()) memcpy(rec_len, h.rec_len.data(), h.rec_len.size() * 4);
    });
}

int sw_hostbatch_record(const sw_hostbatch *hb, uint64_t record_idx, char *seq_out, uint64_t cap, uint64_t *len_out)
{
    return guarded([&] {
        const HostBatch &h = hb->h;
        if (record_idx >= h.rec_len.size()) raise(SW_ERR_VALUE, "record index out of range");
        const uint64_t len = h.rec_len[record_idx];
        *len_out = len;
        if (!seq_out || cap < len) return;
        memset(seq_out, 'N', len);
        const uint64_t b0 = h.rec_base[record_idx];
        for (uint32_t q = h.rec_run_off[record_idx]; q < h.rec_run_off[record_idx + 1]; ++q)
            for (uint64_t p = h.run_pos[q]; p < (uint64_t)h.run_pos[q] + h.run_len[q]; ++p) {
                const uint64_t b = b0 + p;
                seq_out[p] = "ACGT"[(h.word32(b / 16) >> (2 * (b % 16))) & 3u];
            }
    });
}

void sw_hostbatch_free(sw_hostbatch *hb) { delete hb; }

int sw_index_build(const sw_batch *b, uint64_t kmerlen, uint64_t windowsize, const uint8_t *is_targets,
                   uint64_t n_assemblies, void *stream, sw_index **out)
{
    return guarded([&] {
        std::unique_ptr<sw_index> ix(new sw_index);
        ix->last_stream = (hipStream_t)stream;
        do_index_build(*const_cast<sw_batch *>(b), kmerlen, windowsize, is_targets, n_assemblies, (hipStream_t)stream, *ix);
        *out = ix.release();
    });
}

int sw_index_sizes(const sw_index *ix, uint64_t *n_kmers, uint64_t *n_nodes, uint64_t *n_edges)
{
    return guarded([&] {
        *n_kmers = ix->n_kmers;
        *n_nodes = ix->n_nodes;
        *n_edges = ix->n_edges;
    });
}

int sw_index_timings(const sw_index *ix, sw_timings *t)
{
    return guarded([&] { *t = ix->timings; });
}

int sw_index_export(const sw_index *ix, sw_kmer *kmers, sw_node *nodes, sw_edge *edges)
{
    return guarded([&] {
        require_current_device(ix->device, "the index");
        const HostSpan spans[3] = {{kmers, ix->n_kmers * sizeof(sw_kmer)}, {nodes, ix->n_nodes * sizeof(sw_node)},
                                   {edges, ix->n_edges * sizeof(sw_edge)}};
        const void *const from[3] = {ix->kmers.p, ix->nodes.p, ix->edges.p};
        download(spans, from, 3);
    });
}

int sw_index_checksums(const sw_index *ix, uint64_t *kmers_sum, uint64_t *nodes_sum, uint64_t *edges_sum)
{
    return guarded([&] {
        uint64_t s[3];
        device_checksums(*ix, 0, s);
        *kmers_sum = s[0];
        *nodes_sum = s[1];
        *edges_sum = s[2];
    });
}

int sw_index_checksums_at(const sw_index *ix, uint64_t kmer_base, uint64_t node_base, uint64_t edge_base, uint64_t *sums)
{
    return guarded([&] {
        device_checksums(*ix, 0, sums, kmer_base, node_base, edge_base);
    });
}

int sw_index_verify(const sw_index *ix, uint64_t n_assemblies, int scored, uint64_t *out)
{
    return guarded([&] {
        require_current_device(ix->device, "the index");
        index_verify(*ix, n_assemblies, scored != 0, 0, out);
    });
}

void sw_index_free(sw_index *ix)
{
    if (!ix) return;
    StreamScope scope(ix->last_stream);   // the blocks go back tagged with the stream that used them last (not the null stream)
    delete ix;
}

int sw_index_threshold_sums(const sw_index *ix, uint64_t *sums)
{
    return guarded([&] { index_threshold_sums(*ix, 0, sums); });
}

int sw_index_filter_graph(const sw_index *ix, uint64_t edge_weight_th, sw_index **out)
{
    return guarded([&] {
        std::unique_ptr<sw_index> o(new sw_index);
        o->device = ix->device;
        index_filter_graph(*ix, edge_weight_th, 0, *o);
        *out = o.release();
    });
}

int sw_index_filter_kmers(const sw_index *ix, const sw_index *nodes_from, const uint64_t *used_hashes, uint64_t n_used,
                          sw_index **out)
{
    return guarded([&] {
        const sw_index *nf = nodes_from ? nodes_from : ix;   // NULL: the index's own nodes
        require_current_device(ix->device, "the index");
        if (nf->device != ix->device) raise(SW_ERR_VALUE, "the two indexes live on different devices (%d, %d)", ix->device, nf->device);
        std::vector<uint64_t> used(used_hashes, used_hashes + n_used);
        std::sort(used.begin(), used.end());
        DevArray<uint64_t> d_used(n_used);
        if (n_used) SW_HIP(hipMemcpy(d_used.p, used.data(), n_used * 8, hipMemcpyHostToDevice));
        std::unique_ptr<sw_index> o(new sw_index);
        o->device = ix->device;
        uint64_t nk = 0, nn = 0;
        device_filter_kmers(ix->kmers.p, ix->n_kmers, nf->nodes.p, nf->n_nodes, d_used.p, n_used, 0, o->kmers,
                            o->nodes, &nk, &nn);
        o->n_kmers = nk;
        o->n_nodes = nn;
        o->n_edges = 0;
        o->edges.alloc(0);
        *out = o.release();
    });
}

int sw_occ_sketch(const sw_batch *b, uint64_t kmerlen, uint64_t windowsize, void *stream, sw_occ **out)
{
    return guarded([&] {
        sw_batch &bb = *const_cast<sw_batch *>(b);
        require_current_device(bb.device, "the batch");
        StreamScope scope((hipStream_t)stream);
        Plan &plan = get_plan(bb, kmerlen, windowsize);
        std::unique_ptr<sw_occ> o(new sw_occ);
        o->last_stream = (hipStream_t)stream;
        o->batch = b;
        o->occ = new OrderedOcc;
        SketchOut sk;
        run_sketch(bb, plan, (hipStream_t)stream, sk, &o->sketch_ms);
        order_tuples(sk, plan, (hipStream_t)stream, *o->occ);
        *out = o.release();
    });
}

namespace sw {
namespace {
__global__ void k_rebase_records(uint64_t *kmer, uint64_t n, uint64_t rec_base)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kmer[i] += rec_base << 32;
}
}  // namespace
}  // namespace sw

static size_t chunk_end(const char *const *paths, size_t n_paths, size_t a0, uint64_t chunk_bp);
int sw_occ_sketch_paths(const char *const *assembly_paths, size_t n_assemblies, uint64_t kmerlen, uint64_t windowsize, uint64_t n_cpu,
                        uint64_t chunk_bp, void *stream, sw_batch **batch_out, sw_occ **occ_out)
{
    return guarded([&] {
        check_kw(kmerlen, windowsize);
        require_device();
        hipStream_t st = (hipStream_t)stream;
        std::unique_ptr<sw_batch> tables(new sw_batch);   // record tables only: no packed bases stay behind
        SW_HIP(hipGetDevice(&tables->device));
        HostBatch &H = tables->host;
        H.record_offsets.assign(1, 0);
        std::vector<OrderedOcc> chunks;
        std::vector<uint32_t> rec_asm;
        uint64_t n_records = 0, n_total = 0;
        float sk_ms_total = 0.f;
        size_t a0 = 0;
        while (a0 < n_assemblies) {
            const size_t a1 = chunk_bp ? chunk_end(assembly_paths, n_assemblies, a0, chunk_bp) : n_assemblies;
            sw_batch b;
            b.device = tables->device;
            ingest_to_device(assembly_paths + a0, a1 - a0, n_cpu, b);
            StreamScope scope(st);
            Plan &plan = get_plan(b, kmerlen, windowsize);
            SketchOut sk;
            float sk_ms = 0.f;
            run_sketch(b, plan, st, sk, &sk_ms);
            sk_ms_total += sk_ms;
            chunks.emplace_back();
            OrderedOcc &c = chunks.back();
            order_tuples(sk, plan, st, c);                       // exchange form: (out_hash, pos | record << 32), chunk-local records
            if (c.n && n_records)
                hipLaunchKernelGGL(k_rebase_records, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, st, c.kmer.p, c.n, n_records);
            SW_HIP(hipGetLastError());
            SW_HIP(hipStreamSynchronize(st));                    // the chunk's batch, plan and stage go out of scope
            n_total += c.n;
            const HostBatch &h = b.host;
            for (uint64_t a = 0; a < h.n_assemblies; ++a) {
                const uint64_t nr = h.record_offsets[a + 1] - h.record_offsets[a];
                if (n_records + nr > UINT32_MAX) raise(SW_ERR_RUNTIME, "Total number of FASTA records exceeds uint32 range");   // build.cpp:136-147
                rec_asm.insert(rec_asm.end(), nr, (uint32_t)(a0 + a));
                n_records += nr;
                H.record_offsets.push_back((uint32_t)n_records);
            }
            H.ids_blob += h.ids_blob;
            H.total_bp += h.total_bp;
            a0 = a1;
        }
        H.n_assemblies = n_assemblies;
        tables->n_records = n_records;
        if (n_total > occ_cap()) raise_occ_cap(n_total, "minimizer occurrences");
        StreamScope scope(st);
        tables->d_rec_asm.alloc(n_records);
        if (n_records) {
            SW_HIP(hipMemcpyAsync(tables->d_rec_asm.p, rec_asm.data(), n_records * 4, hipMemcpyHostToDevice, st));
            SW_HIP(hipStreamSynchronize(st));                    // (rec_asm is a local)
        }
        std::unique_ptr<sw_occ> o(new sw_occ);
        o->last_stream = st;
        o->batch = tables.get();
        o->sketch_ms = sk_ms_total;
        o->occ = new OrderedOcc;
        if (chunks.size() == 1) {
            *o->occ = std::move(chunks[0]);
        } else {
            OrderedOcc &out = *o->occ;
            out.n = n_total;
            out.hash.alloc(n_total);
            out.kmer.alloc(n_total);
            uint64_t at = 0;
            for (OrderedOcc &c : chunks) {
                if (c.n) {
                    SW_HIP(hipMemcpyAsync(out.hash.p + at, c.hash.p, c.n * 8, hipMemcpyDeviceToDevice, st));
                    SW_HIP(hipMemcpyAsync(out.kmer.p + at, c.kmer.p, c.n * 8, hipMemcpyDeviceToDevice, st));
                }
                at += c.n;
                c = OrderedOcc();                                // (released under st: stream-ordered behind its copies)
            }
        }
        *batch_out = tables.release();
        *occ_out = o.release();
    });
}

int sw_occ_size(const sw_occ *o, uint64_t *n, double *sketch_ms)
{
    return guarded([&] {
        *n = o->occ->n;
        if (sketch_ms) *sketch_ms = o->sketch_ms;
    });
}

void sw_occ_free(sw_occ *o)
{
    if (!o) return;
    StreamScope scope(o->last_stream);
    delete o;
}

int sw_occ_partition(const sw_occ *o, const uint64_t *bounds, uint64_t n_bounds, uint64_t rec_offset, void *rows_dev,
                     void *perm_dev, uint64_t *counts, void *stream)
{
    return guarded([&] {
        StreamScope scope((hipStream_t)stream);
        const_cast<sw_occ *>(o)->last_stream = (hipStream_t)stream;
        occ_partition(*o->occ, bounds, (uint32_t)n_bounds, rec_offset, (uint64_t *)rows_dev, (uint32_t *)perm_dev, counts,
                      (hipStream_t)stream);
    });
}

int sw_occ_adjacency(const sw_occ *o, const void *perm_dev, const void *rank_by_row_dev, uint64_t n_bits, uint64_t asm_bits,
                     uint64_t asm_base, const uint64_t *rank_bounds, uint64_t n_bounds, void *rows_dev, uint64_t *counts,
                     void *stream)
{
    return guarded([&] {
        if (n_bits < 1 || n_bits > 32) raise(SW_ERR_VALUE, "n_bits must be in [1, 32]");
        if (asm_bits && 2 * n_bits + asm_bits > 64) raise(SW_ERR_VALUE, "packed adjacency keys need 2 n_bits + asm_bits <= 64");
        StreamScope scope((hipStream_t)stream);
        const_cast<sw_occ *>(o)->last_stream = (hipStream_t)stream;
        occ_adjacency(*o->occ, o->batch->d_rec_asm.p, (const uint32_t *)perm_dev, (const uint32_t *)rank_by_row_dev,
                      (unsigned)n_bits, (unsigned)asm_bits, asm_base, rank_bounds, (uint32_t)n_bounds, (uint64_t *)rows_dev,
                      counts, (hipStream_t)stream);
    });
}

int sw_slice_edges(sw_index *ix, const void *adj_rows_dev, uint64_t m, uint64_t n_bits, uint64_t asm_bits,
                   const void *rank_hash_dev, void *stream)
{
    return guarded([&] {
        StreamScope scope((hipStream_t)stream);
        const_cast<sw_index *>(ix)->last_stream = (hipStream_t)stream;
        Event e0, e1;
        SW_HIP(hipEventRecord(e0, (hipStream_t)stream));
        slice_edges(*ix, (const uint64_t *)adj_rows_dev, m, (unsigned)n_bits, (unsigned)asm_bits,
                    (const uint64_t *)rank_hash_dev, (hipStream_t)stream);
        SW_HIP(hipEventRecord(e1, (hipStream_t)stream));
        SW_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        SW_HIP(hipEventElapsedTime(&ms, e0, e1));
        ix->timings.edges_ms = ms;
    });
}

int sw_sort_keys64(void *keys_dev, void *alt_dev, uint64_t n, uint64_t begin_bit, uint64_t end_bit, void *stream, int *sorted_in_alt,
                   double *ms)
{
    return guarded([&] {
        require_device();
        if (begin_bit > end_bit || end_bit > 64) raise(SW_ERR_VALUE, "bit range must be inside [0, 64]");
        StreamScope scope((hipStream_t)stream);
        uint64_t *k = (uint64_t *)keys_dev, *a = (uint64_t *)alt_dev;
        DevArray<uint32_t> fail(1);
        SW_HIP(hipMemsetAsync(fail.p, 0, 4, (hipStream_t)stream));
        Event e0, e1;
        SW_HIP(hipEventRecord(e0, (hipStream_t)stream));
        sort_keys64(k, a, n, (unsigned)begin_bit, (unsigned)end_bit, (hipStream_t)stream, fail.p);
        SW_HIP(hipEventRecord(e1, (hipStream_t)stream));
        uint32_t failed = 0;
        SW_HIP(hipMemcpyAsync(&failed, fail.p, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
        SW_HIP(hipEventSynchronize(e1));
        SW_HIP(hipStreamSynchronize((hipStream_t)stream));
        check_sort_failed(failed);
        float t = 0.f;
        SW_HIP(hipEventElapsedTime(&t, e0, e1));
        if (ms) *ms = t;
        *sorted_in_alt = (k == (uint64_t *)alt_dev) ? 1 : 0;
    });
}

int sw_radix_rank_mode(int *mode)
{
    return guarded([&] {
        require_device();
        *mode = radix_rank_mode();
    });
}

int sw_order_guard_trips(uint64_t *node_sort, uint64_t *edge_sort)
{
    return guarded([&] {
        if (node_sort) *node_sort = g_guard_trips[0].load();
        if (edge_sort) *edge_sort = g_guard_trips[1].load();
    });
}

int sw_sort_pairs32(void *keys_dev, void *keys_alt_dev, void *vals_dev, void *vals_alt_dev, uint64_t n, uint64_t end_bit, void *stream,
                    int *sorted_in_alt, double *ms)
{
    return guarded([&] {
        require_device();
        if (end_bit == 0 || end_bit > 32 || end_bit % 8) raise(SW_ERR_VALUE, "end_bit must be 8, 16, 24 or 32");
        StreamScope scope((hipStream_t)stream);
        uint32_t *k = (uint32_t *)keys_dev, *ka = (uint32_t *)keys_alt_dev;
        OccPay *v = (OccPay *)vals_dev, *va = (OccPay *)vals_alt_dev;
        DevArray<uint32_t> fail(1);
        SW_HIP(hipMemsetAsync(fail.p, 0, 4, (hipStream_t)stream));
        Event e0, e1;
        SW_HIP(hipEventRecord(e0, (hipStream_t)stream));
        sort_pairs32(k, ka, v, va, n, (unsigned)end_bit, (hipStream_t)stream, fail.p);
        SW_HIP(hipEventRecord(e1, (hipStream_t)stream));
        uint32_t failed = 0;
        SW_HIP(hipMemcpyAsync(&failed, fail.p, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
        SW_HIP(hipEventSynchronize(e1));
        SW_HIP(hipStreamSynchronize((hipStream_t)stream));
        check_sort_failed(failed);
        float t = 0.f;
        SW_HIP(hipEventElapsedTime(&t, e0, e1));
        if (ms) *ms = t;
        *sorted_in_alt = (k == (uint32_t *)keys_alt_dev) ? 1 : 0;
    });
}

int sw_edge_buckets(void *keys_dev, void *alt_dev, uint64_t m, uint64_t key_bits, uint64_t cap, uint64_t slots, const void *hist_top_dev,
                    void *ukeys_dev, void *ucnt_dev, uint64_t *n_runs, int *done, int *keys_in_alt, void *stream)
{
    return guarded([&] {
        if (!n_runs || !done || !keys_in_alt) raise(SW_ERR_VALUE, "n_runs, done and keys_in_alt must not be NULL");
        if (key_bits < 1 || key_bits > 62) raise(SW_ERR_VALUE, "key_bits must be in [1, 62] (two node ranks of less than 32 bits)");
        if (cap >> 32) raise(SW_ERR_VALUE, "cap must be below 2^32");
        if (m && (!keys_dev || !alt_dev || !ukeys_dev || !ucnt_dev)) raise(SW_ERR_VALUE, "keys, alt, ukeys and ucnt must not be NULL");
        *n_runs = 0;
        *done = 0;
        *keys_in_alt = 0;
        if (m == 0) return;   // (edges_from_pairs never sorts an empty set)
        require_device();
        StreamScope scope((hipStream_t)stream);
        uint64_t *k = (uint64_t *)keys_dev, *a = (uint64_t *)alt_dev;
        DevArray<uint32_t> fail(1);
        SW_HIP(hipMemsetAsync(fail.p, 0, 4, (hipStream_t)stream));
        uint32_t runs = 0;
        const int declined = radix_edge_buckets(k, a, m, (unsigned)key_bits, (1ull << key_bits) - 1ull, (const unsigned long long *)hist_top_dev,
                                                (uint32_t)cap, (uint32_t)std::min<uint64_t>(slots, 0xFFFFFFFFull), (uint64_t *)ukeys_dev,
                                                (uint32_t *)ucnt_dev, &runs, (hipStream_t)stream, fail.p,
                                                getenv("SEQWIN_AMD_DEBUG_EDGE_REPAIR") != nullptr);
        uint32_t failed = 0;
        SW_HIP(hipMemcpyAsync(&failed, fail.p, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
        SW_HIP(hipStreamSynchronize((hipStream_t)stream));
        check_sort_failed(failed);
        *keys_in_alt = (k == (uint64_t *)alt_dev) ? 1 : 0;
        *done = declined ? 0 : 1;
        *n_runs = declined ? 0 : runs;
    });
}

int sw_index_ranks_marked(const sw_index *ix, int *marked)
{
    return guarded([&] { *marked = ix->ranks_marked ? 1 : 0; });
}

int sw_occ_adjacency_pairs(const sw_occ *o, const void *rank_by_row_dev, const uint64_t *node_base, uint64_t n_owners, uint64_t asm_base,
                           const uint64_t *rank_bounds, uint64_t n_bounds, void *keys_dev, uint64_t *counts, uint64_t *cand_counts,
                           uint64_t *key_bits, void *stream)
{
    return guarded([&] {
        if (occ_partition_owners(*o->occ) == 0) raise(SW_ERR_VALUE, "sw_occ_adjacency_pairs needs the tuples partitioned by sw_occ_partition");
        if (n_owners != occ_partition_owners(*o->occ))
            raise(SW_ERR_VALUE, "node_base must hold one entry per owner of the tuple partition, plus the total");
        StreamScope scope((hipStream_t)stream);
        const_cast<sw_occ *>(o)->last_stream = (hipStream_t)stream;
        occ_adjacency_pairs(*o->occ, o->batch->d_rec_asm.p, (const uint32_t *)rank_by_row_dev, node_base, asm_base, rank_bounds,
                            (uint32_t)n_bounds, (uint64_t *)keys_dev, counts, cand_counts, key_bits, (hipStream_t)stream);
    });
}

int sw_occ_candidates(const sw_occ *o, void *rows_dev, void *stream)
{
    return guarded([&] {
        const_cast<sw_occ *>(o)->last_stream = (hipStream_t)stream;
        if (o->occ->cand_rows.n)
            SW_HIP(hipMemcpyAsync(rows_dev, o->occ->cand_rows.p, o->occ->cand_rows.n * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    });
}

int sw_slice_edges_pairs(sw_index *ix, void *keys_dev, uint64_t m, const void *cand_rows_dev, uint64_t n_cand, uint64_t lo_bits,
                         uint64_t hi_bits, uint64_t lo_base, uint64_t asm_bits, const void *rank_hash_dev, const uint64_t *node_base,
                         uint64_t n_owners, uint64_t pad, void *stream)
{
    return guarded([&] {
        StreamScope scope((hipStream_t)stream);
        const_cast<sw_index *>(ix)->last_stream = (hipStream_t)stream;
        Event e0, e1;
        SW_HIP(hipEventRecord(e0, (hipStream_t)stream));
        slice_edges_pairs(*ix, (uint64_t *)keys_dev, m, (const uint64_t *)cand_rows_dev, n_cand, (unsigned)lo_bits, (unsigned)hi_bits,
                          lo_base, (unsigned)asm_bits, (const uint64_t *)rank_hash_dev, node_base, (uint32_t)n_owners, pad,
                          (hipStream_t)stream);
        SW_HIP(hipEventRecord(e1, (hipStream_t)stream));
        SW_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        SW_HIP(hipEventElapsedTime(&ms, e0, e1));
        ix->timings.edges_ms = ms;
    });
}

int sw_index_edge_hash_requests(sw_index *ix, const uint64_t *node_base, uint64_t n_owners, uint64_t *counts, uint64_t *n_requests,
                                void *stream)
{
    return guarded([&] {
        StreamScope scope((hipStream_t)stream);
        ix->last_stream = (hipStream_t)stream;
        *n_requests = edge_hash_requests(*ix, node_base, (uint32_t)n_owners, counts, (hipStream_t)stream);
    });
}

int sw_index_edge_hash_request_rows(const sw_index *ix, void *local_ranks_dev, void *stream)
{
    return guarded([&] { edge_hash_request_rows(*ix, (uint32_t *)local_ranks_dev, (hipStream_t)stream); });
}

int sw_index_node_hash_lookup(const sw_index *ix, const void *local_ranks_dev, uint64_t n, void *hashes_dev, void *stream)
{
    return guarded([&] {
        StreamScope scope((hipStream_t)stream);
        const_cast<sw_index *>(ix)->last_stream = (hipStream_t)stream;
        node_hash_lookup(*ix, (const uint32_t *)local_ranks_dev, n, (uint64_t *)hashes_dev, (hipStream_t)stream);
    });
}

int sw_index_edge_hash_attach(sw_index *ix, const void *replies_dev, uint64_t n, void *stream)
{
    return guarded([&] {
        StreamScope scope((hipStream_t)stream);
        ix->last_stream = (hipStream_t)stream;
        edge_hash_attach(*ix, (const uint64_t *)replies_dev, n, (hipStream_t)stream);
    });
}

int sw_index_node_hashes(const sw_index *ix, void *dst_dev, void *stream)
{
    return guarded([&] {
        StreamScope scope((hipStream_t)stream);
        const_cast<sw_index *>(ix)->last_stream = (hipStream_t)stream;
        index_node_hashes(*ix, (uint64_t *)dst_dev, (hipStream_t)stream);
    });
}

int sw_index_device_ptrs(const sw_index *ix, void **kmers, void **nodes, void **edges)
{
    return guarded([&] {
        if (kmers) *kmers = ix->kmers.p;
        if (nodes) *nodes = ix->nodes.p;
        if (edges) *edges = ix->edges.p;
    });
}

int sw_index_occ_rows(const sw_index *ix, uint64_t rec_offset, void *rows_dev, void *stream)
{
    return guarded([&] {
        StreamScope scope((hipStream_t)stream);
        const_cast<sw_index *>(ix)->last_stream = (hipStream_t)stream;
        index_occ_rows(*ix, rec_offset, (uint64_t *)rows_dev, (hipStream_t)stream);
    });
}

int sw_index_edge_rows(const sw_index *ix, void *rows_dev, void *stream)
{
    return guarded([&] {
        if (ix->n_edges)
            SW_HIP(hipMemcpyAsync(rows_dev, ix->edges.p, ix->n_edges * sizeof(sw_edge), hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream));
    });
}

int sw_index_splits(const sw_index *ix, const uint64_t *node_bounds, const uint64_t *edge_bounds, uint64_t n_bounds,
                    uint64_t *occ_split, uint64_t *edge_split, void *stream)
{
    return guarded([&] {
        StreamScope scope((hipStream_t)stream);
        const_cast<sw_index *>(ix)->last_stream = (hipStream_t)stream;
        index_splits(*ix, node_bounds, edge_bounds, (uint32_t)n_bounds, occ_split, edge_split, (hipStream_t)stream);
    });
}

static void merge_like(const void *occ_rows_dev, uint64_t n_occ, const void *edge_rows_dev, uint64_t n_edge_rows,
                       uint64_t kmer_base, const uint32_t *record_offsets, const uint8_t *is_targets, uint64_t n_assemblies,
                       void *stream, uint32_t *d_rank_out, sw_index **out);

int sw_index_merge(const void *occ_rows_dev, uint64_t n_occ, const void *edge_rows_dev, uint64_t n_edge_rows,
                   uint64_t kmer_base, const uint32_t *record_offsets, const uint8_t *is_targets, uint64_t n_assemblies,
                   void *stream, sw_index **out)
{
    return guarded([&] {
        merge_like(occ_rows_dev, n_occ, edge_rows_dev, n_edge_rows, kmer_base, record_offsets, is_targets, n_assemblies,
                   stream, nullptr, out);
    });
}

int sw_slice_build(const void *rows_dev, uint64_t n, uint64_t kmer_base, const uint32_t *record_offsets,
                   const uint8_t *is_targets, uint64_t n_assemblies, void *ranks_dev, void *stream, sw_index **out)
{
    return guarded([&] {
        merge_like(rows_dev, n, nullptr, 0, kmer_base, record_offsets, is_targets, n_assemblies, stream,
                   (uint32_t *)ranks_dev, out);
    });
}

static void merge_like(const void *occ_rows_dev, uint64_t n_occ, const void *edge_rows_dev, uint64_t n_edge_rows,
                       uint64_t kmer_base, const uint32_t *record_offsets, const uint8_t *is_targets, uint64_t n_assemblies,
                       void *stream, uint32_t *d_rank_out, sw_index **out)
{
    {
        require_device();
        hipStream_t st = (hipStream_t)stream;
        StreamScope scope(st);
        std::unique_ptr<sw_index> ix(new sw_index);
        ix->last_stream = st;
        SW_HIP(hipGetDevice(&ix->device));
        uint64_t n_tar = 0, n_neg = 0;
        DevArray<uint8_t> d_tar;
        DevArray<uint32_t> d_rec_asm;
        uint32_t n_records = 0;
        if (is_targets) check_targets(is_targets, n_assemblies, &n_tar, &n_neg);
        if (record_offsets && (is_targets || d_rank_out)) {   // the record -> assembly table: counts, repeat marks of a slice build
            n_records = record_offsets[n_assemblies];
            std::vector<uint32_t> rec_asm(n_records);
            for (uint64_t a = 0; a < n_assemblies; ++a)
                for (uint32_t r = record_offsets[a]; r < record_offsets[a + 1]; ++r) rec_asm[r] = (uint32_t)a;
            d_rec_asm.alloc(n_records);
            if (n_records) SW_HIP(hipMemcpyAsync(d_rec_asm.p, rec_asm.data(), (size_t)n_records * 4, hipMemcpyHostToDevice, st));
            if (is_targets) {
                d_tar.alloc(n_assemblies);
                SW_HIP(hipMemcpyAsync(d_tar.p, is_targets, n_assemblies, hipMemcpyHostToDevice, st));
            }
            SW_HIP(hipStreamSynchronize(st));
        }
        Event e0, e1;
        SW_HIP(hipEventRecord(e0, st));
        merge_build((const uint64_t *)occ_rows_dev, n_occ, (const uint64_t *)edge_rows_dev, n_edge_rows, kmer_base,
                    d_rec_asm.p, n_records, is_targets ? d_tar.p : nullptr, n_tar, n_neg, st, *ix, d_rank_out);
        SW_HIP(hipEventRecord(e1, st));
        SW_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        SW_HIP(hipEventElapsedTime(&ms, e0, e1));
        ix->timings.total_ms = ms;
        *out = ix.release();
    }
}

int sw_sketch(const sw_batch *b, uint64_t kmerlen, uint64_t windowsize, void *stream, uint64_t *out_hash, sw_kmer *kmers,
              uint64_t cap, uint64_t *n_out)
{
    return guarded([&] {
        sw_batch &bb = *const_cast<sw_batch *>(b);
        StreamScope scope((hipStream_t)stream);
        Plan &plan = get_plan(bb, kmerlen, windowsize);
        SketchOut sk;
        run_sketch(bb, plan, (hipStream_t)stream, sk, nullptr);
        *n_out = sk.n_occ;
        if (!out_hash || !kmers || cap < sk.n_occ) return;
        OrderedOcc occ;
        order_tuples(sk, plan, (hipStream_t)stream, occ);
        *n_out = occ.n;   // (a window above SW_MAX_WINDOW: fewer than the size query's upper bound)
        if (occ.n) {
            SW_HIP(hipMemcpy(out_hash, occ.hash.p, occ.n * 8, hipMemcpyDeviceToHost));
            SW_HIP(hipMemcpy(kmers, occ.kmer.p, occ.n * 8, hipMemcpyDeviceToHost));  // pos | rec << 32 == sw_kmer layout
        }
    });
}

// low_memory (build.cpp:264-325 keeps the peak down by recomputing the sketches in a second pass): here the assemblies
// stream through HBM in consecutive chunks -- ingest, upload, sketch and order one chunk, keep only its 24 B per
// minimizer, release its packed bases / stage slots / host buffers -- and the index is built once from the concatenated
// tuple stream.  That stream is exactly what the one-shot build sorts, so the result is identical by construction.
// consecutive assemblies [a0, a1) of up to ~chunk_bp bases, estimated from the file sizes (gz: x4), at least one
static size_t chunk_end(const char *const *paths, size_t n_paths, size_t a0, uint64_t chunk_bp)
{
    size_t a1 = a0;
    uint64_t est = 0;
    while (a1 < n_paths && (a1 == a0 || est < chunk_bp)) {
        uint64_t sz = 0;
        if (FILE *f = fopen(paths[a1], "rb")) {
            if (fseek(f, 0, SEEK_END) == 0) { const long t = ftell(f); sz = t > 0 ? (uint64_t)t : 0; }
            fclose(f);
        }
        const size_t len = strlen(paths[a1]);
        if (len > 3 && !strcmp(paths[a1] + len - 3, ".gz")) sz *= 4;
        if (a1 > a0 && est + sz > chunk_bp) break;
        est += sz;
        ++a1;
    }
    return a1;
}

static void build_chunked(const char *const *paths, size_t n_paths, uint64_t k, uint64_t w, uint64_t n_cpu, uint64_t chunk_bp,
                          GraphHost &g, double *ingest_ms, double *device_ms)
{
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    StreamScope scope(nullptr);
    std::vector<OrderedOcc> chunks;
    std::vector<uint64_t> rec_base;
    std::vector<uint32_t> rec_asm;
    g.record_offsets.assign(1, 0);
    uint64_t n_records = 0;
    size_t a0 = 0;
    while (a0 < n_paths) {
        const size_t a1 = chunk_end(paths, n_paths, a0, chunk_bp);
        const auto t0 = now();
        sw_batch b;
        SW_HIP(hipGetDevice(&b.device));
        ingest_to_device(paths + a0, a1 - a0, n_cpu, b);
        const auto t1 = now();
        *ingest_ms += ms(t0, t1);
        Plan &plan = get_plan(b, k, w);
        SketchOut sk;
        run_sketch(b, plan, nullptr, sk, nullptr);
        chunks.emplace_back();
        order_tuples(sk, plan, nullptr, chunks.back(), true);
        SW_HIP(hipStreamSynchronize(nullptr));   // the batch and the stage arrays go out of scope
        *device_ms += ms(t1, now());
        rec_base.push_back(n_records);
        const HostBatch &h = b.host;
        for (uint64_t a = 0; a < h.n_assemblies; ++a) {
            const uint64_t nr = h.record_offsets[a + 1] - h.record_offsets[a];
            if (n_records + nr > UINT32_MAX) raise(SW_ERR_RUNTIME, "Total number of FASTA records exceeds uint32 range");   // build.cpp:136-147
            rec_asm.insert(rec_asm.end(), nr, (uint32_t)(a0 + a));
            n_records += nr;
            g.record_offsets.push_back((uint32_t)n_records);
        }
        g.ids_blob += h.ids_blob;
        g.total_bp += h.total_bp;
        a0 = a1;
    }
    g.n_assemblies = n_paths;
    const auto t2 = now();
    OrderedOcc occ;
    concat_occ(chunks, rec_base, nullptr, occ);
    DevArray<uint32_t> d_rec_asm(n_records);
    if (n_records) SW_HIP(hipMemcpyAsync(d_rec_asm.p, rec_asm.data(), n_records * 4, hipMemcpyHostToDevice, nullptr));
    g.ix.device = 0;
    SW_HIP(hipGetDevice(&g.ix.device));
    build_index(d_rec_asm.p, n_records, n_paths, occ, nullptr, 0, 0, nullptr, g.ix);
    SW_HIP(hipStreamSynchronize(nullptr));
    *device_ms += ms(t2, now());
}

// r06 (VERDICT r5 missing #5): ingest and sketch overlapped inside one sw_build.  The reference interleaves reading and minimizing
// per assembly (build.cpp:98-256: every worker thread reads a file and minimizes it); here the files are parsed by the host threads
// in consecutive chunks while a second host thread drives the device through the PREVIOUS chunk -- launch plan, sketch, ordered
// tuples (24 B per minimizer) -- on a stream of its own; the index is then built once from the concatenated tuple stream, exactly
// as the chunked low-memory build does (identical arrays by construction).  What it can hide is the sketch (half of the device
// time); the sorts need every tuple.  What it costs: the ordered copy per chunk instead of the node sort reading the stage, the
// concatenation, a tail of idle parsers at every chunk boundary.  SEQWIN_AMD_PIPELINE=1 takes this route, measurements: NOTES.md.
static void build_pipelined(const char *const *paths, size_t n_paths, uint64_t k, uint64_t w, uint64_t n_cpu, uint64_t chunk_bp, GraphHost &g,
                            double *ingest_ms, double *device_ms)
{
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    int dev = 0;
    SW_HIP(hipGetDevice(&dev));
    std::vector<std::pair<size_t, size_t>> ranges;
    for (size_t a0 = 0; a0 < n_paths;) {
        const size_t a1 = chunk_end(paths, n_paths, a0, chunk_bp);
        ranges.emplace_back(a0, a1);
        a0 = a1;
    }
    std::vector<OrderedOcc> chunks(ranges.size());
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::pair<std::unique_ptr<sw_batch>, size_t>> q;
    bool no_more = false, failed = false;
    std::exception_ptr err;
    double sketch_ms = 0;
    auto dev_work = [&] {
        try {
            SW_HIP(hipSetDevice(dev));
            static std::mutex smu;
            static std::map<int, hipStream_t> *streams = new std::map<int, hipStream_t>;   // one per device, kept: pool blocks remember it
            hipStream_t S = nullptr;
            {
                std::lock_guard<std::mutex> lock(smu);
                hipStream_t &ref = (*streams)[dev];
                if (!ref) SW_HIP(hipStreamCreateWithFlags(&ref, hipStreamNonBlocking));
                S = ref;
            }
            StreamScope scope(S);
            for (;;) {
                std::unique_ptr<sw_batch> b;
                size_t c = 0;
                {
                    std::unique_lock<std::mutex> lock(mu);
                    cv.wait(lock, [&] { return !q.empty() || no_more; });
                    if (q.empty()) break;
                    b = std::move(q.front().first);
                    c = q.front().second;
                    q.pop_front();
                }
                cv.notify_all();
                Plan &plan = get_plan(*b, k, w);
                SketchOut sk;
                float t = 0.f;
                run_sketch(*b, plan, S, sk, &t);
                sketch_ms += t;
                order_tuples(sk, plan, S, chunks[c], true);
                SW_HIP(hipStreamSynchronize(S));   // the batch, its plan and the stage go (released under S)
                sk = SketchOut();
                b.reset();
            }
        } catch (...) {
            std::lock_guard<std::mutex> lock(mu);
            if (!err) err = std::current_exception();
            failed = true;
            q.clear();
            cv.notify_all();
        }
    };
    std::thread dev_thread(dev_work);
    std::vector<uint64_t> rec_base;
    std::vector<uint32_t> rec_asm;
    g.record_offsets.assign(1, 0);
    uint64_t n_records = 0;
    const auto t0 = now();
    try {
        for (size_t c = 0; c < ranges.size(); ++c) {
            const size_t a0 = ranges[c].first, a1 = ranges[c].second;
            std::unique_ptr<sw_batch> b(new sw_batch);
            b->device = dev;
            ingest_to_device(paths + a0, a1 - a0, n_cpu, *b);
            rec_base.push_back(n_records);
            const HostBatch &h = b->host;
            for (uint64_t a = 0; a < h.n_assemblies; ++a) {
                const uint64_t nr = h.record_offsets[a + 1] - h.record_offsets[a];
                if (n_records + nr > UINT32_MAX) raise(SW_ERR_RUNTIME, "Total number of FASTA records exceeds uint32 range");   // build.cpp:136-147
                rec_asm.insert(rec_asm.end(), nr, (uint32_t)(a0 + a));
                n_records += nr;
                g.record_offsets.push_back((uint32_t)n_records);
            }
            g.ids_blob += h.ids_blob;
            g.total_bp += h.total_bp;
            std::unique_lock<std::mutex> lock(mu);
            cv.wait(lock, [&] { return q.size() < 2 || failed; });   // (at most two parsed chunks wait for the device)
            if (failed) break;
            q.emplace_back(std::move(b), c);
            cv.notify_all();
        }
    } catch (...) {
        {
            std::lock_guard<std::mutex> lock(mu);
            if (!err) err = std::current_exception();
            no_more = true;
            q.clear();
        }
        cv.notify_all();
        dev_thread.join();
        std::rethrow_exception(err);
    }
    const auto t1 = now();
    {
        std::lock_guard<std::mutex> lock(mu);
        no_more = true;
    }
    cv.notify_all();
    dev_thread.join();
    if (err) std::rethrow_exception(err);
    *ingest_ms = ms(t0, t1);
    g.n_assemblies = n_paths;
    StreamScope scope(nullptr);
    OrderedOcc occ;
    concat_occ(chunks, rec_base, nullptr, occ);
    DevArray<uint32_t> d_rec_asm(n_records);
    if (n_records) SW_HIP(hipMemcpyAsync(d_rec_asm.p, rec_asm.data(), n_records * 4, hipMemcpyHostToDevice, nullptr));
    SW_HIP(hipGetDevice(&g.ix.device));
    build_index(d_rec_asm.p, n_records, n_paths, occ, nullptr, 0, 0, nullptr, g.ix);
    SW_HIP(hipStreamSynchronize(nullptr));
    g.ix.timings.sketch_ms = sketch_ms;
    g.ix.timings.total_bp = g.total_bp;
    *device_ms = ms(t1, now());   // (what the caller waits for behind the last file: the last chunk's sketch, the concatenation, the index)
}

int sw_build(const char *const *assembly_paths, size_t n_assemblies, uint64_t kmerlen, uint64_t windowsize, uint64_t n_cpu,
             int low_memory, sw_graph **out)
{
    return guarded([&] {
        check_kw(kmerlen, windowsize);
        require_device();
        const bool dbg = getenv("SEQWIN_AMD_DEBUG_TIMING") != nullptr;
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::milli>(b - a).count();
        };
        {   // the previous build's resident index makes room
            Resident &r = resident();
            std::lock_guard<std::mutex> lock(r.mu);
            r.ix.reset();
        }
        {
            ResidentMulti &rm = resident_multi();
            std::lock_guard<std::mutex> lock(rm.mu);
            rm.mg.reset();
        }
        std::unique_ptr<sw_graph> g(new sw_graph);
        double ingest_ms = 0, device_ms = 0;
        // SEQWIN_AMD_LOWMEM_CHUNK_MBP: bases (in Mbp) per chunk of a low-memory build (default 4096: ~1 GiB packed);
        // SEQWIN_AMD_HBM_BUDGET_GB: take the chunked route whenever the files' bases would not fit this budget
        uint64_t chunk_bp = 4096ull << 20;
        if (const char *e = getenv("SEQWIN_AMD_LOWMEM_CHUNK_MBP")) chunk_bp = (uint64_t)std::max(0ll, atoll(e)) << 20;
        bool chunked = low_memory != 0 && n_assemblies > 1;
        if (const char *e = getenv("SEQWIN_AMD_HBM_BUDGET_GB")) {
            // working set of the one-shot build: ~1 B per base at w = 200 (packed bases + stage slots + tuples and their sort buffers)
            const uint64_t budget = (uint64_t)std::max(1.0, atof(e) * 1073741824.0);
            uint64_t est = 0;
            for (size_t i = 0; i < n_assemblies; ++i)
                if (FILE *f = fopen(assembly_paths[i], "rb")) {
                    if (fseek(f, 0, SEEK_END) == 0) { const long t = ftell(f); est += t > 0 ? (uint64_t)t : 0; }
                    fclose(f);
                }
            if (est > budget && n_assemblies > 1) {
                chunked = true;
                chunk_bp = std::min(chunk_bp, budget / 2);
            }
        }
        // SEQWIN_AMD_PIPELINE=1: sketch the chunks already parsed while later files are still being parsed (build_pipelined above);
        // SEQWIN_AMD_PIPELINE_CHUNK_MBP sizes the chunks (default: the input in 8 chunks, at least 512 Mbp each)
        bool pipelined = false;
        uint64_t pipe_chunk_bp = 0;
        if (const char *e = getenv("SEQWIN_AMD_PIPELINE"))
            if (atoi(e) != 0 && !chunked && n_assemblies >= 4) {
                uint64_t est = 0;
                for (size_t i = 0; i < n_assemblies; ++i)
                    if (FILE *f = fopen(assembly_paths[i], "rb")) {
                        if (fseek(f, 0, SEEK_END) == 0) { const long t = ftell(f); est += t > 0 ? (uint64_t)t : 0; }
                        fclose(f);
                    }
                pipe_chunk_bp = std::max<uint64_t>(est / 8, 512ull << 20);
                if (const char *c = getenv("SEQWIN_AMD_PIPELINE_CHUNK_MBP")) pipe_chunk_bp = (uint64_t)std::max(0ll, atoll(c)) << 20;
                pipelined = true;
            }
        const auto t0 = now();
        // r06: never fail where the reference succeeds (its indices are size_t, graph.hpp:28-41).  A build whose occurrences -- of the
        // whole job on one device, of a shard, or the rows of a slice -- exceed what 32-bit indices address ends in OccCapError;
        // the job is then split into more shards: the listed devices (SEQWIN_DEVICES), or the current one, taken round robin as
        // LOGICAL workers of multi.hip until every shard and slice fits (at most 16 owners, at most one per assembly).  On one card
        // the shards share its HBM, so a job of that size needs real devices to fit; the split itself is exercised by lowering the
        // bound (SEQWIN_AMD_OCC_CAP, tests).
        std::vector<int> devs = devices_from_env();
        int cur_dev = 0;
        SW_HIP(hipGetDevice(&cur_dev));
        const std::vector<int> base_devs = devs.size() > 1 ? devs : std::vector<int>(1, cur_dev);
        for (int attempt = 0;; ++attempt) {
            try {
                if (devs.size() > 1 && n_assemblies > 1) {
                    // one worker per listed device, the reference's partition of the assemblies, peer-to-peer exchanges (multi.hip)
                    g->g.multi.reset(new MultiGraph);
                    build_multi_device(assembly_paths, n_assemblies, kmerlen, windowsize, n_cpu, devs, *g->g.multi, chunked ? chunk_bp : 0);
                    MultiGraph &m = *g->g.multi;
                    device_ms = ms(t0, now());
                    g->g.record_offsets = m.record_offsets;
                    g->g.ids_blob = m.ids_blob;
                    g->g.n_assemblies = m.n_assemblies;
                    g->g.total_bp = m.total_bp;
                    g->g.ix.n_kmers = g->g.ix.n_nodes = g->g.ix.n_edges = 0;
                    for (auto &sl : m.slices) {   // (sizes of the whole; the arrays stay per device until sw_graph_export)
                        g->g.ix.n_kmers += sl->n_kmers;
                        g->g.ix.n_nodes += sl->n_nodes;
                        g->g.ix.n_edges += sl->n_edges;
                    }
                    log_message("info", "MI355X build over %zu %s (%s), node hashes to the edge owners by %s; %s%s", m.slices.size(),
                                attempt ? "shards" : "devices", attempt ? "split automatically: more occurrences than 32-bit indices address" : "SEQWIN_DEVICES",
                                m.hash_route, m.copy_route.c_str(), chunked ? "; every worker streams its shard through HBM in chunks (low_memory)" : "");
                } else if (chunked) {
                    build_chunked(assembly_paths, n_assemblies, kmerlen, windowsize, n_cpu, chunk_bp, g->g, &ingest_ms, &device_ms);
                } else if (pipelined) {
                    build_pipelined(assembly_paths, n_assemblies, kmerlen, windowsize, n_cpu, pipe_chunk_bp, g->g, &ingest_ms, &device_ms);
                } else {
                    std::unique_ptr<sw_batch> b(new sw_batch);
                    SW_HIP(hipGetDevice(&b->device));
                    ingest_to_device(assembly_paths, n_assemblies, n_cpu, *b);
                    const auto t1 = now();
                    do_index_build(*b, kmerlen, windowsize, nullptr, 0, 0, g->g.ix);
                    ingest_ms = ms(t0, t1);
                    device_ms = ms(t1, now());
                    g->g.record_offsets = b->host.record_offsets;
                    g->g.ids_blob = b->host.ids_blob;
                    g->g.n_assemblies = b->host.n_assemblies;
                    g->g.total_bp = b->host.total_bp;
                }
                break;
            } catch (const OccCapError &e) {
                const size_t have = devs.size() > 1 ? std::min(devs.size(), n_assemblies) : 1;
                const size_t limit = std::min<size_t>(16, n_assemblies);   // (occ_partition: at most 16 owners; a shard is whole assemblies)
                if (have >= limit) throw;
                // what overflowed was one of `have` parts: aim at 3/4 of the bound per part
                const double parts = (double)e.n / (0.75 * (double)occ_cap());
                size_t want = std::max(have + 1, (size_t)std::ceil(parts * (double)have));
                want = std::min(want, limit);
                log_message("info", "MI355X build: %s -- splitting the job into %zu shards (was %zu)", e.what(), want, have);
                devs.clear();
                for (size_t i = 0; i < want; ++i) devs.push_back(base_devs[i % base_devs.size()]);
                g.reset(new sw_graph);
                ingest_ms = device_ms = 0;
            }
        }
        // the reference logs its stages from native code (build.cpp:358-392 through log_python); two lines here
        log_message("info", "MI355X sketch + index: %llu assemblies, %.1f Mbp%s (ingest + upload %.1f ms, device %.1f ms)",
                    (unsigned long long)g->g.n_assemblies, g->g.total_bp / 1e6, chunked ? ", streamed through HBM in chunks" : "",
                    ingest_ms, device_ms);
        log_message("info", "MI355X index: %llu assemblies -> %llu minimizers, %llu nodes, %llu edges",
                    (unsigned long long)g->g.n_assemblies, (unsigned long long)g->g.ix.n_kmers, (unsigned long long)g->g.ix.n_nodes,
                    (unsigned long long)g->g.ix.n_edges);
        g->g.ingest_ms = ingest_ms;
        g->g.device_ms = device_ms;
        if (dbg)
            fprintf(stderr, "[seqwin_amd] sw_build: ingest+upload %.1f ms, device %.1f ms, total %.1f ms (%.1f Mbp%s)\n", ingest_ms,
                    device_ms, ms(t0, now()), g->g.total_bp / 1e6, chunked ? ", chunked" : "");
        *out = g.release();
    });
}

int sw_graph_sizes(const sw_graph *g, uint64_t *n_kmers, uint64_t *n_nodes, uint64_t *n_edges, uint64_t *n_assemblies,
                   uint64_t *ids_bytes, uint64_t *total_bp)
{
    return guarded([&] {
        *n_kmers = g->g.ix.n_kmers;
        *n_nodes = g->g.ix.n_nodes;
        *n_edges = g->g.ix.n_edges;
        *n_assemblies = g->g.n_assemblies;
        *ids_bytes = g->g.ids_blob.size();
        if (total_bp) *total_bp = g->g.total_bp;
    });
}

int sw_graph_stats(const sw_graph *g, double *out8)
{
    return guarded([&] {
        const GraphHost &h = g->g;
        const sw_timings &t = h.ix.timings;
        const double v[8] = {h.ingest_ms, h.device_ms, t.plan_ms, t.sketch_ms, t.order_ms, t.nodes_ms, t.edges_ms, h.export_ms};
        memcpy(out8, v, sizeof v);
    });
}

int sw_graph_export(const sw_graph *g, sw_kmer *kmers, sw_node *nodes, sw_edge *edges, uint32_t *record_offsets,
                    char *ids_blob)
{
    return guarded([&] {
        const GraphHost &h = g->g;
        struct ExportClock {   // (every way out of the call)
            double *dst;
            std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            ~ExportClock() { *dst = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
        } clock{&const_cast<GraphHost &>(h).export_ms};
        const sw_index &ix = h.ix;   // D2H straight into the caller's (numpy) buffers
        const auto t0 = std::chrono::steady_clock::now();
        const HostSpan spans[3] = {{kmers, ix.n_kmers * sizeof(sw_kmer)}, {nodes, ix.n_nodes * sizeof(sw_node)},
                                   {edges, ix.n_edges * sizeof(sw_edge)}};
        if (h.multi) {
            // the slices in owner order, each from its device (node ranges are already global: sw_slice_build's kmer_base)
            DeviceGuard home;   // (download / device_identity may throw on another device)
            uint64_t ko = 0, no = 0, eo = 0;
            for (auto &sl : h.multi->slices) {
                SW_HIP(hipSetDevice(sl->device));
                const HostSpan part[3] = {{kmers ? kmers + ko : nullptr, sl->n_kmers * sizeof(sw_kmer)},
                                          {nodes ? nodes + no : nullptr, sl->n_nodes * sizeof(sw_node)},
                                          {edges ? edges + eo : nullptr, sl->n_edges * sizeof(sw_edge)}};
                const void *const from[3] = {sl->kmers.p, sl->nodes.p, sl->edges.p};
                download(part, from, 3);
                ko += sl->n_kmers;
                no += sl->n_nodes;
                eo += sl->n_edges;
            }
            if (kmers && nodes && ix.n_kmers && !getenv("SEQWIN_AMD_NO_RESIDENT")) {   // identity of the whole from the slices' shares
                GraphHost &hm = const_cast<GraphHost &>(h);
                uint64_t kb = 0, nb = 0, sum[2] = {0, 0};
                for (auto &sl : h.multi->slices) {
                    SW_HIP(hipSetDevice(sl->device));
                    uint64_t part[2];
                    device_identity(*sl, 0, part, kb, nb);
                    sum[0] += part[0];
                    sum[1] += part[1];
                    kb += sl->n_kmers;
                    nb += sl->n_nodes;
                }
                hm.identity[0] = sum[0];
                hm.identity[1] = sum[1];
                hm.exported = true;
            }
            memcpy(record_offsets, h.record_offsets.data(), h.record_offsets.size() * 4);
            if (!h.ids_blob.empty()) memcpy(ids_blob, h.ids_blob.data(), h.ids_blob.size());
            return;
        }
        // r05: nodes and edges cross PCIe in a packed form when the result is large enough for the ring -- a node as {hash, number of
        // occurrences} (12 of its 40 bytes: start / stop are the running sum, the counts are zero in a graph sw_build made), an edge
        // with a 32-bit weight (20 of 24) -- and the copiers write the arrays out in full: 2 048 genomes 2.28 -> 1.67 GB, 15 000
        // genomes 13.1 -> 10.3 GB over a link that carries 31-34 GB/s.  Declined (device flag) if any node has counts, a range that
        // does not start where its predecessor's stops, or an edge weight above 2^32 - 1; SEQWIN_AMD_EXPORT_WHOLE=1 forces the plain form.
        bool packed = false;
        const size_t whole_total = ix.n_kmers * sizeof(sw_kmer) + ix.n_nodes * sizeof(sw_node) + ix.n_edges * sizeof(sw_edge);
        if (kmers && nodes && edges && ix.n_nodes && ix.n_edges && ix.n_kmers < (1ull << 32) && download_is_pipelined(whole_total) &&
            !SW_TEST_GETENV("SEQWIN_AMD_EXPORT_WHOLE")) {
            const uint64_t per = download_slot_bytes() / PACKED_NODE, n_chunks = (ix.n_nodes + per - 1) / per;
            DevArray<uint32_t> pn, pe, flag(1);
            DevArray<uint64_t> bases(n_chunks);
            bool room = true;
            try {   // (the packed copies need 12 B per node + 20 B per edge of HBM next to the index: without it the arrays go whole -- ADVICE r5)
                pn.alloc(ix.n_nodes * 3);
                pe.alloc(ix.n_edges * 5);
            } catch (const Error &e) {
                if (e.code != SW_ERR_DEVICE) throw;
                room = false;
                log_message("info", "sw_graph_export: no room in HBM for the packed form of nodes and edges: whole arrays");
            }
            SW_HIP(hipMemsetAsync(flag.p, 0, 4, nullptr));
            if (room)
            pack_export(ix.nodes.p, ix.n_nodes, ix.n_kmers, ix.edges.p, ix.n_edges, per, pn.p, bases.p, pe.p, flag.p, nullptr);
            uint32_t declined = room ? 0 : 1;
            std::vector<uint64_t> h_bases(n_chunks);
            if (room) SW_HIP(hipMemcpy(&declined, flag.p, 4, hipMemcpyDeviceToHost));
            if (!declined) {
                SW_HIP(hipMemcpy(h_bases.data(), bases.p, n_chunks * 8, hipMemcpyDeviceToHost));
                HostSpan ps[3] = {{kmers, ix.n_kmers * sizeof(sw_kmer)}, {nodes, ix.n_nodes * PACKED_NODE}, {edges, ix.n_edges * PACKED_EDGE}};
                ps[1].expand = EXPAND_NODES;
                ps[1].chunk_base = h_bases.data();
                ps[2].expand = EXPAND_EDGES;
                const void *const from[3] = {ix.kmers.p, pn.p, pe.p};
                download(ps, from, 3);
                packed = true;
            }
        }
        if (!packed) {
            const void *const from[3] = {ix.kmers.p, ix.nodes.p, ix.edges.p};
            download(spans, from, 3);
        }
        memcpy(record_offsets, h.record_offsets.data(), h.record_offsets.size() * 4);
        if (!h.ids_blob.empty()) memcpy(ids_blob, h.ids_blob.data(), h.ids_blob.size());
        if (kmers && nodes && ix.n_kmers && !getenv("SEQWIN_AMD_NO_RESIDENT")) {
            GraphHost &hm = const_cast<GraphHost &>(h);
            device_identity(ix, 0, hm.identity);
            hm.exported = true;
        }
        if (getenv("SEQWIN_AMD_DEBUG_TIMING"))
            fprintf(stderr, "[seqwin_amd] sw_graph_export: %.1f ms for %.1f MB\n",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                    (ix.n_kmers * sizeof(sw_kmer) + ix.n_nodes * sizeof(sw_node) + ix.n_edges * sizeof(sw_edge)) / 1e6);
    });
}

void sw_graph_free(sw_graph *g)
{
    if (g && g->g.exported && g->g.multi) {   // a multi-device graph: its slices stay on their devices for sw_get_penalty
        ResidentMulti &rm = resident_multi();
        std::lock_guard<std::mutex> lock(rm.mu);
        rm.mg = std::move(g->g.multi);
        rm.n_kmers = rm.n_nodes = 0;
        for (auto &sl : rm.mg->slices) {
            sl->edges.release();              // (get_penalty reads kmers and nodes only)
            sl->n_edges = 0;
            rm.n_kmers += sl->n_kmers;
            rm.n_nodes += sl->n_nodes;
        }
        rm.kmer_sum = g->g.identity[0];
        rm.node_sum = g->g.identity[1];
        delete g;
        return;
    }
    if (g && g->g.exported) {   // the exported index stays resident for the get_penalty / filter_kmers calls that follow
        Resident &r = resident();
        std::lock_guard<std::mutex> lock(r.mu);
        r.ix = std::move(g->g.ixp);
        if (r.ix) {   // get_penalty / filter_kmers read kmers and nodes only: the edges go back to the pool at once
            r.ix->edges.release();
            r.ix->n_edges = 0;
        }
        r.kmer_sum = g->g.identity[0];
        r.node_sum = g->g.identity[1];
    }
    delete g;
}

namespace {
struct FilterStash {
    const void *kmers = nullptr, *nodes = nullptr;
    uint64_t n_kmers = 0, n_nodes = 0, n_used = 0, used_sum = 0, nk = 0, nn = 0;
    uint64_t id[2] = {0, 0};   // position-dependent checksums of the caller's kmers / nodes (host_identity) at the size phase
    DevArray<sw_kmer> kout;
    DevArray<sw_node> nout;
    bool valid = false;
};
thread_local FilterStash g_filter_stash;
}  // namespace

void sw_resident_stats(uint64_t *out)
{
    Resident &r = resident();
    std::lock_guard<std::mutex> lock(r.mu);
    out[0] = r.ix ? r.ix->n_kmers : 0;
    out[1] = r.penalty_hits;
    out[2] = r.filter_hits;
    {
        ResidentMulti &rm = resident_multi();
        std::lock_guard<std::mutex> mlock(rm.mu);
        if (rm.mg) out[0] += rm.n_kmers;
        out[1] += rm.penalty_hits;
    }
}

void sw_pool_trim(void) { dev_pool_trim(); }
void sw_pool_debug_stats(uint64_t *out)
{
    out[0] = pool_debug() ? 1 : 0;
    out[1] = pool_debug_violations();
    out[2] = pool_handover_syncs();
}

void sw_release_resident(void)
{
    {
        ResidentMulti &rm = resident_multi();
        std::lock_guard<std::mutex> lock(rm.mu);
        rm.mg.reset();
    }
    Resident &r = resident();
    std::lock_guard<std::mutex> lock(r.mu);
    r.ix.reset();
    g_filter_stash = FilterStash();   // (this thread's pending sw_filter_kmers result as well)
}

int sw_get_penalty(const sw_kmer *kmers, uint64_t n_kmers, sw_node *nodes, uint64_t n_nodes, const uint32_t *record_offsets,
                   uint64_t n_record_offsets, const uint8_t *is_targets, uint64_t n_assemblies, uint64_t n_cpu)
{
    (void)n_cpu;
    return guarded([&] {
        // argument validation, messages as in filter.cpp:33-60
        if (n_record_offsets != n_assemblies + 1) raise(SW_ERR_VALUE, "len(record_offsets) must equal len(is_targets) + 1");
        if (n_record_offsets == 0 || record_offsets[0] != 0) raise(SW_ERR_VALUE, "record_offsets must start with 0");
        if (n_assemblies > UINT32_MAX) raise(SW_ERR_VALUE, "Number of assemblies exceeds uint32 range");
        for (uint64_t i = 0; i < n_assemblies; ++i)
            if (record_offsets[i + 1] < record_offsets[i]) raise(SW_ERR_VALUE, "record_offsets must be nondecreasing");
        uint64_t n_tar = 0, n_neg = 0;
        check_targets(is_targets, n_assemblies, &n_tar, &n_neg);
        if (n_kmers >= 0xFFFFFFFFull) raise(SW_ERR_VALUE, "more than 2^32-2 k-mers are not supported on one device");
        require_device();
        if (n_nodes == 0) return;

        const uint32_t n_records = record_offsets[n_assemblies];
        std::vector<uint32_t> rec_asm(n_records);
        for (uint64_t a = 0; a < n_assemblies; ++a)  // filter.cpp:68-87
            for (uint32_t r = record_offsets[a]; r < record_offsets[a + 1]; ++r) rec_asm[r] = (uint32_t)a;
        DevArray<uint32_t> d_rec_asm(n_records);
        DevArray<uint8_t> d_tar(n_assemblies);
        if (n_records) SW_HIP(hipMemcpy(d_rec_asm.p, rec_asm.data(), (size_t)n_records * 4, hipMemcpyHostToDevice));
        SW_HIP(hipMemcpy(d_tar.p, is_targets, n_assemblies, hipMemcpyHostToDevice));
        {   // a graph built over several devices whose slices are still where they were built: score every slice in place
            ResidentMulti &rm = resident_multi();
            std::unique_lock<std::mutex> mlock(rm.mu);
            if (rm.mg && rm.n_kmers == n_kmers && rm.n_nodes == n_nodes) {
                uint64_t id[2];
                host_identity(kmers, n_kmers, nodes, n_nodes, (unsigned)std::min<uint64_t>(std::max<uint64_t>(n_cpu, 1), 64), id);
                if (id[0] == rm.kmer_sum && id[1] == rm.node_sum) {
                    MultiGraph &mg = *rm.mg;
                    const size_t S = mg.slices.size();
                    std::vector<uint64_t> kb(S + 1, 0), nbv(S + 1, 0), errs(S, 0);
                    for (size_t q = 0; q < S; ++q) {
                        kb[q + 1] = kb[q] + mg.slices[q]->n_kmers;
                        nbv[q + 1] = nbv[q] + mg.slices[q]->n_nodes;
                    }
                    DeviceGuard home;   // (this thread scores slice 0 on that slice's device)
                    std::mutex emu;
                    std::exception_ptr eptr;
                    auto work = [&](size_t q) {
                        try {
                            sw_index &sl = *mg.slices[q];
                            SW_HIP(hipSetDevice(sl.device));
                            if (sl.n_nodes) {
                                DevArray<uint32_t> ra(n_records);
                                DevArray<uint8_t> tg(n_assemblies);
                                if (n_records) SW_HIP(hipMemcpy(ra.p, rec_asm.data(), (size_t)n_records * 4, hipMemcpyHostToDevice));
                                SW_HIP(hipMemcpy(tg.p, is_targets, n_assemblies, hipMemcpyHostToDevice));
                                slice_get_penalty(sl, kb[q], ra.p, n_records, tg.p, n_tar, n_neg, 0, &errs[q]);
                                SW_HIP(hipMemcpy(nodes + nbv[q], sl.nodes.p, sl.n_nodes * sizeof(sw_node), hipMemcpyDeviceToHost));
                            }
                        } catch (...) {
                            std::lock_guard<std::mutex> g(emu);
                            if (!eptr) eptr = std::current_exception();
                        }
                    };
                    std::vector<std::thread> th;
                    size_t started = 1;
                    try {
                        for (size_t q = 1; q < S; ++q, ++started) th.emplace_back(work, q);
                    } catch (...) {   // a thread could not be started: its slices are scored on this thread (joinable threads must be joined)
                    }
                    if (S) work(0);
                    for (size_t q = started; q < S; ++q) work(q);
                    for (auto &t : th) t.join();
                    if (eptr) std::rethrow_exception(eptr);
                    uint64_t err = 0;
                    for (uint64_t e : errs) err |= e;
                    if (err & 1) raise(SW_ERR_VALUE, "node range is outside kmers");
                    if (err & 2) raise(SW_ERR_VALUE, "record_idx is outside record_offsets range");
                    if (err & 4) raise(SW_ERR_VALUE, "record_idx must be nondecreasing within each node range");
                    ++rm.penalty_hits;
                    return;
                }
            }
        }
        // the arrays of the last sw_build are usually still in HBM (Resident): use them when the caller's are the same
        Resident &res = resident();
        ResidentLock rlock(res.mu);
        int dev = -1;
        SW_HIP(hipGetDevice(&dev));
        bool use_resident = false;
        uint64_t err = 0;
        if (res.ix && res.ix->device == dev && res.ix->n_kmers == n_kmers && res.ix->n_nodes == n_nodes) {
            // r05: while host threads verify that the caller's arrays are the resident ones (1.5 GB read for 2 048 genomes: half of this
            // call), the device already scores the resident arrays; if the check fails, the counts it wrote there are never read
            uint64_t id[2] = {0, 0}, spec_err = 0;
            std::exception_ptr id_fail;
            std::thread checker([&] {
                try {
                    host_identity(kmers, n_kmers, nodes, n_nodes, (unsigned)std::min<uint64_t>(std::max<uint64_t>(n_cpu, 1), 64), id);
                } catch (...) {
                    id_fail = std::current_exception();
                }
            });
            struct Join {
                std::thread &t;
                ~Join() { if (t.joinable()) t.join(); }
            } join{checker};
            device_get_penalty(res.ix->kmers.p, n_kmers, res.ix->nodes.p, n_nodes, d_rec_asm.p, n_records, d_tar.p, n_tar, n_neg, 0, &spec_err);
            checker.join();
            if (id_fail) std::rethrow_exception(id_fail);
            use_resident = id[0] == res.kmer_sum && id[1] == res.node_sum;
            if (use_resident) err = spec_err;
        }
        DevArray<sw_kmer> d_kmers;
        DevArray<sw_node> d_nodes;
        const sw_kmer *dk;
        sw_node *dn;
        if (use_resident) {
            dk = res.ix->kmers.p;
            dn = res.ix->nodes.p;
            ++res.penalty_hits;
        } else {
            rlock.unlock();
            d_kmers.alloc(n_kmers);
            d_nodes.alloc(n_nodes);
            if (n_kmers) SW_HIP(hipMemcpy(d_kmers.p, kmers, n_kmers * sizeof(sw_kmer), hipMemcpyHostToDevice));
            SW_HIP(hipMemcpy(d_nodes.p, nodes, n_nodes * sizeof(sw_node), hipMemcpyHostToDevice));
            dk = d_kmers.p;
            dn = d_nodes.p;
            device_get_penalty(dk, n_kmers, dn, n_nodes, d_rec_asm.p, n_records, d_tar.p, n_tar, n_neg, 0, &err);
        }
        if (err & 1) raise(SW_ERR_VALUE, "node range is outside kmers");
        if (err & 2) raise(SW_ERR_VALUE, "record_idx is outside record_offsets range");                    // filter.cpp:104-106,120-122
        if (err & 4) raise(SW_ERR_VALUE, "record_idx must be nondecreasing within each node range");        // filter.cpp:113-115
        // (measured at the end of r05: sending back only the 16 bytes per node that changed -- packed on the device, put into place
        // by the download's copiers -- saves 60 % of the PCIe bytes and no time: 28.6 against 24.4 ms on 17.3 M nodes; the strided
        // writes cost the host what the link saves, and the host-side identity check is half of the call.  Not kept.)
        const HostSpan span[1] = {{nodes, n_nodes * sizeof(sw_node)}};
        const void *const from[1] = {dn};
        download(span, from, 1);
    });
}

// sw_filter_kmers is called twice per logical call (sizes, then data): the size phase leaves its device result here and
// the data phase only copies it out when it is called with the same arguments (same host pointers and sizes, same
// used_hashes content) on the same thread -- one upload and one compute per logical call.


int sw_filter_kmers(const sw_kmer *kmers, uint64_t n_kmers, const sw_node *nodes, uint64_t n_nodes,
                    const uint64_t *used_hashes, uint64_t n_used, sw_kmer *kmers_out, sw_node *nodes_out,
                    uint64_t *n_kmers_out, uint64_t *n_nodes_out)
{
    return guarded([&] {
        require_device();
        uint64_t used_sum = 0;
        for (uint64_t i = 0; i < n_used; ++i) used_sum += mix64(used_hashes[i]);   // order-independent, as the hash set is
        FilterStash &st = g_filter_stash;
        const bool data_phase = kmers_out || nodes_out;
        const unsigned id_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        uint64_t id_now[2] = {0, 0};
        if ((data_phase && st.valid) || !data_phase) host_identity(kmers, n_kmers, nodes, n_nodes, id_threads, id_now);
        // (the contents count, not only the addresses: a caller may have rewritten its arrays in place between the two phases)
        if (data_phase && st.valid && st.kmers == kmers && st.nodes == nodes && st.n_kmers == n_kmers && st.n_nodes == n_nodes &&
            st.n_used == n_used && st.used_sum == used_sum && st.id[0] == id_now[0] && st.id[1] == id_now[1]) {
            *n_kmers_out = st.nk;
            *n_nodes_out = st.nn;
            if (kmers_out && st.nk) SW_HIP(hipMemcpy(kmers_out, st.kout.p, st.nk * sizeof(sw_kmer), hipMemcpyDeviceToHost));
            if (nodes_out && st.nn) SW_HIP(hipMemcpy(nodes_out, st.nout.p, st.nn * sizeof(sw_node), hipMemcpyDeviceToHost));
            st = FilterStash();
            return;
        }
        st = FilterStash();
        for (uint64_t i = 0; i < n_nodes; ++i)
            if (nodes[i].start > nodes[i].stop || nodes[i].stop > n_kmers) raise(SW_ERR_VALUE, "node range is outside kmers");
        std::vector<uint64_t> used(used_hashes, used_hashes + n_used);
        std::sort(used.begin(), used.end());  // filter.cpp:145
        // kmers: the resident copy of the last sw_build when the caller's array is that one (Resident)
        Resident &res = resident();
        ResidentLock rlock(res.mu);
        int dev = -1;
        SW_HIP(hipGetDevice(&dev));
        bool use_resident = false;
        if (res.ix && res.ix->device == dev && res.ix->n_kmers == n_kmers && n_kmers) {
            uint64_t id[2] = {id_now[0], 0};
            if (data_phase && !st.valid) host_identity(kmers, n_kmers, nullptr, 0, id_threads, id);
            use_resident = id[0] == res.kmer_sum;
        }
        DevArray<sw_kmer> d_kmers, d_kout;
        DevArray<sw_node> d_nodes(n_nodes), d_nout;
        DevArray<uint64_t> d_used(n_used);
        const sw_kmer *dk;
        if (use_resident) {
            dk = res.ix->kmers.p;
            ++res.filter_hits;
        } else {
            rlock.unlock();
            d_kmers.alloc(n_kmers);
            if (n_kmers) SW_HIP(hipMemcpy(d_kmers.p, kmers, n_kmers * sizeof(sw_kmer), hipMemcpyHostToDevice));
            dk = d_kmers.p;
        }
        if (n_nodes) SW_HIP(hipMemcpy(d_nodes.p, nodes, n_nodes * sizeof(sw_node), hipMemcpyHostToDevice));
        if (n_used) SW_HIP(hipMemcpy(d_used.p, used.data(), n_used * 8, hipMemcpyHostToDevice));
        uint64_t nk = 0, nn = 0;
        device_filter_kmers(dk, n_kmers, d_nodes.p, n_nodes, d_used.p, n_used, 0, d_kout, d_nout, &nk, &nn);
        *n_kmers_out = nk;
        *n_nodes_out = nn;
        if (kmers_out && nk) SW_HIP(hipMemcpy(kmers_out, d_kout.p, nk * sizeof(sw_kmer), hipMemcpyDeviceToHost));
        if (nodes_out && nn) SW_HIP(hipMemcpy(nodes_out, d_nout.p, nn * sizeof(sw_node), hipMemcpyDeviceToHost));
        if (!data_phase) {   // size phase: keep the result for the data phase
            st.kmers = kmers;
            st.nodes = nodes;
            st.n_kmers = n_kmers;
            st.n_nodes = n_nodes;
            st.n_used = n_used;
            st.used_sum = used_sum;
            st.id[0] = id_now[0];
            st.id[1] = id_now[1];
            st.nk = nk;
            st.nn = nn;
            st.kout = std::move(d_kout);
            st.nout = std::move(d_nout);
            st.valid = true;
        }
    });
}

}  // extern "C"
