// omm_host.cpp -- the C ABI (include/omm_mi355x.h) and the host orchestration of a bake.
//
// Host code is C++ like the reference's (libraries/omm-lib/src/bake.cpp, bake_cpu_impl.cpp); it only
// validates, builds the work-item list and drives the HIP kernels.  There is NO CPU classification
// path here: without a working HIP device every bake returns ommResult_FAILURE with a Fatal log line.
#include "../../include/omm_mi355x.h"
#include "../../include/omm_mi355x_ext.h"
#include "bake_types.h"
#include "bake_kernels.h"
#include "bake_host.h"
#include "host_tail.h"
#include "host_expand.h"
#include "lookup_kernels.h"
#include "stats_kernels.h"
#include "geometry_kernels.h"
#include "geometry_cut.h"
#include "coarsen_kernels.h"
#include "merge_kernels.h"
#include "fit_kernels.h"
#include "combine_kernels.h"
#include "compare_kernels.h"
#include "compare_count.h"
#include "gather_kernels.h"
#include "reorient_kernels.h"
#include "raster_kernels.h"
#include "png_store.h"
#include "texture_kernels.h"
#include "block_kernels.h"
#include "bc7_kernels.h"

#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <malloc.h>
#include <math.h>
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <memory>
#include <new>
#include <exception>
#include <thread>
#include <sys/mman.h>
#include <unistd.h>
#include <unordered_map>
#include <vector>
#include <functional>
#include <xmmintrin.h>
#include <emmintrin.h>

using namespace ommx;

namespace {

// ---- handle tagging (src/omm_handle.h:17-54) ----
enum HandleType : uintptr_t { kGpuBaker = 1, kCpuBaker = 3, kTexture = 4 };
template <class T> T* untag(const void* h) { return reinterpret_cast<T*>((uintptr_t)h & ~(uintptr_t)7); }
inline uintptr_t tag_of(const void* h) { return (uintptr_t)h & 7; }

// ---- allocator plumbing (src/std_allocator.h:45-117) ----
void* default_alloc(void*, size_t size, size_t alignment)
{
    void* p = nullptr;
    if (alignment < sizeof(void*)) alignment = sizeof(void*);
    if (posix_memalign(&p, alignment, size ? size : 1) != 0) return nullptr;
    return p;
}
void* default_realloc(void* u, void* mem, size_t size, size_t alignment)
{
    void* n = default_alloc(u, size, alignment);
    if (n && mem) { const size_t old = malloc_usable_size(mem); memcpy(n, mem, old < size ? old : size); free(mem); } // never reads past the old block
    return n;
}
void default_free(void*, void* mem) { free(mem); }

struct Allocator {
    ommAllocate alloc = default_alloc; ommReallocate realloc_ = default_realloc; ommFree free_ = default_free; void* user = nullptr;
    void* allocate(size_t bytes, size_t align = 16) const { return alloc(user, bytes ? bytes : 1, align); }
    void release(void* p) const { if (p) free_(user, p); }
    template <class T, class... A> T* make(A&&... a) const { void* p = allocate(sizeof(T), alignof(T) < 16 ? 16 : alignof(T)); return p ? new (p) T(static_cast<A&&>(a)...) : nullptr; }
    template <class T> void destroy(T* p) const { if (p) { p->~T(); release(p); } }
};

// ---- logger (src/log.h:33-140): invalid arguments are reported at Fatal severity ----
struct Logger {
    ommMessageInterface iface = { nullptr, nullptr };
    bool has() const { return iface.messageCallback != nullptr; }
    void msg(ommMessageSeverity s, const char* m) const { if (iface.messageCallback) iface.messageCallback(s, m, iface.userArg); }
    ommResult invalid(const char* m) const { msg(ommMessageSeverity_Fatal, m); return ommResult_INVALID_ARGUMENT; }
    ommResult failure(const char* m) const { msg(ommMessageSeverity_Fatal, m); return ommResult_FAILURE; }
};

// ---- nothing may unwind through the C ABI (the SDK "never throws"): std::bad_alloc / length_error from the
//      host-side containers become ommResult_FAILURE with a log line ----
template <class F> ommResult guarded(const Logger* log, F&& body) noexcept
{
    try { return body(); }
    catch (const std::bad_alloc&) { if (log) log->msg(ommMessageSeverity_Fatal, "[Failure] - out of host memory"); }
    catch (const std::exception& e) { if (log) { char buf[256]; snprintf(buf, sizeof buf, "[Failure] - %s", e.what()); log->msg(ommMessageSeverity_Fatal, buf); } }
    catch (...) { if (log) log->msg(ommMessageSeverity_Fatal, "[Failure] - unexpected exception"); }
    return ommResult_FAILURE;
}

// ---- device arena: one grow-only HBM block per baker, reused across bakes ----
constexpr size_t kHostBlockBytes = 64u << 10;
// 64 KiB blocks of pinned host memory, the destination of a bake's small read-backs (counters, tail summary, histograms), which otherwise go through the
// runtime's staging buffer -- a wait and a host copy per read-back.  Process-wide free list: pinning costs a system call and a page-table update, and
// applications (and the test suite) create and destroy bakers by the hundred; blocks are never unpinned (a handful per concurrent bake).
struct HostBlockPool {
    std::mutex mu; std::vector<uint8_t*> idle;
    uint8_t* acquire() {
        { std::lock_guard<std::mutex> g(mu); if (!idle.empty()) { uint8_t* p = idle.back(); idle.pop_back(); return p; } }
        uint8_t* p = nullptr;
        if (hipHostMalloc((void**)&p, kHostBlockBytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return p;
    }
    void release(uint8_t* p) { if (p) { std::lock_guard<std::mutex> g(mu); idle.push_back(p); } }
    static HostBlockPool& get() { static HostBlockPool* pool = new HostBlockPool(); return *pool; }   // (never destroyed: no HIP calls at process exit)
};
// ---- ommxBakerKnob_PoisonMemory: the one fill of the device pool and of the working-set arenas, and its two counters ----
// One object per baker (the shadow bakers of a multi-device bake share their owner's).  Off (word == 0) costs the hand-out points one relaxed load: fill() is
// only ever called behind on().  The fill runs on the null stream of the current device and is waited for, so it is complete before any stream of the caller's
// (the bake streams do not synchronise with the null stream) can touch the memory; what used the memory before has drained by the time it is handed out again.
struct PoisonFill {
    std::atomic<uint64_t> word{ 0 };   // 0: off; else bit 32 | the 32-bit fill word
    std::atomic<uint64_t> poolBytes{ 0 }, workingSetBytes{ 0 };
    bool on() const { return word.load(std::memory_order_relaxed) != 0; }
    bool fill(void* p, size_t bytes, bool workingSet) {
        const uint32_t w = (uint32_t)word.load(std::memory_order_relaxed);
        bool ok = bytes < 4 || hipMemsetD32Async((hipDeviceptr_t)p, (int)w, bytes / 4, nullptr) == hipSuccess;
        for (size_t k = 0; ok && k < (bytes & 3); ++k)   // (a capacity that is no multiple of 4: the word's low bytes come first)
            ok = hipMemsetAsync((uint8_t*)p + (bytes & ~(size_t)3) + k, (int)((w >> (8 * k)) & 0xFFu), 1, nullptr) == hipSuccess;
        ok = ok && hipStreamSynchronize(nullptr) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); return false; }
        (workingSet ? workingSetBytes : poolBytes).fetch_add(bytes, std::memory_order_relaxed);
        return true;
    }
};
struct DeviceArena {
    uint8_t* base = nullptr; size_t cap = 0, used = 0;
    uint8_t* hostBlock = nullptr; bool hostBlockTried = false;
    ~DeviceArena() { if (base) (void)hipFree(base); HostBlockPool::get().release(hostBlock); }
    // (null when pinning fails: the caller reads into pageable memory)
    uint8_t* host_block() {
        if (!hostBlockTried) { hostBlockTried = true; hostBlock = HostBlockPool::get().acquire(); }
        return hostBlock;
    }
    // (every caller reserves an arena once per bake, ahead of the first write of that bake into it: the contents are undefined by contract, kept memory or fresh)
    bool reserve(size_t bytes, PoisonFill& poison) {
        if (bytes <= cap) used = 0;
        else {
            if (base) { (void)hipFree(base); base = nullptr; cap = 0; }
            if (hipMalloc((void**)&base, bytes) != hipSuccess) { base = nullptr; (void)hipGetLastError(); return false; }
            cap = bytes; used = 0;
        }
        return !poison.on() || poison.fill(base, cap, true);
    }
    template <class T> T* take(size_t count) {
        const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        T* p = (T*)(base + used); used += bytes; return p;
    }
};

// The device working set of one bake in flight: per-item tables + scratch, packed states + tile queue, and (sharded bakes) the exchange
// buffers.  A baker keeps a small pool of these sets: a bake takes one for its duration -- concurrent bakes on one baker get different
// sets, a sharded bake keeps its set from Begin to Destroy without holding any lock in between -- and steady-state bakes never hipMalloc.
// pinned host memory of a working set (grow-only like the device arenas): staging of the blocks that ommCpuBake streams out during classification
struct HostArena {
    uint8_t* base = nullptr; size_t cap = 0;
    ~HostArena() { if (base) (void)hipHostFree(base); }
    bool reserve(size_t bytes) {
        if (bytes <= cap) return true;
        if (base) { (void)hipHostFree(base); base = nullptr; cap = 0; }
        const size_t want = (bytes + (bytes >> 3) + ((size_t)2 << 20)) & ~(((size_t)2 << 20) - 1);   // 12 % head room: bakes of similar size do not re-pin
        if (hipHostMalloc((void**)&base, want, hipHostMallocDefault) != hipSuccess) { base = nullptr; (void)hipGetLastError(); return false; }
        cap = want; return true;
    }
};
// (the three HIP streams of a bake belong to the working set too: creating and destroying them costs ~0.3 ms per bake)
struct ArenaSet {
    DeviceArena tables, states, xchg; HostArena pinned;
    hipStream_t stream = nullptr, commStream = nullptr, placeStream = nullptr;
    ~ArenaSet() { for (hipStream_t s : { placeStream, commStream, stream }) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};
struct ArenaPool {
    std::mutex mu; std::vector<std::unique_ptr<ArenaSet>> idle;
    std::unique_ptr<ArenaSet> acquire() {
        { std::lock_guard<std::mutex> g(mu); if (!idle.empty()) { std::unique_ptr<ArenaSet> a = std::move(idle.back()); idle.pop_back(); return a; } }
        return std::unique_ptr<ArenaSet>(new ArenaSet());
    }
    std::atomic<bool> retain{ true };
    // Idle sets kept: two whatever their size, and up to sixteen as long as the idle ones together stay below 1 GiB -- K caller threads that bake small
    // meshes on one baker (docs/integration_guide.md:434) would otherwise free and re-create K - 2 working sets (arenas: hipMalloc / hipFree, both
    // device-synchronising; three streams) on every round.
    static size_t bytes_of(const ArenaSet& a) { return a.tables.cap + a.states.cap + a.xchg.cap + a.pinned.cap; }
    void release(std::unique_ptr<ArenaSet> a) {
        std::unique_ptr<ArenaSet> drop;   // (freed outside the lock)
        {
            std::lock_guard<std::mutex> g(mu);
            size_t held = bytes_of(*a); for (const auto& i : idle) held += bytes_of(*i);
            if (retain.load() && (idle.size() < 2 || (idle.size() < 16 && held <= ((size_t)1 << 30)))) idle.push_back(std::move(a)); else drop = std::move(a);
        }
    }
    void trim() { std::vector<std::unique_ptr<ArenaSet>> drop; { std::lock_guard<std::mutex> g(mu); drop.swap(idle); } }   // (freed outside the lock)
};

// ---- device blocks of bake results, reused across bakes (hipMalloc / hipFree of a 1.3 GB block are synchronous and cost ~1 ms) ----
struct DevPool {
    struct Blk { void* p; size_t cap; bool used; bool exempt; };
    std::mutex mu; std::vector<Blk> blks; std::atomic<bool> retain{ true };
    std::shared_ptr<PoisonFill> poison = std::make_shared<PoisonFill>();   // (the baker's; a shadow baker's pool points at its owner's)
    ~DevPool() { for (auto& b : blks) (void)hipFree(b.p); }
    // (the block is marked used before it is filled: nobody else can be handed it, and the caller has not seen it yet)
    void* poisoned(void* p, size_t cap) {
        if (!poison->on() || poison->fill(p, cap, false)) return p;
        release(p); return nullptr;
    }
    void* acquire(size_t bytes) {
        if (bytes == 0) bytes = 1;
        {
            void* p = nullptr; size_t cap = 0;
            {
                std::lock_guard<std::mutex> g(mu);
                for (auto& b : blks) if (!b.used && b.cap >= bytes && b.cap / 2 <= bytes + 4096) { b.used = true; p = b.p; cap = b.cap; break; }
            }
            if (p) return poisoned(p, cap);
        }
        void* p = nullptr;
        const size_t cap = (bytes + 4095) & ~(size_t)4095;
        if (hipMalloc(&p, cap) != hipSuccess) {
            (void)hipGetLastError();
            trim(0);                                  // give the idle blocks back and retry once
            if (hipMalloc(&p, cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        }
        { std::lock_guard<std::mutex> g(mu); blks.push_back({ p, cap, true, false }); }
        return poisoned(p, cap);
    }
    void release(void* p) {
        if (!p) return;
        { std::lock_guard<std::mutex> g(mu); for (auto& b : blks) if (b.p == p) b.used = false; }
        trim(retain.load() ? 6 : 0, retain.load() ? (size_t)256 << 20 : 0);
    }
    // at most keepIdle idle blocks (two result sets: arrayData, descs, index) -- not counting up to 64 SMALL idle blocks of at most smallBytes together:
    // concurrent small bakes on one baker hand dozens of kilobyte-sized blocks back and forth, and hipFree synchronises the device
    void trim(size_t keepIdle, size_t smallBytes = 0) {
        std::vector<void*> drop;   // (hipFree outside the lock)
        {
            std::lock_guard<std::mutex> g(mu);
            size_t small = 0, smallCount = 0, idle = 0;
            for (auto& b : blks) if (!b.used) { if (b.cap <= ((size_t)4 << 20) && small + b.cap <= smallBytes && smallCount < 64) { small += b.cap; smallCount++; b.exempt = true; } else { b.exempt = false; idle++; } }
            for (size_t i = 0; i < blks.size() && idle > keepIdle; )
                if (!blks[i].used && !blks[i].exempt) { drop.push_back(blks[i].p); blks.erase(blks.begin() + (long)i); idle--; } else ++i;
        }
        for (void* p : drop) (void)hipFree(p);
    }
};
// One block of a DevPool.  Owns it from acquire() until release() or the destructor hands it back: declare it BEFORE the StreamDrain of the stream
// that uses it (destructors run in reverse), so that it goes back only when the device is done with it.
struct PoolBlock {
    DevPool* pool = nullptr; void* p = nullptr;
    PoolBlock() = default;
    PoolBlock(DevPool* from, size_t bytes) { (void)acquire(from, bytes); }
    PoolBlock(const PoolBlock&) = delete; PoolBlock& operator=(const PoolBlock&) = delete;
    ~PoolBlock() { release(); }
    bool acquire(DevPool* from, size_t bytes) { release(); pool = from; p = from->acquire(bytes); return p != nullptr; }
    void release() { if (p) pool->release(p); p = nullptr; }
    uint8_t* bytes() const { return (uint8_t*)p; }
};
// waits for a stream when the scope is left, whichever way: declared right BEHIND the memory that asynchronous copies on the stream read or write
struct StreamDrain { hipStream_t s; ~StreamDrain() { (void)hipStreamSynchronize(s); } };

// ---- warm, pinned host memory for the (large) result array -------------------------------------------------
// A fresh 1.3 GB malloc costs more in page faults (70-100 ms) and munmap (95 ms) than the PCIe copy itself (24 ms at 57 GB/s), so
// with the DEFAULT allocator the arrayData block of a destroyed result is kept by its baker and handed to the next bake.  The blocks are
// page-locked (hipHostMalloc): device-to-host copies into them run on the SDMA engines, truly asynchronous and without occupying compute
// units -- a copy into pageable memory is a blit KERNEL that competes with the classification it is supposed to overlap (measured: the
// streamed bake's classification 37 ms instead of 28).  If pinning fails the block is ordinary memory, 2 MiB aligned (transparent huge
// pages) and pre-faulted by a few threads.  User-supplied allocators are always honoured as given.
struct HostPool {
    struct Blk { void* p; size_t cap; bool used; bool pinned; };
    std::mutex mu; std::vector<Blk> blks; std::atomic<bool> retain{ true };
    static constexpr size_t kMinBytes = 8u << 20, kHuge = 2u << 20;
    // Results between kSmallBytes and kMinBytes (a configs[1]-sized bake: 6.5 MB): a fresh malloc of that size is an mmap whose pages fault in under the
    // device-to-host copy -- 0.46 of the call's 1.16 ms -- and an munmap at ommCpuDestroyBakeResult.  They come from this pool too, but only kSmallInUse of them
    // at a time: an application that keeps thousands of small results alive must not find them all pinned (2 MB each at least).
    static constexpr size_t kSmallBytes = 256u << 10; static constexpr unsigned kSmallInUse = 8;
    bool wants(size_t bytes) {
        if (bytes >= kMinBytes) return true;
        if (bytes < kSmallBytes) return false;
        std::lock_guard<std::mutex> g(mu);
        unsigned n = 0; for (auto& b : blks) if (b.used && b.cap < kMinBytes) ++n;
        return n < kSmallInUse;
    }
    static void drop(const Blk& b) { if (b.pinned) (void)hipHostFree(b.p); else free(b.p); }
    ~HostPool() { for (auto& b : blks) drop(b); }
    // an IDLE block that fits, or null: never allocates (the zeroing ahead of a compressed result takes what the last bake left)
    void* acquire_idle(size_t bytes, size_t* cap, bool* pinned) {
        std::lock_guard<std::mutex> g(mu);
        for (auto& b : blks) if (!b.used && b.cap >= bytes && b.cap / 2 <= bytes + kHuge) { b.used = true; *cap = b.cap; *pinned = b.pinned; return b.p; }
        return nullptr;
    }
    void* acquire(size_t bytes, bool* pinned = nullptr) {
        if (pinned) *pinned = false;
        {
            std::lock_guard<std::mutex> g(mu);
            for (auto& b : blks) if (!b.used && b.cap >= bytes && b.cap / 2 <= bytes + kHuge) { b.used = true; if (pinned) *pinned = b.pinned; return b.p; }
        }
        const size_t cap = (bytes + kHuge - 1) & ~(kHuge - 1);
        void* p = nullptr;
        if (hipHostMalloc(&p, cap, hipHostMallocDefault) == hipSuccess && p) {   // (pinning touches every page: no pre-fault pass needed)
            std::lock_guard<std::mutex> g(mu);
            blks.push_back({ p, cap, true, true });
            if (pinned) *pinned = true;
            return p;
        }
        (void)hipGetLastError();
        p = aligned_alloc(kHuge, cap);
        if (!p) return nullptr;
        (void)madvise(p, cap, MADV_HUGEPAGE);
        unsigned nt = std::thread::hardware_concurrency(); nt = nt > 8 ? 8 : (nt ? nt : 1);
        if (cap < (64u << 20)) nt = 1;
        std::vector<std::thread> th;
        const size_t per = ((cap / nt) + kHuge - 1) & ~(kHuge - 1);
        auto touch = [p](size_t lo, size_t hi) { for (size_t o = lo; o < hi; o += 4096) ((volatile uint8_t*)p)[o] = 0; };
        for (unsigned k = 1; k < nt; ++k) { const size_t lo = per * k, hi = lo + per < cap ? lo + per : cap; if (lo < cap) th.emplace_back(touch, lo, hi); }
        touch(0, per < cap ? per : cap);
        for (auto& t : th) t.join();
        std::lock_guard<std::mutex> g(mu);
        blks.push_back({ p, cap, true, false });
        return p;
    }
    void release(void* p) {
        std::lock_guard<std::mutex> g(mu);
        // idle blocks kept: two large ones, and as many small ones as may be in use at once (<= 8 x 8 MB: concurrent callers of small bakes would otherwise
        // free and pin a block per bake); none with ommxBakerKnob_RetainMemory = 1
        size_t idle[2] = { 0, 0 };
        for (auto& b : blks) { if (b.p == p) b.used = false; if (!b.used) idle[b.cap < kMinBytes ? 1 : 0]++; }
        const size_t keep[2] = { retain.load() ? (size_t)2 : (size_t)0, retain.load() ? (size_t)kSmallInUse : (size_t)0 };
        for (size_t i = 0; i < blks.size(); ) {
            const int k = blks[i].cap < kMinBytes ? 1 : 0;
            if (!blks[i].used && idle[k] > keep[k] && (blks[i].p != p || keep[k] == 0)) { drop(blks[i]); blks.erase(blks.begin() + (long)i); idle[k]--; } else ++i;
        }
    }
    void trim() {
        std::lock_guard<std::mutex> g(mu);
        for (size_t i = 0; i < blks.size(); ) if (!blks[i].used) { drop(blks[i]); blks.erase(blks.begin() + (long)i); } else ++i;
    }
};

// ---- device-to-host copies on the SDMA engines ------------------------------------------------------------------------------------
// hipMemcpyAsync moves device -> host data with a blit KERNEL (__amd_rocclr_copyBuffer, also into pinned memory): a kernel that sits on
// compute-unit slots waiting for PCIe, next to the persistent classification launch it is meant to overlap -- measured: the classification
// launches that ran beside such a copy took 2.5x as long.  The streamed result therefore goes through the HSA runtime that HIP itself
// sits on: hsa_amd_memory_async_copy runs on one of the chip's DMA engines and needs no compute unit.  Destination must be pinned
// (the baker's result pool); anything else keeps to hipMemcpyAsync.
struct SdmaCopier {
    hsa_agent_t gpu{ 0 }, cpu{ 0 }; hsa_signal_t sig{ 0 }; bool ok = false; int64_t pending = 0;
    struct Find { int wantOrdinal, seen; uint32_t wantBdf, wantDomain; bool haveBdf; hsa_agent_t gpu, cpu; bool gotGpu, gotCpu; };
    static hsa_status_t visit(hsa_agent_t a, void* u) {
        Find& f = *(Find*)u; hsa_device_type_t t;
        if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
        if (t == HSA_DEVICE_TYPE_CPU && !f.gotCpu) { f.cpu = a; f.gotCpu = true; }
        if (t == HSA_DEVICE_TYPE_GPU) {
            uint32_t bdf = 0; const bool hb = hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) == HSA_STATUS_SUCCESS;
            // (bus / device / function alone is not unique on hosts with several PCI domains: the domain has to agree too, where the runtime reports it)
            uint32_t dom = 0; const bool hd = hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom) == HSA_STATUS_SUCCESS;
            const bool match = f.haveBdf && hb ? (bdf & 0xFFFFu) == f.wantBdf && (!hd || dom == f.wantDomain) : f.seen == f.wantOrdinal;
            if (match && !f.gotGpu) { f.gpu = a; f.gotGpu = true; }
            f.seen++;
        }
        return HSA_STATUS_SUCCESS;
    }
    bool open(int hipDevice) {
        if (hsa_init() != HSA_STATUS_SUCCESS) return false;   // (reference counted: HIP holds the runtime open already)
        Find f; memset(&f, 0, sizeof f); f.wantOrdinal = hipDevice;
        char bus[32] = { 0 };
        if (hipDeviceGetPCIBusId(bus, sizeof bus, hipDevice) == hipSuccess) { unsigned dom = 0, b = 0, d = 0, fn = 0; if (sscanf(bus, "%x:%x:%x.%x", &dom, &b, &d, &fn) == 4) { f.wantBdf = (b << 8) | (d << 3) | fn; f.wantDomain = dom; f.haveBdf = true; } }
        if (hsa_iterate_agents(visit, &f) != HSA_STATUS_SUCCESS || !f.gotGpu || !f.gotCpu) { (void)hsa_shut_down(); return false; }
        gpu = f.gpu; cpu = f.cpu;
        if (hsa_signal_create(0, 0, nullptr, &sig) != HSA_STATUS_SUCCESS) { (void)hsa_shut_down(); return false; }
        ok = true; return true;
    }
    ~SdmaCopier() { if (ok) { (void)wait(); (void)hsa_signal_destroy(sig); (void)hsa_shut_down(); } }
    bool copy_to_host(void* dstHostPinned, const void* srcDevice, size_t bytes) {   // asynchronous; wait() before the data is read
        hsa_signal_add_relaxed(sig, 1); pending++;
        if (hsa_amd_memory_async_copy(dstHostPinned, cpu, srcDevice, gpu, bytes, 0, nullptr, sig) != HSA_STATUS_SUCCESS) { hsa_signal_subtract_relaxed(sig, 1); pending--; return false; }
        return true;
    }
    bool wait() {
        if (!ok || pending == 0) return true;
        const hsa_signal_value_t v = hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
        pending = 0;
        if (v != 0) { hsa_signal_store_relaxed(sig, 0); return false; }   // (negative: a copy failed)
        return true;
    }
};

// A baker works on ONE HIP device: the device that is current on the calling thread when its first texture is created.  HIP's current
// device is per thread (default 0), so every later entry point switches to the baker's device for the duration of the call and restores
// the caller's -- a worker thread of a multi-GPU host can bake without calling hipSetDevice itself, and a texture is never sampled from
// the wrong GPU.  One process driving several GPUs uses one baker per device.
struct DeviceScope {
    int prev = -1; bool changed = false;
    explicit DeviceScope(int dev) { if (dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess; }
    ~DeviceScope() { if (changed) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope&) = delete; DeviceScope& operator=(const DeviceScope&) = delete;
};

struct Baker {
    Allocator mem; Logger log; ommBakerType type;
    std::atomic<int> device{ -1 };   // bound by the first ommCpuCreateTexture / deserialised texture
    int bind_device() {
        int d = device.load();
        if (d >= 0) return d;
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) return -1;
        int expected = -1;
        return device.compare_exchange_strong(expected, cur) ? cur : expected;
    }
    std::shared_ptr<HostPool> hostPool = std::make_shared<HostPool>();
    std::shared_ptr<DevPool> devPool = std::make_shared<DevPool>();
    std::shared_ptr<ArenaPool> arenas = std::make_shared<ArenaPool>();   // device working sets, one per bake in flight
    // multi-device ommCpuBake (ommxBakerKnob_Devices): one shadow baker per further device (own pools and working sets; allocator, logger and knobs of this one)
    std::mutex peersMu; std::vector<std::unique_ptr<Baker>> peers;
    // helper threads of the compressed result (host_expand.h): started by the first bake that may use them (ommCpuBakeFlags_EnableInternalThreads)
    std::mutex workersMu; std::shared_ptr<WorkerPool> workers; unsigned workersWanted = 0;
    std::shared_ptr<WorkerPool> worker_pool(unsigned threads) {
        std::lock_guard<std::mutex> g(workersMu);
        const unsigned want = threads > 1 ? threads - 1 : 0;   // (the calling thread is one of them)
        if (!workers || workersWanted != want) { workers = std::make_shared<WorkerPool>(want); workersWanted = want; }   // (a bake in flight keeps the pool it took)
        return workers;
    }
    std::mutex timingsMu; ommxBakeTimings timings; bool haveTimings = false;
    std::atomic<uint64_t> knobs[ommxBakerKnob_MAX_NUM];   // ommxSetBakerKnob: 0 = default
    std::atomic<uint64_t> lastCompressedArrayBytes{ 0 };   // arrayDataSize of the last bake whose result took the compressed transfer (what the next one zeroes ahead)
    std::atomic<uint32_t> activeBakes{ 0 };               // ommCpuBake calls inside bake_impl right now (callers may bake concurrently on one baker)
    Baker() { for (auto& k : knobs) k.store(0); }
    uint64_t knob(ommxBakerKnob k) const { return knobs[k].load(std::memory_order_relaxed); }
};
void store_timings(Baker& b, const ommxBakeTimings& tm) { std::lock_guard<std::mutex> g(b.timingsMu); b.timings = tm; b.haveTimings = true; }
// helper threads of an expansion: three quarters of the CPUs the process may use, at most 12 -- the probe's rate is flat from 12 threads on, and a process that runs
// as many busy threads as its cgroup quota allows is throttled for the rest of the scheduler period as soon as anything else (the HIP runtime's threads, the
// caller's) runs beside them: measured 6 - 19 ms per expansion with 16 threads on 16 CPUs of quota (ommxBakerKnob_ExpandThreads overrides)
unsigned expand_thread_count(const Baker& b)
{
    if (const uint64_t k = b.knob(ommxBakerKnob_ExpandThreads)) return (unsigned)k;
    const unsigned n = effective_cpus() * 3u / 4u;
    return n > 12u ? 12u : (n < 1u ? 1u : n);
}

// HIP events on the bake's own stream (torch / the caller never see this stream)
struct EventTimer {
    hipStream_t s; hipEvent_t ev[24]; int n = 0;
    explicit EventTimer(hipStream_t st) : s(st) { for (auto& e : ev) e = nullptr; }
    ~EventTimer() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
    int mark() { if (n >= 24) return -1; if (hipEventCreate(&ev[n]) != hipSuccess) return -1; (void)hipEventRecord(ev[n], s); return n++; }
    float ms(int a, int b) const { float v = 0.f; if (a < 0 || b < 0 || hipEventElapsedTime(&v, ev[a], ev[b]) != hipSuccess) return 0.f; return v; }
};
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct TexMip { int w = 0, h = 0; void* texels = nullptr; uint32_t* sat = nullptr; };
struct Texture {
    Allocator mem; const Logger* log = nullptr;
    ommCpuTextureFormat format = ommCpuTextureFormat_MAX_NUM; ommCpuTextureFlags flags = ommCpuTextureFlags_None; float alphaCutoff = -1.f;
    std::vector<TexMip> mips;
    int device = -1;   // the HIP device the texels live on (the baker's)
    const Baker* owner = nullptr;   // the baker that created it (ommxResolveHits samples only textures of its own baker)
    // multi-device ommCpuBake (ommxBakerKnob_Devices): copies of the texels and summed-area tables on the other devices, made by the first bake that needs them
    std::mutex replicaMu; std::vector<std::unique_ptr<Texture>> replicas;
    ~Texture() { for (auto& m : mips) { if (m.texels) (void)hipFree(m.texels); if (m.sat) (void)hipFree(m.sat); } }
};

struct BakeResult {
    Allocator mem;
    void* arrayData = nullptr; ommCpuOpacityMicromapDesc* descs = nullptr;
    ommCpuOpacityMicromapUsageCount* arrayHist = nullptr; ommCpuOpacityMicromapUsageCount* indexHist = nullptr;
    int32_t* index = nullptr;
    float* triArea = nullptr;       // UV-space area per input triangle (bake_cpu_impl.cpp:1904-1915): ommDebugGetStats2's side channel
    std::shared_ptr<HostPool> pool; // set when arrayData came from the baker's warm pool (results may outlive their baker)
    ommCpuBakeResultDesc desc;
    BakeResult() { memset(&desc, 0, sizeof desc); }
    ~BakeResult() { if (pool) pool->release(arrayData); else mem.release(arrayData); mem.release(descs); mem.release(arrayHist); mem.release(indexHist); mem.release(index); mem.release(triArea); }
};
// Whatever a host BakeResult still lacks of its arrays: arrayData and descriptors of E OMMs, index buffer, triangle areas, the two histogram lists.
// (ommCpuBake's main path arrives with all but the histograms: ResultArray places its array, the others are allocated ahead of the copies that fill them.)
ommResult alloc_host_result(Baker& baker, BakeResult* res, uint32_t E, size_t arrayBytes, uint32_t T)
{
    const Allocator& mem = baker.mem;
    if (E && !res->arrayData) res->arrayData = mem.allocate(arrayBytes, 64);
    if (E && !res->descs) res->descs = (ommCpuOpacityMicromapDesc*)mem.allocate(sizeof(ommCpuOpacityMicromapDesc) * (size_t)E, 16);
    if (!res->index) res->index = (int32_t*)mem.allocate(sizeof(int32_t) * (size_t)(T ? T : 1), 16);
    if (!res->triArea) res->triArea = (float*)mem.allocate(sizeof(float) * (size_t)(T ? T : 1), 16);
    if (!res->arrayHist) res->arrayHist = (ommCpuOpacityMicromapUsageCount*)mem.allocate(sizeof(ommCpuOpacityMicromapUsageCount) * 2 * kNumLevels, 16);
    if (!res->indexHist) res->indexHist = (ommCpuOpacityMicromapUsageCount*)mem.allocate(sizeof(ommCpuOpacityMicromapUsageCount) * 2 * kNumLevels, 16);
    if ((E && (!res->arrayData || !res->descs)) || !res->index || !res->triArea || !res->arrayHist || !res->indexHist)
        return baker.log.failure("[Failure] - the memory allocator returned null for the bake result");
    return ommResult_SUCCESS;
}

// ---- XXH64 of a constant byte stream: digests of uniform OMMs (bake_cpu_impl.cpp:1038-1040 applied to 4^level equal bytes) ----
struct UniformDigests {
    uint64_t v[kNumLevels * 4];
    UniformDigests() {
        const uint64_t P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL, P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
        auto rotl = [](uint64_t x, int r) { return (x << r) | (x >> (64 - r)); };
        auto round = [&](uint64_t acc, uint64_t in) { acc += in * P2; acc = rotl(acc, 31); return acc * P1; };
        auto merge = [&](uint64_t h, uint64_t val) { h ^= round(0, val); return h * P1 + P4; };
        for (int l = 0; l < kNumLevels; ++l)
            for (int st = 0; st < 4; ++st) {
                const uint64_t len = (uint64_t)1 << (2 * l), seed = 42;
                const uint64_t w8 = 0x0101010101010101ULL * (uint64_t)st; const uint32_t w4 = 0x01010101u * (uint32_t)st;
                uint64_t h, rem = len;
                if (len >= 32) {
                    uint64_t a = seed + P1 + P2, b = seed + P2, c = seed, d = seed - P1;
                    for (uint64_t k = 0; k < len / 32; ++k) { a = round(a, w8); b = round(b, w8); c = round(c, w8); d = round(d, w8); }
                    h = rotl(a, 1) + rotl(b, 7) + rotl(c, 12) + rotl(d, 18);
                    h = merge(h, a); h = merge(h, b); h = merge(h, c); h = merge(h, d);
                    rem = 0; // 4^l is a multiple of 32 from level 3 on
                } else h = seed + P5;
                h += len;
                for (; rem >= 8; rem -= 8) { h ^= round(0, w8); h = rotl(h, 27) * P1 + P4; }
                if (rem >= 4) { h ^= (uint64_t)w4 * P1; h = rotl(h, 23) * P2 + P3; rem -= 4; }
                for (; rem > 0; --rem) { h ^= (uint64_t)st * P5; h = rotl(h, 11) * P1; }
                h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
                v[l * 4 + st] = h;
            }
    }
};
const UniformDigests& uniform_digests() { static const UniformDigests t; return t; }
// what a bake's first transfer carries: the zeroed counters block (its 256-byte arena slot) and, in the slot behind it, the digest table -- one copy instead
// of a copy and a fill (two fill launches: 200 bytes are not a multiple of 16)
struct BakeHead { uint8_t counters[256]; uint64_t uniform[kNumLevels * 4]; BakeHead() { memset(counters, 0, sizeof counters); memcpy(uniform, uniform_digests().v, sizeof uniform); } };
static_assert(sizeof(SetupCounters) <= kBakeCountersSlot && sizeof(BakeHead) == kBakeCountersSlot + sizeof(uint64_t) * kNumLevels * 4, "the counters block must fit its arena slot, the digest table the one behind it");
static_assert(kBakeLevels == kNumLevels && kBakeFineWords == (size_t)kFineSlots * kFineStride && kBakeMaxRanks == (size_t)kMaxRanks && kBakePreviewSlotBytes == kPreviewSlotBytes && kBakeStreamCtlWords == kStreamCtlWords,
              "bake_host.h restates these constants of the kernel headers");
const BakeHead& bake_head() { static const BakeHead h; return h; }

// ---- x86 conversion semantics used by the reference's host-side arithmetic ----
inline int f2i(float f) { return _mm_cvtt_ss2si(_mm_set_ss(f)); }
inline uint32_t f2u(float f) { return (uint32_t)_mm_cvttss_si64(_mm_set_ss(f)); }

struct HostTri { float p[6]; };

bool tri_degenerate(const HostTri& t) // util/geometry.h:44-47
{
    const float* p = t.p;
    const float area = 0.5f * fabsf(p[0] * (p[3] - p[5]) + p[2] * (p[5] - p[1]) + p[4] * (p[1] - p[3]));
    return (double)area < 1e-9;
}
float area2d(float ax, float ay, float bx, float by, float cx, float cy) // util/geometry.h:141-145
{
    const float v0x = cx - ax, v0y = cy - ay, v1x = bx - ax, v1y = by - ay;
    const float nx = v0y * 0.f - v1y * 0.f, ny = 0.f * v1x - 0.f * v0x, nz = v0x * v1y - v1x * v0y;
    return 0.5f * sqrtf(nx * nx + ny * ny + nz * nz);
}

// bake_cpu_impl.cpp:470-560
int32_t level_for_primitive(const ommCpuBakeInputDesc& d, uint32_t flags, uint32_t i, const HostTri& t, int w, int h)
{
    if (d.subdivisionLevels && d.subdivisionLevels[i] <= 12) return d.subdivisionLevels[i];
    if (!(d.dynamicSubdivisionScale > 0)) return d.maxSubdivisionLevel;
    const float fw = (float)(uint32_t)w, fh = (float)(uint32_t)h;
    const float* p = t.p;
    if (tri_degenerate(t) || has_flag(flags, kBakeFlag_EnableEdgeHeuristic)) { // edge heuristic (glibc log2f, stays on the host)
        const float e0x = fw * (p[2] - p[0]), e0y = fh * (p[3] - p[1]);
        const float e1x = fw * (p[4] - p[0]), e1y = fh * (p[5] - p[1]);
        const float e2x = fw * (p[4] - p[2]), e2y = fh * (p[5] - p[3]);
        const float l0 = e0x * e0x + e0y * e0y, l1 = e1x * e1x + e1y * e1y, l2 = e2x * e2x + e2y * e2y;
        float eMax = l0; if (eMax < l1) eMax = l1; if (eMax < l2) eMax = l2;
        const float n = (double)eMax < 1e-6 ? 0 : log2f(eMax) / 2.f - log2f(d.dynamicSubdivisionScale);
        int lvl = f2i(ceilf(n));
        if (lvl < 0) lvl = 0; if (lvl > (int)d.maxSubdivisionLevel) lvl = d.maxSubdivisionLevel;
        return lvl;
    }
    const float area = area2d(p[0] * fw, p[1] * fh, p[2] * fw, p[3] * fh, p[4] * fw, p[5] * fh);
    const float target = d.dynamicSubdivisionScale * d.dynamicSubdivisionScale;
    uint32_t v = f2u(area / target);
    v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; v++;
    static const uint32_t bm[5] = { 0xAAAAAAAAu, 0xCCCCCCCCu, 0xF0F0F0F0u, 0xFF00FF00u, 0xFFFF0000u };
    uint32_t r = (v & bm[0]) != 0;
    for (uint32_t k = 4; k > 0; k--) r |= (uint32_t)((v & bm[k]) != 0) << k;
    const uint32_t lvl = r >> 1;
    return (int32_t)(lvl < d.maxSubdivisionLevel ? lvl : d.maxSubdivisionLevel);
}

const char* special_name(int s)
{
    switch (s) { case -1: return "Fully Transparent"; case -2: return "Fully Opaque"; case -3: return "Fully Unknown Transparent"; case -4: return "Fully Unknown Opaque"; default: return "Unknown State"; }
}
const char* state_name(int s) { switch (s) { case 0: return "Transparent"; case 1: return "Opaque"; case 2: return "UnknownTransparent"; case 3: return "UnknownOpaque"; default: return "Unknown"; } }
const char* format_name(int f) { return f == 1 ? "OC1_2_State" : (f == 2 ? "OC1_4_State" : "Unknown"); }
bool compatible(int state, int format) { return format == ommFormat_OC1_2_State ? (state == 0 || state == 1) : true; }

// bake_cpu_impl.cpp:235-290 -- message strings are pinned by support/tests/test_omm_log.cpp:146-209
ommResult validate_desc(const Baker& b, const ommCpuBakeInputDesc& d)
{
    const Logger& L = b.log; const uint32_t flags = (uint32_t)d.bakeFlags; char buf[256];
    if (d.texture == 0) return L.invalid("[Invalid Argument] - texture is not set");
    if (tag_of(d.texture) != kTexture) return L.invalid("[Invalid Argument] - desc.texture is of incorrect type");
    if (d.alphaMode == ommAlphaMode_MAX_NUM) return L.invalid("[Invalid Argument] - alphaMode is not set");
    if (d.runtimeSamplerDesc.addressingMode == ommTextureAddressMode_MAX_NUM) return L.invalid("[Invalid Argument] - runtimeSamplerDesc.addressingMode is not set");
    if (d.runtimeSamplerDesc.filter == ommTextureFilterMode_MAX_NUM) return L.invalid("[Invalid Argument] - runtimeSamplerDesc.filter is not set");
    if (d.texCoordFormat == ommTexCoordFormat_MAX_NUM) return L.invalid("[Invalid Argument] - texCoordFormat is not set");
    if (d.texCoords == nullptr) return L.invalid("[Invalid Argument] - texCoords is not set");
    if (d.indexFormat == ommIndexFormat_MAX_NUM) return L.invalid("[Invalid Argument] - indexFormat is not set");
    if (d.indexBuffer == nullptr) return L.invalid("[Invalid Argument] - indexBuffer is not set");
    if (d.indexCount == 0) return L.invalid("[Invalid Argument] - indexCount is not set");
    if (d.maxSubdivisionLevel > kMaxLevel) {
        snprintf(buf, sizeof buf, "[Invalid Argument] - maxSubdivisionLevel (%d) is greater than maximum supported (%d)", d.maxSubdivisionLevel, kMaxLevel);
        return L.invalid(buf);
    }
    if ((flags & (ommCpuBakeFlags_EnableNearDuplicateDetection | kBakeFlag_NearDuplicateBruteForce)) && has_flag(flags, ommCpuBakeFlags_DisableDuplicateDetection))
        return L.invalid("[Invalid Argument] - EnableNearDuplicateDetection or EnableNearDuplicateDetectionBruteForce is used together with DisableDuplicateDetection");
    if (has_flag(flags, ommCpuBakeFlags_EnableValidation) && !L.has())
        return L.invalid("[Invalid Argument] - EnableValidation is set but no message callback was provided");
    const Texture* tex = untag<Texture>(d.texture);
    if (tex->alphaCutoff >= 0.f && tex->alphaCutoff != d.alphaCutoff) {
        snprintf(buf, sizeof buf, "[Invalid Argument] - Texture object alpha cutoff threshold (%.6f) is different from alpha cutoff threshold in bake input (%.6f)", tex->alphaCutoff, d.alphaCutoff);
        return L.invalid(buf);
    }
    if (!compatible(d.alphaCutoffGreater, d.format)) {
        snprintf(buf, sizeof buf, "[Invalid Argument] - alphaCutoffGreater=%s is not compatible with %s", state_name(d.alphaCutoffGreater), format_name(d.format));
        return L.invalid(buf);
    }
    if (!compatible(d.alphaCutoffLessEqual, d.format)) {
        snprintf(buf, sizeof buf, "[Invalid Argument] - alphaCutoffLessEqual=%s is not compatible with %s", state_name(d.alphaCutoffLessEqual), format_name(d.format));
        return L.invalid(buf);
    }
    return ommResult_SUCCESS;
}

uint32_t ctz32(uint32_t n) { if (!n) return 32; uint32_t c = 0; while (!(n & 1)) { c++; n >>= 1; } return c; }
bool is_pow2(int x) { return x > 0 && !(x & (x - 1)); }

#define HIP_OK(call) ((call) == hipSuccess)

// HIP events without timing, destroyed with the scope: declared in the scope that holds the last wait on them.  create(count): `count` events in all.
template <uint32_t N> struct EventList {
    hipEvent_t ev[N]; uint32_t n = 0;
    EventList() = default;
    EventList(const EventList&) = delete; EventList& operator=(const EventList&) = delete;
    bool create(uint32_t count) { while (n < count && n < N && HIP_OK(hipEventCreateWithFlags(&ev[n], hipEventDisableTiming))) ++n; return n == count; }
    ~EventList() { for (uint32_t k = 0; k < n; ++k) (void)hipEventDestroy(ev[k]); }
};

uint32_t device_cu_count() // of the current device; sizes the persistent classification grid
{
    static std::mutex mu; static int cached[64]; static bool have[64];
    int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    std::lock_guard<std::mutex> g(mu);
    if (!have[dev]) { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256; cached[dev] = n; have[dev] = true; }
    return (uint32_t)cached[dev];
}

// Device-resident result of a bake (what ommxBakeDevice hands out, and what ommCpuBake copies to the host).
struct DeviceResult {
    uint8_t* arrayData = nullptr; uint64_t arrayDataSize = 0;
    ommCpuOpacityMicromapDesc* descs = nullptr; uint32_t numDescs = 0;
    void* index = nullptr; uint32_t numTris = 0; ommIndexFormat indexFormat = ommIndexFormat_UINT_32;
    uint32_t hist[2 * kNumLevels]; int bits = 2;
    const float* triAreaScratch = nullptr; // per-triangle UV areas in the bake's arena: valid until the session ends (ommCpuBake copies them out)
    float* triArea = nullptr;              // ommxBakeDevice: the result's own device copy of them (ommxDebugGetStatsDevice2's side channel); null for sharded results
    std::shared_ptr<DevPool> pool;   // the baker's (results may outlive their baker)
    // ommCpuBake's compressed transfer: asked right before the gather, when the array's size is known and every OMM is a multiple of 16 bytes; may hand out a byte per
    // 16-byte unit and a zeroed word per 256-unit block (+ 1) for the gather to fill with the exchange codec's codes and raw counts (launch_gather_omms)
    std::function<bool(uint64_t arrayDataSize, uint8_t** unitCodes, uint32_t** blockRawCounts)> gatherCodes;
    DeviceResult() { memset(hist, 0, sizeof hist); }
    DeviceResult(const DeviceResult&) = delete;
    DeviceResult& operator=(const DeviceResult&) = delete;
    void* dev_alloc(size_t bytes) { return pool ? pool->acquire(bytes) : nullptr; }
    ~DeviceResult() { if (pool) { pool->release(arrayData); pool->release(descs); pool->release(index); pool->release(triArea); } }
};

struct DeviceInputs {           // raw triangle data, device resident
    const void* texCoords; const void* indices; const uint8_t* perTriLevels;
};

// Multi-GPU: state kept between the phases of a sharded bake (ommxSharded*).  The rank classifies its share of the active
// work items; per-item metadata and surviving blocks are exchanged by the caller's collectives; the tail is replicated.
struct ShardCtx {
    uint32_t rank = 0, world = 1;
    ShardBounds bounds;
    TailInputs ti; TailOutputs to; TailCounts counts;
    SetupCounters hc;
    BakeTables tab = BakeTables();   // the working set bake_core carved from the session's tables arena (bake_host.h): phases 2 and 3 read through it
    uint8_t* dStates = nullptr;      // (from the states arena)
    uint32_t flags = 0, T = 0; int bits = 2; bool asyncBegin = false;
    bool mergeStates = false;   // host-tail bakes: the packed states are zeroed first so that a SUM all-reduce over them is a merge
    int ev[5] = { -1, -1, -1, -1, -1 };   // HIP event marks of Begin: setup | triage | classify | digest
    // exchange buffers: carved from the session's arenas (tables: tab.meta .. tab.totals; xchg: contribution + gather staging), nothing to free
    ExchangeArena x = ExchangeArena();   // contribution | RCCL path: gather staging, block exchange codec (own stream, all ranks' streams, own size word, count / scan scratch)
    uint64_t totals[kMaxRanks]; uint64_t strideBytes = 0;
};

// opt-in lossy reducers (near-duplicate merge, maxArrayDataSize): classification on the device, serial tail on the host
struct HostTailRequest { std::vector<HostItem> items; };

// ommCpuBake: the result has to end up in host memory, and the 1.3 GB of arrayData of the metric configuration need 23 ms of PCIe time -- nearly
// as long as the classification itself.  The final ORDER of the blocks is known up front (descending level / spatial key / item index over the items
// that are emitted), so the tile queue of the levels >= 6 is cut into `chunks` consecutive ranges of that order, which one persistent launch drains in
// turn; when a range is complete (device-side count), its blocks are packed behind those of the earlier ranges -- a contiguous piece of the final
// arrayData -- on a second stream, and ONE SDMA copy moves that piece to its final place in the caller's array while the launch classifies the
// following ranges (tail_kernels.hip: "Streamed result").  The placement is verified against the ordinary tail at the end; on a mismatch (a duplicate
// block whose first occurrence was classified later) the bake falls back to the ordinary gather + copy.
struct StreamOut {
    // in
    uint32_t chunksWanted = 0;        // 0 = decide from the size of the bake
    bool forced = false;              // (knob set: stream whatever the size)
    bool compressedAvailable = false; // the caller can send the finished array as a codec stream instead (helper threads): stream only when that is the faster of the two
    ArenaSet* set = nullptr; hipStream_t copyStream = nullptr, placeStream = nullptr;
    void* allocUser = nullptr; uint8_t* (*alloc)(void* user, uint64_t upperBoundBytes, bool* pinned) = nullptr;   // the host arrayData, before the first block leaves
    int device = 0;
    // out
    bool used = false, fellBack = false; uint32_t chunks = 0; uint64_t streamedBytes = 0;
    double classifyEndMs = 0, lastByteMs = 0;
    SdmaCopier sdma;   // copies in flight when bake_core returns: the caller queues its small read-backs behind the bake, THEN waits for these (finish())
    bool finish() { bool ok = true; if (copyStream) ok = hipStreamSynchronize(copyStream) == hipSuccess; ok = sdma.wait() && ok; lastByteMs = now_ms(); return ok; }
};
struct StreamCtx {   // what the hook behind a classification launch needs
    hipStream_t stream, place; hipEvent_t* fences; const uint32_t* activeIds; uint32_t numActive; StreamSegment proto; void* scratch; size_t scratchBytes;
    uint64_t* digests; unsigned long long* cursor; uint8_t* stage; uint64_t* placed; uint32_t* ctl; unsigned long long* hostCursor; hipEvent_t* events; uint32_t numEvents, recorded; bool ok;
    const uint32_t* queueCtl; bool paired;                 // paired: two queue sections per range (bake_kernels.h: ClassifyChunks)
    const uint32_t* earlyList; uint32_t earlyCapacity; const uint8_t* itemLevel;   // the early class ordered by the range it is classified with (ctl: start / count per range)
    double waitSeconds;   // how long the placement stream waits for a range before it gives the stream up (scaled with the estimated classification time)
};
// in front of the persistent launch: the placement stream starts behind the tile triage (the section tails are final from here on)
void stream_mark_hook(void* user)
{
    StreamCtx& c = *(StreamCtx*)user;
    c.ok = c.ok && hipEventRecord(c.fences[0], c.stream) == hipSuccess && hipStreamWaitEvent(c.place, c.fences[0], 0) == hipSuccess;
}
void stream_hook(void* user, uint32_t chunk, const ClassifySegment* segs, uint32_t numSegs, bool last)
{
    // The placement runs on a second, high-priority stream next to the ONE persistent classification launch: a one-lane kernel holds that stream until
    // the range's section of the tile queue is complete (device-side count, no launch boundary, no host round trip), then the digest / placement kernels
    // of the range run in the workgroup slot the classification leaves free on every CU.
    StreamCtx& c = *(StreamCtx*)user;
    if (chunk >= c.numEvents) { c.ok = false; return; }
    if (last) c.ok = c.ok && hipEventRecord(c.fences[1], c.stream) == hipSuccess && hipStreamWaitEvent(c.place, c.fences[1], 0) == hipSuccess;   // (the lower levels: behind everything)
    else launch_stream_wait_sections(c.queueCtl, c.paired ? 2u * chunk : chunk, c.paired ? 2u : 1u, c.ctl, c.waitSeconds, c.place);
    // CalcDigest (bake_cpu_impl.cpp:1038-1040).  A range of the levels >= 6: its own items (the early ones among them have their digest from this range
    // or an earlier one) and, in the same launch, the early items classified WITH this range -- the families that start in it, wherever their members lie --,
    // which then enter the table ahead of the range's placement
    const bool lists = !last && !c.proto.disableDedup;
    StreamSegment e = c.proto; e.ids = c.earlyList; e.count = c.earlyList ? c.earlyCapacity : 0u; e.level = 6; e.range = chunk;
    e.liveStart = c.ctl + kStreamCtlEarlyStart + chunk; e.liveCount = c.ctl + kStreamCtlEarlyCount + chunk; e.itemLevel = c.itemLevel;
    for (uint32_t k = 0; lists && k < (numSegs ? numSegs : 1u); ++k) {
        DigestLists D; memset(&D, 0, sizeof D);
        if (k < numSegs) { D.ids = c.activeIds + segs[k].first; D.count = segs[k].count; D.level = segs[k].level; D.only = c.proto.early; D.want = 0; }
        if (k == 0) { D.listB = e.ids; D.capacityB = e.count; D.liveStart = e.liveStart; D.liveCount = e.liveCount; D.itemLevel = e.itemLevel; }
        launch_digest_lists(c.proto.states, c.proto.stateOfs, D, (uint32_t)c.proto.bits, c.digests, c.place);
    }
    if (lists && e.count) launch_stream_insert_list(e, c.numActive, c.scratch, c.scratchBytes, c.place);
    for (uint32_t k = 0; k < numSegs && c.ok; ++k) {
        StreamSegment g = c.proto; g.ids = c.activeIds + segs[k].first; g.count = segs[k].count; g.level = segs[k].level; g.range = chunk;
        if (last && !g.disableDedup) launch_digest(g.states, g.stateOfs, g.ids, g.count, g.level, (uint32_t)g.bits, c.digests, c.place);   // (the levels below 6)
        c.ok = run_stream_segment(g, c.numActive, c.scratch, c.scratchBytes, c.cursor, c.stage, c.placed, c.ctl, c.place) == hipSuccess;
    }
    launch_stream_publish(c.cursor, c.hostCursor + chunk, c.place);
    c.ok = c.ok && hipEventRecord(c.events[chunk], c.place) == hipSuccess;
    if (c.ok) c.recorded = chunk + 1u;
}
struct MarkCtx { EventTimer* et; int mark, markGeneric; };
void mark_hook(void* user) { MarkCtx& c = *(MarkCtx*)user; c.mark = c.et->mark(); }
void mark_generic_hook(void* user) { MarkCtx& c = *(MarkCtx*)user; c.markGeneric = c.et->mark(); }

// One byte per micro-triangle of every work item on the host, for the serial reducers (host_tail.cpp): near-duplicate merge and the
// maxArrayDataSize budget work on the reference's own data layout (bake_cpu_impl.cpp:401-411).  Synchronises the stream.
ommResult gather_host_items(const Logger& L, hipStream_t stream, uint32_t U, uint32_t T, const SetupCounters& hc, const float* dUv, const uint8_t* dLevel,
                            const uint8_t* dActive, const uint32_t* dMask, const uint64_t* dStateOfs, const uint8_t* dStates, const int32_t* dTriToItem, int bits,
                            std::vector<HostItem>& items)
{
    {   // refuse cleanly when that cannot fit in host memory instead of dying in std::bad_alloc half way
        const uint64_t bytes = 2 * hc.stateBytes * (bits == 1 ? 2u : 1u);   // the packed states of the non-uniform items, once as read back and once per item
        const uint64_t phys = (uint64_t)sysconf(_SC_PHYS_PAGES) * (uint64_t)sysconf(_SC_PAGE_SIZE);
        if (bytes > phys / 2) return L.failure("[Failure] - near-duplicate merging / maxArrayDataSize need the packed states of every non-uniform work item on the host: not enough host memory for this bake");
    }
    std::vector<float> hUv((size_t)U * 6); std::vector<uint8_t> hLevel(U), hActive(U), hStates((size_t)hc.stateBytes);
    std::vector<uint32_t> hMask(U); std::vector<uint64_t> hOfs(U); std::vector<int32_t> hTri(T);
    bool ok = true;
    if (U) {
        ok = HIP_OK(hipMemcpyAsync(hUv.data(), dUv, (size_t)U * 24, hipMemcpyDeviceToHost, stream)) && HIP_OK(hipMemcpyAsync(hLevel.data(), dLevel, U, hipMemcpyDeviceToHost, stream))
          && HIP_OK(hipMemcpyAsync(hActive.data(), dActive, U, hipMemcpyDeviceToHost, stream)) && HIP_OK(hipMemcpyAsync(hMask.data(), dMask, (size_t)U * 4, hipMemcpyDeviceToHost, stream))
          && HIP_OK(hipMemcpyAsync(hOfs.data(), dStateOfs, (size_t)U * 8, hipMemcpyDeviceToHost, stream));
    }
    if (ok && hc.stateBytes) ok = HIP_OK(hipMemcpyAsync(hStates.data(), dStates, (size_t)hc.stateBytes, hipMemcpyDeviceToHost, stream));
    if (ok && T) ok = HIP_OK(hipMemcpyAsync(hTri.data(), dTriToItem, (size_t)T * 4, hipMemcpyDeviceToHost, stream));
    ok = ok && HIP_OK(hipStreamSynchronize(stream));
    if (!ok) return L.failure("[Failure] - device to host transfer of the micro-triangle states failed");
    items.resize(U);
    for (uint32_t i = 0; i < U; ++i) {
        HostItem& it = items[i];
        it.level = hLevel[i]; it.format = bits; memcpy(it.uv, &hUv[(size_t)i * 6], 24);
        const size_t n = (size_t)1 << (2 * it.level);
        // uniform items stay (state, level); the others keep the device's 2-bit packing (1-bit states of a 2-state bake are widened to it)
        if (!hActive[i]) { uint32_t st = 0; while (!((hMask[i] >> st) & 1u) && st < 3) ++st; it.uniform = (int)st; }
        else {
            const uint8_t* p = hStates.data() + hOfs[i];
            it.uniform = -1; it.packed.assign(n >= 4 ? n / 4 : 1, 0);
            if (bits == 2) memcpy(it.packed.data(), p, n >= 4 ? n / 4 : 1);
            else for (size_t u = 0; u < n; ++u) it.packed[u >> 2] = (uint8_t)(it.packed[u >> 2] | (((p[u >> 3] >> (u & 7)) & 1u) << ((u & 3) << 1)));
        }
    }
    for (uint32_t t = 0; t < T; ++t) if (hTri[t] >= 0) items[(size_t)hTri[t]].prims.push_back(t);
    return ommResult_SUCCESS;
}

// the serial tail itself (reference: bake_cpu_impl.cpp:1068-1688 on the classified states) + index narrowing in place (:1872-1902)
ommResult run_host_tail_for(const ommCpuBakeInputDesc& d, uint32_t T, std::vector<HostItem>& items, HostTailResult& hres, ommIndexFormat& ifmt)
{
    const uint32_t fl = (uint32_t)d.bakeFlags;
    HostTailDesc td; td.format = (int)d.format; td.disableSpecial = has_flag(fl, ommCpuBakeFlags_DisableSpecialIndices); td.disableDedup = has_flag(fl, ommCpuBakeFlags_DisableDuplicateDetection);
    td.nearDup = has_flag(fl, ommCpuBakeFlags_EnableNearDuplicateDetection); td.nearDupBrute = has_flag(fl, kBakeFlag_NearDuplicateBruteForce); td.rejectionThreshold = d.rejectionThreshold;
    td.nearDupFactor = d.nearDuplicateDeduplicationFactor; td.maxArrayDataSize = d.maxArrayDataSize; td.numTris = T; td.unresolved = (int32_t)d.unresolvedTriState;
    if (run_host_tail(td, items, hres)) return ommResult_FAILURE;
    hres.index.resize(T ? T : 1);
    ifmt = index_format_for(T, fl);
    if (ifmt == ommIndexFormat_UINT_8) { int8_t* p8 = (int8_t*)hres.index.data(); for (uint32_t i = 0; i < T; ++i) { const int32_t v = hres.index[i]; p8[i] = (int8_t)v; } }
    else if (ifmt == ommIndexFormat_UINT_16) { int16_t* p16 = (int16_t*)hres.index.data(); for (uint32_t i = 0; i < T; ++i) { const int32_t v = hres.index[i]; p16[i] = (int16_t)v; } }
    return ommResult_SUCCESS;
}

static_assert(kBakeMaxStreamRanges == kMaxStreamRanges && kBakeClassifyCtlWords == kClassifyCtlWords && kBakeHostBlockBytes == kHostBlockBytes && sizeof(((ShardBounds*)nullptr)->b[0]) == sizeof(uint32_t) * (kBakeMaxRanks + 1),
              "bake_host.h restates these constants of the kernel headers and of the pinned host block");

// what the kernels read of one mip level (bake_core's classification, ommxResolveHits)
DevMip dev_mip(const TexMip& tmip)
{
    DevMip dm; memset(&dm, 0, sizeof dm);
    dm.texels = tmip.texels; dm.sat = tmip.sat; dm.w = tmip.w; dm.h = tmip.h;
    dm.log2w = (int)ctz32((uint32_t)tmip.w); dm.log2h = (int)ctz32((uint32_t)tmip.h);
    dm.pow2 = is_pow2(tmip.w) && is_pow2(tmip.h);
    dm.fw = (float)tmip.w; dm.fh = (float)tmip.h; dm.rw = 1.f / (float)tmip.w; dm.rh = 1.f / (float)tmip.h;
    return dm;
}

// ---- a bake in flight: the inputs of bake_core, what its stages hand on, and the stages themselves in the order they run ----
struct BakeRun;
// The streamed-result protocol (StreamOut above): the events behind the classification launches, what the hooks behind those launches need, the preview, the
// loop that sends what each launch placed, and the comparison with the tail's exact layout.  The hooks point into `sc`: it outlives launch_classify.
struct StreamRun {
    EventList<2 * kMaxClassifyChunks + 3> events;   // range placed [K + 1] | fences [K + 2]
    StreamCtx sc;
    uint64_t sent = 0;        // bytes of the staging copy that are on their way to the caller's array
    int pv0 = -1, pv1 = -1;   // HIP event marks around the preview
    ommResult begin(BakeRun& b);    // reads the plan of the states; leaves the placement tables cleared, the events created, `sc` and b.cc set up, the preview's early flags
    ommResult follow(BakeRun& b);   // reads the cursor each range publishes; leaves the placed bytes queued for the host array (SDMA or HIP copy), the range-ready times
    ommResult verify(BakeRun& b);   // reads the tail's order and offsets; leaves b.streamed, after a discarded stream the fallback's PerfWarning, the stream fields of `so` and `tm`
};
struct BakeRun {
    // ---- the call ----
    Baker& baker; const ommCpuBakeInputDesc& d; const DeviceInputs& din; DeviceArena* const arena; DeviceArena* const statesArena; const hipStream_t stream;
    EventTimer& et; DeviceResult& R; ommxBakeTimings& tm;
    ShardCtx* const sh; HostTailRequest* const ht; StreamOut* const so;   // the mode, each null when it is not the one: sharded begin | host tail | streamed result on offer
    const Logger& L; const Texture& tex;
    const uint32_t flags, T, maxItems; const int bits;
    // DisableFineClassification with the 2-state format (internal flag bit 9): unresolved micro-triangles keep UnknownOpaque (3), which has no 1-bit form -- the
    // reference digests the unpacked states and ORs `3 << (i & 7)` into the packed bytes (bake_cpu_impl.cpp:1811).  The states are therefore kept in the
    // 2-bit packing up to the final gather, which applies that rule (launch_gather_omms: storeBits != bits).
    const int storeBits;
    const bool noDedup;
    // ---- what the stages hand on ----
    BakeTables tab; SetupParams S; SetupCounters hc; ClassifyParams P;
    uint8_t* hostBlock = nullptr;   // the arena's pinned block, layout: [0, 256) counters, [256, 512) tail summary, [1 KiB, ..) the final read-backs (readback_slots)
    uint32_t U = 0, numActive = 0; double microAll = 0;   // work items, active ones, micro-triangles of all
    ShardBounds bounds; uint32_t lvlFirst[kNumLevels], lvlCount[kNumLevels];   // this rank's range of every level's active list
    uint32_t streamChunks = 0; uint8_t* hostArray = nullptr; unsigned long long* hCursor = nullptr; bool hostPinned = false;   // streamed result: ranges (0: none), the caller's array, the pinned cursor words
    uint64_t genericCapacity = 0;   // entries of the deferred generic pass (0: none)
    BakeStates st;
    ItemArrays A; ClassifyChunks cc; MarkCtx mk;
    TailInputs ti; TailOutputs to; TailCounts counts;
    bool streamed = false;   // the streamed result stands: no gather, no array on the device
    unsigned long long fineCount = 0, genericMicro = 0; uint32_t queueTails[2] = { 0u, 0u };   // read-back statistics; open tiles of the two tile sizes
    double coreT0 = 0; int e0 = -1, e1 = -1, e1b = -1, e2 = -1, e3 = -1, e4 = -1, e5 = -1;   // HIP event marks: setup | triage | classify | digest | tail | gather

    BakeRun(Baker& baker_, const ommCpuBakeInputDesc& d_, const DeviceInputs& din_, DeviceArena* arena_, DeviceArena* statesArena_, hipStream_t stream_, EventTimer& et_, DeviceResult& R_,
            ommxBakeTimings& tm_, ShardCtx* sh_, HostTailRequest* ht_, StreamOut* so_)
        : baker(baker_), d(d_), din(din_), arena(arena_), statesArena(statesArena_), stream(stream_), et(et_), R(R_), tm(tm_), sh(sh_), ht(ht_), so(so_), L(baker_.log),
          tex(*untag<Texture>(d_.texture)), flags((uint32_t)d_.bakeFlags), T(d_.indexCount / 3u), maxItems(T ? T : 1), bits((int)d_.format), storeBits(no_fine_two_state(d_) ? 2 : bits),
          noDedup(has_flag(flags, ommCpuBakeFlags_DisableDuplicateDetection))
    {
        if (!R.pool) R.pool = baker.devPool;
        memset(&hc, 0, sizeof hc);
    }

    // reads the triangle count and the mode; leaves the working set reserved and carved (worst case: every triangle is its own work item)
    ommResult carve_tables()
    {
        const size_t setupBytes = setup_scratch_bytes(T), tailBytes = tail_scratch_bytes(maxItems, T), streamScratch = so ? stream_scratch_bytes(maxItems) : 0;
        const size_t scratchBytes = std::max(std::max(setupBytes, tailBytes), streamScratch);
        // size and pointers from the same traversal (bake_host.h): first over offsets, then over the arena
        if (!arena->reserve(carve_bake_tables(0, maxItems, scratchBytes, sh != nullptr, so != nullptr).bytes, *baker.devPool->poison)) return L.failure("[Failure] - out of device memory for the bake working set");
        tab = carve_bake_tables((uintptr_t)arena->base, maxItems, scratchBytes, sh != nullptr, so != nullptr);
        R.triAreaScratch = tab.triArea;
        return ommResult_SUCCESS;
    }
    // SetupWorkItems (bake_cpu_impl.cpp:589-660) on the device: reads the raw triangles; leaves the work items (uv, level, degen, triToItem, itemIds) and their counters
    ommResult setup_work_items()
    {
        coreT0 = now_ms();
        e0 = et.mark();
        memset(&S, 0, sizeof S);
        S.texCoords = din.texCoords; S.indices = din.indices; S.perTriLevels = din.perTriLevels;
        S.stride = uv_stride(d);
        S.uvFormat = d.texCoordFormat; S.indexFormat = d.indexFormat; S.numTris = T;
        S.globalLevel = d.maxSubdivisionLevel; S.dynScale = d.dynamicSubdivisionScale; S.edgeHeuristic = has_flag(flags, kBakeFlag_EnableEdgeHeuristic);   // (bake_cpu_impl.cpp:48,547)
        S.texW = tex.mips[0].w; S.texH = tex.mips[0].h; S.disableDedup = noDedup;
        S.wantWorkload = 1;   // (also the input of the two shape decisions of plan_states: streamed result, deferred generic pass)
        S.degenerateInvalid = has_flag(flags, kBakeFlag_DisableLevelLineIntersection);
        S.format = (int)d.format;   // (per-triangle formats other than the global one are refused above: one format per bake)
        bool ok = HIP_OK(hipMemcpyAsync(tab.counters, &bake_head(), sizeof(BakeHead), hipMemcpyHostToDevice, stream));   // (counters and digest table are adjacent slots of the carve: see BakeHead)
        ok = ok && HIP_OK(run_setup_fetch(S, tab.scratch, tab.scratchBytes, tab.counters, tab.known, maxItems, (uint32_t*)tab.fine, 2u * kFineSlots * kFineStride, tab.triArea, stream));
        if (!ok) return L.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)");
        if (d.dynamicSubdivisionScale > 0.f && T) { // degenerate triangles under dynamic subdivision need glibc's log2f: host (bake_cpu_impl.cpp:511-528)
            if (!HIP_OK(hipMemcpyAsync(&hc, tab.counters, sizeof hc, hipMemcpyDeviceToHost, stream)) || !HIP_OK(hipStreamSynchronize(stream)))
                return L.failure("[Failure] - device work-item setup failed");
            if (hc.numPending) if (const ommResult r = fix_pending_levels()) return r;
        }
        if (!HIP_OK(run_setup_items(S, tab.scratch, tab.scratchBytes, tab.counters, tab.uv, tab.level, tab.degen, tab.triToItem, tab.itemIds, stream)))
            return L.failure("[Failure] - device work-item setup failed");
        e1 = et.mark();
        return ommResult_SUCCESS;
    }
    // reads the hc.numPending triangles the device left undecided (setup scratch); leaves their levels, computed on the host, in the setup scratch
    ommResult fix_pending_levels()
    {
        std::vector<uint32_t> pend(hc.numPending); std::vector<float> puv((size_t)hc.numPending * 6); std::vector<uint8_t> plv(hc.numPending);
        const PoolBlock tmp(baker.devPool.get(), (size_t)hc.numPending * 24 + 256);
        if (!tmp.p) return L.failure("[Failure] - device work-item setup failed");
        if (!HIP_OK(copy_pending_to_host(tab.scratch, tab.scratchBytes, T, hc.numPending, pend.data(), puv.data(), tmp.p, stream))) return L.failure("[Failure] - device work-item setup failed");
        {   // (tiny triangles under dynamic subdivision are degenerate by the tens of thousands -- configs[4]: 1.5 ms of log2f on one thread; four share it)
            ommCpuBakeInputDesc tmpDesc = d; tmpDesc.subdivisionLevels = nullptr;   // per-triangle overrides were already honoured on the device
            auto part = [&](uint32_t k0, uint32_t k1) {
                for (uint32_t k = k0; k < k1; ++k) { HostTri t; memcpy(t.p, &puv[(size_t)k * 6], 24); plv[k] = (uint8_t)level_for_primitive(tmpDesc, flags, 0, t, S.texW, S.texH); }
            };
            // helper threads only with the caller's permission (ommCpuBakeFlags_EnableInternalThreads, omm.h:303: what the reference spends on its OpenMP
            // loops); a thread that cannot be started (std::system_error: thread limit, cgroup pids) leaves its share to this thread -- nothing escapes the C ABI
            const uint32_t n = hc.numPending, ways = (n >= 8192u && (flags & (uint32_t)ommCpuBakeFlags_EnableInternalThreads)) ? 4u : 1u;
            std::vector<std::thread> helpers;
            uint32_t started = 0;
            try {
                helpers.reserve(ways);
                for (uint32_t w = 1; w < ways; ++w) { helpers.emplace_back(part, (uint32_t)((uint64_t)n * w / ways), (uint32_t)((uint64_t)n * (w + 1u) / ways)); started = w; }
            } catch (...) {}
            part(0u, (uint32_t)((uint64_t)n / ways));
            for (auto& h : helpers) h.join();
            for (uint32_t w = started + 1u; w < ways; ++w) part((uint32_t)((uint64_t)n * w / ways), (uint32_t)((uint64_t)n * (w + 1u) / ways));   // (shares whose thread did not start)
        }
        if (!HIP_OK(run_setup_fix_pending(S, tab.scratch, tab.scratchBytes, pend.data(), plv.data(), hc.numPending, tmp.p, stream))) return L.failure("[Failure] - device work-item setup failed");
        return ommResult_SUCCESS;
    }
    // reads the desc and the texture; leaves the classification parameters P
    void classify_params()
    {
        memset(&P, 0, sizeof P);
        P.mipCount = (int)tex.mips.size();
        for (int m = 0; m < P.mipCount; ++m) P.mips[m] = dev_mip(tex.mips[m]);
        P.pow2Dispatch = P.mips[0].pow2;
        P.texIsFp32 = tex.format == ommCpuTextureFormat_FP32;
        P.addrMode = d.runtimeSamplerDesc.addressingMode;
        P.filterLinear = d.runtimeSamplerDesc.filter == ommTextureFilterMode_Linear;
        P.format = storeBits; P.promotion = d.unknownStatePromotion; P.stateGT = d.alphaCutoffGreater; P.stateLE = d.alphaCutoffLessEqual;
        P.useCoarse = tex.mips[0].sat != nullptr && P.mipCount == 1 && P.filterLinear;
        P.cutoff = d.alphaCutoff; P.borderAlpha = d.runtimeSamplerDesc.borderAlpha;
        P.wantKnownCount = d.rejectionThreshold > 0.f;
        P.noFine = has_flag(flags, kBakeFlag_DisableFineClassification);   // (bake_cpu_impl.cpp:45,822-823)
        P.altKernel = has_flag(flags, kBakeFlag_DisableLevelLineIntersection) ? (has_flag(flags, kBakeFlag_EnableAABBTesting) ? 2 : 1) : 0;   // (bake_cpu_impl.cpp:44-45,915-966)
    }
    // level-0 hierarchical query per item + compaction of the items that need per-micro-triangle work: reads the work items; leaves mask, active, activeIds, stateOfs
    // and the final counters on the host (hc, U) -- the ONE synchronisation of a bake before its result
    ommResult triage_and_compact()
    {
        launch_triage(P, tab.uv, tab.level, tab.degen, tab.counters, maxItems, tab.mask, tab.active, tab.scratch, stream);
        hostBlock = arena->host_block();
        SetupCounters* const hcDst = hostBlock ? (SetupCounters*)hostBlock : &hc;
        if (!HIP_OK(run_prep(tab.itemIds, tab.active, tab.level, storeBits, maxItems, tab.counters, tab.activeIds, tab.stateOfs, tab.scratch, tab.scratchBytes, stream)) ||
            !HIP_OK(hipMemcpyAsync(hcDst, tab.counters, sizeof hc, hipMemcpyDeviceToHost, stream)) || !HIP_OK(hipStreamSynchronize(stream)))
            return L.failure("[Failure] - device work-list compaction failed");
        if (hostBlock) memcpy(&hc, hcDst, sizeof hc);
        U = hc.numItems; numActive = hc.activeStart[kNumLevels]; microAll = (double)micro_triangles_of(hc.levelCount);
        return ommResult_SUCCESS;
    }
    // reads the counters; leaves the reference's messages about the workload, or its refusals
    ommResult report_workload()
    {
        if (has_flag(flags, ommCpuBakeFlags_EnableValidation) && hc.numDisabled != 0) { // bake_cpu_impl.cpp:652-657
            char buf[256];
            snprintf(buf, sizeof buf, "[Info] - The workload consists of %d unclassifiable triangles, these will be classified as unresolvedTriState = %s.", hc.numDisabled, special_name(d.unresolvedTriState));
            L.msg(ommMessageSeverity_Info, buf);
        }
        // ---- ValidateWorkloadSize (bake_cpu_impl.cpp:662-713) ----
        if (has_flag(flags, ommCpuBakeFlags_EnableWorkloadValidation) || d.maxWorkloadSize != 0xFFFFFFFFFFFFFFFFull) {
            if (d.maxWorkloadSize != 0xFFFFFFFFFFFFFFFFull && hc.workload > d.maxWorkloadSize) return ommResult_WORKLOAD_TOO_BIG;
            if (has_flag(flags, ommCpuBakeFlags_EnableWorkloadValidation) && hc.workload > (1ull << 27)) {
                char buf[256];
                snprintf(buf, sizeof buf, "[Perf Warning] - The workload consists of %lld work items (number of texels to classify), which corresponds to roughly %lld 1024x1024 textures."
                         " This is unusually large and may result in long bake times.", (long long)hc.workload, (long long)(hc.workload >> 20));
                L.msg(ommMessageSeverity_PerfWarning, buf);
            }
        }
        if (has_flag(flags, kBakeFlag_EnableAABBTesting) && !has_flag(flags, kBakeFlag_DisableLevelLineIntersection))   // bake_cpu_impl.cpp:718-719 (ResampleCoarse is the first to look, behind the workload validation)
            return L.invalid("[Invalid Arg] - EnableAABBTesting can't be used without also setting DisableLevelLineIntersection");
        return ommResult_SUCCESS;
    }
    // reads the counters and the mode; leaves this rank's ranges, the two shape decisions (streamed result, with its host array; deferred generic pass) and the states arena
    // reserved and carved.  The decisions themselves are bake_host.h's.
    ommResult plan_states()
    {
        memset(&bounds, 0, sizeof bounds);
        bounds.rank = sh ? sh->rank : 0; bounds.world = sh ? sh->world : 1;
        rank_ranges(hc.activeStart, bounds.rank, bounds.world, bounds.b, lvlFirst, lvlCount);
        // streamed result (ommCpuBake)?  (with special indices disabled every uniform item is a block too: the plain path handles that)
        if (so && numActive && !has_flag(flags, ommCpuBakeFlags_DisableSpecialIndices) && !P.altKernel && storeBits == bits) {
            const uint32_t k = stream_range_count(hc.stateBytes, microAll, hc.workload, so->compressedAvailable, so->forced, so->chunksWanted);
            if (k && so->set->pinned.reserve(4096) && (hostArray = so->alloc(so->allocUser, hc.stateBytes, &hostPinned)) != nullptr) { streamChunks = k; hCursor = (unsigned long long*)so->set->pinned.base; }
        }
        // the queue of open tiles (kTileRecordBytes records, bake_kernels.hip)
        const size_t queueBytes = (size_t)classify_queue_records(lvlCount, streamChunks > 1) * kTileRecordBytes + 16;
        // deferred generic pass?  Not for streamed bakes (a range must be complete when its queue sections are); a sharded rank defers the walks of its share like a
        // single GPU does (asset-sized cards, 8 ranks: 15.0 -> 12 ms per step), except when the ranks merge their states by summation.
        if (generic_pass_wanted(baker.knob(ommxBakerKnob_GenericPass), microAll, hc.workload) && !streamChunks && !(sh && sh->mergeStates) && !ht && numActive)
            genericCapacity = generic_pass_capacity(hc.stateBytes, storeBits);
        if (!statesArena->reserve(carve_bake_states(0, hc.stateBytes, queueBytes, streamChunks != 0, genericCapacity).bytes, *baker.devPool->poison)) return L.failure("[Failure] - out of device memory for the packed micro-triangle states");
        st = carve_bake_states((uintptr_t)statesArena->base, hc.stateBytes, queueBytes, streamChunks != 0, genericCapacity);
        e1b = et.mark();
        return ommResult_SUCCESS;
    }
    // sharded bakes only: reads the active lists; leaves the states zeroed where the ranks merge them by summation, and every level's list interleaved, which evens
    // out the per-rank cost (tail_kernels.hip: shard_interleave)
    ommResult permute_for_ranks()
    {
        if (sh && sh->mergeStates && !HIP_OK(hipMemsetAsync(st.states, 0, st.stateBytes, stream))) return L.failure("[Failure] - device memset failed");
        if (!sh || sh->world <= 1) return ommResult_SUCCESS;
        // the permuted copy goes through the (idle) setup / tail scratch block: no allocation, no synchronisation, stream ordered
        uint32_t* tmp = (uint32_t*)tab.scratch;
        bool okp = (size_t)numActive * 4 <= tab.scratchBytes;
        for (int l = 0; l < kNumLevels && okp; ++l) {
            const uint32_t a = hc.activeStart[l], cnt = hc.activeStart[l + 1] - hc.activeStart[l];
            if (cnt < 3) continue;
            launch_shard_interleave(tab.activeIds + a, tmp + a, cnt, interleave_stride(cnt), stream);
            okp = HIP_OK(hipMemcpyAsync(tab.activeIds + a, tmp + a, (size_t)cnt * 4, hipMemcpyDeviceToDevice, stream));
        }
        return okp ? ommResult_SUCCESS : L.failure("[Failure] - shard permutation failed");
    }
    // ResampleCoarse + ResampleFine (bake_cpu_impl.cpp:715-1029) on the active items: reads the work items, this rank's ranges and the plan; leaves the packed states
    // (streamed: the placement enqueued behind every range, through `sr`)
    ommResult classify(StreamRun& sr)
    {
        A.uv = tab.uv; A.degenerate = tab.degen; A.stateOfs = tab.stateOfs; A.states = st.states; A.stateMask = tab.mask; A.knownCount = tab.known; A.fineCount = tab.fine;
        // (tab.fine was zeroed by the first set-up launch, with the known counts)
        memset(&cc, 0, sizeof cc); cc.count = 1;
        mk.et = &et; mk.mark = -1; mk.markGeneric = -1;
        if (streamChunks) { if (const ommResult r = sr.begin(*this)) return r; }
        else { cc.mark = mark_hook; cc.user = &mk; cc.early = nullptr; }   // (HIP event in front of the persistent launch of the levels >= 6)
        if (genericCapacity) {
            if (!HIP_OK(hipMemsetAsync(st.genericCount, 0, 256, stream))) return L.failure("[Failure] - device memset failed");
            cc.generic.count = (unsigned long long*)st.genericCount; cc.generic.entries = (uint2*)st.genericEntries; cc.generic.capacity = (uint32_t)genericCapacity;
            cc.markGeneric = mark_generic_hook;   // (cc.user is the MarkCtx: a deferred pass and a streamed result exclude each other)
        }
        if (!HIP_OK(launch_classify(P, A, tab.activeIds, lvlFirst, lvlCount, st.tileQueue, st.queueCtl, device_cu_count(), stream, &cc))) return L.failure("[Failure] - kernel launch failed");
        if (streamChunks && !sr.sc.ok) return L.failure("[Failure] - kernel launch failed");
        e2 = et.mark();
        return ommResult_SUCCESS;
    }
    // host-tail bakes end here: reads the per-micro-triangle states; leaves them on the host for the serial tail (host_tail.cpp), and the timings so far
    ommResult gather_for_host_tail()
    {
        const ommResult gr = gather_host_items(L, stream, U, T, hc, tab.uv, tab.level, tab.active, tab.mask, tab.stateOfs, st.states, tab.triToItem, bits, ht->items);
        tm.setupMs = et.ms(e0, e1); tm.triageMs = et.ms(e1, e1b); tm.classifyMs = et.ms(e1b, e2); tm.uniqueItems = U;
        return gr;
    }
    // CalcDigest (bake_cpu_impl.cpp:1038-1040): reads the packed states of the active items; leaves their digests (uniform items: from the table, in the tail)
    ommResult digest()
    {
        if (!noDedup && !streamChunks)   // (a streamed bake computed them range by range)
            launch_digest_levels(st.states, tab.stateOfs, tab.activeIds, lvlFirst, lvlCount, (uint32_t)storeBits, tab.digests, stream);
        if (!HIP_OK(hipGetLastError())) return L.failure("[Failure] - kernel launch failed");
        e3 = et.mark();
        return ommResult_SUCCESS;
    }
    // reads the tables; leaves the tail's inputs and outputs (promote / dedup / sort / offsets on the device) -- what a sharded bake hands to its later phases
    void tail_inputs()
    {
        memset(&ti, 0, sizeof ti);
        ti.numItems = U; ti.numTris = T; ti.uv = tab.uv; ti.level = tab.level; ti.stateMask = tab.mask; ti.knownCount = tab.known; ti.digests = tab.digests;
        ti.uniformDigest = tab.uniformDigest; ti.triToItem = tab.triToItem; ti.format = bits;
        ti.maxDistinctDigests = max_distinct_digests(numActive);
        ti.disableSpecial = has_flag(flags, ommCpuBakeFlags_DisableSpecialIndices); ti.disableDedup = noDedup;
        ti.rejectionThreshold = d.rejectionThreshold; ti.unresolved = (int32_t)d.unresolvedTriState; ti.errorFlag = tab.err;
        memset(&to, 0, sizeof to);
        to.special = tab.special; to.rep = tab.rep; to.order = tab.order; to.dstOfs = tab.dstOfs; to.sizes = tab.sizes; to.itemValue = tab.itemValue;
        to.indexBuffer = tab.index; to.arrayHist = tab.arrayHist; to.indexHist = tab.indexHist;
    }
    // sharded bakes end here (ommxShardedBegin): reads everything above; leaves it in the ShardCtx, with the metadata words of this rank's share packed for the exchange
    ommResult hand_to_shard()
    {
        sh->bounds = bounds; sh->ti = ti; sh->to = to; sh->hc = hc; sh->dStates = st.states; sh->tab = tab;
        sh->flags = flags; sh->T = T; sh->bits = bits;
        launch_shard_pack_meta(bounds, tab.activeIds, numActive, tab.mask, tab.known, tab.digests, tab.meta, stream);
        if (!sh->asyncBegin && !HIP_OK(hipStreamSynchronize(stream))) return L.failure("[Failure] - sharded classification failed");   // (the one-call RCCL path stays on the stream)
        sh->ev[0] = e0; sh->ev[1] = e1; sh->ev[2] = e1b; sh->ev[3] = e2; sh->ev[4] = e3;   // (read in Finish, when the events are complete)
        tm.uniqueItems = U; tm.activeItems = numActive; tm.stateBytes = hc.stateBytes;
        tm.microTriangles += micro_triangles_of(hc.levelCount);
        return ommResult_SUCCESS;
    }
    // promote / dedup / sort / offsets on the device: reads ti; leaves the tail's tables, the index buffer of the result, `counts`, and the result's sizes in R
    ommResult tail()
    {
        // the index format depends on the triangle count alone: the tail's index kernel writes the narrowed buffer next to the int32 one (bake_cpu_impl.cpp:1872-1902)
        R.indexFormat = index_format_for(T, flags);
        R.index = R.dev_alloc((size_t)(T ? T : 1) * 4); // the reference narrows in place inside an int32 vector (:1882-1900)
        if (!R.index) return L.failure("[Failure] - could not allocate the device result");
        to.narrowIndex = R.index; to.narrowBytes = (int)index_bytes(R.indexFormat);
        if (!HIP_OK(run_tail(ti, to, tab.scratch, tab.scratchBytes, &counts, stream, hostBlock ? hostBlock + 256 : nullptr))) return L.failure("[Failure] - device tail failed");
        if (counts.arrayDataSize > 0xFFFFFFFFull) return ommResult_FAILURE; // bake_cpu_impl.cpp:1774-1775
        e4 = et.mark();
        R.bits = bits; R.numDescs = counts.numOmms; R.arrayDataSize = counts.numOmms ? counts.arrayDataSize : 0; R.numTris = T;
        return ommResult_SUCCESS;
    }
    // Serialize (bake_cpu_impl.cpp:1756-1920): reads the tail's order and offsets; leaves the descriptors and, unless the streamed result stands, the surviving blocks
    // gathered into arrayData order.  false: an allocation failed (reported by read_back_statistics, behind the read-backs it still queues)
    bool materialise()
    {
        const uint32_t E = counts.numOmms;
        if (!E) return true;
        R.descs = (ommCpuOpacityMicromapDesc*)R.dev_alloc(sizeof(ommCpuOpacityMicromapDesc) * (size_t)E);
        if (!streamed) R.arrayData = (uint8_t*)R.dev_alloc((size_t)counts.arrayDataSize);
        if (R.descs == nullptr || (!streamed && R.arrayData == nullptr)) return false;
        if (!streamed) {
            uint8_t* unitCodes = nullptr; uint32_t* blockRawCounts = nullptr;
            if (R.gatherCodes && storeBits == bits && counts.smallOmms == 0 && !R.gatherCodes(counts.arrayDataSize, &unitCodes, &blockRawCounts)) { unitCodes = nullptr; blockRawCounts = nullptr; }
            launch_gather_omms(st.states, tab.stateOfs, tab.active, tab.mask, tab.level, bits, storeBits, tab.order, tab.dstOfs, tab.sizes, E, R.arrayData, stream, unitCodes, blockRawCounts, R.descs);
        } else launch_write_descs(tab.order, tab.dstOfs, tab.level, bits, E, R.descs, stream);   // (the gather writes the descriptors of its OMMs itself)
        return true;
    }
    // reads the two histograms, the consistency word and the striped statistic counters, taken from the arena back to back (ONE read-back), the classification's
    // control words and the generic pass's; leaves R.hist and the statistics, and the stream idle -- the second and last wait of a bake
    ommResult read_back_statistics(bool ok)
    {
        std::vector<unsigned long long> fineSlots((size_t)kFineSlots * kFineStride, 0ull);
        const size_t spanBytes = tab.readback_bytes();
        // (into the arena's pinned block when there is one: three copies queued, ONE wait -- into pageable memory each copy is a wait of its own)
        uint32_t hostCtlLocal[kClassifyCtlWords];
        unsigned long long genericLocal[3] = { 0, 0, 0 };
        static_assert(sizeof genericLocal == kGenericReadbackBytes, "the generic pass's words as readback_slots places them");
        const ReadbackSlots at = readback_slots(spanBytes);
        const bool pinnedBack = hostBlock && at.fits;
        std::vector<uint8_t> spanLocal(pinnedBack ? 0 : spanBytes);
        uint8_t* const span = pinnedBack ? hostBlock + at.spanAt : spanLocal.data();
        uint32_t* const hostCtl = pinnedBack ? (uint32_t*)(hostBlock + at.ctlAt) : hostCtlLocal;
        unsigned long long* const genericWords = pinnedBack ? (unsigned long long*)(hostBlock + at.genAt) : genericLocal;
        memset(hostCtl, 0, sizeof hostCtlLocal); memset(genericWords, 0, sizeof genericLocal);
        ok = ok && HIP_OK(hipMemcpyAsync(span, tab.arrayHist, spanBytes, hipMemcpyDeviceToHost, stream));
        if (numActive) ok = ok && HIP_OK(hipMemcpyAsync(hostCtl, st.queueCtl, sizeof hostCtlLocal, hipMemcpyDeviceToHost, stream));
        if (genericCapacity) ok = ok && HIP_OK(hipMemcpyAsync(genericWords, st.genericCount, sizeof genericLocal, hipMemcpyDeviceToHost, stream));
        e5 = et.mark();
        ok = ok && HIP_OK(hipStreamSynchronize(stream));
        // (a streamed result may still be on its way to the host: the caller queues its small read-backs first and then waits, StreamOut::finish)
        if (!ok) return L.failure("[Failure] - could not materialise the bake result on the device");
        memcpy(R.hist, span, sizeof(uint32_t) * kNumLevels);
        memcpy(R.hist + kNumLevels, span + ((const uint8_t*)tab.indexHist - (const uint8_t*)tab.arrayHist), sizeof(uint32_t) * kNumLevels);
        memcpy(fineSlots.data(), span + ((const uint8_t*)tab.fine - (const uint8_t*)tab.arrayHist), sizeof(unsigned long long) * fineSlots.size());
        for (int k = 0; k < kFineSlots; ++k) fineCount += fineSlots[(size_t)k * kFineStride];
        queueTails[1] = hostCtl[kCtl1024 + kSecTails]; for (uint32_t k = 0; k < kMaxClassifyChunks; ++k) queueTails[0] += hostCtl[kSecTails + k];   // (1024-tile queue; sections of the 4096-tile queue)
        genericMicro = genericWords[2];
        return ommResult_SUCCESS;
    }
    // reads the event marks (all complete) and the statistics; leaves the timings of a whole bake
    void fill_timings(const StreamRun& sr)
    {
        tm.uploadMs = 0.f; tm.hostSetupMs = 0.f; tm.setupMs = et.ms(e0, e1); tm.triageMs = et.ms(e1, e1b); tm.classifyMs = et.ms(e1b, e2); tm.digestMs = et.ms(e2, e3);
        tm.streamPreviewMs = sr.pv0 >= 0 ? et.ms(sr.pv0, sr.pv1) : 0.f;
        tm.tailMs = et.ms(e3, e4); tm.gatherMs = et.ms(e4, e5); tm.persistentMs = mk.mark >= 0 ? et.ms(mk.mark, mk.markGeneric >= 0 ? mk.markGeneric : e2) : 0.f;
        tm.genericMs = mk.markGeneric >= 0 ? et.ms(mk.markGeneric, e2) : 0.f; tm.genericMicroTriangles = genericMicro;
        tm.openTiles = queueTails[0] + queueTails[1]; tm.openTileMicroTriangles = (uint64_t)queueTails[0] * 4096u + (uint64_t)queueTails[1] * 1024u;
        tm.fineMicroTriangles = fineCount; tm.uniqueItems = U; tm.activeItems = numActive; tm.stateBytes = hc.stateBytes; tm.microTriangles = micro_triangles_of(hc.levelCount);
        tm.classifyLaunches += classify_launches(hc.activeStart);
    }
};

// streamed: the active lists in the order of the final result, events behind the classification launches, the cursor published to a pinned word after each
ommResult StreamRun::begin(BakeRun& b)
{
    const BakeTables& tab = b.tab; const hipStream_t stream = b.stream; const uint32_t streamChunks = b.streamChunks, numActive = b.numActive;
    ClassifyChunks& cc = b.cc;
    bool oks = HIP_OK(hipMemsetAsync(tab.placed, 0xFF, (size_t)b.maxItems * 8, stream)) && HIP_OK(hipMemsetAsync(tab.cursor, 0, 8, stream)) && HIP_OK(hipMemsetAsync(tab.streamCtl, 0, sizeof(uint32_t) * kStreamCtlWords, stream));
    oks = oks && HIP_OK(run_stream_begin(tab.activeIds, numActive, tab.uv, tab.level, tab.scratch, tab.scratchBytes, stream));
    oks = oks && events.create(2u * streamChunks + 3u);
    if (!oks) return b.L.failure("[Failure] - could not set up the streamed result");
    sc.stream = stream; sc.place = b.so->placeStream; sc.fences = events.ev + streamChunks + 1u; sc.activeIds = tab.activeIds; sc.numActive = numActive; sc.scratch = tab.scratch; sc.scratchBytes = tab.scratchBytes; sc.digests = tab.digests;
    sc.cursor = tab.cursor; sc.stage = b.st.stage; sc.placed = tab.placed; sc.ctl = tab.streamCtl; sc.hostCursor = b.hCursor; sc.events = events.ev; sc.numEvents = streamChunks + 1u; sc.recorded = 0; sc.ok = true;
    memset(&sc.proto, 0, sizeof sc.proto);
    sc.proto.stateMask = tab.mask; sc.proto.knownCount = tab.known; sc.proto.digests = tab.digests; sc.proto.states = b.st.states; sc.proto.stateOfs = tab.stateOfs;
    sc.proto.rejectionThreshold = b.d.rejectionThreshold; sc.proto.bits = b.bits; sc.proto.disableDedup = b.noDedup ? 1 : 0;
    cc.count = streamChunks; cc.after = stream_hook; cc.mark = stream_mark_hook; cc.user = &sc; cc.early = nullptr; sc.queueCtl = b.st.queueCtl;
    sc.paired = streamChunks > 1; sc.earlyList = nullptr; sc.earlyCapacity = 0; sc.itemLevel = tab.level;
    sc.waitSeconds = stream_wait_seconds(b.microAll, b.hc.workload);
    // preview (tail_kernels.hip): level-5 classification of the items of level >= 6 into buffers of its own; items that share their preview are classified early
    const uint32_t first6 = b.hc.activeStart[6], count6 = numActive - b.hc.activeStart[6];
    if (count6 && streamChunks > 1) {
        pv0 = b.et.mark();
        ClassifyParams P2 = b.P; P2.format = 2; P2.promotion = 1; P2.wantKnownCount = 0; P2.noFine = 0;
        ItemArrays A2 = b.A; A2.uv = tab.uv2; A2.stateOfs = tab.ofs2; A2.states = tab.states2; A2.stateMask = tab.mask2; A2.fineCount = tab.fine2;   // (its level-line statistic goes nowhere)
        bool okp = HIP_OK(hipMemsetAsync(tab.early, 0, b.maxItems, stream)) && HIP_OK(hipMemsetAsync(tab.mask2, 0, (size_t)b.maxItems * 4, stream));
        launch_stream_preview_prepare(tab.activeIds + first6, count6, tab.uv, b.P.mips[0].fw, b.P.mips[0].fh, tab.uv2, tab.ofs2, tab.early, stream);
        {   // the preview items as ONE level-5 class of the ordinary classification: a 1024-tile each, tile triage (most previews are settled by one SAT
            // query), LDS window and the single-texel pass for the rest -- through the bake's own tile queue, which is free until the real launch
            static_assert(kPreviewLevel == 5, "the preview is the 1024-tile class");
            uint32_t first2[kNumLevels], count2[kNumLevels];
            for (int l = 0; l < kNumLevels; ++l) { first2[l] = 0; count2[l] = 0; }
            first2[kPreviewLevel] = first6; count2[kPreviewLevel] = count6;
            okp = okp && HIP_OK(launch_classify(P2, A2, tab.activeIds, first2, count2, b.st.tileQueue, b.st.queueCtl, device_cu_count(), stream, nullptr));
        }
        ClassifyPlan plan; classify_plan(b.lvlFirst, b.lvlCount, streamChunks, &plan);   // (the ranges launch_classify will cut)
        okp = okp && HIP_OK(run_stream_preview_flags(tab.activeIds + first6, count6, first6, numActive, tab.states2, tab.level, tab.early, tab.streamCtl, tab.scratch, tab.scratchBytes, tab.earlyLead, tab.earlyList, plan, stream));
        if (!okp) return b.L.failure("[Failure] - could not set up the streamed result");
        cc.early = tab.early; cc.earlyLead = tab.earlyLead; cc.earlyStage = b.st.stage; sc.proto.early = tab.early; sc.earlyList = tab.earlyList; sc.earlyCapacity = count6;
        pv1 = b.et.mark();
    }
    return ommResult_SUCCESS;
}
// everything is enqueued: follow the classification launches and send what each one placed
ommResult StreamRun::follow(BakeRun& b)
{
    StreamOut& so = *b.so; ommxBakeTimings& tm = b.tm;
    SdmaCopier& sdma = so.sdma;   // (ommCpuBake's: it outlives the bake, the caller waits for the copies in flight, StreamOut::finish)
    const bool useSdma = b.hostPinned && sdma.open(so.device);
    for (uint32_t k = 0; k < sc.recorded; ++k) {
        if (!HIP_OK(hipEventSynchronize(events.ev[k]))) return b.L.failure("[Failure] - the classification failed");
        if (k + 1u == sc.recorded) so.classifyEndMs = now_ms();
        if (k < 32u) tm.streamRangeReadyMs[k] = (float)(now_ms() - b.coreT0);
        const uint64_t cur = *(volatile unsigned long long*)(b.hCursor + k);
        if (cur > sent) {
            // (a copy the DMA engine refuses goes through the HIP runtime instead of failing the bake)
            const bool okc = cur <= b.hc.stateBytes && ((useSdma && sdma.copy_to_host(b.hostArray + sent, b.st.stage + sent, (size_t)(cur - sent)))
                                                        || HIP_OK(hipMemcpyAsync(b.hostArray + sent, b.st.stage + sent, (size_t)(cur - sent), hipMemcpyDeviceToHost, so.copyStream)));
            if (!okc) return b.L.failure("[Failure] - device to host transfer of the bake result failed");
            if (sent == 0) tm.streamFirstCopyMs = (float)(now_ms() - b.coreT0);
            tm.streamLastCopyMs = (float)(now_ms() - b.coreT0);
            sent = cur;
        }
    }
    return ommResult_SUCCESS;
}
// the blocks are (or will shortly be) at their final offsets in the caller's array, provided the speculative placement equals the exact layout the tail has just
// produced: compare, and fall back to the ordinary gather + copy otherwise
ommResult StreamRun::verify(BakeRun& b)
{
    const BakeTables& tab = b.tab; StreamOut& so = *b.so; const uint32_t E = b.counts.numOmms;
    uint32_t hctl[4] = { 0u, 0u, 0u, 0u };
    launch_stream_verify(tab.order, tab.dstOfs, E, tab.placed, tab.streamCtl, b.stream);
    if (!HIP_OK(hipMemcpyAsync(hctl, tab.streamCtl, sizeof hctl, hipMemcpyDeviceToHost, b.stream)) || !HIP_OK(hipStreamSynchronize(b.stream)))
        return b.L.failure("[Failure] - could not verify the streamed result");
    const bool streamed = hctl[2] == 0u && sent == b.R.arrayDataSize;
    if (!streamed) {
        (void)so.finish();   // (the caller is about to overwrite the host array with the ordinary copy: nothing of the discarded stream may still be landing in it)
        char buf[256];
        snprintf(buf, sizeof buf, "[Perf Warning] - the streamed result was discarded (%u blocks placed / %u expected, %llu bytes / %llu expected, duplicate owned by a later range: %u): "
                 "falling back to one copy after the bake", hctl[0], E, (unsigned long long)sent, (unsigned long long)b.R.arrayDataSize, hctl[1]);
        b.L.msg(ommMessageSeverity_PerfWarning, buf);
    }
    so.chunks = b.streamChunks; so.streamedBytes = sent; so.used = streamed; so.fellBack = !streamed;
    b.tm.streamChunks = streamed ? b.streamChunks : 0u; b.tm.streamedBytes = sent; b.tm.streamEarlyItems = hctl[3];
    b.streamed = streamed;
    return ommResult_SUCCESS;
}

// The bake proper: bake_cpu_impl.cpp:1923-1985 re-organised for the device.  `din` points at device copies of the caller's texCoords / indexBuffer /
// subdivisionLevels.  The mode pointers: `sh` a sharded begin (stops behind the digests), `ht` a host tail (stops behind the classification), `so` a streamed
// result on offer (ommCpuBake).  Two waits on the stream per bake (three with degenerate triangles under dynamic subdivision, or a streamed result to verify).
// What goes when, on every path out: the stages' own temporaries go when the stage returns (the pooled block of fix_pending_levels before the work items are
// written, the read-back buffers with read_back_statistics); `streamRun`, declared first, goes last and destroys the events behind the ranges of a streamed
// result.  The SdmaCopier of a streamed result is `so`'s and outlives the call: the copies in flight are the caller's to wait for (StreamOut::finish), on error
// paths too, while those events are already gone -- as before, when a copier of this function's own (never opened: streaming needs `so`) went first.
ommResult bake_core(Baker& baker, const ommCpuBakeInputDesc& d, const DeviceInputs& din, DeviceArena* arena, DeviceArena* statesArena, hipStream_t stream, EventTimer& et,
                    DeviceResult& R, ommxBakeTimings& tm, ShardCtx* sh = nullptr, HostTailRequest* ht = nullptr, StreamOut* so = nullptr)
{
    StreamRun streamRun;
    BakeRun b(baker, d, din, arena, statesArena, stream, et, R, tm, sh, ht, so);
    if (const ommResult r = b.carve_tables()) return r;
    if (const ommResult r = b.setup_work_items()) return r;
    b.classify_params();
    if (const ommResult r = b.triage_and_compact()) return r;
    if (const ommResult r = b.report_workload()) return r;
    if (const ommResult r = b.plan_states()) return r;
    if (const ommResult r = b.permute_for_ranks()) return r;
    if (const ommResult r = b.classify(streamRun)) return r;
    if (ht) return b.gather_for_host_tail();
    if (const ommResult r = b.digest()) return r;
    if (b.streamChunks) if (const ommResult r = streamRun.follow(b)) return r;
    b.tail_inputs();
    if (sh) return b.hand_to_shard();
    if (const ommResult r = b.tail()) return r;
    if (b.streamChunks) if (const ommResult r = streamRun.verify(b)) return r;
    if (const ommResult r = b.read_back_statistics(b.materialise())) return r;
    b.fill_timings(streamRun);
    return ommResult_SUCCESS;
}

ommResult scope_fences(const Baker& baker, const ommCpuBakeInputDesc& d, bool formatsOnHost, bool hostTailOk = true, bool plainEntry = true)
{
    const Logger& L = baker.log;
    if (wants_host_tail(d) && !hostTailOk) // the serial reducers run on the host over the merged states: not in the caller-driven four-phase protocol
        { L.msg(ommMessageSeverity_Fatal, "[Not Implemented] - near-duplicate merging / maxArrayDataSize budgets are available through ommCpuBake, ommxBakeDevice and ommxShardedBakeRccl, not through ommxShardedBegin/Tail/Finish"); return ommResult_NOT_IMPLEMENTED; }
    // internal flags (bake_cpu_impl.cpp:43-48): EnableAABBTesting (7) / DisableLevelLineIntersection (8) select the reference's ConservativeBilinearKernel
    // (ClassifyParams::altKernel), DisableFineClassification (9), the brute-force near-duplicate search (10) and EnableEdgeHeuristic (11) are honoured
    // without the fine pass unresolved micro-triangles keep the state UnknownOpaque (3), which the reference ORs into ONE bit of a 2-state block together with
    // its neighbour's (bake_cpu_impl.cpp:1811) while digesting the unpacked value: bake_core keeps such a bake in the 2-bit packing up to the final gather --
    // on the two single-device entry points; not where blocks travel between ranks or to the host tail in their packed form
    if (no_fine_two_state(d) && (!plainEntry || wants_host_tail(d)))
        { L.msg(ommMessageSeverity_Fatal, "[Not Implemented] - internal bake flag DisableFineClassification (bit 9) with OC1_2_State is supported by ommCpuBake / ommxBakeDevice without near-duplicate merging or a size budget"); return ommResult_NOT_IMPLEMENTED; }
    if (d.formats) { // the reference sizes its arrays from the global format only (bake_cpu_impl.cpp:1763-1772): mixed formats corrupt its heap
        if (!formatsOnHost) return L.failure("[Failure] - per-triangle formats are not supported on the device-resident entry point");
        for (uint32_t i = 0; i < d.indexCount / 3u; ++i)
            if (d.formats[i] != ommFormat_INVALID && d.formats[i] != d.format)
                return L.failure("[Failure] - per-triangle formats that differ from the global format are not supported");
    }
    return ommResult_SUCCESS;
}

// the dispatch table lookup precedes ValidateDesc (bake_cpu_impl.cpp:297-304): unknown sampler enums of a bake from a texture of this library -> FAILURE
bool sampler_enums_unknown(const ommCpuBakeInputDesc& desc)
{
    return tag_of(desc.texture) == kTexture &&
           ((unsigned)desc.runtimeSamplerDesc.addressingMode >= (unsigned)ommTextureAddressMode_MAX_NUM ||
            (unsigned)desc.runtimeSamplerDesc.filter >= (unsigned)ommTextureFilterMode_MAX_NUM);
}
// What every bake entry point checks first, in the reference's order.  `outIsSet`: ommxBakeDevice reports a null result pointer together with a null desc.
ommResult check_bake_entry(ommBaker baker, const ommCpuBakeInputDesc* desc, Baker** outB, bool outIsSet = true)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    Baker* b = untag<Baker>(baker);
    if (desc == 0 || !outIsSet) return b->log.invalid("input desc was not set");
    if (tag_of(baker) != kCpuBaker) return b->log.invalid("Baker was not created as the right type");
    if (desc->texture == 0) return b->log.invalid("[Invalid Argument] - ommCpuBakeInputDesc has no texture set"); // bake_cpu_impl.cpp:97-103
    if (sampler_enums_unknown(*desc)) return ommResult_FAILURE;
    *outB = b;
    return validate_desc(*b, *desc);
}

struct DeviceBakeResult {
    Allocator mem; DeviceResult R;
    ommCpuOpacityMicromapUsageCount arrayHist[2 * kNumLevels], indexHist[2 * kNumLevels];
    ommCpuBakeResultDesc desc;
};
// The one maker of a DeviceBakeResult handle and its owner until release(): a handle that is given up -- give_up(), or the scope is left -- is destroyed only
// after `drain` is idle (pooled blocks go back only when the stream is idle).  A null `drain`: the scope has drained the stream by other means.
struct DeviceResultOwner {
    Allocator mem; hipStream_t drain; DeviceBakeResult* p;
    DeviceResultOwner(const Allocator& mem_, hipStream_t drain_, DeviceBakeResult* adopted = nullptr) : mem(mem_), drain(drain_), p(adopted) {}
    DeviceResultOwner(const DeviceResultOwner&) = delete; DeviceResultOwner& operator=(const DeviceResultOwner&) = delete;
    ~DeviceResultOwner() { give_up(); }
    bool make() { p = mem.make<DeviceBakeResult>(); if (p) { p->mem = mem; memset(&p->desc, 0, sizeof p->desc); } return p != nullptr; }
    void give_up() { if (!p) return; if (drain) (void)hipStreamSynchronize(drain); mem.destroy(p); p = nullptr; }
    DeviceBakeResult* release() { DeviceBakeResult* r = p; p = nullptr; return r; }
    DeviceBakeResult* operator->() const { return p; }
    explicit operator bool() const { return p != nullptr; }
};
// histogram lists and descriptor of a device-resident result whose arrays and R.hist are complete (ommxBakeDevice, the sharded bake's phase 3)
void finish_device_result(DeviceBakeResult* res)
{
    const DeviceResult& R = res->R;
    uint32_t nAH = 0, nIH = 0;
    compact_histograms(R.hist, R.bits, res->arrayHist, res->indexHist, &nAH, &nIH);
    fill_result_desc(&res->desc, R.arrayData, R.arrayDataSize, R.descs, R.numDescs, R.index, R.numTris, R.indexFormat, res->arrayHist, nAH, res->indexHist, nIH);
}

// ---- the entries that take device-resident results: what a caller's result must be; and, for ommxCoarsenMicromap, ommxCombineMicromaps and ommxGatherMicromaps, the new handle ----
bool is_index_format(ommIndexFormat f) { return f == ommIndexFormat_UINT_8 || f == ommIndexFormat_UINT_16 || f == ommIndexFormat_UINT_32; }
bool has_null_array(const ommCpuBakeResultDesc& r)
{
    return r.indexCount && (r.indexBuffer == nullptr || (r.descArrayCount && (r.descArray == nullptr || (r.arrayData == nullptr && r.arrayDataSize))));
}
bool usable_device()
{
    int deviceCount = 0;
    if (HIP_OK(hipGetDeviceCount(&deviceCount)) && deviceCount >= 1) return true;
    (void)hipGetLastError();
    return false;
}
// the baker of such an entry; null: the handle is not a baker's (INVALID_ARGUMENT, with nobody to tell)
Baker* baker_for_device_results(ommBaker baker) { return baker != 0 && (tag_of(baker) == kCpuBaker || tag_of(baker) == kGpuBaker) ? untag<Baker>(baker) : nullptr; }
// the sources of ommxCombineMicromaps and ommxGatherMicromaps: the entry's checks, in the documented order (descName: the entry's desc struct, null when unset)
ommResult check_result_array(const Logger& log, const ommCpuBakeResultDesc* const* results, uint32_t count, const char* descName, bool haveDesc, const char* limitName,
                             uint32_t limit, bool haveOutput)
{
    char buf[160];
    if (results == nullptr) return log.invalid("[Invalid Arg] - deviceResults was not set");
    if (!haveDesc) { snprintf(buf, sizeof buf, "[Invalid Arg] - %s was not set", descName); return log.invalid(buf); }
    if (count == 0 || count > limit) { snprintf(buf, sizeof buf, "[Invalid Arg] - resultCount must be 1..%s (%u)", limitName, limit); return log.invalid(buf); }
    for (uint32_t k = 0; k < count; ++k)
        if (results[k] == nullptr) return log.invalid("[Invalid Arg] - an element of deviceResults was not set");
    if (!haveOutput) return log.invalid("[Invalid Arg] - neither outResult nor outInfo was set");
    return ommResult_SUCCESS;
}
// the one source of ommxCoarsenMicromap, ommxCoarsenMicromapLevels and ommxReorientMicromap: the entry's first checks, in the documented order; *b <- the baker
ommResult check_one_result(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const char* descName, bool haveDesc, bool haveOutput, Baker** b)
{
    char buf[160];
    *b = baker_for_device_results(baker);
    if (!*b) return ommResult_INVALID_ARGUMENT;
    if (deviceResult == nullptr) return (*b)->log.invalid("[Invalid Arg] - deviceResult was not set");
    if (!haveDesc) { snprintf(buf, sizeof buf, "[Invalid Arg] - %s was not set", descName); return (*b)->log.invalid(buf); }
    if (!haveOutput) return (*b)->log.invalid("[Invalid Arg] - neither outResult nor outInfo was set");
    return ommResult_SUCCESS;
}
ommResult check_source_formats(const Logger& log, const ommCpuBakeResultDesc* const* results, uint32_t count)
{
    for (uint32_t k = 0; k < count; ++k)
        if (!is_index_format(results[k]->indexFormat)) return log.invalid("[Invalid Arg] - a source's indexFormat is not an index format");
    return ommResult_SUCCESS;
}
ommResult check_source_arrays(const Logger& log, const ommCpuBakeResultDesc* const* results, uint32_t count)
{
    for (uint32_t k = 0; k < count; ++k)
        if (has_null_array(*results[k])) return log.invalid("[Invalid Arg] - a source has a null array with a non-zero count");
    return ommResult_SUCCESS;
}
// One call that derives a new device-resident result: the handle, and the skeleton around the operation's own stages (run).
struct DerivedResult {
    Baker& b; hipStream_t stream;
    const char *noun, *work;                          // in a message: the new result ("coarsened", "combined", "gathered"), the operation ("coarsening", "combine", "gather")
    DeviceResultOwner res;                            // stays null when the caller wants the info only
    uint32_t hist[2 * kRebuildHist];                  // array | index by (level, format - 1): the operation's last stage fills it
    DerivedResult(Baker& b_, hipStream_t stream_, const char* noun_, const char* work_) : b(b_), stream(stream_), noun(noun_), work(work_), res(b_.mem, stream_) { memset(hist, 0, sizeof hist); }
    ommResult failure(const char* format, const char* word) { char buf[160]; snprintf(buf, sizeof buf, format, word); return b.log.failure(buf); }
    ommResult failure(const char* format) { return failure(format, noun); }
    // scratch of the operation; false: it could not be had, and no_memory() is the answer
    bool acquire(PoolBlock& block, size_t bytes) { return block.acquire(b.devPool.get(), bytes); }
    ommResult no_memory() { return give_up(failure("[Failure] - out of device memory for the %s scratch", work)); }
    // after a failed launch: the scratch goes back only when nothing can still touch it
    ommResult failed() { (void)hipGetLastError(); (void)hipStreamSynchronize(stream); return give_up(failure("[Failure] - the %s kernels could not run", work)); }
    // The skeleton.  stages(): the operation on the baker's device, there is at least one primitive -- it acquires its scratch (acquire / no_memory),
    // runs its stages up to the counts of the tail (failed) and ends in emit().
    template <class Stages> ommResult run(ommxDeviceBakeResult* outResult, uint32_t numTris, ommIndexFormat indexFormat, Stages&& stages)
    {
        const ommResult made = outResult ? create(numTris, indexFormat) : ommResult_SUCCESS;
        if (made != ommResult_SUCCESS) return made;
        if (numTris) {
            if (!usable_device()) return give_up(b.log.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)"));
            const DeviceScope onBakersDevice(b.device.load());   // (a baker that has no device yet works on the caller's current one)
            const ommResult done = stages();
            if (done != ommResult_SUCCESS) return done;
        }
        finish(outResult);
        return ommResult_SUCCESS;
    }
    // judges the output's size; with a handle, allocates its arrays and has the operation's last stage fill them
    template <class Emit> ommResult emit(const RebuildCounts& n, Emit&& fill)
    {
        const ommResult sized = allocate(n);
        if (sized != ommResult_SUCCESS || !res) return sized;
        RebuildOutputs o; o.arrayData = res->R.arrayData; o.descs = res->R.descs; o.index = res->R.index; o.hist = hist;
        return fill(o) == hipSuccess ? ommResult_SUCCESS : failed();
    }
    ommResult create(uint32_t numTris, ommIndexFormat indexFormat)
    {
        if (!res.make()) return failure("[Failure] - the memory allocator returned null for the %s result");
        res->R.pool = b.devPool; res->R.numTris = numTris; res->R.indexFormat = indexFormat;
        return ommResult_SUCCESS;
    }
    ommResult give_up(ommResult code) { res.give_up(); return code; }
    // judges the output's size; with a handle, allocates its three arrays
    ommResult allocate(const RebuildCounts& n)
    {
        if (n.arrayBytes > 0xFFFFFFFFull) return give_up(failure("[Failure] - the %s arrayData would exceed what a 32-bit descriptor offset can express"));
        if (!res) return ommResult_SUCCESS;
        DeviceResult& R = res->R;
        R.numDescs = n.descCount; R.arrayDataSize = n.arrayBytes;
        if (n.descCount) { R.arrayData = (uint8_t*)R.dev_alloc((size_t)n.arrayBytes); R.descs = (ommCpuOpacityMicromapDesc*)R.dev_alloc(sizeof(ommCpuOpacityMicromapDesc) * (size_t)n.descCount); }
        R.index = R.dev_alloc((size_t)R.numTris * (R.indexFormat == ommIndexFormat_UINT_8 ? 1u : R.indexFormat == ommIndexFormat_UINT_16 ? 2u : 4u));
        if (!R.index || (n.descCount && (!R.arrayData || !R.descs))) return give_up(failure("[Failure] - out of device memory for the %s result"));
        return ommResult_SUCCESS;
    }
    // the histogram lists are built here, not by finish_device_result: a caller's source may hold both formats
    void finish(ommxDeviceBakeResult* outResult)
    {
        if (!res) return;
        uint32_t nAH = 0, nIH = 0;
        for (uint32_t l = 0; l < kRebuildLevels; ++l)
            for (uint32_t f = 0; f < 2; ++f) {
                const uint32_t ah = hist[2 * l + f], ih = hist[kRebuildHist + 2 * l + f];
                if (ah) res->arrayHist[nAH++] = ommCpuOpacityMicromapUsageCount{ ah, (uint16_t)l, (uint16_t)(f + 1) };
                if (ih) res->indexHist[nIH++] = ommCpuOpacityMicromapUsageCount{ ih, (uint16_t)l, (uint16_t)(f + 1) };
            }
        const DeviceResult& R = res->R;
        fill_result_desc(&res->desc, R.arrayData, R.arrayDataSize, R.descs, R.numDescs, R.index, R.numTris, R.indexFormat, res->arrayHist, nAH, res->indexHist, nIH);
        *outResult = (ommxDeviceBakeResult)res.release();
    }
};

// result of the serial host tail -> device-resident result (ommxBakeDevice / ommxShardedBakeRccl with the opt-in lossy reducers)
ommResult upload_host_tail(Baker& b, const HostTailResult& hres, ommIndexFormat ifmt, uint32_t T, int bits, hipStream_t stream, DeviceBakeResult* res)
{
    DeviceResult& R = res->R;
    R.pool = b.devPool; R.bits = bits; R.numTris = T; R.indexFormat = ifmt;
    const uint32_t E = (uint32_t)hres.descs.size();
    R.numDescs = E; R.arrayDataSize = E ? hres.arrayData.size() : 0;
    bool ok = true;
    if (E) {
        R.arrayData = (uint8_t*)R.dev_alloc(hres.arrayData.size()); R.descs = (ommCpuOpacityMicromapDesc*)R.dev_alloc(sizeof(ommCpuOpacityMicromapDesc) * (size_t)E);
        ok = R.arrayData && R.descs && HIP_OK(hipMemcpyAsync(R.arrayData, hres.arrayData.data(), hres.arrayData.size(), hipMemcpyHostToDevice, stream))
          && HIP_OK(hipMemcpyAsync(R.descs, hres.descs.data(), sizeof(ommCpuOpacityMicromapDesc) * (size_t)E, hipMemcpyHostToDevice, stream));
    }
    R.index = R.dev_alloc((size_t)(T ? T : 1) * 4);
    ok = ok && R.index && (!T || HIP_OK(hipMemcpyAsync(R.index, hres.index.data(), (size_t)T * 4, hipMemcpyHostToDevice, stream)));
    ok = ok && HIP_OK(hipStreamSynchronize(stream));
    if (!ok) return b.log.failure("[Failure] - could not materialise the bake result on the device");
    memcpy(res->arrayHist, hres.arrayHist.data(), sizeof(ommCpuOpacityMicromapUsageCount) * clamp_hist_count(hres.arrayHist.size()));
    memcpy(res->indexHist, hres.indexHist.data(), sizeof(ommCpuOpacityMicromapUsageCount) * clamp_hist_count(hres.indexHist.size()));
    fill_result_desc(&res->desc, R.arrayData, R.arrayDataSize, R.descs, E, R.index, T, ifmt, res->arrayHist, hres.arrayHist.size(), res->indexHist, hres.indexHist.size());
    return ommResult_SUCCESS;
}

// ommxBakeDevice: the per-triangle UV areas leave the bake's arena with the result -- one device-to-device copy of T floats, released with the result
bool keep_tri_areas(DeviceResult& R, const float* areaScratch, uint32_t T, hipStream_t stream)
{
    if (!T || !areaScratch) return true;
    R.triArea = (float*)R.dev_alloc(sizeof(float) * (size_t)T);
    return R.triArea && HIP_OK(hipMemcpyAsync(R.triArea, areaScratch, sizeof(float) * (size_t)T, hipMemcpyDeviceToDevice, stream)) && HIP_OK(hipStreamSynchronize(stream));
}

struct BakeSession { // device working set + streams of one bake in flight
    std::shared_ptr<ArenaPool> pool; std::unique_ptr<ArenaSet> set; DeviceArena* arena; DeviceArena* states; hipStream_t stream = nullptr, commStream = nullptr, placeStream = nullptr;
    explicit BakeSession(Baker& b) : pool(b.arenas), set(pool->acquire()) { arena = &set->tables; states = &set->states; }
    ~BakeSession() {
        // the set goes back to the pool only when nothing on the device can still touch it (the streams stay with the set)
        if (placeStream) (void)hipStreamSynchronize(placeStream);
        if (commStream) (void)hipStreamSynchronize(commStream);
        if (stream) (void)hipStreamSynchronize(stream);
        pool->release(std::move(set));
    }
    bool open() { if (!set->stream && hipStreamCreateWithFlags(&set->stream, hipStreamNonBlocking) != hipSuccess) return false; stream = set->stream; return true; }
    bool open_comm() { if (!set->commStream && hipStreamCreateWithFlags(&set->commStream, hipStreamNonBlocking) != hipSuccess) return false; commStream = set->commStream; return true; }
    // high priority: its (small) kernels are dispatched ahead of the next persistent classification launch instead of behind it
    bool open_place() {
        if (!set->placeStream) {
            int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (hipStreamCreateWithPriority(&set->placeStream, hipStreamNonBlocking, hi) != hipSuccess) return false;
        }
        placeStream = set->placeStream; return true;
    }
};

// largest vertex index of the caller's index buffer (3 M entries at the metric configuration: vectorised where the CPU has AVX2, 0.2 instead of 1.3 ms)
template <class T> inline uint32_t max_of(const T* p, size_t n) { uint32_t m = 0; for (size_t i = 0; i < n; ++i) m = p[i] > m ? p[i] : m; return m; }
__attribute__((target("avx2"))) uint32_t max_of_u32_avx2(const uint32_t* p, size_t n) { uint32_t m = 0; for (size_t i = 0; i < n; ++i) m = p[i] > m ? p[i] : m; return m; }
__attribute__((target("avx2"))) uint32_t max_of_u16_avx2(const uint16_t* p, size_t n) { uint32_t m = 0; for (size_t i = 0; i < n; ++i) m = p[i] > m ? p[i] : m; return m; }
uint32_t max_index(const void* idx, ommIndexFormat fmt, size_t n)
{
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (fmt == ommIndexFormat_UINT_8) return max_of((const uint8_t*)idx, n);
    if (fmt == ommIndexFormat_UINT_16) return avx2 ? max_of_u16_avx2((const uint16_t*)idx, n) : max_of((const uint16_t*)idx, n);
    return avx2 ? max_of_u32_avx2((const uint32_t*)idx, n) : max_of((const uint32_t*)idx, n);
}

ommResult bake_impl_multi(Baker& baker, const ommCpuBakeInputDesc& d, ommCpuBakeResult* out, uint32_t devices);   // (below, next to the sharded bake it is made of)
// Sizes of the device block that holds the codec stream of `arrayBytes` of arrayData: size word (256 B) | scan scratch | [unit codes | block counts] | the stream.
// (here, not with host_codec_layout in host_expand.h: the scratch size is the device code's to say, bake_kernels.h)
struct CodecBlockLayout { uint64_t padded = 0, cap = 0; HostCodecLayout L{}; size_t scratchBytes = 0; bool fits = false; };
CodecBlockLayout codec_block_layout(uint64_t arrayBytes)
{
    CodecBlockLayout B;
    B.padded = (arrayBytes + 255u) & ~255ull; B.L = host_codec_layout(B.padded);
    B.cap = codec_stream_cap(B.L, B.padded);
    B.scratchBytes = pad256(shard_codec_scratch_bytes(B.padded));
    B.fits = B.L.blocks < 0x7FFFFFFFull;
    return B;
}
constexpr uint64_t kCompressedMinBytes = 32ull << 20;   // smaller arrays cross the link as they are (0.6 ms at 57 GB/s)

// ---- result delivery of ommCpuBake (and of the multi-device bake made of the same parts): one owner per resource ----
// The device block of ONE codec stream (slots: carve_codec_block, host_expand.h): ommCpuBake's compressed result, a rank's contribution of the multi-device bake.
// Owns the pool block from reserve() until it is destroyed -- declared BEFORE the StreamDrain of the stream that compresses into it.
struct CodecBlock : CodecBlockLayout {
    PoolBlock block; CodecBlockCarve at = CodecBlockCarve(); uint64_t arrayBytes = 0;
    bool on = false;   // (ommCpuBake: the stream of the finished array has been queued)
    bool reserved() const { return block.p != nullptr; }
    bool has_codes() const { return at.unitCodes != nullptr; }   // the gather fills (has filled) the codes of the units and the raw counts of the blocks
    bool reserve(DevPool* pool, uint64_t bytes, bool withCodes) {
        static_cast<CodecBlockLayout&>(*this) = codec_block_layout(bytes); arrayBytes = bytes;
        if (!block.acquire(pool, carve_codec_block(0, bytes, scratchBytes, withCodes).bytes) || !fits) return false;
        at = carve_codec_block((uintptr_t)block.p, bytes, scratchBytes, withCodes);
        return true;
    }
    // in front of the gather that fills them: the units of the padding behind the array count as zeros, the counts start at zero
    bool prepare_codes(hipStream_t stream) {
        const uint64_t units = arrayBytes / 16u, paddedUnits = padded / 16u;
        bool ok = HIP_OK(hipMemsetAsync(at.blockRawCounts, 0, ((size_t)L.blocks + 1) * 4, stream));
        if (ok && paddedUnits > units) ok = HIP_OK(hipMemsetAsync(at.unitCodes + units, 0, (size_t)(paddedUnits - units), stream));
        if (!ok) { at.unitCodes = nullptr; at.blockRawCounts = nullptr; }
        return ok;
    }
    // the codec stream of dArray[0 .. padded) into at.stream (with the gather's codes the array is read for its raw units only)
    bool compress(const uint8_t* dArray, hipStream_t stream) const {
        return HIP_OK(has_codes() ? run_shard_compress_coded(dArray, padded, at.unitCodes, at.blockRawCounts, at.stream, cap, at.sizeWord, at.scratch, scratchBytes, stream)
                                  : run_shard_compress(dArray, padded, at.stream, cap, at.sizeWord, at.scratch, scratchBytes, stream));
    }
};
// A host BakeResult until release() hands it to the caller.  Let go of earlier -- an error, an exception -- it is destroyed only after the session's streams are
// idle (the comm stream, which may have been opened after the guard was made, then the bake's): nothing may still be copying into the result's arrays when they
// are freed.  Without a session (the multi-device bake) the caller's own StreamDrain stands behind the guard.
struct HostResultGuard {
    Baker& b; BakeResult* r; const BakeSession* drain;
    ~HostResultGuard() {
        if (!r) return;
        if (drain) { if (drain->commStream) (void)hipStreamSynchronize(drain->commStream); (void)hipStreamSynchronize(drain->stream); }
        b.mem.destroy(r);
    }
    BakeResult* release() { BakeResult* p = r; r = nullptr; return p; }
};
struct ActiveBake { std::atomic<uint32_t>& n; explicit ActiveBake(std::atomic<uint32_t>& c) : n(c) { n.fetch_add(1); } ~ActiveBake() { n.fetch_sub(1); } };   // Baker::activeBakes

// The host arrayData of an ommCpuBake result, and the block that is zeroed ahead for it.
// Zeroing ahead (round 6, compressed transfer).  The expansion of the result is bound by what twelve threads can store (1.27 GB in 3.6 ms), and a quarter of
// the metric configuration's 4-KiB codec blocks repeat state 0 = zeros.  While the device bakes the host is idle: the baker's helper threads zero an IDLE block
// of the result pool (what the previous bake left; never a fresh allocation, never a user allocator's memory) in pieces of 2 MiB, up to the size of the last
// compressed result; if the block then fits this bake's result it becomes the result, and the expansion leaves zero blocks of complete pieces alone.
// Owns that block and the helper threads' run on it: the threads are stopped before anybody else writes the block and before it is released, and the block
// is either made the result's array by get() or goes back to the pool (get(), the destructor) -- whatever happens: another transfer, a larger result, an error.
// The array that get() has placed belongs to the BakeResult: freed with it, on an error path by the HostResultGuard this object is declared BEHIND (after the
// streams are drained -- it is never freed while a copy can land in it).
struct ResultArray {
    Baker& b; BakeResult* res;
    uint64_t cap = 0; bool pinned = false;   // of res->arrayData
    bool fromPrefill = false;                // res->arrayData is the block zeroed ahead, and nothing but the zeroing has written into it
    std::shared_ptr<WorkerPool> workers; std::shared_ptr<HostPool> host; uint8_t* block = nullptr; size_t blockCap = 0; bool blockPinned = false, started = false;
    ZeroPlan plan{ 0, 0, 0 };   // (host_expand.h: the pieces, and the extent the expansion may trust -- a larger result's bytes beyond it are stale)
    std::unique_ptr<std::atomic<uint8_t>[]> done; std::atomic<bool> cancel{ false };
    ResultArray(Baker& baker, BakeResult* r) : b(baker), res(r) {}
    ~ResultArray() { stop(); if (block) host->release(block); }
    void stop() { if (started) { cancel.store(true); workers->wait(); started = false; } }   // (pieces not begun stay unmarked: the expansion writes them like any other)
    // takes an idle pool block of the last compressed result's size, if there is one, and starts zeroing it
    void zero_ahead(unsigned expandThreads) {
        const uint64_t last = b.lastCompressedArrayBytes.load();
        if (last < kCompressedMinBytes || (block = (uint8_t*)b.hostPool->acquire_idle((size_t)last, &blockCap, &blockPinned)) == nullptr) return;
        host = b.hostPool; workers = b.worker_pool(expandThreads);
        plan = zero_plan(blockCap, (size_t)last);
        done.reset(new (std::nothrow) std::atomic<uint8_t>[plan.pieces]);
        if (!done || ((uintptr_t)block & 4095u) != 0u) return;
        for (size_t j = 0; j < plan.pieces; ++j) done[j].store(0);
        if (b.knob(ommxBakerKnob_HelperAffinity) == 0) (void)workers->bind_near(block);
        started = workers->start((uint32_t)plan.pieces, [this](uint32_t j) {
            if (cancel.load(std::memory_order_relaxed)) return;
            size_t lo, hi; zero_piece_range(plan, j, &lo, &hi);
            fill_zero_nt(block, lo, hi);
            done[j].store(1, std::memory_order_release);
        });
    }
    // res->arrayData with room for `bytes`, from: the array it has if that is large enough | the block zeroed ahead | the baker's host pool | the allocator
    uint8_t* get(uint64_t bytes, bool* outPinned) {
        if (outPinned) *outPinned = false;
        if (res->arrayData && cap >= bytes) { if (outPinned) *outPinned = pinned; return (uint8_t*)res->arrayData; }
        if (!res->arrayData && block) {   // the block that was zeroed ahead, if it holds this result (its threads have stopped before anybody writes into it)
            stop();
            if (blockCap >= bytes) {
                res->arrayData = block; res->pool = host; pinned = blockPinned; cap = bytes; fromPrefill = true; block = nullptr;
                if (outPinned) *outPinned = pinned;
                return (uint8_t*)res->arrayData;
            }
            host->release(block); block = nullptr;
        }
        if (res->arrayData) { if (res->pool) { res->pool->release(res->arrayData); res->pool.reset(); } else b.mem.release(res->arrayData); res->arrayData = nullptr; cap = 0; }
        // (small results are pooled -- pinned -- only while this is the baker's one bake in flight: sixteen callers copying into pinned blocks at once take
        //  turns on the copy engines -- measured on configs[1]: 2 278 -> 1 190 bakes/s at 16 threads --, while one caller gains 0.28 ms per bake)
        if (b.mem.alloc == default_alloc && ((size_t)bytes >= HostPool::kMinBytes || (b.activeBakes.load() <= 1u && b.hostPool->wants((size_t)bytes)))) {
            res->arrayData = b.hostPool->acquire((size_t)bytes, &pinned);
            if (res->arrayData) res->pool = b.hostPool;
        }
        if (!res->arrayData) { res->arrayData = b.mem.allocate((size_t)bytes, 64); pinned = false; }
        cap = res->arrayData ? bytes : 0;
        if (outPinned) *outPinned = pinned;
        return (uint8_t*)res->arrayData;
    }
    // StreamOut::alloc: a block the streamed placement writes into is no longer only zeroed -- if the stream is discarded, the compressed transfer that follows
    // must write every byte
    static uint8_t* get_for_stream(void* self, uint64_t bytes, bool* outPinned) { ResultArray& a = *(ResultArray*)self; uint8_t* p = a.get(bytes, outPinned); a.fromPrefill = false; return p; }
    ZeroedPieces zeroed() const { return zeroed_pieces(plan, done.get()); }
    bool trust_zeroed() const { return fromPrefill && done; }   // the expansion may leave zeros inside zeroed() alone
};

// the caller's raw triangle data into its device block (raw_input_layout, bake_host.h); a null stream: blocking copies.  All null: no block / a copy failed
DeviceInputs upload_raw_inputs(const RawInputLayout& raw, const ommCpuBakeInputDesc& d, uint8_t* dRaw, hipStream_t stream)
{
    const auto put = [&](size_t at, const void* src, size_t bytes) {
        return !bytes || HIP_OK(stream ? hipMemcpyAsync(dRaw + at, src, bytes, hipMemcpyHostToDevice, stream) : hipMemcpy(dRaw + at, src, bytes, hipMemcpyHostToDevice));
    };
    if (!dRaw || !put(raw.offUv, d.texCoords, raw.uvBytes) || !put(raw.offIdx, d.indexBuffer, raw.idxBytes) || !put(raw.offLvl, d.subdivisionLevels, raw.lvlBytes))
        return DeviceInputs{ nullptr, nullptr, nullptr };
    return DeviceInputs{ dRaw + raw.offUv, dRaw + raw.offIdx, raw.lvlBytes ? dRaw + raw.offLvl : nullptr };
}
// descriptors, index buffer and triangle areas of a device result into the host result's arrays (8.6 MB at the metric configuration, into the caller's pageable
// arrays: each copy holds its thread until it is done)
bool copy_small_arrays(BakeResult* res, const ommCpuOpacityMicromapDesc* descs, const void* index, const float* triArea, uint32_t E, uint32_t T, size_t indexBytes, hipStream_t s)
{
    bool k = true;
    if (E) k = HIP_OK(hipMemcpyAsync(res->descs, descs, sizeof(ommCpuOpacityMicromapDesc) * (size_t)E, hipMemcpyDeviceToHost, s));
    if (k && T) k = HIP_OK(hipMemcpyAsync(res->index, index, indexBytes * T, hipMemcpyDeviceToHost, s));
    if (k && T) k = HIP_OK(hipMemcpyAsync(res->triArea, triArea, sizeof(float) * (size_t)T, hipMemcpyDeviceToHost, s));
    return k;
}
// With a compressed result the small arrays cross the link on the second stream WHILE the helper threads expand the array: that stream waits for the device
// result (an event behind everything on the bake's stream).  False: no second stream / no event -- the small arrays go in front of the wait, on the bake's stream.
bool defer_small_arrays(BakeSession& ses, EventList<1>& resultEvent)
{
    if (!ses.open_comm() || !resultEvent.create(1)) return false;
    return HIP_OK(hipEventRecord(resultEvent.ev[0], ses.stream)) && HIP_OK(hipStreamWaitEvent(ses.commStream, resultEvent.ev[0], 0));
}
// result of the serial host tail -> host result (ommCpuBake with the opt-in lossy reducers): the host twin of upload_host_tail; the triangle areas come from the device
ommResult host_result_from_tail(Baker& baker, const BakeSession& ses, const HostTailResult& hres, ommIndexFormat ifmt, uint32_t T, const float* dTriArea, BakeResult** out)
{
    HostResultGuard guard{ baker, baker.mem.make<BakeResult>(), &ses };
    BakeResult* const res = guard.r;
    if (!res) return ommResult_FAILURE;
    res->mem = baker.mem;
    const uint32_t E = (uint32_t)hres.descs.size();
    if (alloc_host_result(baker, res, E, hres.arrayData.size(), T) != ommResult_SUCCESS) return ommResult_FAILURE;
    if (T && (!HIP_OK(hipMemcpyAsync(res->triArea, dTriArea, sizeof(float) * (size_t)T, hipMemcpyDeviceToHost, ses.stream)) || !HIP_OK(hipStreamSynchronize(ses.stream))))
        return baker.log.failure("[Failure] - device to host transfer of the bake result failed");
    if (E) { memcpy(res->arrayData, hres.arrayData.data(), hres.arrayData.size()); memcpy(res->descs, hres.descs.data(), sizeof(ommCpuOpacityMicromapDesc) * (size_t)E); }
    memcpy(res->index, hres.index.data(), sizeof(int32_t) * (size_t)T);
    memcpy(res->arrayHist, hres.arrayHist.data(), sizeof(ommCpuOpacityMicromapUsageCount) * clamp_hist_count(hres.arrayHist.size()));
    memcpy(res->indexHist, hres.indexHist.data(), sizeof(ommCpuOpacityMicromapUsageCount) * clamp_hist_count(hres.indexHist.size()));
    fill_result_desc(&res->desc, res->arrayData, hres.arrayData.size(), res->descs, E, res->index, T, ifmt, res->arrayHist, hres.arrayHist.size(), res->indexHist, hres.indexHist.size());
    *out = guard.release();
    return ommResult_SUCCESS;
}

// Which slices of a codec stream are on the host.  A task whose slice is not there yet polls the slices' events in order -- whichever thread gets there first
// moves the `arrived` mark -- so the threads never meet at a barrier between slices (12 runs, one per slice, cost ~0.5 ms of joins and idle tails).
struct SliceArrivals {
    const hipEvent_t* evs; std::atomic<uint32_t> arrived{ 0 }; std::atomic<bool> failed{ false };
    // false: a slice's event failed (here or on another thread).  A few polls back to back -- a slice is ~0.1 ms of PCIe time --, then short sleeps: up to twelve
    // threads spinning on hipEventQuery burn the process's CPU quota for nothing, and a throttled process expands slower
    bool wait_for(uint32_t need) {
        uint32_t polls = 0;
        for (uint32_t a; (a = arrived.load(std::memory_order_acquire)) <= need && !failed.load(std::memory_order_relaxed); ) {
            const hipError_t q = hipEventQuery(evs[a]);
            if (q == hipSuccess) { uint32_t expect = a; arrived.compare_exchange_strong(expect, a + 1u, std::memory_order_acq_rel); polls = 0; }
            else if (q != hipErrorNotReady) { (void)hipGetLastError(); failed.store(true); }
            else { (void)hipGetLastError(); if (++polls < 32u) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(20)); }
        }
        return !failed.load(std::memory_order_relaxed);
    }
};
// ommCpuBake's compressed delivery, once the bake's stream is idle and the head of the codec stream (its length, the per-block offsets of the raw units) is in
// `head`: the rest of the stream lands in the working set's pinned block slice by slice (plan_codec_slices, host_expand.h) and the helper threads expand slice k
// into res->arrayData while slice k + 1 is on the link; with `deferSmall` one of the tasks issues the small arrays on the second stream.  Noise-like states (the
// stream would not be below half of the array): the array itself crosses the link.  Returns whether the result is complete; fills the transfer's timings.
bool deliver_compressed(Baker& baker, BakeSession& ses, const CodecBlock& codec, const std::vector<uint8_t>& head, const DeviceResult& R, BakeResult* res, uint32_t T,
                        const ResultArray& array, bool deferSmall, unsigned expandThreads, double c0, ommxBakeTimings& tm)
{
    constexpr uint32_t kSlices = CodecSlicePlan::kSlices;
    hipStream_t stream = ses.stream;
    const uint32_t E = R.numDescs; const size_t outIdx = index_bytes(R.indexFormat);
    const double c1 = now_ms();
    bool ok = true;
    uint64_t streamBytes = 0; memcpy(&streamBytes, head.data(), 8);   // (shard_codec_finish: the length the stream has, or would have had)
    const bool fits = streamBytes <= codec.cap && streamBytes >= codec.L.offRaw && ses.set->pinned.reserve((size_t)streamBytes + 4096);   // (pinned staging of the stream's size)
    if (!fits) {
        ok = HIP_OK(hipMemcpyAsync(res->arrayData, R.arrayData, (size_t)R.arrayDataSize, hipMemcpyDeviceToHost, stream))
          && (!deferSmall || copy_small_arrays(res, R.descs, R.index, R.triAreaScratch, E, T, outIdx, stream)) && HIP_OK(hipStreamSynchronize(stream));
        tm.resultTransfer = ommxResultTransfer_Plain;
    } else {
        uint8_t* hStream = ses.set->pinned.base; const uint8_t* dComp = codec.at.stream;
        memcpy(hStream, head.data(), head.size());
        const HostCodecLayout L = codec.L;
        const CodecSlicePlan plan = plan_codec_slices(L, (const uint32_t*)(hStream + L.offOfs), streamBytes);
        EventList<kSlices> evs;   // one per slice: on the host
        ok = evs.create(kSlices) && plan.ok;
        for (uint32_t k = 0; ok && k < kSlices; ++k) {
            const CodecSlicePlan::Slice& s = plan.slice[k];
            if (s.c1 > s.c0) ok = HIP_OK(hipMemcpyAsync(hStream + s.c0, dComp + s.c0, (size_t)(s.c1 - s.c0), hipMemcpyDeviceToHost, stream));
            if (ok && s.r1 > s.r0) ok = HIP_OK(hipMemcpyAsync(hStream + s.r0, dComp + s.r0, (size_t)(s.r1 - s.r0), hipMemcpyDeviceToHost, stream));
            ok = ok && HIP_OK(hipEventRecord(evs.ev[k], stream));
        }
        if (ok) {
            const std::shared_ptr<WorkerPool> poolRef = baker.worker_pool(expandThreads); WorkerPool& pool = *poolRef;
            // the helper threads next to the memory they fill: on the two-socket host of the GPU box a process whose threads happened to run on the other socket
            // expanded at half the rate (five process pairs on one lease: 17.0 - 25.0 ms per call without, 17.0 - 19.8 with the binding)
            if (baker.knob(ommxBakerKnob_HelperAffinity) == 0) (void)pool.bind_near(res->arrayData);
            uint8_t* dst = (uint8_t*)res->arrayData; const uint64_t dstBytes = R.arrayDataSize;
            SliceArrivals arrivals{ evs.ev };
            // (the result array is the block that was zeroed ahead: blocks and lines of zeros inside its zeroed extent, in complete pieces, are left alone)
            std::atomic<uint64_t> skippedBytes{ 0 };
            const ZeroedPieces zeroedPieces = array.zeroed();
            const ZeroedPieces* const zeroedPtr = array.trust_zeroed() ? &zeroedPieces : nullptr;
            ok = HIP_OK(hipEventSynchronize(evs.ev[0]));
            if (ok) arrivals.arrived.store(1);
            const int dev = baker.bind_device();
            const uint32_t extra = deferSmall ? 1u : 0u;   // task 0: the small arrays, on the second stream
            // ONE run over all tasks (2 MiB of the array each, in slice order)
            if (ok) pool.run((uint32_t)codec_task_count(L) + extra, [&](uint32_t t0) {
                if (extra && t0 == 0u) {
                    const DeviceScope onDev(dev);
                    if (!copy_small_arrays(res, R.descs, R.index, R.triAreaScratch, E, T, outIdx, ses.commStream) || !HIP_OK(hipStreamSynchronize(ses.commStream))) arrivals.failed.store(true);
                    return;
                }
                uint64_t s0, s1; codec_task_range(L, t0 - extra, &s0, &s1);
                if (!arrivals.wait_for(last_slice_needed(plan, s1))) return;
                uint64_t skippedHere = 0;
                codec_expand_blocks(dst, dstBytes, hStream, L, s0, s1, zeroedPtr, &skippedHere);
                if (skippedHere) skippedBytes.fetch_add(skippedHere, std::memory_order_relaxed);
            });
            ok = ok && !arrivals.failed.load();
            tm.expandThreads = pool.workers() + 1u;
            tm.expandSkippedBytes = skippedBytes.load(); tm.prefilledBytes = zeroedPtr ? zeroed_bytes(zeroedPieces) : 0;
        }
        if (!ok) (void)hipStreamSynchronize(stream);   // (nothing may still be landing in the pinned block when the session hands it back)
        tm.resultTransfer = ommxResultTransfer_Compressed; tm.compressedBytes = streamBytes;
        if (ok) baker.lastCompressedArrayBytes.store(R.arrayDataSize);   // (what the next bake of this baker zeroes ahead)
    }
    tm.compressMs = (float)(c1 - c0); tm.expandMs = (float)(now_ms() - c1);
    return ok;
}

// ommCpuBake: host arrays in, host arrays out.
// What is let go of in which order (whichever way the function is left) is the reverse of the order of the named objects below:
//   the result event (after the last wait on it) -> StreamOut (its DMA copies have landed) -> ResultArray (zeroing stopped, then its block back to the pool)
//   -> HostResultGuard (comm stream, then the bake's stream drained, then an undelivered result destroyed) -> StreamDrain (the bake's stream idle)
//   -> CodecBlock, DeviceResult, the raw upload (pooled device blocks go back) -> EventTimer -> BakeSession (working set back to its pool).
// Top to bottom: fences | session | upload | host-tail bakes leave early | choice of the transfer | zeroing ahead | bake_core | compress | allocate | deliver
// (plain, the rest of a streamed result, or compressed) | descriptor and timings.
ommResult bake_impl(Baker& baker, const ommCpuBakeInputDesc& d, ommCpuBakeResult* out)
{
    const Logger& L = baker.log;
    const double t0 = now_ms();
    const ActiveBake activeGuard(baker.activeBakes);
    const ommResult fr = scope_fences(baker, d, true);
    if (fr != ommResult_SUCCESS) return fr;
    const uint32_t T = d.indexCount / 3u;
    // several devices behind the one call (ommxBakerKnob_Devices): the work items are shared out, every device hands its own blocks to the host
    // (not where blocks cannot travel in their packed form -- the lossy reducers, bit 9 with the 2-state format -- and not with per-triangle formats: one device)
    if (const uint64_t nd = baker.knob(ommxBakerKnob_Devices))
        if (nd >= 2 && !wants_host_tail(d) && !d.formats && !no_fine_two_state(d)) return bake_impl_multi(baker, d, out, (uint32_t)nd);
    const DeviceScope onBakersDevice(baker.bind_device());
    BakeSession ses(baker);
    if (!ses.open()) return L.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)");
    hipStream_t stream = ses.stream;

    // ---- upload the caller's triangle data (the C ABI gives no vertex count: it is max(index)+1, as serialize_impl.cpp:60-79) ----
    const RawInputLayout raw = raw_input_layout(d, T, max_index(d.indexBuffer, d.indexFormat, 3ull * T));
    const PoolBlock dRaw(baker.devPool.get(), raw.total);
    if (!dRaw.p) return L.failure("[Failure] - out of device memory for the triangle data");
    EventTimer et(stream);
    const int u0 = et.mark();
    const DeviceInputs din = upload_raw_inputs(raw, d, dRaw.bytes(), stream);
    if (!din.texCoords) return L.failure("[Failure] - host to device transfer failed");
    const int u1 = et.mark();

    DeviceResult R; ommxBakeTimings tm; memset(&tm, 0, sizeof tm);
    CodecBlock codec;   // (compressed transfer: the device block of the codec stream)
    const StreamDrain idleBeforeBlocksGoBack{ stream };
    if (wants_host_tail(d)) {
        // near-duplicate merge / size budget: device classification, then the reference's serial tail on the host (host_tail.cpp)
        HostTailRequest ht;
        const ommResult hr = bake_core(baker, d, din, ses.arena, ses.states, stream, et, R, tm, nullptr, &ht);
        if (hr != ommResult_SUCCESS) return hr;
        HostTailResult hres; ommIndexFormat ifmt = ommIndexFormat_UINT_32;
        if (run_host_tail_for(d, T, ht.items, hres, ifmt) != ommResult_SUCCESS) return ommResult_FAILURE;
        BakeResult* tailRes = nullptr;
        const ommResult rr = host_result_from_tail(baker, ses, hres, ifmt, T, R.triAreaScratch, &tailRes);
        if (rr != ommResult_SUCCESS) return rr;
        tm.totalMs = (float)(now_ms() - t0);
        store_timings(baker, tm);
        *out = (ommCpuBakeResult)tailRes;
        return ommResult_SUCCESS;
    }
    // the finished blocks travel to their final place in the result array while the classification is still running (StreamOut): the array is allocated
    // when the first block is about to leave, from an upper bound of its size (every active work item a block)
    HostResultGuard resGuard{ baker, baker.mem.make<BakeResult>(), &ses };
    BakeResult* const res = resGuard.r;
    if (!res) return ommResult_FAILURE;
    res->mem = baker.mem;
    ResultArray array(baker, res);
    StreamOut so; so.set = ses.set.get(); so.allocUser = &array; so.alloc = &ResultArray::get_for_stream;
    if (const uint64_t k = baker.knob(ommxBakerKnob_StreamChunks)) { so.chunksWanted = (uint32_t)k; so.forced = true; }
    // How a large arrayData reaches the caller (ommxBakerKnob_ResultTransfer).  COMPRESSED (round 5): the bake finishes on the device, the array crosses PCIe as
    // a codec stream (tail_kernels.hip: 6 % of its bytes at the metric configuration) and host threads expand it into the caller's array -- 190 - 250 GB/s with
    // 8 - 16 threads on the GPU box (profiles/r05_host_fill_rates.txt) against the 57 GB/s of the link.  It needs the caller's permission to use threads
    // (ommCpuBakeFlags_EnableInternalThreads, omm.h:303) and CPUs to run them on (below six, the STREAMED form -- blocks placed and copied by the DMA engine
    // while the classification runs -- is the faster one: one thread expands 30 GB/s).
    const uint64_t transferKnob = baker.knob(ommxBakerKnob_ResultTransfer);
    const unsigned expandThreads = expand_thread_count(baker);
    const bool wantCompressed = !so.forced && (transferKnob == ommxResultTransfer_Compressed ||
                                               (transferKnob == ommxResultTransfer_Auto && ((uint32_t)d.bakeFlags & (uint32_t)ommCpuBakeFlags_EnableInternalThreads) != 0 && effective_cpus() >= 6u));
    // (automatic choice with threads: both transfers are on offer, bake_core prices them once it knows the size of the bake -- a classification of 100 ms hides the
    //  whole copy of a streamed result, configs[4]; a short one is better off with the compressed transfer behind it, the metric configuration)
    so.compressedAvailable = wantCompressed && transferKnob == ommxResultTransfer_Auto;
    const bool canStream = (!wantCompressed || so.compressedAvailable) && transferKnob != ommxResultTransfer_Plain && ses.open_comm() && ses.open_place();
    so.copyStream = ses.commStream; so.placeStream = ses.placeStream; so.device = baker.bind_device();
    // (asked by bake_core right before the gather: from 32 MiB, every OMM a multiple of 16 bytes -- the gather then leaves the codec's codes next to the array)
    if (wantCompressed) R.gatherCodes = [&](uint64_t bytes, uint8_t** unitCodes, uint32_t** blockRawCounts) {
        const bool k = bytes >= kCompressedMinBytes && (bytes & 15u) == 0 && codec.reserve(baker.devPool.get(), bytes, true) && codec.prepare_codes(stream);
        *unitCodes = k ? codec.at.unitCodes : nullptr; *blockRawCounts = k ? codec.at.blockRawCounts : nullptr; return k; };
    // zeroing ahead: only with the default allocator, the compressed transfer on offer, helper threads, and an idle pool block of the last compressed result's size
    if (wantCompressed && baker.mem.alloc == default_alloc && baker.knob(ommxBakerKnob_RetainMemory) == 0 && baker.knob(ommxBakerKnob_ZeroAhead) == 0) array.zero_ahead(expandThreads);
    const ommResult br = bake_core(baker, d, din, ses.arena, ses.states, stream, et, R, tm, nullptr, nullptr, canStream ? &so : nullptr);
    R.gatherCodes = nullptr;
    if (br != ommResult_SUCCESS) return br;

    // ---- copy the (rest of the) result out through the user's allocator ----
    const int d0 = et.mark();
    const uint32_t E = R.numDescs;
    // ---- compressed result: codec stream of the finished array (device), one copy of the stream, expansion by the baker's helper threads ----
    std::vector<uint8_t> codecHead;   // header + offsets of the codec stream (1 MB per GB of arrayData)
    const double c0 = now_ms();
    if (E && wantCompressed && !so.used && R.arrayDataSize >= kCompressedMinBytes) {
        // (the device array was taken from the result pool, whose blocks are multiples of 4096 bytes: the codec may read the padding, the host never writes it)
        if (codec.has_codes() || (!codec.reserved() && codec.reserve(baker.devPool.get(), R.arrayDataSize, false))) codec.on = codec.compress(R.arrayData, stream);
        (void)hipGetLastError();
    }
    bool ok = true;
    if (E) {
        ok = array.get(R.arrayDataSize, nullptr) != nullptr;   // (a streamed bake has it already; every other path asks for the exact size)
        res->descs = (ommCpuOpacityMicromapDesc*)baker.mem.allocate(sizeof(ommCpuOpacityMicromapDesc) * (size_t)E, 16);
        ok = ok && res->descs;
        if (codec.on) {   // the stream's header (its length) and the per-block offsets of the raw units: the first piece of the stream, needed before the others can be cut
            codecHead.resize((size_t)codec.L.offCodes);
            ok = ok && HIP_OK(hipMemcpyAsync(codecHead.data(), codec.at.stream, (size_t)codec.L.offCodes, hipMemcpyDeviceToHost, stream));
        } else if (!so.used) ok = ok && HIP_OK(hipMemcpyAsync(res->arrayData, R.arrayData, (size_t)R.arrayDataSize, hipMemcpyDeviceToHost, stream));
    }
    res->index = (int32_t*)baker.mem.allocate(sizeof(int32_t) * (size_t)(T ? T : 1), 16);
    res->triArea = (float*)baker.mem.allocate(sizeof(float) * (size_t)(T ? T : 1), 16);
    ok = ok && res->index != nullptr && res->triArea != nullptr;
    const size_t outIdx = index_bytes(R.indexFormat);
    // the small arrays: behind the expansion's back on the second stream with a compressed result (defer_small_arrays), otherwise here, in front of the wait
    EventList<1> resultEvent;   // the device result is complete (everything in front of it on the bake's stream)
    const bool deferSmall = ok && codec.on && defer_small_arrays(ses, resultEvent);
    if (ok && !deferSmall) ok = copy_small_arrays(res, R.descs, R.index, R.triAreaScratch, E, T, outIdx, stream);
    const int d1 = et.mark();
    ok = ok && HIP_OK(hipStreamSynchronize(stream));
    if (so.chunks) { ok = so.finish() && ok; if (so.used) tm.streamTailMs = (float)(so.lastByteMs - so.classifyEndMs); }   // (the last streamed bytes arrive while the small arrays above are read back)
    if (ok && codec.on) ok = deliver_compressed(baker, ses, codec, codecHead, R, res, T, array, deferSmall, expandThreads, c0, tm);
    else tm.resultTransfer = so.used ? ommxResultTransfer_Streamed : ommxResultTransfer_Plain;
    if (!ok) { return L.failure("[Failure] - device to host transfer of the bake result failed"); }

    // histograms: format {2-state, 4-state} x level ascending, non-zero entries only (:1833-1850); one global format here
    if (alloc_host_result(baker, res, E, (size_t)R.arrayDataSize, T) != ommResult_SUCCESS) return ommResult_FAILURE;   // (the lists: everything else is in place)
    uint32_t nAH = 0, nIH = 0;
    compact_histograms(R.hist, R.bits, res->arrayHist, res->indexHist, &nAH, &nIH);
    fill_result_desc(&res->desc, res->arrayData, R.arrayDataSize, res->descs, E, res->index, T, R.indexFormat, res->arrayHist, nAH, res->indexHist, nIH);
    tm.uploadMs = et.ms(u0, u1); tm.downloadMs = et.ms(d0, d1); tm.totalMs = (float)(now_ms() - t0);
    store_timings(baker, tm);
    *out = (ommCpuBakeResult)resGuard.release();   // (handed over: the guard lets go)
    return ommResult_SUCCESS;
}

} // namespace

// ================================================================================================
// C ABI
// ================================================================================================
OMM_MI355X_API ommLibraryDesc ommGetLibraryDesc(void)
{
    ommLibraryDesc d = { OMM_VERSION_MAJOR, OMM_VERSION_MINOR, OMM_VERSION_BUILD };
    return d;
}

OMM_MI355X_API ommResult ommCreateBaker(const ommBakerCreationDesc* desc, ommBaker* outBaker)
{
    if (desc == nullptr) return ommResult_INVALID_ARGUMENT;
    if (desc->type != ommBakerType_CPU && desc->type != ommBakerType_GPU) return ommResult_INVALID_ARGUMENT;
    Allocator mem;
    if (desc->memoryAllocatorInterface.allocate != nullptr) {
        mem.alloc = desc->memoryAllocatorInterface.allocate; mem.realloc_ = desc->memoryAllocatorInterface.reallocate;
        mem.free_ = desc->memoryAllocatorInterface.free; mem.user = desc->memoryAllocatorInterface.userArg;
    }
    // ommBakerType_GPU bakers are creatable and destroyable like in the SDK (support/tests/test_basic.cpp:46-51); every ommGpu* entry
    // point answers NOT_IMPLEMENTED and the ommCpu* ones reject them ("Baker was not created as the right type")
    return guarded(nullptr, [&] {
        Baker* b = mem.make<Baker>();
        if (!b) return ommResult_FAILURE;
        b->mem = mem; b->log.iface = desc->messageInterface; b->type = desc->type;
        *outBaker = (ommBaker)((uintptr_t)b | (desc->type == ommBakerType_CPU ? kCpuBaker : kGpuBaker));
        return ommResult_SUCCESS;
    });
}

OMM_MI355X_API ommResult ommDestroyBaker(ommBaker baker)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    const uintptr_t t = tag_of(baker);
    if (t != kCpuBaker && t != kGpuBaker) return ommResult_FAILURE;
    Baker* b = untag<Baker>(baker);
    const Allocator mem = b->mem;
    mem.destroy(b);
    return ommResult_SUCCESS;
}

namespace {
// ---- texture creation: what ommCpuCreateTexture (texels from host memory) and ommxCreateTextureDevice (a channel of an image in device memory) share ----
// texture_impl.cpp:44-65
template <class Mip, class DataOf>
ommResult check_texture_mips(const Logger& L, uint32_t mipCount, bool formatSet, const Mip* mips, DataOf dataOf)
{
    if (mipCount == 0) return L.invalid("[Invalid Arg] - mipCount must be non-zero");
    if (!formatSet) return L.invalid("[Invalid Arg] - format is not set");
    for (uint32_t i = 0; i < mipCount; ++i) {
        if (!dataOf(mips[i])) return L.invalid("[Invalid Arg] - mips.textureData is not set");
        if (mips[i].width == 0) return L.invalid("[Invalid Arg] - mips.width must be non-zero");
        if (mips[i].height == 0) return L.invalid("[Invalid Arg] - mips.height must be non-zero");
        if (mips[i].width > 65536) return L.invalid("[Invalid Arg] - mips.width must be less than kMaxDim.x (65536)");
        if (mips[i].height > 65536) return L.invalid("[Invalid Arg] - mips.height must be less than kMaxDim.y (65536)");
    }
    if (mipCount > (uint32_t)kMaxMips) return L.invalid("[Invalid Arg] - more than 17 mips");
    return ommResult_SUCCESS;
}

// The Texture under construction: its mips' device memory, the summed-area tables and their pooled scratch, and the one way out.  The caller fills the
// texels of each mip between add_mip and build_sat, on the stream it hands to build_sat, and synchronises that stream before finish.
struct TextureBuild {
    Baker* b; Texture* t; bool ok = true; std::vector<void*> satScratch;
    TextureBuild(Baker* baker, ommCpuTextureFormat format, ommCpuTextureFlags flags, float alphaCutoff) : b(baker), t(baker->mem.make<Texture>()) {
        if (!t) return;
        t->mem = b->mem; t->log = &b->log; t->format = format; t->flags = flags; t->alphaCutoff = alphaCutoff; t->device = b->bind_device(); t->owner = b;
    }
    size_t texel_bytes() const { return t->format == ommCpuTextureFormat_FP32 ? 4 : 1; }
    bool enableSAT() const { return t->alphaCutoff >= 0; } // texture_impl.cpp:91
    // (the mip is recorded whether or not its memory could be had: ~Texture frees what exists)
    TexMip& add_mip(uint32_t w, uint32_t h) {
        TexMip m; m.w = (int)w; m.h = (int)h;
        ok = ok && HIP_OK(hipMalloc(&m.texels, texel_bytes() * (size_t)m.w * (size_t)m.h));
        t->mips.push_back(m);
        return t->mips.back();
    }
    void build_sat(TexMip& m, hipStream_t stream) {
        if (!ok || !enableSAT()) return;
        ok = HIP_OK(hipMalloc((void**)&m.sat, sizeof(uint32_t) * (size_t)m.w * (size_t)m.h));
        if (!ok) return;   // (the pooled scratch block goes back after the caller's synchronisation, in finish)
        uint32_t* scratch = (uint32_t*)b->devPool->acquire(sat_scratch_bytes(m.w, m.h));
        ok = scratch != nullptr;
        if (ok) { satScratch.push_back(scratch); launch_sat_build(m.texels, t->format == ommCpuTextureFormat_FP32, m.sat, scratch, m.w, m.h, t->alphaCutoff, stream); ok = HIP_OK(hipGetLastError()); }
    }
    ommResult finish(bool synchronised, ommCpuTexture* outTexture) {
        ok = ok && synchronised;
        for (void* p : satScratch) b->devPool->release(p);
        if (!ok) { (void)hipGetLastError(); b->mem.destroy(t); return b->log.failure("[Failure] - could not create the texture on the HIP device (no CPU fallback)"); }
        *outTexture = (ommCpuTexture)((uintptr_t)t | kTexture);
        return ommResult_SUCCESS;
    }
};

ommResult create_texture_impl(Baker* b, const ommCpuTextureDesc* desc, ommCpuTexture* outTexture)
{
    const Logger& L = b->log;
    const DeviceScope onBakersDevice(b->bind_device());
    const ommResult checked = check_texture_mips(L, desc->mipCount, desc->format != ommCpuTextureFormat_MAX_NUM, desc->mips, [](const ommCpuTextureMipDesc& m) { return m.textureData; });
    if (checked != ommResult_SUCCESS) return checked;
    TextureBuild tb(b, desc->format, desc->flags, desc->alphaCutoff);
    if (!tb.t) return ommResult_FAILURE;
    const bool linear = ((uint32_t)desc->flags & (uint32_t)ommCpuTextureFlags_DisableZOrder) != 0;
    const size_t px = tb.texel_bytes();
    std::vector<uint8_t> staging;
    for (uint32_t mi = 0; mi < desc->mipCount && tb.ok; ++mi) {
        const ommCpuTextureMipDesc& md = desc->mips[mi];
        TexMip& m = tb.add_mip(md.width, md.height);
        const size_t rowBytes = px * (size_t)m.w, bytes = rowBytes * (size_t)m.h;
        // rowPitch is in bytes for DisableZOrder textures and in texels otherwise (texture_impl.cpp:141-142,169,179)
        const size_t pitch = linear ? (md.rowPitch == 0 ? rowBytes : (size_t)md.rowPitch) : px * (md.rowPitch == 0 ? (size_t)md.width : (size_t)md.rowPitch);
        const uint8_t* src = (const uint8_t*)md.textureData;
        if (pitch != rowBytes) {
            staging.resize(bytes);
            for (int j = 0; j < m.h; ++j) memcpy(staging.data() + rowBytes * (size_t)j, src + pitch * (size_t)j, rowBytes);
            src = staging.data();
        }
        tb.ok = tb.ok && HIP_OK(hipMemcpy(m.texels, src, bytes, hipMemcpyHostToDevice));
        tb.build_sat(m, nullptr);   // (null stream)
    }
    return tb.finish(HIP_OK(hipDeviceSynchronize()), outTexture);
}

// memory a kernel of device `dev` may read: device memory of that device, managed memory, pinned host memory.  Anything the runtime does not know
// (pageable host memory, a stale pointer) or that lives on another device must never reach a launch.
bool device_readable(const void* p, int dev)
{
    hipPointerAttribute_t a; memset(&a, 0, sizeof a);
    if (!HIP_OK(hipPointerGetAttributes(&a, p))) { (void)hipGetLastError(); return false; }
    if (a.type == hipMemoryTypeDevice) return a.device == dev;
    return a.type == hipMemoryTypeHost || a.type == hipMemoryTypeManaged;
}

ommResult create_texture_device_impl(Baker* b, const ommxDeviceTextureDesc* desc, hipStream_t stream, ommCpuTexture* outTexture)
{
    const Logger& L = b->log;
    // ---- everything that can be judged without a device ----
    if (desc->mipCount != 0 && desc->mips == nullptr) return L.invalid("[Invalid Arg] - mips is not set");
    const ommResult checked = check_texture_mips(L, desc->mipCount, (unsigned)desc->channelFormat < (unsigned)ommxTexelFormat_MAX_NUM, desc->mips, [](const ommxDeviceTextureMipDesc& m) { return m.deviceData; });
    if (checked != ommResult_SUCCESS) return checked;
    const int gatherFormat = desc->channelFormat == ommxTexelFormat_UNORM8 ? kTexGatherUnorm8 : desc->channelFormat == ommxTexelFormat_FP16 ? kTexGatherFp16 : kTexGatherFp32;
    const uint64_t cb = tex_gather_channel_bytes(gatherFormat);
    const uint64_t stride = desc->pixelStrideInBytes ? (uint64_t)desc->pixelStrideInBytes : cb, off = desc->channelOffsetInBytes;
    if (stride < cb) return L.invalid("[Invalid Arg] - pixelStrideInBytes is smaller than one channel of channelFormat");
    if (off + cb > stride) return L.invalid("[Invalid Arg] - channelOffsetInBytes + the size of the channel exceeds pixelStrideInBytes");
    if (stride % cb != 0 || off % cb != 0) return L.invalid("[Invalid Arg] - pixelStrideInBytes and channelOffsetInBytes must be multiples of the size of the channel");
    for (uint32_t i = 0; i < desc->mipCount; ++i) {
        const ommxDeviceTextureMipDesc& md = desc->mips[i];
        if (md.rowPitchInBytes != 0 && (uint64_t)md.rowPitchInBytes < (uint64_t)md.width * stride) return L.invalid("[Invalid Arg] - mips.rowPitchInBytes is smaller than width * pixelStrideInBytes");
        if ((uint64_t)md.rowPitchInBytes % cb != 0 || (uintptr_t)md.deviceData % cb != 0) return L.invalid("[Invalid Arg] - mips.rowPitchInBytes and mips.deviceData must be multiples of the size of the channel");
    }
    // ---- the device ----
    const int dev = b->bind_device();
    int deviceCount = 0;
    if (dev < 0 || !HIP_OK(hipGetDeviceCount(&deviceCount)) || deviceCount < 1) { (void)hipGetLastError(); return L.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)"); }
    const DeviceScope onBakersDevice(dev);
    for (uint32_t i = 0; i < desc->mipCount; ++i) {   // first and last byte of every mip, before any launch
        const ommxDeviceTextureMipDesc& md = desc->mips[i];
        const uint64_t pitch = md.rowPitchInBytes ? (uint64_t)md.rowPitchInBytes : (uint64_t)md.width * stride;
        const uint8_t* first = (const uint8_t*)md.deviceData;
        if (!device_readable(first, dev) || !device_readable(first + (uint64_t)(md.height - 1) * pitch + (uint64_t)md.width * stride - 1, dev))
            return L.invalid("[Invalid Arg] - mips.deviceData is not memory the baker's device can read (device memory of that device, managed or pinned host memory)");
    }
    TextureBuild tb(b, desc->channelFormat == ommxTexelFormat_UNORM8 ? ommCpuTextureFormat_UNORM8 : ommCpuTextureFormat_FP32, desc->flags, desc->alphaCutoff);
    if (!tb.t) return ommResult_FAILURE;
    for (uint32_t mi = 0; mi < desc->mipCount && tb.ok; ++mi) {
        const ommxDeviceTextureMipDesc& md = desc->mips[mi];
        const uint64_t pitch = md.rowPitchInBytes ? (uint64_t)md.rowPitchInBytes : (uint64_t)md.width * stride;
        TexMip& m = tb.add_mip(md.width, md.height);
        if (tb.ok) { (void)launch_texture_gather(md.deviceData, (size_t)pitch, (uint32_t)stride, (uint32_t)off, gatherFormat, m.texels, m.w, m.h, stream); tb.ok = HIP_OK(hipGetLastError()); }
        tb.build_sat(m, stream);
    }
    return tb.finish(HIP_OK(hipStreamSynchronize(stream)), outTexture);
}

// What ommxCreateTextureBC and ommxCreateTextureBC7 share behind their format checks: the pitch (and, on the device entry, alignment) rules, the device,
// and the one loop over the mips.  fromDevice: the blocks are read in place on `stream`; otherwise they are host memory, uploaded with tight rows into pooled
// scratch (hipMalloc blocks: 256-byte aligned) and decoded on the null stream (`stream` is null then).  decode(blocks, pitch, mip, stream) launches the kernel.
struct BlockSource {
    ommCpuTextureFlags flags; const ommxBlockTextureMipDesc* mips; uint32_t mipCount; float alphaCutoff;
    uint64_t blockBytes;          // 8 or 16
    uint64_t align;               // device entry: data and a non-zero pitch are multiples of this (8 or 16: the size of the kernel's one load per block)
    ommCpuTextureFormat format;   // of the texture made
};
template <class Decode>
ommResult create_texture_blocks_impl(Baker* b, const BlockSource& s, bool fromDevice, hipStream_t stream, Decode decode, ommCpuTexture* outTexture)
{
    const Logger& L = b->log;
    auto row_bytes = [&](const ommxBlockTextureMipDesc& md) { return (((uint64_t)md.width + 3u) / 4u) * s.blockBytes; };
    for (uint32_t i = 0; i < s.mipCount; ++i) {
        const ommxBlockTextureMipDesc& md = s.mips[i];
        if (md.rowPitchInBytes != 0 && (uint64_t)md.rowPitchInBytes < row_bytes(md)) return L.invalid("[Invalid Arg] - mips.rowPitchInBytes is smaller than ceil(width / 4) * the size of a block");
        if (fromDevice && ((uint64_t)md.rowPitchInBytes % s.align != 0 || (uintptr_t)md.data % s.align != 0))
            return L.invalid(s.align == 8u ? "[Invalid Arg] - mips.rowPitchInBytes and mips.data must be multiples of 8" : "[Invalid Arg] - mips.rowPitchInBytes and mips.data must be multiples of 16");
    }
    // ---- the device ----
    const int dev = b->bind_device();
    int deviceCount = 0;
    if (dev < 0 || !HIP_OK(hipGetDeviceCount(&deviceCount)) || deviceCount < 1) { (void)hipGetLastError(); return L.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)"); }
    const DeviceScope onBakersDevice(dev);
    if (fromDevice) for (uint32_t i = 0; i < s.mipCount; ++i) {   // first and last byte of every mip, before any launch
        const ommxBlockTextureMipDesc& md = s.mips[i];
        const uint64_t pitch = md.rowPitchInBytes ? (uint64_t)md.rowPitchInBytes : row_bytes(md);
        const uint8_t* first = (const uint8_t*)md.data;
        if (!device_readable(first, dev) || !device_readable(first + (((uint64_t)md.height + 3u) / 4u - 1u) * pitch + row_bytes(md) - 1, dev))
            return L.invalid("[Invalid Arg] - mips.data is not memory the baker's device can read (device memory of that device, managed or pinned host memory)");
    }
    TextureBuild tb(b, s.format, s.flags, s.alphaCutoff);
    if (!tb.t) return ommResult_FAILURE;
    struct Uploads { DevPool* pool; std::vector<void*> blocks; ~Uploads() { for (void* p : blocks) pool->release(p); } } uploads{ b->devPool.get(), {} };   // (released behind the synchronisation below)
    std::vector<uint8_t> staging;
    for (uint32_t mi = 0; mi < s.mipCount && tb.ok; ++mi) {
        const ommxBlockTextureMipDesc& md = s.mips[mi];
        const uint64_t rowBytes = row_bytes(md), blockRows = ((uint64_t)md.height + 3u) / 4u;
        uint64_t pitch = md.rowPitchInBytes ? (uint64_t)md.rowPitchInBytes : rowBytes;
        const void* blocks = md.data;
        TexMip& m = tb.add_mip(md.width, md.height);
        if (!fromDevice && tb.ok) {
            const size_t bytes = (size_t)(rowBytes * blockRows);
            const uint8_t* src = (const uint8_t*)md.data;
            if (pitch != rowBytes) {
                staging.resize(bytes);
                for (uint64_t j = 0; j < blockRows; ++j) memcpy(staging.data() + rowBytes * j, src + pitch * j, (size_t)rowBytes);
                src = staging.data();
            }
            void* up = b->devPool->acquire(bytes);
            tb.ok = up != nullptr;
            if (tb.ok) { uploads.blocks.push_back(up); tb.ok = HIP_OK(hipMemcpy(up, src, bytes, hipMemcpyHostToDevice)); }
            blocks = up; pitch = rowBytes;
        }
        if (tb.ok) { decode(blocks, (size_t)pitch, m, stream); tb.ok = HIP_OK(hipGetLastError()); }
        tb.build_sat(m, stream);
    }
    return tb.finish(fromDevice ? HIP_OK(hipStreamSynchronize(stream)) : HIP_OK(hipDeviceSynchronize()), outTexture);
}

// ommxCreateTextureBC / ommxCreateTextureBCDevice: the alpha of BC1..BC5 blocks, decoded by block_kernels.hip.
ommResult create_texture_bc_impl(Baker* b, const ommxBlockTextureDesc* desc, bool fromDevice, hipStream_t stream, ommCpuTexture* outTexture)
{
    const Logger& L = b->log;
    // ---- everything that can be judged without a device (the pitch and alignment rules follow in create_texture_blocks_impl) ----
    if (desc->mipCount != 0 && desc->mips == nullptr) return L.invalid("[Invalid Arg] - mips is not set");
    const ommResult checked = check_texture_mips(L, desc->mipCount, (unsigned)desc->format < (unsigned)ommxBlockFormat_MAX_NUM, desc->mips, [](const ommxBlockTextureMipDesc& m) { return m.data; });
    if (checked != ommResult_SUCCESS) return checked;
    if (desc->channel > 1u) return L.invalid("[Invalid Arg] - channel must be 0 or 1");
    if (desc->channel != 0u && desc->format != ommxBlockFormat_BC5) return L.invalid("[Invalid Arg] - channel must be 0 for every format but BC5");
    const bool small = desc->format == ommxBlockFormat_BC1 || desc->format == ommxBlockFormat_BC4;
    const uint32_t blockBytes = small ? 8u : 16u, byteOffset = 8u * desc->channel;
    const int kind = desc->format == ommxBlockFormat_BC1 ? kBlockBC1 : desc->format == ommxBlockFormat_BC2 ? kBlockBC2 : kBlockBC4;
    const BlockSource src{ desc->flags, desc->mips, desc->mipCount, desc->alphaCutoff, blockBytes, 8u, kind == kBlockBC4 ? ommCpuTextureFormat_FP32 : ommCpuTextureFormat_UNORM8 };
    return create_texture_blocks_impl(b, src, fromDevice, stream, [&](const void* blocks, size_t pitch, TexMip& m, hipStream_t st) {
        launch_block_decode(blocks, pitch, blockBytes, byteOffset, kind, m.texels, m.w, m.h, st); }, outTexture);
}

// ommxCreateTextureBC7 / ommxCreateTextureBC7Device: the alpha of BC7 blocks, decoded by bc7_kernels.hip; always a UNORM8 texture.
ommResult create_texture_bc7_impl(Baker* b, const ommxBC7TextureDesc* desc, bool fromDevice, hipStream_t stream, ommCpuTexture* outTexture)
{
    const Logger& L = b->log;
    if (desc->mipCount != 0 && desc->mips == nullptr) return L.invalid("[Invalid Arg] - mips is not set");
    const ommResult checked = check_texture_mips(L, desc->mipCount, true, desc->mips, [](const ommxBlockTextureMipDesc& m) { return m.data; });
    if (checked != ommResult_SUCCESS) return checked;
    const BlockSource src{ desc->flags, desc->mips, desc->mipCount, desc->alphaCutoff, 16u, 16u, ommCpuTextureFormat_UNORM8 };
    return create_texture_blocks_impl(b, src, fromDevice, stream, [](const void* blocks, size_t pitch, TexMip& m, hipStream_t st) {
        launch_bc7_decode(blocks, pitch, m.texels, m.w, m.h, st); }, outTexture);
}
} // namespace

OMM_MI355X_API ommResult ommCpuCreateTexture(ommBaker baker, const ommCpuTextureDesc* desc, ommCpuTexture* outTexture)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    Baker* b = untag<Baker>(baker);
    if (desc == 0) return b->log.invalid("texture desc was not set");
    if (tag_of(baker) != kCpuBaker) return b->log.invalid("Baker was not created as the right type");
    return guarded(&b->log, [&] { return create_texture_impl(b, desc, outTexture); });
}

// A texture from one channel of an image that is already in device memory (include/omm_mi355x_ext.h): the gather kernel of texture_kernels.hip in place of
// the host staging and the upload, everything behind it as for ommCpuCreateTexture.
OMM_MI355X_API ommResult ommxCreateTextureDevice(ommBaker baker, const ommxDeviceTextureDesc* desc, void* hipStream, ommCpuTexture* outTexture)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    Baker* b = untag<Baker>(baker);
    if (desc == 0) return b->log.invalid("texture desc was not set");
    if (tag_of(baker) != kCpuBaker) return b->log.invalid("Baker was not created as the right type");
    if (outTexture == nullptr) return b->log.invalid("[Invalid Arg] - outTexture is not set");
    return guarded(&b->log, [&] { return create_texture_device_impl(b, desc, (hipStream_t)hipStream, outTexture); });
}

// A texture from the alpha of BC1..BC5 blocks, or of BC7 blocks (include/omm_mi355x_ext.h): the decode kernel of block_kernels.hip / bc7_kernels.hip in front
// of what ommCpuCreateTexture does.  `impl` is create_texture_bc_impl or create_texture_bc7_impl.
template <class Desc, class Impl>
static ommResult create_texture_from_blocks(ommBaker baker, const Desc* desc, bool fromDevice, void* hipStream, ommCpuTexture* outTexture, Impl impl)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    Baker* b = untag<Baker>(baker);
    if (desc == 0) return b->log.invalid("texture desc was not set");
    if (tag_of(baker) != kCpuBaker) return b->log.invalid("Baker was not created as the right type");
    if (outTexture == nullptr) return b->log.invalid("[Invalid Arg] - outTexture is not set");
    return guarded(&b->log, [&] { return impl(b, desc, fromDevice, (hipStream_t)hipStream, outTexture); });
}
OMM_MI355X_API ommResult ommxCreateTextureBC(ommBaker baker, const ommxBlockTextureDesc* desc, ommCpuTexture* outTexture)
{
    return create_texture_from_blocks(baker, desc, false, nullptr, outTexture, create_texture_bc_impl);
}
OMM_MI355X_API ommResult ommxCreateTextureBCDevice(ommBaker baker, const ommxBlockTextureDesc* desc, void* hipStream, ommCpuTexture* outTexture)
{
    return create_texture_from_blocks(baker, desc, true, hipStream, outTexture, create_texture_bc_impl);
}
OMM_MI355X_API ommResult ommxCreateTextureBC7(ommBaker baker, const ommxBC7TextureDesc* desc, ommCpuTexture* outTexture)
{
    return create_texture_from_blocks(baker, desc, false, nullptr, outTexture, create_texture_bc7_impl);
}
OMM_MI355X_API ommResult ommxCreateTextureBC7Device(ommBaker baker, const ommxBC7TextureDesc* desc, void* hipStream, ommCpuTexture* outTexture)
{
    return create_texture_from_blocks(baker, desc, true, hipStream, outTexture, create_texture_bc7_impl);
}

OMM_MI355X_API ommResult ommCpuGetTextureDesc(ommCpuTexture texture, ommCpuTextureDesc* outDesc)
{
    if (texture == 0) return ommResult_INVALID_ARGUMENT;
    Texture* t = untag<Texture>(texture);
    if (t == 0 || outDesc == nullptr) return ommResult_INVALID_ARGUMENT;
    outDesc->format = t->format; outDesc->flags = t->flags; outDesc->alphaCutoff = t->alphaCutoff; outDesc->mipCount = (uint32_t)t->mips.size();
    if (outDesc->mips == nullptr) return ommResult_SUCCESS;
    const size_t px = t->format == ommCpuTextureFormat_FP32 ? 4 : 1;
    for (uint32_t i = 0; i < outDesc->mipCount; ++i) { // texture_impl.cpp:280-325
        ommCpuTextureMipDesc& m = const_cast<ommCpuTextureMipDesc&>(outDesc->mips[i]);
        m.width = (uint32_t)t->mips[i].w; m.height = (uint32_t)t->mips[i].h; m.rowPitch = (uint32_t)t->mips[i].w;
        if (m.textureData != nullptr)
            if (!HIP_OK(hipMemcpy(const_cast<void*>(m.textureData), t->mips[i].texels, px * (size_t)m.width * m.height, hipMemcpyDeviceToHost))) return ommResult_FAILURE;
    }
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommCpuDestroyTexture(ommBaker baker, ommCpuTexture texture)
{
    if (texture == 0) return ommResult_INVALID_ARGUMENT;
    Baker* b = untag<Baker>(baker);
    if (tag_of(baker) != kCpuBaker) return b ? b->log.invalid("Baker was not created as the right type") : ommResult_INVALID_ARGUMENT;
    Texture* t = untag<Texture>(texture);
    b->mem.destroy(t);
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommCpuBake(ommBaker baker, const ommCpuBakeInputDesc* desc, ommCpuBakeResult* outBakeResult)
{
    Baker* b = nullptr;
    const ommResult v = check_bake_entry(baker, desc, &b);
    if (v != ommResult_SUCCESS) return v;
    return guarded(&b->log, [&] { return bake_impl(*b, *desc, outBakeResult); });
}

OMM_MI355X_API ommResult ommCpuDestroyBakeResult(ommCpuBakeResult bakeResult)
{
    if (bakeResult == 0) return ommResult_INVALID_ARGUMENT;
    BakeResult* r = (BakeResult*)bakeResult;
    const Allocator mem = r->mem;
    mem.destroy(r);
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommCpuGetBakeResultDesc(ommCpuBakeResult bakeResult, const ommCpuBakeResultDesc** desc)
{
    if (bakeResult == 0) return ommResult_INVALID_ARGUMENT;
    if (desc == nullptr) return ommResult_INVALID_ARGUMENT;
    *desc = &((BakeResult*)bakeResult)->desc;
    return ommResult_SUCCESS;
}

namespace {
// CollectStats (debug_impl.cpp:512-641), in the reference's evaluation order: per-descriptor micro-triangle counts are uint32, the
// per-reference products are taken in 32 bits before they are added to the 64-bit totals (`uint * uint32_t`, :630-633), the areas of
// the triangles that share a descriptor are summed in triangle order and the descriptors are visited in ascending index order
// (std::map, :523,621).  `area` == nullptr (ommDebugGetStats) leaves knownAreaMetric at 0.
ommResult collect_stats(const ommCpuBakeResultDesc* res, const float* area, ommDebugStats* out)
{
    if (res == nullptr || out == nullptr) return ommResult_INVALID_ARGUMENT;
    ommDebugStats st; memset(&st, 0, sizeof st);
    const uint32_t T = res->indexCount;
    float totalArea = 0.f, knownArea = 0.f;
    if (area) for (uint32_t i = 0; i < T; ++i) totalArea += area[i];
    std::vector<uint32_t> refs((size_t)res->descArrayCount + 1, 0);
    std::vector<float> refArea(area ? (size_t)res->descArrayCount + 1 : 0, 0.f);
    for (uint32_t i = 0; i < T; ++i) {
        int32_t v;
        if (res->indexFormat == ommIndexFormat_UINT_8) v = ((const int8_t*)res->indexBuffer)[i];
        else if (res->indexFormat == ommIndexFormat_UINT_16) v = ((const int16_t*)res->indexBuffer)[i];
        else v = ((const int32_t*)res->indexBuffer)[i];
        if (v == ommSpecialIndex_FullyTransparent) { st.totalFullyTransparent++; knownArea += area ? area[i] : 0; }
        else if (v == ommSpecialIndex_FullyOpaque) { st.totalFullyOpaque++; knownArea += area ? area[i] : 0; }
        else if (v == ommSpecialIndex_FullyUnknownTransparent) st.totalFullyUnknownTransparent++;
        else if (v == ommSpecialIndex_FullyUnknownOpaque) st.totalFullyUnknownOpaque++;
        else if (v >= 0 && (uint32_t)v < res->descArrayCount) {
            if (area) { if (refs[(size_t)v] == 0) refArea[(size_t)v] = area[i]; else refArea[(size_t)v] += area[i]; }
            refs[(size_t)v]++;
        }
    }
    for (uint32_t i = 0; i < res->descArrayCount; ++i) {
        if (!refs[i]) continue;
        const ommCpuOpacityMicromapDesc& dd = res->descArray[i];
        const uint8_t* data = (const uint8_t*)res->arrayData + dd.offset;
        const uint32_t nM = 1u << (dd.subdivisionLevel << 1);
        const uint32_t is2 = dd.format == ommFormat_OC1_2_State;
        uint32_t c[4] = { 0, 0, 0, 0 };
        for (uint32_t u = 0; u < nM; ++u) {
            const uint8_t v = data[u >> (2 + is2)];
            c[is2 ? ((v >> (u & 7)) & 1u) : ((v >> ((u << 1) & 7)) & 3u)]++;
        }
        if (area) {
            const uint32_t totalKnown = c[0] + c[1], totalUnknown = c[2] + c[3];
            const float known = (float)totalKnown / (float)(totalKnown + totalUnknown);
            knownArea += known * refArea[i];
        }
        st.totalTransparent += (uint32_t)(refs[i] * c[0]); st.totalOpaque += (uint32_t)(refs[i] * c[1]);
        st.totalUnknownTransparent += (uint32_t)(refs[i] * c[2]); st.totalUnknownOpaque += (uint32_t)(refs[i] * c[3]);
    }
    st.knownAreaMetric = area ? knownArea / totalArea : 0;
    *out = st;
    return ommResult_SUCCESS;
}
const Logger* baker_log(ommBaker baker) { return baker ? &untag<Baker>(baker)->log : nullptr; }
} // namespace

// include/omm.h:1201, bake.cpp:338-357
OMM_MI355X_API ommResult ommDebugGetStats(ommBaker baker, const ommCpuBakeResultDesc* res, ommDebugStats* out)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    if (tag_of(baker) != kCpuBaker && tag_of(baker) != kGpuBaker) return ommResult_INVALID_ARGUMENT;
    return guarded(baker_log(baker), [&] { return collect_stats(res, nullptr, out); });
}

// include/omm.h:1202, bake.cpp:359-386: statistics of a result OBJECT, with the per-triangle areas it carries
OMM_MI355X_API ommResult ommDebugGetStats2(ommBaker baker, ommCpuBakeResult res, ommDebugStats* out)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    if (res == 0) return ommResult_INVALID_ARGUMENT;   // (the reference dereferences a null result here)
    if (tag_of(baker) != kCpuBaker && tag_of(baker) != kGpuBaker) return ommResult_INVALID_ARGUMENT;
    const BakeResult* r = (const BakeResult*)res;
    return guarded(baker_log(baker), [&] { return collect_stats(&r->desc, r->triArea, out); });
}

// include/omm.h:1204, bake.cpp:388-408, debug_impl.cpp:654-670
OMM_MI355X_API ommResult ommDebugSaveBinaryToDisk(ommBaker baker, const ommCpuBlobDesc* data, const char* path)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    if (path == 0) return ommResult_INVALID_ARGUMENT;
    if (tag_of(baker) != kCpuBaker && tag_of(baker) != kGpuBaker) return ommResult_INVALID_ARGUMENT;
    const Logger& L = untag<Baker>(baker)->log;
    FILE* f = data ? fopen(path, "wb") : nullptr;
    bool ok = f != nullptr;
    if (ok && data->size) ok = fwrite(data->data, 1, (size_t)data->size, f) == (size_t)data->size;
    if (f) ok = (fclose(f) == 0) && ok;
    if (!ok) { char buf[512]; snprintf(buf, sizeof buf, "Unable to save file %s", path); L.msg(ommMessageSeverity_Error, buf); return ommResult_INVALID_ARGUMENT; } // log.ErrorArgf
    return ommResult_SUCCESS;
}

// ---- link-compatible stubs of the SDK's GPU baker and PNG dump (include/omm.h:1127-1141,1199; bake.cpp:262-336) ----
// Argument checks follow the reference; past them the answer is NOT_IMPLEMENTED (+ a log line where a baker is at hand).
namespace {
ommResult gpu_baker_not_built(const Logger* L, const char* fn)
{
    if (L) { char buf[256]; snprintf(buf, sizeof buf, "[Not Implemented] - %s: the SDK's D3D12/Vulkan GPU baker is not part of the MI355X build (use ommCpuBake, which runs on the GPU here)", fn); L->msg(ommMessageSeverity_Fatal, buf); }
    return ommResult_NOT_IMPLEMENTED;
}
}
OMM_MI355X_API ommResult ommGpuGetStaticResourceData(ommGpuResourceType, uint8_t*, size_t* outByteSize)
{
    if (outByteSize == nullptr) return ommResult_INVALID_ARGUMENT;
    return gpu_baker_not_built(nullptr, "ommGpuGetStaticResourceData");
}
OMM_MI355X_API ommResult ommGpuCreatePipeline(ommBaker baker, const ommGpuPipelineConfigDesc* config, ommGpuPipeline* outPipeline)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    const Logger& L = untag<Baker>(baker)->log;
    if (config == 0) return L.invalid("[Invalid Arg] - pipeline config desc must be provided");
    if (tag_of(baker) != kGpuBaker) return L.invalid("[Invalid Arg] - invalid baker type");
    if (outPipeline) *outPipeline = nullptr;
    return gpu_baker_not_built(&L, "ommGpuCreatePipeline");
}
OMM_MI355X_API ommResult ommGpuDestroyPipeline(ommBaker baker, ommGpuPipeline pipeline)
{
    if (pipeline == 0 || baker == 0 || tag_of(baker) != kGpuBaker) return ommResult_INVALID_ARGUMENT;
    return gpu_baker_not_built(&untag<Baker>(baker)->log, "ommGpuDestroyPipeline");
}
OMM_MI355X_API ommResult ommGpuGetPipelineDesc(ommGpuPipeline pipeline, const ommGpuPipelineInfoDesc**)
{
    if (pipeline == 0) return ommResult_INVALID_ARGUMENT;
    return gpu_baker_not_built(nullptr, "ommGpuGetPipelineDesc");   // (no pipeline handle can exist: CreatePipeline never succeeds)
}
OMM_MI355X_API ommResult ommGpuGetPreDispatchInfo(ommGpuPipeline pipeline, const ommGpuDispatchConfigDesc* config, ommGpuPreDispatchInfo*)
{
    if (pipeline == 0 || config == 0) return ommResult_INVALID_ARGUMENT;
    return gpu_baker_not_built(nullptr, "ommGpuGetPreDispatchInfo");
}
OMM_MI355X_API ommResult ommGpuDispatch(ommGpuPipeline pipeline, const ommGpuDispatchConfigDesc* config, const ommGpuDispatchChain**)
{
    if (pipeline == 0 || config == 0) return ommResult_INVALID_ARGUMENT;
    return gpu_baker_not_built(nullptr, "ommGpuDispatch");
}
OMM_MI355X_API ommResult ommDebugSaveAsImages(ommBaker baker, const ommCpuBakeInputDesc* bakeInputDesc, const ommCpuBakeResultDesc*, const ommDebugSaveImagesDesc* desc)
{
    if (baker == 0 || bakeInputDesc == 0 || desc == 0) return ommResult_INVALID_ARGUMENT;
    if (tag_of(baker) != kCpuBaker && tag_of(baker) != kGpuBaker) return ommResult_INVALID_ARGUMENT;
    const Logger& L = untag<Baker>(baker)->log;
    L.msg(ommMessageSeverity_Fatal, "[Not Implemented] - ommDebugSaveAsImages: the PNG overlay dump (stb) is not part of the MI355X build");
    return ommResult_NOT_IMPLEMENTED;
}

OMM_MI355X_API ommResult ommxBakeDevice(ommBaker baker, const ommCpuBakeInputDesc* desc, ommxDeviceBakeResult* outResult)
{
    Baker* b = nullptr;
    ommResult r = check_bake_entry(baker, desc, &b, outResult != 0);
    if (r != ommResult_SUCCESS) return r;
    r = scope_fences(*b, *desc, false);
    if (r != ommResult_SUCCESS) return r;
    return guarded(&b->log, [&]() -> ommResult {
    const double t0 = now_ms();
    const DeviceScope onBakersDevice(b->bind_device());
    BakeSession ses(*b);
    if (!ses.open()) return b->log.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)");
    DeviceResultOwner res(b->mem, ses.stream);
    if (!res.make()) return ommResult_FAILURE;
    EventTimer et(ses.stream);
    ommxBakeTimings tm; memset(&tm, 0, sizeof tm);
    DeviceInputs din; din.texCoords = desc->texCoords; din.indices = desc->indexBuffer; din.perTriLevels = desc->subdivisionLevels;
    if (wants_host_tail(*desc)) {
        // near-duplicate merge / size budget: classification on the device, the reference's serial tail on the host, result uploaded again
        HostTailRequest ht; DeviceResult scratchR;
        ommResult hr = bake_core(*b, *desc, din, ses.arena, ses.states, ses.stream, et, scratchR, tm, nullptr, &ht);
        HostTailResult hres; ommIndexFormat ifmt = ommIndexFormat_UINT_32;
        if (hr == ommResult_SUCCESS) hr = run_host_tail_for(*desc, desc->indexCount / 3u, ht.items, hres, ifmt);
        if (hr == ommResult_SUCCESS) hr = upload_host_tail(*b, hres, ifmt, desc->indexCount / 3u, (int)desc->format, ses.stream, res.p);
        if (hr == ommResult_SUCCESS && !keep_tri_areas(res->R, scratchR.triAreaScratch, desc->indexCount / 3u, ses.stream)) hr = b->log.failure("[Failure] - could not keep the triangle areas on the device");
        if (hr != ommResult_SUCCESS) return hr;
        tm.totalMs = (float)(now_ms() - t0);
        store_timings(*b, tm);
        *outResult = (ommxDeviceBakeResult)res.release();
        return ommResult_SUCCESS;
    }
    r = bake_core(*b, *desc, din, ses.arena, ses.states, ses.stream, et, res->R, tm);
    if (r == ommResult_SUCCESS && !keep_tri_areas(res->R, res->R.triAreaScratch, desc->indexCount / 3u, ses.stream)) r = b->log.failure("[Failure] - could not keep the triangle areas on the device");
    if (r != ommResult_SUCCESS) return r;
    finish_device_result(res.p);
    tm.totalMs = (float)(now_ms() - t0);
    store_timings(*b, tm);
    *outResult = (ommxDeviceBakeResult)res.release();
    return ommResult_SUCCESS;
    });
}

// ---- multi-GPU sharded bake (include/omm_mi355x_ext.h) ----
namespace {
struct ShardedBake {
    Allocator mem; Baker* baker = nullptr; BakeSession ses; ShardCtx ctx; ommxBakeTimings tm; double t0 = 0;
    std::unique_ptr<EventTimer> et;
    explicit ShardedBake(Baker& b) : baker(&b), ses(b) { memset(&tm, 0, sizeof tm); }
};

// ---- RCCL, bound at first use ----
// The collectives of the sharded bake are RCCL calls made from this library on its own streams (ommxShardedBakeRccl).  librccl is
// resolved with dlopen at the first call, so the drop-in keeps loading on machines (and for callers) that never shard a bake; when the
// process already holds an RCCL (e.g. torch's) its SONAME librccl.so.1 resolves to that instance.
typedef void* rcclComm_t;
struct RcclUniqueId { char internal[128]; };                       // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
enum { kRcclSum = 0, kRcclMax = 2, kRcclMin = 3, kRcclUint8 = 1, kRcclUint32 = 3 };   // ncclRedOp_t (sum, max, min) / ncclDataType_t (uint8, uint32) values of rccl.h
struct RcclApi {
    void* dso = nullptr; std::string error;
    int (*getUniqueId)(RcclUniqueId*) = nullptr;
    int (*commInitRank)(rcclComm_t*, int, RcclUniqueId, int) = nullptr;
    int (*commDestroy)(rcclComm_t) = nullptr;
    int (*commCount)(rcclComm_t, int*) = nullptr;
    int (*commUserRank)(rcclComm_t, int*) = nullptr;
    int (*allReduce)(const void*, void*, size_t, int, int, rcclComm_t, hipStream_t) = nullptr;
    int (*allGather)(const void*, void*, size_t, int, rcclComm_t, hipStream_t) = nullptr;
    const char* (*getErrorString)(int) = nullptr;
    bool ok() const { return dso != nullptr && error.empty(); }
};
const RcclApi& rccl()
{
    static const RcclApi api = [] {
        RcclApi a;
        for (const char* name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) { a.dso = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (a.dso) break; }
        if (!a.dso) { a.error = "librccl.so.1 could not be loaded"; return a; }
        auto sym = [&](const char* n) { void* p = dlsym(a.dso, n); if (!p && a.error.empty()) a.error = std::string("librccl lacks ") + n; return p; };
        a.getUniqueId = (int (*)(RcclUniqueId*))sym("ncclGetUniqueId");
        a.commInitRank = (int (*)(rcclComm_t*, int, RcclUniqueId, int))sym("ncclCommInitRank");
        a.commDestroy = (int (*)(rcclComm_t))sym("ncclCommDestroy");
        a.commCount = (int (*)(rcclComm_t, int*))sym("ncclCommCount");
        a.commUserRank = (int (*)(rcclComm_t, int*))sym("ncclCommUserRank");
        a.allReduce = (int (*)(const void*, void*, size_t, int, int, rcclComm_t, hipStream_t))sym("ncclAllReduce");
        a.allGather = (int (*)(const void*, void*, size_t, int, rcclComm_t, hipStream_t))sym("ncclAllGather");
        a.getErrorString = (const char* (*)(int))sym("ncclGetErrorString");
        return a;
    }();
    return api;
}
struct RcclComm {
    rcclComm_t comm = nullptr; bool owned = false; int rank = 0, world = 1;
    uint32_t* dStatus = nullptr; hipStream_t statusStream = nullptr;   // status agreement (rccl_agree): two device words and a stream for ranks that have no bake stream
    int statusDevice = -1;                                             // ... and the device they live on (rccl_status_on_device)
    bool custom = false; ommxCollectives user{};                       // ommxCommFromCollectives: the caller's transport instead of RCCL
    // the two collectives of the sharded bake (uint32 all-reduce, byte all-gather), stream-ordered; 0 = success
    int all_reduce(const void* send, void* recv, size_t count, int rcclOp, hipStream_t stream) const
    {
        if (!custom) return rccl().allReduce(send, recv, count, kRcclUint32, rcclOp, comm, stream);
        return user.allReduceU32(user.user, send, recv, count, rcclOp == kRcclSum ? ommxReduceOp_Sum : (rcclOp == kRcclMax ? ommxReduceOp_Max : ommxReduceOp_Min), (void*)stream);
    }
    int all_gather(const void* send, void* recv, size_t bytesPerRank, hipStream_t stream) const
    {
        if (!custom) return rccl().allGather(send, recv, bytesPerRank, kRcclUint8, comm, stream);
        return user.allGatherBytes(user.user, send, recv, bytesPerRank, (void*)stream);
    }
    const char* error_string(int code) const { return custom ? "the caller's collective reported a failure" : (rccl().getErrorString ? rccl().getErrorString(code) : "RCCL error"); }
};
// The two status words and the stream of idle ranks are set up when the communicator is made (on the device that is current then), so that a rank
// that has run out of device memory later can still take part in every agreement; rccl_agree() only allocates if that did not succeed.
void rccl_prepare_status(RcclComm* c)
{
    if (!HIP_OK(hipGetDevice(&c->statusDevice))) { c->statusDevice = -1; (void)hipGetLastError(); }
    if (!c->dStatus && !HIP_OK(hipMalloc((void**)&c->dStatus, 2 * sizeof(uint32_t)))) { c->dStatus = nullptr; (void)hipGetLastError(); }
    if (!c->statusStream && !HIP_OK(hipStreamCreateWithFlags(&c->statusStream, hipStreamNonBlocking))) { c->statusStream = nullptr; (void)hipGetLastError(); }
}
// The communicator may have been made before the caller selected the rank's device (ommxCommFromCollectives / ommxRcclCommWrap in front of
// torch.cuda.set_device): status words and stream of another GPU than the bake's would mix devices inside one collective.  Called under the baker's
// DeviceScope: anything that lives elsewhere is released and made again here.
void rccl_status_on_device(RcclComm* c, int device)
{
    if (c->statusDevice == device && c->dStatus && c->statusStream) return;
    if (c->statusDevice != device) {
        if (c->statusStream) { (void)hipStreamSynchronize(c->statusStream); (void)hipStreamDestroy(c->statusStream); c->statusStream = nullptr; }
        if (c->dStatus) { (void)hipFree(c->dStatus); c->dStatus = nullptr; }
        (void)hipGetLastError();
    }
    rccl_prepare_status(c);   // (on the current device = `device`)
}
// A rank-local failure (out of memory, mostly) must not leave the other ranks waiting in the next collective: before every data collective each rank
// contributes its status to a one-element all-reduce and all of them go on, or none.  The one routine behind both forms:
//   plain (dWord null)   MIN over the ranks' status words; a rank that has no bake stream (null) uses the communicator's own
//   carrying a number    MAX over the device words *dWord, 0xFFFFFFFF written there only if this rank failed; *outMax = the largest one
// false = a rank failed (this one or another).
bool rccl_agree(RcclComm* rc, hipStream_t stream, bool mineOk, const Logger& L, const char* stage, uint32_t* dWord = nullptr, uint32_t* outMax = nullptr)
{
    const bool carries = dWord != nullptr;
    bool ok = true;
    if (!rc->dStatus) ok = HIP_OK(hipMalloc((void**)&rc->dStatus, 2 * sizeof(uint32_t)));
    if (ok && !carries && !stream) { if (!rc->statusStream) ok = HIP_OK(hipStreamCreateWithFlags(&rc->statusStream, hipStreamNonBlocking)); stream = rc->statusStream; }
    if (!ok) { (void)hipGetLastError(); L.failure("[Failure] - sharded bake: no device memory for the status word (the other ranks may be waiting in a collective)"); return false; }
    uint32_t* const dMine = carries ? dWord : rc->dStatus;
    const uint32_t failed = carries ? 0xFFFFFFFFu : 0u, mine = mineOk ? 1u : failed; uint32_t all = failed;
    if (!carries || !mineOk) ok = HIP_OK(hipMemcpyAsync(dMine, &mine, sizeof mine, hipMemcpyHostToDevice, stream)) && HIP_OK(hipStreamSynchronize(stream));
    ok = ok && rc->all_reduce(dMine, rc->dStatus + 1, 1, carries ? kRcclMax : kRcclMin, stream) == 0;
    ok = ok && HIP_OK(hipMemcpyAsync(&all, rc->dStatus + 1, sizeof all, hipMemcpyDeviceToHost, stream)) && HIP_OK(hipStreamSynchronize(stream));
    if (!ok) { L.failure("[Failure] - sharded bake: the status all-reduce failed"); return false; }
    if (mineOk && all == failed) { char buf[200]; snprintf(buf, sizeof buf, "[Failure] - sharded bake: another rank failed (%s); this rank stops with it", stage); L.failure(buf); }
    if (outMax) *outMax = all;
    return mineOk && all != failed;
}

ommResult sharded_checks(ommBaker baker, const ommCpuBakeInputDesc* desc, Baker** outB, bool hostTailOk)
{
    const ommResult r = check_bake_entry(baker, desc, outB);
    return r != ommResult_SUCCESS ? r : scope_fences(**outB, *desc, false, hostTailOk, false);
}

// phase 1: replicated setup + triage, classification and digests of this rank's share, metadata words packed for the all-reduce.
// async: nothing is synchronised at the end (the RCCL all-reduce follows on the same stream).
ommResult sharded_begin(Baker* b, const ommCpuBakeInputDesc* desc, uint32_t rank, uint32_t worldSize, bool async, ShardedBake** out, bool mergeStates = false)
{
    ShardedBake* sb = b->mem.make<ShardedBake>(*b);
    if (!sb) return ommResult_FAILURE;
    sb->mem = b->mem; sb->t0 = now_ms();
    if (!sb->ses.open()) { b->mem.destroy(sb); return b->log.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)"); }
    sb->ctx.rank = rank; sb->ctx.world = worldSize; sb->ctx.asyncBegin = async; sb->ctx.mergeStates = mergeStates;
    sb->et.reset(new EventTimer(sb->ses.stream));
    DeviceResult unused;
    DeviceInputs din; din.texCoords = desc->texCoords; din.indices = desc->indexBuffer; din.perTriLevels = desc->subdivisionLevels;
    const ommResult r = bake_core(*b, *desc, din, sb->ses.arena, sb->ses.states, sb->ses.stream, *sb->et, unused, sb->tm, &sb->ctx);
    if (r != ommResult_SUCCESS) { b->mem.destroy(sb); return r; }
    *out = sb;
    return ommResult_SUCCESS;
}

// phase 2 (after the metadata all-reduce): replicated tail, per-rank layout, this rank's surviving blocks packed into its contribution.
// Ends with the contribution complete on the stream (not synchronised); the two host read-backs inside (OMM count, per-rank totals) remain.
ommResult sharded_tail(ShardedBake* sb)
{
    ShardCtx& c = sb->ctx; const Logger& L = sb->baker->log; hipStream_t stream = sb->ses.stream;
    const uint32_t numActive = c.hc.activeStart[kNumLevels];
    if (!HIP_OK(hipMemsetAsync(c.tab.owner, 0xFF, c.ti.numItems ? c.ti.numItems : 1, stream))) return L.failure("[Failure] - device memset failed");
    launch_shard_unpack_meta(c.bounds, c.tab.activeIds, numActive, c.tab.meta, c.tab.mask, (uint32_t*)c.ti.knownCount, c.ti.digests, c.tab.owner, stream);
    if (!HIP_OK(run_tail(c.ti, c.to, c.tab.scratch, c.tab.scratchBytes, &c.counts, stream))) return L.failure("[Failure] - device tail failed");
    if (c.counts.arrayDataSize > 0xFFFFFFFFull) return ommResult_FAILURE; // bake_cpu_impl.cpp:1774-1775
    if (!HIP_OK(run_shard_layout(c.to.order, c.to.sizes, c.tab.active, c.tab.owner, c.counts.numOmms, c.world, c.tab.cofs, c.tab.totals, c.totals, c.tab.scratch, c.tab.scratchBytes, stream)))
        return L.failure("[Failure] - sharded layout failed");
    c.strideBytes = contribution_stride(c.totals, c.world);
    // the exchange buffers: one grow-only block of the session's working set, size and pointers from the same traversal (bake_host.h)
    DeviceArena& xchg = sb->ses.set->xchg;
    const size_t codecScratch = c.asyncBegin ? shard_codec_scratch_bytes(c.strideBytes) : 0;
    if (!xchg.reserve(carve_exchange_arena(0, c.strideBytes, c.world, c.asyncBegin, codecScratch).bytes, *sb->baker->devPool->poison)) return L.failure("[Failure] - out of device memory for the shard contribution");
    c.x = carve_exchange_arena((uintptr_t)xchg.base, c.strideBytes, c.world, c.asyncBegin, codecScratch);
    // (the padding behind this rank's blocks travels too: zeros, which the codec folds away)
    if (c.strideBytes > c.totals[c.rank] && !HIP_OK(hipMemsetAsync(c.x.contrib + c.totals[c.rank], 0, (size_t)(c.strideBytes - c.totals[c.rank]), stream))) return L.failure("[Failure] - device memset failed");
    launch_shard_gather(c.dStates, c.tab.stateOfs, c.tab.active, c.tab.owner, c.rank, c.to.order, c.tab.cofs, c.to.sizes, c.counts.numOmms, c.x.contrib, stream);
    return HIP_OK(hipGetLastError()) ? ommResult_SUCCESS : L.failure("[Failure] - shard gather failed");
}

// The timings of a sharded bake once its stream has been synchronised (Begin may have returned without that): the event marks of the begin phase as
// times -- the host-tail form has no digest pass of its own to time --, the total, and the whole to the baker.
void store_begin_timings(ShardedBake* sb, bool withDigest)
{
    const int* e = sb->ctx.ev; const EventTimer& et = *sb->et; ommxBakeTimings& tm = sb->tm;
    tm.setupMs = et.ms(e[0], e[1]); tm.triageMs = et.ms(e[1], e[2]); tm.classifyMs = et.ms(e[2], e[3]);
    if (withDigest) tm.digestMs = et.ms(e[3], e[4]);
    tm.totalMs = (float)(now_ms() - sb->t0);
    store_timings(*sb->baker, tm);
}
// the gathered blocks to their final offsets in arrayData: bytes [lo, hi) of every rank's contribution, from `src` (byte lo of rank 0; rank r `pitch` bytes behind rank r - 1) ...
void shard_scatter(const ShardCtx& c, const uint8_t* src, uint64_t pitch, uint64_t lo, uint64_t hi, uint8_t* arrayData, hipStream_t stream)
{
    launch_shard_scatter(src, pitch, lo, hi, c.tab.active, c.tab.owner, c.tab.mask, c.tab.level, c.bits, c.to.order, c.tab.cofs, c.to.dstOfs, c.to.sizes, c.counts.numOmms, arrayData, stream);
}
// ... or every block straight from its owner's codec stream of `sendBytes` among the gathered ones (no expanded copy of the contributions)
void shard_scatter_streams(const ShardCtx& c, size_t sendBytes, uint8_t* arrayData, hipStream_t stream)
{
    launch_shard_scatter_streams(c.x.gatherComp, sendBytes, c.strideBytes, c.tab.active, c.tab.owner, c.tab.mask, c.tab.level, c.bits, c.to.order, c.tab.cofs, c.to.dstOfs, c.to.sizes, c.counts.numOmms, arrayData, stream);
}

// phase 3: result buffers, descriptors, index buffer; `scatter` places the gathered blocks (one call or one per chunk)
template <class ScatterFn>
ommResult sharded_finish(ShardedBake* sb, ScatterFn&& scatter, ommxDeviceBakeResult* outResult, bool wantArray = true)
{
    ShardCtx& c = sb->ctx; Baker* b = sb->baker; const Logger& L = b->log; hipStream_t stream = sb->ses.stream;
    const uint32_t E = c.counts.numOmms, T = c.T;
    DeviceResultOwner res(b->mem, stream);
    if (!res.make()) return ommResult_FAILURE;
    DeviceResult& R = res->R;
    R.pool = b->devPool;
    R.bits = c.bits; R.numDescs = E; R.arrayDataSize = E ? c.counts.arrayDataSize : 0; R.numTris = T;
    bool ok = true;
    if (E) {
        R.arrayData = wantArray ? (uint8_t*)R.dev_alloc((size_t)c.counts.arrayDataSize) : nullptr; R.descs = (ommCpuOpacityMicromapDesc*)R.dev_alloc(sizeof(ommCpuOpacityMicromapDesc) * (size_t)E);
        ok = (R.arrayData != nullptr || !wantArray) && R.descs != nullptr;
        ok = scatter(ok ? R.arrayData : nullptr) && ok;   // (called either way: the RCCL form agrees on the allocation across ranks before its all-gathers)
        if (ok) launch_write_descs(c.to.order, c.to.dstOfs, c.tab.level, c.bits, E, R.descs, stream);
    }
    R.indexFormat = index_format_for(T, c.flags);
    R.index = R.dev_alloc((size_t)(T ? T : 1) * 4);
    ok = ok && R.index != nullptr;
    if (ok) launch_narrow_indices(c.tab.index, T, (int)index_bytes(R.indexFormat), R.index, stream);
    ok = ok && HIP_OK(hipMemcpyAsync(R.hist, c.tab.arrayHist, sizeof(uint32_t) * kNumLevels, hipMemcpyDeviceToHost, stream));
    ok = ok && HIP_OK(hipMemcpyAsync(R.hist + kNumLevels, c.tab.indexHist, sizeof(uint32_t) * kNumLevels, hipMemcpyDeviceToHost, stream));
    ok = ok && HIP_OK(hipStreamSynchronize(stream));
    if (!ok) return L.failure("[Failure] - could not materialise the merged bake result on the device");
    finish_device_result(res.p);
    store_begin_timings(sb, true);
    *outResult = (ommxDeviceBakeResult)res.release();
    return ommResult_SUCCESS;
}

// ================================================================================================
// ommCpuBake over several devices of one process (ommxBakerKnob_Devices = N; SURVEY.md section 8e behind the SDK's entry point, omm.h:574).
//
// One host thread per device ("rank"; rank 0 = the caller's thread on the baker's device, rank r on device (primary + r) mod the device count -- with fewer
// devices than ranks several ranks share one, which is how the path is tested on a one-GPU box).  Every rank uploads the triangle data over its own PCIe
// link and runs the sharded bake's phases on its device: set-up and triage replicated, classification and digests of ITS share of the active work items
// (sharded_begin), the 16 bytes of metadata per active item summed across the ranks THROUGH HOST MEMORY (no device-to-device traffic at all), the
// deterministic tail replicated (sharded_tail).  Then every rank turns the blocks it owns into ONE codec stream and sends it over its own link; the host
// writes every block of the result from its owner's stream (codec_scatter_omms, the helper threads).  Descriptors, index buffer and histograms come from rank 0.
// No all-gather of the array: the 1.27 GB of the metric configuration cross the links as N streams of ~82 / N MB.
// ================================================================================================
struct RankTeam {
    uint32_t n = 1; std::mutex mu; std::condition_variable cv; uint32_t arrived = 0; uint64_t generation = 0; bool allOk = true, result = true, aborted = false;
    // every rank arrives with its status; all leave with the conjunction.  A rank that cannot go on at all (an exception) calls abort(): every rank that waits
    // or arrives later leaves with false at once, so nobody waits for a rank that is gone.
    bool barrier(bool ok) {
        std::unique_lock<std::mutex> lk(mu);
        if (aborted) return false;
        allOk = allOk && ok;
        if (++arrived == n) { result = allOk; allOk = true; arrived = 0; ++generation; cv.notify_all(); return result; }
        const uint64_t g = generation;
        cv.wait(lk, [&] { return generation != g || aborted; });
        return aborted ? false : result;
    }
    void abort() { std::lock_guard<std::mutex> g(mu); aborted = true; cv.notify_all(); }
};
// the texture of `d` on device `dev` (the original when that is where it lives)
Texture* texture_on_device(Texture* t, int dev)
{
    if (t->device < 0 || t->device == dev) return t;
    std::lock_guard<std::mutex> g(t->replicaMu);
    for (auto& r : t->replicas) if (r->device == dev) return r.get();
    const DeviceScope onDev(dev);
    std::unique_ptr<Texture> r(new (std::nothrow) Texture());
    if (!r) return nullptr;
    r->mem = t->mem; r->log = t->log; r->format = t->format; r->flags = t->flags; r->alphaCutoff = t->alphaCutoff; r->device = dev;
    const size_t px = t->format == ommCpuTextureFormat_FP32 ? 4 : 1;
    for (const TexMip& m : t->mips) {
        TexMip c = m; c.texels = nullptr; c.sat = nullptr;
        const size_t n = (size_t)m.w * (size_t)m.h;
        bool ok = HIP_OK(hipMalloc((void**)&c.texels, n * px)) && HIP_OK(hipMemcpy(c.texels, m.texels, n * px, hipMemcpyDefault));
        if (ok && m.sat) ok = HIP_OK(hipMalloc((void**)&c.sat, n * 4)) && HIP_OK(hipMemcpy(c.sat, m.sat, n * 4, hipMemcpyDefault));
        r->mips.push_back(c);   // (freed by ~Texture, also when the copy failed half way)
        if (!ok) { (void)hipGetLastError(); return nullptr; }
    }
    t->replicas.push_back(std::move(r));
    return t->replicas.back().get();
}
Baker* peer_baker(Baker& b, uint32_t rank, int dev)
{
    if (rank == 0) return &b;
    std::lock_guard<std::mutex> g(b.peersMu);
    while (b.peers.size() < rank) {
        std::unique_ptr<Baker> p(new (std::nothrow) Baker());
        if (!p) return nullptr;
        p->mem = b.mem; p->log = b.log; p->type = b.type;
        p->devPool->poison = b.devPool->poison;   // (ommxBakerKnob_PoisonMemory: the owner's word, and its fills count into the owner's counters)
        b.peers.push_back(std::move(p));
    }
    Baker* p = b.peers[rank - 1].get();
    p->device.store(dev);
    for (int k = 0; k < (int)ommxBakerKnob_MAX_NUM; ++k) p->knobs[k].store(k == (int)ommxBakerKnob_Devices ? 0 : b.knobs[k].load());
    p->arenas->retain.store(b.arenas->retain.load()); p->devPool->retain.store(b.devPool->retain.load()); p->hostPool->retain.store(b.hostPool->retain.load());
    return p;
}

// rank 0's layout tables on the host: what the host scatter reads
struct HostLayout { std::vector<uint32_t> order, dstOfs, sizes, mask; std::vector<uint64_t> cofs; std::vector<uint8_t> active, owner, level; };
// One such bake: what its stages hand on, and the stages themselves in the order they run (bake_impl_multi below calls them).
struct MultiBake {
    struct Rank {
        int dev = 0; Baker* baker = nullptr; Texture* tex = nullptr; ShardedBake* sb = nullptr; PoolBlock dRaw; CodecBlock codec;
        std::vector<uint32_t> meta; const uint8_t* hStream = nullptr; bool raw = false; ommResult status = ommResult_SUCCESS;
        // on the rank's device: the sharded bake first (its session drains the rank's streams), then the pooled blocks those streams used
        ~Rank() { const DeviceScope onDev(dev); if (sb) baker->mem.destroy(sb); dRaw.release(); codec.block.release(); }
    };
    // ---- the call ----
    Baker& baker; const ommCpuBakeInputDesc& d; const Logger& L; const uint32_t N, T; const double t0 = now_ms();
    // ---- what the stages hand on ----
    int primary = -1; std::vector<Rank> ranks; RawInputLayout raw;
    RankTeam team; std::vector<uint32_t> metaSum; size_t metaWords = 0;   // the metadata words of the active items, summed across the ranks in host memory
    HostCodecLayout layout{}; uint64_t strideBytes = 0;                   // of every rank's codec stream (rank 0's say)
    double tA = 0;                                                        // the ranks are done
    MultiBake(Baker& baker_, const ommCpuBakeInputDesc& d_, uint32_t devices)
        : baker(baker_), d(d_), L(baker_.log), N(devices > (uint32_t)kMaxRanks ? (uint32_t)kMaxRanks : devices), T(d_.indexCount / 3u), ranks(N) { team.n = N; }

    // reads the baker's device and the texture; leaves per rank its device, baker and texture (made before the threads start: replicas and shadow bakers are created once and kept), the upload's layout
    ommResult setup_ranks()
    {
        primary = baker.bind_device();
        int deviceCount = 0;
        if (primary < 0 || !HIP_OK(hipGetDeviceCount(&deviceCount)) || deviceCount < 1) return L.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)");
        Texture* tex0 = untag<Texture>(d.texture);
        for (uint32_t r = 0; r < N; ++r) {
            ranks[r].dev = (primary + (int)r) % deviceCount;
            ranks[r].baker = peer_baker(baker, r, ranks[r].dev);
            ranks[r].tex = texture_on_device(tex0, ranks[r].dev);
            if (!ranks[r].baker || !ranks[r].tex) return L.failure("[Failure] - multi-device bake: could not set up a device (texture copy / memory)");
        }
        raw = raw_input_layout(d, T, max_index(d.indexBuffer, d.indexFormat, 3ull * T));
        return ommResult_SUCCESS;
    }
    // reads the caller's triangle data; leaves it on the rank's device over the rank's own link, and R.sb with the rank's share classified (R.status)
    bool upload_and_begin(Rank& R, uint32_t r)
    {
        Baker& sub = *R.baker;
        (void)R.dRaw.acquire(sub.devPool.get(), raw.total);
        const DeviceInputs din = upload_raw_inputs(raw, d, R.dRaw.bytes(), nullptr);
        if (din.texCoords == nullptr) { R.status = ommResult_FAILURE; return false; }
        ommCpuBakeInputDesc dd = d;
        dd.texture = (ommCpuTexture)((uintptr_t)R.tex | kTexture);
        dd.texCoords = din.texCoords; dd.indexBuffer = din.indices; dd.subdivisionLevels = din.perTriLevels;
        R.status = sharded_begin(&sub, &dd, r, N, false, &R.sb);
        if (R.status != ommResult_SUCCESS) R.sb = nullptr;
        return R.status == ommResult_SUCCESS;
    }
    // reads the rank's metadata words (mask, known count, digest: 4 words per active item; zero outside its share); leaves them in R.meta, rank 0 also the sum's size
    bool meta_to_host(Rank& R, uint32_t r)
    {
        const ShardCtx& c = R.sb->ctx;
        const size_t words = 4ull * c.hc.activeStart[kNumLevels];
        R.meta.resize(words ? words : 1);
        if (r == 0) { metaWords = words; metaSum.assign(words ? words : 1, 0u); }
        return !words || HIP_OK(hipMemcpy(R.meta.data(), c.tab.meta, words * 4, hipMemcpyDeviceToHost));
    }
    // reads every rank's R.meta; leaves this rank's share of metaSum
    void sum_meta_share(uint32_t r)
    {
        size_t lo, hi; meta_sum_share(metaWords, r, N, &lo, &hi);
        for (size_t k = lo; k < hi; ++k) { uint32_t a = 0; for (uint32_t q = 0; q < N; ++q) a += ranks[q].meta[k]; metaSum[k] = a; }
    }
    // reads metaSum; leaves it on the rank's device, the replicated tail and layout run, the rank's blocks packed into its contribution (R.status)
    bool meta_to_device_and_tail(Rank& R)
    {
        if (metaWords && !HIP_OK(hipMemcpy(R.sb->ctx.tab.meta, metaSum.data(), metaWords * 4, hipMemcpyHostToDevice))) return false;
        R.status = sharded_tail(R.sb);
        return R.status == ommResult_SUCCESS;
    }
    // reads the rank's contribution; leaves it in the session's pinned memory (R.hStream), as a codec stream or raw (R.raw), sent over this device's own link
    bool contribution_to_host(Rank& R, uint32_t r)
    {
        const ShardCtx& c = R.sb->ctx; hipStream_t stream = R.sb->ses.stream; CodecBlock& cb = R.codec; HostArena& pinned = R.sb->ses.set->pinned;
        if (!cb.reserve(R.baker->devPool.get(), c.strideBytes, false)) return false;   // (a multiple of 256 already: cb.padded is the stride)
        uint64_t streamBytes = 0;
        bool ok = cb.compress(c.x.contrib, stream) && HIP_OK(hipMemcpyAsync(&streamBytes, cb.at.stream, 8, hipMemcpyDeviceToHost, stream)) && HIP_OK(hipStreamSynchronize(stream));
        const RankSend send = ok ? rank_send(streamBytes, cb.cap, cb.L.offRaw, c.totals[r]) : RankSend{ false, 0 };
        R.raw = send.raw;
        ok = ok && pinned.reserve((size_t)send.bytes + 4096);
        if (ok && send.bytes) ok = HIP_OK(hipMemcpyAsync(pinned.base, R.raw ? c.x.contrib : cb.at.stream, (size_t)send.bytes, hipMemcpyDeviceToHost, stream)) && HIP_OK(hipStreamSynchronize(stream));
        R.hStream = pinned.base;
        return ok;
    }
    // One rank, on its device; every barrier of the team is here.  Reads the set-up of the ranks; leaves R.sb, R.hStream, R.raw, R.status, rank 0 also `layout` and `strideBytes`.
    void rank_phase(uint32_t r)
    {
        Rank& R = ranks[r];
        const DeviceScope onDev(R.dev);
        if (!team.barrier(upload_and_begin(R, r))) return;
        if (!team.barrier(meta_to_host(R, r))) return;
        if (!team.barrier(4ull * R.sb->ctx.hc.activeStart[kNumLevels] == metaWords)) return;   // (every rank ran the same set-up: anything else is an internal error -- and nobody may read a shorter copy)
        sum_meta_share(r);
        if (!team.barrier(true)) return;
        const bool ok = meta_to_device_and_tail(R) && contribution_to_host(R, r);
        if (r == 0) { layout = R.codec.L; strideBytes = R.codec.padded; }
        (void)team.barrier(ok);
    }
    // reads the ranks' set-up; leaves every rank's phase run -- rank 0 on the calling thread, the others on a thread each -- and `tA`
    ommResult run_team()
    {
        // (nothing may leave a rank's thread: an exception -- std::bad_alloc of a host vector -- fails the rank and releases the others from their barriers)
        auto guardedPhase = [this](uint32_t r) { try { rank_phase(r); } catch (...) { ranks[r].status = ommResult_FAILURE; team.abort(); } };
        // a rank whose thread cannot be started is run by the caller AFTER the others would deadlock the barriers: refuse instead
        std::vector<std::thread> threads;
        bool spawned = true;
        try { threads.reserve(N); for (uint32_t r = 1; r < N; ++r) threads.emplace_back(guardedPhase, r); } catch (...) { spawned = false; }
        if (!spawned) {
            team.abort();   // (threads that did start wait in the first barrier for ranks that never come)
            for (auto& t : threads) t.join();
            return L.failure("[Failure] - multi-device bake: could not start a thread per device");
        }
        guardedPhase(0);
        for (auto& t : threads) t.join();
        for (const Rank& R : ranks) if (R.status != ommResult_SUCCESS) return R.status;
        for (const Rank& R : ranks) if (!R.sb || !R.hStream) return L.failure("[Failure] - multi-device bake: a device failed");
        tA = now_ms();
        return ommResult_SUCCESS;
    }
    // reads rank 0's tail outputs; leaves its layout tables in `lay` and descriptors, index buffer and histograms in `dres` (sharded_finish synchronises the stream: the copies into `lay` are complete)
    ommResult read_layout(HostLayout& lay, DeviceResultOwner& dres)
    {
        ShardedBake* sb0 = ranks[0].sb; const ShardCtx& c0 = sb0->ctx; hipStream_t stream0 = sb0->ses.stream;
        const uint32_t E = c0.counts.numOmms, U = c0.ti.numItems;
        lay.order.resize(E ? E : 1); lay.dstOfs.resize(E ? E : 1); lay.sizes.resize(E ? E : 1); lay.cofs.resize(E ? E : 1);
        lay.mask.resize(U ? U : 1); lay.active.resize(U ? U : 1); lay.owner.resize(U ? U : 1); lay.level.resize(U ? U : 1);
        bool ok = true;
        if (E) ok = HIP_OK(hipMemcpyAsync(lay.order.data(), c0.to.order, (size_t)E * 4, hipMemcpyDeviceToHost, stream0)) && HIP_OK(hipMemcpyAsync(lay.dstOfs.data(), c0.to.dstOfs, (size_t)E * 4, hipMemcpyDeviceToHost, stream0))
                  && HIP_OK(hipMemcpyAsync(lay.sizes.data(), c0.to.sizes, (size_t)E * 4, hipMemcpyDeviceToHost, stream0)) && HIP_OK(hipMemcpyAsync(lay.cofs.data(), c0.tab.cofs, (size_t)E * 8, hipMemcpyDeviceToHost, stream0));
        if (ok && U) ok = HIP_OK(hipMemcpyAsync(lay.active.data(), c0.tab.active, U, hipMemcpyDeviceToHost, stream0)) && HIP_OK(hipMemcpyAsync(lay.owner.data(), c0.tab.owner, U, hipMemcpyDeviceToHost, stream0))
                       && HIP_OK(hipMemcpyAsync(lay.level.data(), c0.tab.level, U, hipMemcpyDeviceToHost, stream0)) && HIP_OK(hipMemcpyAsync(lay.mask.data(), c0.tab.mask, (size_t)U * 4, hipMemcpyDeviceToHost, stream0));
        if (!ok) return L.failure("[Failure] - device to host transfer of the bake result failed");
        ommxDeviceBakeResult made = nullptr;
        const ommResult fr = sharded_finish(sb0, [](uint8_t*) { return true; }, &made, false);
        dres.p = (DeviceBakeResult*)made;
        return fr;
    }
    // reads `lay` and every rank's stream; leaves every block of res->arrayData written from its owner's stream: OMM ranges of ~2 MiB each to the helper threads.  Returns the threads used.
    uint32_t scatter_on_host(const HostLayout& lay, BakeResult* res)
    {
        HostScatter S; memset(&S, 0, sizeof S);
        S.world = N; S.L = layout; S.bits = ranks[0].sb->ctx.bits;
        for (uint32_t r = 0; r < N; ++r) { S.stream[r] = ranks[r].hStream; S.raw[r] = ranks[r].raw; }
        S.active = lay.active.data(); S.owner = lay.owner.data(); S.level = lay.level.data(); S.stateMask = lay.mask.data(); S.order = lay.order.data(); S.dstOfs = lay.dstOfs.data();
        S.sizes = lay.sizes.data(); S.cofs = lay.cofs.data(); S.arrayData = (uint8_t*)res->arrayData;
        const std::vector<uint32_t> cut = scatter_cuts(lay.sizes.data(), ranks[0].sb->ctx.counts.numOmms);
        const std::shared_ptr<WorkerPool> pool = baker.worker_pool(expand_thread_count(baker));
        if (baker.knob(ommxBakerKnob_HelperAffinity) == 0) (void)pool->bind_near(res->arrayData);
        pool->run((uint32_t)cut.size() - 1u, [&](uint32_t t) { codec_scatter_omms(S, cut[t], cut[t + 1]); });
        return pool->workers() + 1u;
    }
    // reads `lay`, `dr` and the ranks' streams; leaves the caller's result -- arrays, blocks, histograms -- and the baker's timings
    ommResult deliver(const HostLayout& lay, DeviceBakeResult* dr, ommCpuBakeResult* out)
    {
        const ShardCtx& c0 = ranks[0].sb->ctx; hipStream_t stream0 = ranks[0].sb->ses.stream;
        DeviceResult& DR = dr->R; const uint32_t E = c0.counts.numOmms;
        HostResultGuard resGuard{ baker, baker.mem.make<BakeResult>(), nullptr };
        BakeResult* const res = resGuard.r;
        if (!res) return ommResult_FAILURE;
        res->mem = baker.mem;
        const StreamDrain drainBeforeResult{ stream0 };   // (right behind the memory it protects, like the one in front of `lay`)
        if (E && baker.mem.alloc == default_alloc && baker.hostPool->wants((size_t)DR.arrayDataSize)) { res->arrayData = baker.hostPool->acquire((size_t)DR.arrayDataSize); if (res->arrayData) res->pool = baker.hostPool; }
        if (alloc_host_result(baker, res, E, (size_t)DR.arrayDataSize, T) != ommResult_SUCCESS) return ommResult_FAILURE;
        bool ok = copy_small_arrays(res, DR.descs, DR.index, c0.tab.triArea, E, T, index_bytes(DR.indexFormat), stream0);
        // the blocks, while the small arrays above are on their way
        const uint32_t threadsUsed = ok && E ? scatter_on_host(lay, res) : 1u;
        ok = ok && HIP_OK(hipStreamSynchronize(stream0));
        if (!ok) return L.failure("[Failure] - device to host transfer of the bake result failed");
        memcpy(res->arrayHist, dr->arrayHist, sizeof(ommCpuOpacityMicromapUsageCount) * 2 * kNumLevels);
        memcpy(res->indexHist, dr->indexHist, sizeof(ommCpuOpacityMicromapUsageCount) * 2 * kNumLevels);
        fill_result_desc(&res->desc, res->arrayData, DR.arrayDataSize, res->descs, E, res->index, T, DR.indexFormat, res->arrayHist, dr->desc.descArrayHistogramCount, res->indexHist, dr->desc.indexHistogramCount);
        {
            std::lock_guard<std::mutex> g(baker.timingsMu);   // (sharded_finish stored rank 0's phase clocks)
            uint64_t wire = 0; for (uint32_t r = 0; r < N; ++r) wire += ranks[r].raw ? c0.totals[r] : (ranks[r].hStream ? *(const uint64_t*)ranks[r].hStream : 0);
            baker.timings.devices = N; baker.timings.resultTransfer = ommxResultTransfer_Compressed; baker.timings.compressedBytes = wire; baker.timings.expandThreads = threadsUsed;
            baker.timings.expandMs = (float)(now_ms() - tA); baker.timings.totalMs = (float)(now_ms() - t0); baker.timings.contributionBytes = strideBytes;
        }
        *out = (ommCpuBakeResult)resGuard.release();
        return ommResult_SUCCESS;
    }
};

ommResult bake_impl_multi(Baker& baker, const ommCpuBakeInputDesc& d, ommCpuBakeResult* out, uint32_t N)
{
    MultiBake m(baker, d, N);
    // phase A (all ranks): upload, share of the classification, metadata through the host, tail, own contribution as a codec stream on the host
    ommResult r = m.setup_ranks();
    if (r == ommResult_SUCCESS) r = m.run_team();
    if (r != ommResult_SUCCESS) return r;
    // rank 0: layout tables to the host, descriptors / index buffer / histograms, then the blocks from their owners' streams.
    // Asynchronous copies into `lay` (and, in deliver, into the result's arrays) are queued on rank 0's stream: whatever way this function is left -- a failed
    // copy half way down a chain, an exception of a host container or of the thread pool -- the stream is drained BEFORE their memory is released
    // (destructors run in reverse order of declaration: each guard is declared right behind the memory it protects).
    const DeviceScope onPrimary(m.primary);
    HostLayout lay;
    const StreamDrain drainBeforeVectors{ m.ranks[0].sb->ses.stream };
    DeviceResultOwner dres(baker.mem, nullptr);   // (no drain of its own: deliver's guard has drained the stream when this one goes)
    r = m.read_layout(lay, dres);
    return r != ommResult_SUCCESS ? r : m.deliver(lay, dres.p, out);
}
} // namespace

OMM_MI355X_API ommResult ommxShardedBegin(ommBaker baker, const ommCpuBakeInputDesc* desc, uint32_t rank, uint32_t worldSize, ommxShardedBake* out)
{
    Baker* b = nullptr;
    if (out == 0) return ommResult_INVALID_ARGUMENT;
    const ommResult r = sharded_checks(baker, desc, &b, false);
    if (r != ommResult_SUCCESS) return r;
    if (!rank_in_world(rank, worldSize)) return b->log.invalid("[Invalid Argument] - rank / worldSize out of range (at most 16 ranks)");
    return guarded(&b->log, [&]() -> ommResult {
        const DeviceScope onBakersDevice(b->bind_device());
        ShardedBake* sb = nullptr;
        const ommResult rr = sharded_begin(b, desc, rank, worldSize, false, &sb);
        if (rr == ommResult_SUCCESS) *out = (ommxShardedBake)sb;
        return rr;
    });
}

OMM_MI355X_API ommResult ommxShardedGetMeta(ommxShardedBake h, void** deviceWords, uint64_t* numWords)
{
    if (h == 0 || deviceWords == nullptr || numWords == nullptr) return ommResult_INVALID_ARGUMENT;
    ShardedBake* sb = (ShardedBake*)h;
    *deviceWords = sb->ctx.tab.meta; *numWords = 4ull * sb->ctx.hc.activeStart[kNumLevels];
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommxShardedTail(ommxShardedBake h, void** contribution, uint64_t* contributionBytes, uint64_t* strideBytes)
{
    if (h == 0 || contribution == nullptr || contributionBytes == nullptr || strideBytes == nullptr) return ommResult_INVALID_ARGUMENT;
    ShardedBake* sb = (ShardedBake*)h; ShardCtx& c = sb->ctx;
    return guarded(&sb->baker->log, [&]() -> ommResult {
        const DeviceScope onBakersDevice(sb->baker->bind_device());
        const double t1 = now_ms();
        const ommResult r = sharded_tail(sb);   // (a second call re-uses the same exchange block: nothing leaks)
        if (r != ommResult_SUCCESS) return r;
        if (!HIP_OK(hipStreamSynchronize(sb->ses.stream))) return sb->baker->log.failure("[Failure] - shard gather failed");
        *contribution = c.x.contrib; *contributionBytes = c.totals[c.rank]; *strideBytes = c.strideBytes;
        sb->tm.tailMs = (float)(now_ms() - t1);
        return ommResult_SUCCESS;
    });
}

OMM_MI355X_API ommResult ommxShardedFinish(ommxShardedBake h, const void* gathered, ommxDeviceBakeResult* outResult)
{
    if (h == 0 || outResult == nullptr) return ommResult_INVALID_ARGUMENT;
    ShardedBake* sb = (ShardedBake*)h; ShardCtx& c = sb->ctx;
    if (c.counts.numOmms && gathered == nullptr) return sb->baker->log.invalid("[Invalid Argument] - gathered contributions missing");
    return guarded(&sb->baker->log, [&]() -> ommResult {
        const DeviceScope onBakersDevice(sb->baker->bind_device());
        const double t1 = now_ms();
        const ommResult r = sharded_finish(sb, [&](uint8_t* arrayData) {
            if (!arrayData) return false;   // (the result could not be allocated)
            // the chunk walk of the RCCL path (there each chunk arrives separately)
            for (ShardChunks w(c.strideBytes, sb->baker->knob(ommxBakerKnob_ShardChunkBytes)); w.next();)
                shard_scatter(c, (const uint8_t*)gathered + w.lo, c.strideBytes, w.lo, w.hi, arrayData, sb->ses.stream);
            return true;
        }, outResult);
        sb->tm.gatherMs = (float)(now_ms() - t1);
        return r;
    });
}

OMM_MI355X_API ommResult ommxShardedDestroy(ommxShardedBake h)
{
    if (h == 0) return ommResult_INVALID_ARGUMENT;
    ShardedBake* sb = (ShardedBake*)h;
    const Allocator mem = sb->mem;
    mem.destroy(sb);   // (the session waits for its streams before its working set returns to the baker's pool)
    return ommResult_SUCCESS;
}

// ---- RCCL communicator helpers + the one-call sharded bake ----
OMM_MI355X_API ommResult ommxRcclGetUniqueId(void* outId, size_t idBytes)
{
    if (outId == nullptr || idBytes < sizeof(RcclUniqueId)) return ommResult_INVALID_ARGUMENT;
    if (!rccl().ok()) return ommResult_FAILURE;
    return rccl().getUniqueId((RcclUniqueId*)outId) == 0 ? ommResult_SUCCESS : ommResult_FAILURE;
}

// The one way a communicator handle is made: `fill` sets what the entry knows (a failure of it is the entry's answer), the status words follow.
template <class Fill> static ommResult make_comm(ommxRcclComm* outComm, Fill&& fill)
{
    RcclComm* c = new (std::nothrow) RcclComm();
    if (!c) return ommResult_FAILURE;
    const ommResult r = fill(*c);
    if (r != ommResult_SUCCESS) { delete c; return r; }
    rccl_prepare_status(c);
    *outComm = (ommxRcclComm)c;
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommxRcclCommInitRank(const void* id, size_t idBytes, uint32_t rank, uint32_t worldSize, ommxRcclComm* outComm)
{
    if (id == nullptr || idBytes < sizeof(RcclUniqueId) || outComm == nullptr || !rank_in_world(rank, worldSize)) return ommResult_INVALID_ARGUMENT;
    if (!rccl().ok()) return ommResult_FAILURE;
    RcclUniqueId uid; memcpy(&uid, id, sizeof uid);
    return make_comm(outComm, [&](RcclComm& c) {
        if (rccl().commInitRank(&c.comm, (int)worldSize, uid, (int)rank) != 0) return ommResult_FAILURE;
        c.owned = true; c.rank = (int)rank; c.world = (int)worldSize;
        return ommResult_SUCCESS;
    });
}

OMM_MI355X_API ommResult ommxRcclCommWrap(void* ncclComm, ommxRcclComm* outComm)
{
    if (ncclComm == nullptr || outComm == nullptr) return ommResult_INVALID_ARGUMENT;
    if (!rccl().ok()) return ommResult_FAILURE;
    return make_comm(outComm, [&](RcclComm& c) {
        c.comm = ncclComm; c.owned = false;
        const bool known = rccl().commCount(c.comm, &c.world) == 0 && rccl().commUserRank(c.comm, &c.rank) == 0 && c.world >= 1 && c.world <= kMaxRanks;
        return known ? ommResult_SUCCESS : ommResult_INVALID_ARGUMENT;
    });
}

OMM_MI355X_API ommResult ommxCommFromCollectives(const ommxCollectives* collectives, uint32_t rank, uint32_t worldSize, ommxRcclComm* outComm)
{
    if (collectives == nullptr || collectives->allReduceU32 == nullptr || collectives->allGatherBytes == nullptr || outComm == nullptr || !rank_in_world(rank, worldSize)) return ommResult_INVALID_ARGUMENT;
    return make_comm(outComm, [&](RcclComm& c) {
        c.custom = true; c.user = *collectives; c.rank = (int)rank; c.world = (int)worldSize;
        return ommResult_SUCCESS;
    });
}

OMM_MI355X_API ommResult ommxRcclCommInfo(ommxRcclComm comm, uint32_t* outRank, uint32_t* outWorldSize)
{
    if (comm == 0 || outRank == nullptr || outWorldSize == nullptr) return ommResult_INVALID_ARGUMENT;
    RcclComm* c = (RcclComm*)comm;
    int rank = c->rank, world = c->world;
    if (!c->custom && c->comm && rccl().ok() && (rccl().commCount(c->comm, &world) != 0 || rccl().commUserRank(c->comm, &rank) != 0)) return ommResult_FAILURE;
    *outRank = (uint32_t)rank; *outWorldSize = (uint32_t)world;
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommxRcclCommDestroy(ommxRcclComm comm)
{
    if (comm == 0) return ommResult_INVALID_ARGUMENT;
    RcclComm* c = (RcclComm*)comm;
    if (c->statusStream) { (void)hipStreamSynchronize(c->statusStream); (void)hipStreamDestroy(c->statusStream); }
    if (c->dStatus) (void)hipFree(c->dStatus);
    if (c->owned && c->comm) (void)rccl().commDestroy(c->comm);
    delete c;
    return ommResult_SUCCESS;
}

namespace {
// One ommxShardedBakeRccl: what its stages hand on, and the stages themselves in the order they run.  Collectives that every rank must enter are
// preceded by an agreement (rccl_agree): a rank that failed answers with its own code, one that stops for another's sake with FAILURE (stopped).
struct RcclBake {
    // ---- the call ----
    Baker* const b; const ommCpuBakeInputDesc& desc; RcclComm* const rc; const Logger& L; const bool hostTail;
    // ---- what the stages hand on ----
    ShardedBake* sb = nullptr; hipStream_t stream = nullptr;   // the bake, this object's to destroy, and its stream
    double t1 = 0;                                             // the ranks' shares are classified
    RcclBake(Baker* b_, const ommCpuBakeInputDesc& desc_, RcclComm* rc_) : b(b_), desc(desc_), rc(rc_), L(b_->log), hostTail(wants_host_tail(desc_)) {}
    RcclBake(const RcclBake&) = delete; RcclBake& operator=(const RcclBake&) = delete;
    ~RcclBake() { if (sb) b->mem.destroy(sb); }
    ommResult nccl_fail(int code, const char* what) const { char buf[256]; snprintf(buf, sizeof buf, "[Failure] - %s: %s", what, rc->error_string(code)); return L.failure(buf); }
    static ommResult stopped(ommResult mine) { return mine != ommResult_SUCCESS ? mine : ommResult_FAILURE; }

    // reads the call; leaves `sb` with this rank's share classified and its metadata packed (nothing synchronised), and every rank's word that it got that far
    ommResult begin()
    {
        const ommResult r = sharded_begin(b, &desc, (uint32_t)rc->rank, (uint32_t)rc->world, true, &sb, hostTail);
        if (r != ommResult_SUCCESS) sb = nullptr;
        if (!rccl_agree(rc, sb ? sb->ses.stream : nullptr, r == ommResult_SUCCESS, L, "classification of its share")) return stopped(r);
        stream = sb->ses.stream; t1 = now_ms();
        return ommResult_SUCCESS;
    }
    // The opt-in lossy reducers (near-duplicate merge, maxArrayDataSize): the serial reference algorithms need the states of ALL work items.  Every rank
    // classified its share into a zeroed buffer, so SUM all-reduces of the metadata words and of the packed states merge them; each rank then runs the
    // identical serial tail on the host and uploads the (identical) result.  Reads the ranks' shares; leaves the result and the baker's timings.
    ommResult host_tail(ommxDeviceBakeResult* outResult)
    {
        ShardCtx& c = sb->ctx;
        const size_t words = 4ull * c.hc.activeStart[kNumLevels], stateWords = (size_t)(c.hc.stateBytes / 4);
        int e = words ? rc->all_reduce(c.tab.meta, c.tab.meta, words, kRcclSum, stream) : 0;
        if (e == 0 && stateWords) e = rc->all_reduce(c.dStates, c.dStates, stateWords, kRcclSum, stream);
        if (e != 0) return nccl_fail(e, "ncclAllReduce of the micro-triangle states");
        launch_shard_unpack_meta(c.bounds, c.tab.activeIds, c.hc.activeStart[kNumLevels], c.tab.meta, c.tab.mask, (uint32_t*)c.ti.knownCount, c.ti.digests, c.tab.owner, stream);
        std::vector<HostItem> items;
        ommResult r = gather_host_items(L, stream, c.ti.numItems, c.T, c.hc, c.ti.uv, c.tab.level, c.tab.active, c.tab.mask, c.tab.stateOfs, c.dStates, c.ti.triToItem, c.bits, items);
        HostTailResult hres; ommIndexFormat ifmt = ommIndexFormat_UINT_32;
        if (r == ommResult_SUCCESS) r = run_host_tail_for(desc, c.T, items, hres, ifmt);
        if (r != ommResult_SUCCESS) return r;
        DeviceResultOwner res(b->mem, stream);
        if (!res.make()) return ommResult_FAILURE;
        r = upload_host_tail(*b, hres, ifmt, c.T, c.bits, stream, res.p);
        if (r != ommResult_SUCCESS) return r;
        sb->tm.tailMs = (float)(now_ms() - t1);
        store_begin_timings(sb, false);
        *outResult = (ommxDeviceBakeResult)res.release();
        return ommResult_SUCCESS;
    }
    // exchange 1.  Reads the metadata words of this rank's share; leaves every rank's, by a SUM all-reduce in place on the bake's own stream right behind the digests
    ommResult exchange_meta()
    {
        ShardCtx& c = sb->ctx;
        const size_t words = 4ull * c.hc.activeStart[kNumLevels];
        const int e = words ? rc->all_reduce(c.tab.meta, c.tab.meta, words, kRcclSum, stream) : 0;
        return e != 0 ? nccl_fail(e, "ncclAllReduce of the work-item metadata") : ommResult_SUCCESS;
    }
    // reads the summed metadata; leaves the replicated tail run, this rank's contribution packed, and every rank's word that it got that far
    ommResult tail()
    {
        const ommResult r = sharded_tail(sb);
        if (!rccl_agree(rc, stream, r == ommResult_SUCCESS, L, "tail of the bake")) return stopped(r);
        sb->tm.tailMs = (float)(now_ms() - t1);
        return ommResult_SUCCESS;
    }
    // exchange 2.  Reads the ranks' contributions; leaves the result (sharded_finish, with scatter_blocks for the array) and the exchange's fields of the baker's timings
    ommResult exchange_blocks(ommxDeviceBakeResult* outResult)
    {
        const double t2 = now_ms();
        const ommResult r = sharded_finish(sb, [this](uint8_t* arrayData) { return scatter_blocks(arrayData); }, outResult);
        sb->tm.gatherMs = (float)(now_ms() - t2);
        if (r == ommResult_SUCCESS) { std::lock_guard<std::mutex> g(b->timingsMu); b->timings.tailMs = sb->tm.tailMs; b->timings.gatherMs = sb->tm.gatherMs; b->timings.exchangeBytes = sb->tm.exchangeBytes; b->timings.contributionBytes = sb->tm.contributionBytes; }
        return r;
    }
    // Reads this rank's contribution; leaves every rank's blocks at their final offsets in arrayData -- null when this rank could not allocate the result: it
    // still takes part in the agreement, so that nobody waits for it.  (A one-rank communicator takes the same route: the collectives degenerate to copies.)
    // The contribution becomes a codec stream (tail_kernels.hip "block exchange codec"), and the agreement on the ranks' status carries the stream sizes:
    // MAX over the ranks = what every rank sends (the all-gather needs equal counts), or "one of them does not shrink" = everybody sends raw.
    bool scatter_blocks(uint8_t* arrayData)
    {
        ShardCtx& c = sb->ctx;
        EventList<1 + kShardMaxChunks> evs;   // contribution ready | chunk k gathered: they go with this scope, behind the last wait on either stream
        bool ok = arrayData != nullptr && sb->ses.open_comm() && evs.create(1);
        ok = ok && HIP_OK(run_shard_compress(c.x.contrib, c.strideBytes, c.x.comp, c.x.compCap, c.x.compSize, c.x.codecScratch, c.x.codecScratchBytes, stream));
        uint32_t maxUnits = 0;
        ok = rccl_agree(rc, stream, ok, L, "allocation of the result", c.x.compSize, &maxUnits) && ok;
        if (!ok) return false;
        sb->tm.contributionBytes = c.strideBytes;
        return maxUnits != kCodecIncompressible ? blocks_as_streams((size_t)maxUnits * 16u, arrayData) : blocks_raw_in_chunks(evs, arrayData);
    }
    // reads this rank's codec stream, `sendBytes` of it (<= compCap by construction); leaves the blocks placed, the stream synchronised
    bool blocks_as_streams(size_t sendBytes, uint8_t* arrayData)
    {
        ShardCtx& c = sb->ctx;
        sb->tm.exchangeBytes = sendBytes;
        const int e = rc->all_gather(c.x.comp, c.x.gatherComp, sendBytes, stream);
        if (e != 0) { (void)nccl_fail(e, "ncclAllGather of the OMM blocks"); return false; }
        shard_scatter_streams(c, sendBytes, arrayData, stream);
        return HIP_OK(hipGetLastError()) && HIP_OK(hipStreamSynchronize(stream));
    }
    // Reads the padded contributions, all-gathered in chunks on the communication stream: every chunk is scattered to its final arrayData offsets on the bake's
    // stream while the next one is on the wire.  Leaves the blocks placed and BOTH streams synchronised, also when a step failed.
    bool blocks_raw_in_chunks(EventList<1 + kShardMaxChunks>& evs, uint8_t* arrayData)
    {
        ShardCtx& c = sb->ctx; hipStream_t cs = sb->ses.commStream;
        sb->tm.exchangeBytes = c.strideBytes;
        bool ok = HIP_OK(hipEventRecord(evs.ev[0], stream)) && HIP_OK(hipStreamWaitEvent(cs, evs.ev[0], 0));
        int ncclErr = 0; uint32_t k = 0;
        for (ShardChunks w(c.strideBytes, b->knob(ommxBakerKnob_ShardChunkBytes)); ok && w.next(); ++k) {
            uint8_t* stage = c.x.gathered + w.lo * (uint64_t)rc->world;               // chunk k of all ranks: world x (hi - lo) bytes
            ncclErr = rc->all_gather(c.x.contrib + w.lo, stage, (size_t)(w.hi - w.lo), cs);
            ok = ncclErr == 0 && evs.create(k + 2u) && HIP_OK(hipEventRecord(evs.ev[k + 1u], cs)) && HIP_OK(hipStreamWaitEvent(stream, evs.ev[k + 1u], 0));
            if (ok) shard_scatter(c, stage, w.hi - w.lo, w.lo, w.hi, arrayData, stream);
        }
        ok = ok && HIP_OK(hipStreamSynchronize(stream));
        (void)hipStreamSynchronize(cs);
        if (ncclErr != 0) (void)nccl_fail(ncclErr, "ncclAllGather of the OMM blocks");
        return ok;
    }
};
} // namespace

OMM_MI355X_API ommResult ommxShardedBakeRccl(ommBaker baker, const ommCpuBakeInputDesc* desc, ommxRcclComm comm, ommxDeviceBakeResult* outResult)
{
    Baker* b = nullptr;
    if (comm == 0 || outResult == nullptr) return ommResult_INVALID_ARGUMENT;
    const ommResult r0 = sharded_checks(baker, desc, &b, true);
    if (r0 != ommResult_SUCCESS) return r0;
    const Logger& L = b->log;
    RcclComm* rc = (RcclComm*)comm;
    if (!rc->custom && !rccl().ok()) return L.failure(("[Failure] - RCCL is not available: " + rccl().error).c_str());
    return guarded(&L, [&]() -> ommResult {
        const DeviceScope onBakersDevice(b->bind_device());
        rccl_status_on_device(rc, b->bind_device());          // (status words / idle-rank stream on the bake's device, whatever was current when the communicator was made)
        RcclBake run(b, *desc, rc);
        ommResult r = run.begin();
        if (r != ommResult_SUCCESS) return r;
        if (run.hostTail) return run.host_tail(outResult);
        r = run.exchange_meta();
        if (r == ommResult_SUCCESS) r = run.tail();
        return r != ommResult_SUCCESS ? r : run.exchange_blocks(outResult);
    });
}

OMM_MI355X_API ommResult ommxGetDeviceBakeResultDesc(ommxDeviceBakeResult result, const ommCpuBakeResultDesc** desc)
{
    if (result == 0 || desc == nullptr) return ommResult_INVALID_ARGUMENT;
    *desc = &((DeviceBakeResult*)result)->desc;
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommxDestroyDeviceBakeResult(ommxDeviceBakeResult result)
{
    if (result == 0) return ommResult_INVALID_ARGUMENT;
    DeviceBakeResult* r = (DeviceBakeResult*)result;
    const Allocator mem = r->mem;
    mem.destroy(r);
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommxGetDeviceBakeResultTriangleAreas(ommxDeviceBakeResult result, const float** deviceAreas)
{
    if (result == 0 || deviceAreas == nullptr) return ommResult_INVALID_ARGUMENT;
    *deviceAreas = ((DeviceBakeResult*)result)->R.triArea;
    return ommResult_SUCCESS;
}

// ommDebugStats of a result whose arrays are device memory (include/omm_mi355x_ext.h; kernels in stats_kernels.hip): the integer fields are
// collect_stats' own, 32-bit products included; the area metric is the same quantity summed in fp64 in a fixed order.
namespace {
ommResult stats_device(Baker& b, const ommCpuBakeResultDesc& r, const float* areas, const ommxDeviceStatsOutputs* outputs, ommDebugStats* out,
                       uint32_t* outSkipped, hipStream_t stream)
{
    if (!is_index_format(r.indexFormat)) return ommResult_INVALID_ARGUMENT;
    ommDebugStats st; memset(&st, 0, sizeof st);
    if (r.indexCount == 0) {   // nothing to launch; the host's 0 / 0 where areas were handed in
        if (areas) { const float zero = 0.f; st.knownAreaMetric = zero / zero; }
        *out = st; if (outSkipped) *outSkipped = 0;
        return ommResult_SUCCESS;
    }
    if (has_null_array(r)) return ommResult_INVALID_ARGUMENT;
    StatsArgs a; a.result = r; a.areas = areas;
    a.stateCounts = outputs ? outputs->stateCounts : nullptr; a.referenceCounts = outputs ? outputs->referenceCounts : nullptr;
    a.knownFraction = outputs ? outputs->knownFraction : nullptr;
    const DeviceScope onBakersDevice(b.device.load());   // (a baker that has no device yet works on the caller's current one)
    const PoolBlock scratch(b.devPool.get(), stats_scratch_bytes(a));
    if (!scratch.p) return b.log.failure("[Failure] - out of device memory for the statistics scratch");
    StatsTotals t;
    if (launch_stats(a, scratch.p, &t, stream) != hipSuccess) {
        (void)hipGetLastError(); (void)hipStreamSynchronize(stream);   // (the scratch goes back only when nothing can still touch it)
        return b.log.failure("[Failure] - the statistics kernels could not run");
    }
    st.totalTransparent = t.state[0]; st.totalOpaque = t.state[1]; st.totalUnknownTransparent = t.state[2]; st.totalUnknownOpaque = t.state[3];
    st.totalFullyTransparent = t.special[0]; st.totalFullyOpaque = t.special[1]; st.totalFullyUnknownTransparent = t.special[2]; st.totalFullyUnknownOpaque = t.special[3];
    st.knownAreaMetric = areas ? (float)(t.knownArea / t.totalArea) : 0.f;
    *out = st; if (outSkipped) *outSkipped = t.skipped;
    return ommResult_SUCCESS;
}
}

OMM_MI355X_API ommResult ommxDebugGetStatsDevice(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const float* deviceTriangleAreas,
                                                 const ommxDeviceStatsOutputs* outputs, ommDebugStats* out, uint32_t* outSkippedPrimitives, void* hipStream)
{
    Baker* b = baker_for_device_results(baker);
    if (!b || deviceResult == nullptr || out == nullptr) return ommResult_INVALID_ARGUMENT;
    return guarded(&b->log, [&] { return stats_device(*b, *deviceResult, deviceTriangleAreas, outputs, out, outSkippedPrimitives, (hipStream_t)hipStream); });
}

OMM_MI355X_API ommResult ommxDebugGetStatsDevice2(ommBaker baker, ommxDeviceBakeResult result, ommDebugStats* out)
{
    if (result == 0) return ommResult_INVALID_ARGUMENT;
    const DeviceBakeResult* r = (const DeviceBakeResult*)result;
    return ommxDebugGetStatsDevice(baker, &r->desc, r->R.triArea, nullptr, out, nullptr, nullptr);
}

// Opacity-sorted nodes of the bird curve from a result whose arrays are device memory (include/omm_mi355x_ext.h; kernels in geometry_kernels.hip): count,
// judge the caller's capacities on the host, then write -- so that a call that fails for capacity has written nothing.
namespace {
ommResult extract_geometry(Baker& b, const ommCpuBakeResultDesc& r, const ommxMicroGeometryDesc& g, const ommxMicroGeometryOutputs* outputs, uint64_t outCounts[4],
                           uint32_t* outSkipped, hipStream_t stream)
{
    if (!is_index_format(r.indexFormat)) return b.log.invalid("[Invalid Arg] - deviceResult.indexFormat is not an index format");
    GeoArgs a; memset(&a, 0, sizeof a);
    for (int s = 0; s < 5; ++s) {
        const uint8_t v = s < 4 ? g.listOfState[s] : g.mixedList;
        if (v > 3 && v != OMMX_GEOMETRY_DROP) return b.log.invalid(s < 4 ? "[Invalid Arg] - listOfState must name a list 0..3 or OMMX_GEOMETRY_DROP" : "[Invalid Arg] - mixedList must name a list 0..3 or OMMX_GEOMETRY_DROP");
        (s < 4 ? a.cls[s] : a.mixed) = v == OMMX_GEOMETRY_DROP ? (uint8_t)kGeoDrop : v;
    }
    if (g.reserved[0] || g.reserved[1] || g.reserved[2]) return b.log.invalid("[Invalid Arg] - ommxMicroGeometryDesc.reserved must be 0");
    a.result = r; a.emitLevel = g.maxEmitLevel < kResultMaxLevel ? g.maxEmitLevel : kResultMaxLevel;
    for (int k = 0; k < 4; ++k) outCounts[k] = 0;
    if (outSkipped) *outSkipped = 0;
    if (r.indexCount == 0) return ommResult_SUCCESS;   // nothing to launch
    if (has_null_array(r)) return b.log.invalid("[Invalid Arg] - deviceResult has a null array with a non-zero count");
    if (!usable_device()) return b.log.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)");
    const DeviceScope onBakersDevice(b.device.load());   // (a baker that has no device yet works on the caller's current one)
    PoolBlock head(b.devPool.get(), geo_head_bytes(a)), tiles;
    if (!head.p) return b.log.failure("[Failure] - out of device memory for the geometry scratch");
    // (after a failed launch the scratch goes back only when nothing can still touch it)
    const auto failed = [&] { (void)hipGetLastError(); (void)hipStreamSynchronize(stream); return b.log.failure("[Failure] - the geometry kernels could not run"); };
    unsigned long long tileCount = 0;
    if (geo_count_tiles(a, head.p, &tileCount, stream) != hipSuccess) return failed();
    if (tileCount) {
        if (!tiles.acquire(b.devPool.get(), geo_tile_bytes(tileCount))) return b.log.failure("[Failure] - out of device memory for the geometry scratch");
    }
    bool wantNodes = false, wantAny = false;
    if (outputs) for (int k = 0; k < 4; ++k) { wantNodes = wantNodes || outputs->nodes[k]; wantAny = wantAny || outputs->nodes[k] || outputs->primitiveOffsets[k]; }
    GeoTotals t;
    if (geo_count(a, head.p, tiles.p, tileCount, wantNodes, &t, stream) != hipSuccess) return failed();
    for (int k = 0; k < 4; ++k) outCounts[k] = t.counts[k];
    if (outSkipped) *outSkipped = t.skipped;
    if (!wantAny) return ommResult_SUCCESS;
    for (int k = 0; k < 4; ++k)
        if (outputs->nodes[k] && outputs->capacity[k] < t.counts[k]) {
            b.log.msg(ommMessageSeverity_Fatal, "[Failure] - ommxMicroGeometryOutputs.capacity is smaller than the list's record count (see outCounts); nothing was written");
            return ommResult_INSUFFICIENT_SCRATCH_MEMORY;
        }
    if (geo_emit(a, head.p, tiles.p, tileCount, t, *outputs, stream) != hipSuccess) return failed();
    return ommResult_SUCCESS;
}
}

OMM_MI355X_API ommResult ommxExtractMicroGeometry(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxMicroGeometryDesc* desc,
                                                  const ommxMicroGeometryOutputs* outputs, uint64_t outCounts[4], uint32_t* outSkippedPrimitives, void* hipStream)
{
    Baker* b = baker_for_device_results(baker);
    if (!b) return ommResult_INVALID_ARGUMENT;
    if (deviceResult == nullptr) return b->log.invalid("[Invalid Arg] - deviceResult was not set");
    if (desc == nullptr) return b->log.invalid("[Invalid Arg] - ommxMicroGeometryDesc was not set");
    if (outCounts == nullptr) return b->log.invalid("[Invalid Arg] - outCounts was not set");
    return guarded(&b->log, [&] { return extract_geometry(*b, *deviceResult, *desc, outputs, outCounts, outSkippedPrimitives, (hipStream_t)hipStream); });
}

// A device-resident result capped at a subdivision level, for all blocks alike or block by block (include/omm_mi355x_ext.h; kernels in
// coarsen_kernels.hip): read the index buffer, size the staging arena, reduce and compare, judge the output's size on the host, then allocate the new
// result's arrays and fill them.
namespace {
// the checks of a coarsening's desc that the three entries share (what: the struct's name)
ommResult check_coarsen_desc(const Logger& log, const ommCpuBakeResultDesc& r, const char* what, uint8_t mixedState, uint32_t flags, const uint8_t reserved[3])
{
    char buf[160];
    if (!is_index_format(r.indexFormat)) return log.invalid("[Invalid Arg] - deviceResult.indexFormat is not an index format");
    if (mixedState != 2 && mixedState != 3) { snprintf(buf, sizeof buf, "[Invalid Arg] - %s.mixedState must be 2 (UnknownTransparent) or 3 (UnknownOpaque)", what); return log.invalid(buf); }
    if ((flags & ~(uint32_t)(ommxCoarsenFlags_DisableSpecialIndices | ommxCoarsenFlags_DisableDuplicateDetection)) != 0) { snprintf(buf, sizeof buf, "[Invalid Arg] - %s.flags has unknown bits", what); return log.invalid(buf); }
    if (reserved[0] || reserved[1] || reserved[2]) { snprintf(buf, sizeof buf, "[Invalid Arg] - %s.reserved must be 0", what); return log.invalid(buf); }
    if (has_null_array(r)) return log.invalid("[Invalid Arg] - deviceResult has a null array with a non-zero count");
    return ommResult_SUCCESS;
}
CoarsenArgs coarsen_args(const ommCpuBakeResultDesc& r, uint32_t maxLevel, const uint8_t* blockLevels, uint32_t mixedState, uint32_t flags)
{
    CoarsenArgs a; a.result = r; a.maxLevel = maxLevel < kRebuildLevels - 1u ? maxLevel : kRebuildLevels - 1u; a.blockLevels = blockLevels; a.mixedState = mixedState; a.flags = flags;
    return a;
}
// the stages of a coarsening inside DerivedResult::run
ommResult coarsen_stages(DerivedResult& out, const CoarsenArgs& a, ommxCoarsenInfo* info)
{
    PoolBlock head, staging;
    if (!out.acquire(head, coarsen_head_bytes(a))) return out.no_memory();
    CoarsenPlan plan;
    if (coarsen_plan(a, head.p, &plan, out.stream) != hipSuccess) return out.failed();
    if (plan.stagingBytes && !out.acquire(staging, (size_t)plan.stagingBytes)) return out.no_memory();
    RebuildCounts n;
    if (coarsen_reduce(a, head.p, staging.p, plan, &n, out.stream) != hipSuccess) return out.failed();
    info->arrayDataSize = n.arrayBytes; info->descArrayCount = n.descCount; info->referencedBlocks = plan.referenced; info->coarsenedBlocks = plan.coarsened;
    info->uniformBlocks = n.uniform; info->duplicateBlocks = n.duplicate; info->skippedPrimitives = plan.skipped;
    return out.emit(n, [&](const RebuildOutputs& o) { return coarsen_emit(a, head.p, staging.p, n, o, out.stream); });
}
ommResult coarsen_device(Baker& b, const ommCpuBakeResultDesc& r, const uint8_t* blockLevels, const ommxCoarsenDesc& c, ommxDeviceBakeResult* outResult, ommxCoarsenInfo* outInfo,
                         hipStream_t stream)
{
    const ommResult ok = check_coarsen_desc(b.log, r, "ommxCoarsenDesc", c.mixedState, c.flags, c.reserved);
    if (ok != ommResult_SUCCESS) return ok;
    ommxCoarsenInfo info; memset(&info, 0, sizeof info);
    DerivedResult out(b, stream, "coarsened", "coarsening");
    const CoarsenArgs a = coarsen_args(r, c.maxSubdivisionLevel, blockLevels, c.mixedState, c.flags);
    const ommResult done = out.run(outResult, r.indexCount, r.indexFormat, [&] { return coarsen_stages(out, a, &info); });
    if (done == ommResult_SUCCESS && outInfo) *outInfo = info;
    return done;
}
ommResult coarsen_entry(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const uint8_t* blockLevels, const ommxCoarsenDesc* desc, ommxDeviceBakeResult* outResult,
                        ommxCoarsenInfo* outInfo, void* hipStream)
{
    Baker* b;
    const ommResult checked = check_one_result(baker, deviceResult, "ommxCoarsenDesc", desc != nullptr, outResult != nullptr || outInfo != nullptr, &b);
    if (checked != ommResult_SUCCESS) return checked;
    return guarded(&b->log, [&] { return coarsen_device(*b, *deviceResult, blockLevels, *desc, outResult, outInfo, (hipStream_t)hipStream); });
}
}

OMM_MI355X_API ommResult ommxCoarsenMicromap(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxCoarsenDesc* desc,
                                             ommxDeviceBakeResult* outResult, ommxCoarsenInfo* outInfo, void* hipStream)
{
    return coarsen_entry(baker, deviceResult, nullptr, desc, outResult, outInfo, hipStream);
}

OMM_MI355X_API ommResult ommxCoarsenMicromapLevels(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const uint8_t* deviceBlockLevels, const ommxCoarsenDesc* desc,
                                                   ommxDeviceBakeResult* outResult, ommxCoarsenInfo* outInfo, void* hipStream)
{
    return coarsen_entry(baker, deviceResult, deviceBlockLevels, desc, outResult, outInfo, hipStream);
}

// Near-copies among the 4-state blocks of a device-resident result merged into leaders (include/omm_mi355x_ext.h; kernels in merge_kernels.hip): read
// the index buffer, size the staging arena, copy, run the rounds in place, then the tail as for a coarsening.
namespace {
ommResult check_merge_desc(const Logger& log, const ommCpuBakeResultDesc& r, const ommxMergeDesc& m)
{
    if (!is_index_format(r.indexFormat)) return log.invalid("[Invalid Arg] - deviceResult.indexFormat is not an index format");
    if (m.maxDistance > kMergeUnit) return log.invalid("[Invalid Arg] - ommxMergeDesc.maxDistance must be at most 4^12 (16777216)");
    if (m.rounds > OMMX_MERGE_MAX_ROUNDS) return log.invalid("[Invalid Arg] - ommxMergeDesc.rounds must be at most OMMX_MERGE_MAX_ROUNDS (32)");
    if (m.samples > OMMX_MERGE_MAX_SAMPLES) return log.invalid("[Invalid Arg] - ommxMergeDesc.samples must be at most OMMX_MERGE_MAX_SAMPLES (28)");
    if (m.mixedState != 2 && m.mixedState != 3) return log.invalid("[Invalid Arg] - ommxMergeDesc.mixedState must be 2 (UnknownTransparent) or 3 (UnknownOpaque)");
    if ((m.flags & ~(uint32_t)ommxCoarsenFlags_DisableSpecialIndices) != 0) return log.invalid("[Invalid Arg] - ommxMergeDesc.flags has bits other than DisableSpecialIndices");
    if (m.reserved[0] || m.reserved[1] || m.reserved[2]) return log.invalid("[Invalid Arg] - ommxMergeDesc.reserved must be 0");
    if (has_null_array(r)) return log.invalid("[Invalid Arg] - deviceResult has a null array with a non-zero count");
    return ommResult_SUCCESS;
}
// the stages of a merge inside DerivedResult::run
ommResult merge_stages(DerivedResult& out, const MergeArgs& a, ommxMergeInfo* info)
{
    PoolBlock head, staging;
    if (!out.acquire(head, merge_head_bytes(a))) return out.no_memory();
    MergePlan plan;
    if (merge_plan(a, head.p, &plan, out.stream) != hipSuccess) return out.failed();
    if (plan.stagingBytes && !out.acquire(staging, (size_t)plan.stagingBytes)) return out.no_memory();
    RebuildCounts n; MergeRounds rounds;
    if (merge_stage(a, head.p, staging.p, plan, &rounds, &n, out.stream) != hipSuccess) return out.failed();
    info->arrayDataSize = n.arrayBytes; info->descArrayCount = n.descCount; info->referencedBlocks = plan.referenced; info->candidateBlocks = plan.candidates;
    info->absorbedBlocks = rounds.absorbed; info->uniformBlocks = n.uniform; info->duplicateBlocks = n.duplicate; info->skippedPrimitives = plan.skipped;
    memcpy(info->absorbedPerRound, rounds.perRound, sizeof info->absorbedPerRound);
    return out.emit(n, [&](const RebuildOutputs& o) { return merge_emit(a, head.p, staging.p, n, o, out.stream); });
}
ommResult merge_device(Baker& b, const ommCpuBakeResultDesc& r, const ommxMergeDesc& m, uint32_t* outRoots, ommxDeviceBakeResult* outResult, ommxMergeInfo* outInfo,
                       hipStream_t stream)
{
    const ommResult ok = check_merge_desc(b.log, r, m);
    if (ok != ommResult_SUCCESS) return ok;
    ommxMergeInfo info; memset(&info, 0, sizeof info);
    DerivedResult out(b, stream, "merged", "merge");
    MergeArgs a; a.result = r; a.maxDistance = m.maxDistance; a.rounds = m.rounds ? m.rounds : 8u; a.samples = m.samples ? m.samples : 16u; a.seed = m.seed;
    a.mixedState = m.mixedState; a.flags = m.flags; a.roots = outRoots;
    const ommResult done = out.run(outResult, r.indexCount, r.indexFormat, [&] { return merge_stages(out, a, &info); });
    if (done == ommResult_SUCCESS && outInfo) *outInfo = info;
    return done;
}
}

OMM_MI355X_API ommResult ommxMergeSimilarMicromaps(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxMergeDesc* desc, uint32_t* outDeviceBlockRoots,
                                                   ommxDeviceBakeResult* outResult, ommxMergeInfo* outInfo, void* hipStream)
{
    Baker* b = baker_for_device_results(baker);
    if (!b) return ommResult_INVALID_ARGUMENT;
    if (deviceResult == nullptr) return b->log.invalid("[Invalid Arg] - deviceResult was not set");
    if (desc == nullptr) return b->log.invalid("[Invalid Arg] - ommxMergeDesc was not set");
    if (!outDeviceBlockRoots && !outResult && !outInfo) return b->log.invalid("[Invalid Arg] - none of outDeviceBlockRoots, outResult and outInfo was set");
    return guarded(&b->log, [&] { return merge_device(*b, *deviceResult, *desc, outDeviceBlockRoots, outResult, outInfo, (hipStream_t)hipStream); });
}

// What every block of a device-resident result would keep at every coarser level, and a result fitted to a byte budget from those rows
// (include/omm_mi355x_ext.h; kernels in fit_kernels.hip, the planner in fit_plan.h).
namespace {
// one profile in flight: its scratch, its arrays
struct ProfileRun {
    PoolBlock head, roots; ProfileArgs a; ProfilePlan plan;
    // false: out of device memory (*launched false) or a failed launch (*launched true)
    bool run(Baker& b, const ProfileArgs& args, hipStream_t stream, bool* launched)
    {
        *launched = false;
        if (!head.acquire(b.devPool.get(), profile_head_bytes(args))) return false;
        a = profile_arrays(args, head.p);
        *launched = true;
        if (profile_plan(args, head.p, &plan, stream) != hipSuccess) return false;
        *launched = false;
        if (plan.units && !roots.acquire(b.devPool.get(), (size_t)plan.units)) return false;
        *launched = true;
        return profile_count_blocks(args, head.p, roots.p, plan, stream) == hipSuccess;
    }
};
ProfileArgs profile_args(const ommCpuBakeResultDesc& r, const float* weights, const ommxLevelProfileOutputs* o, bool wantShape)
{
    ProfileArgs a; a.result = r; a.weights = weights;
    a.known = o ? o->knownCounts : nullptr; a.opaque = o ? o->knownOpaqueCounts : nullptr; a.refs = o ? o->referenceCounts : nullptr;
    a.blockWeights = o ? (unsigned long long*)o->blockWeights : nullptr; a.shape = nullptr; a.wantShape = wantShape;
    return a;
}
ommResult profile_device(Baker& b, const ommCpuBakeResultDesc& r, const float* weights, const ommxLevelProfileOutputs* outputs, ommxLevelProfileInfo* outInfo, hipStream_t stream)
{
    if (!is_index_format(r.indexFormat)) return b.log.invalid("[Invalid Arg] - deviceResult.indexFormat is not an index format");
    if (has_null_array(r)) return b.log.invalid("[Invalid Arg] - deviceResult has a null array with a non-zero count");
    ommxLevelProfileInfo info; memset(&info, 0, sizeof info);
    if (r.indexCount) {
        if (!usable_device()) return b.log.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)");
        const DeviceScope onBakersDevice(b.device.load());   // (a baker that has no device yet works on the caller's current one)
        ProfileRun p; bool launched;
        if (!p.run(b, profile_args(r, weights, outputs, false), stream, &launched)) {
            if (!launched) return b.log.failure("[Failure] - out of device memory for the profile scratch");
            (void)hipGetLastError(); (void)hipStreamSynchronize(stream);   // (the scratch goes back only when nothing can still touch it)
            return b.log.failure("[Failure] - the profile kernels could not run");
        }
        info.referencedBlocks = p.plan.referenced; info.skippedPrimitives = p.plan.skipped; info.weightExponent = p.plan.weightExponent;
    }
    if (outInfo) *outInfo = info;
    return ommResult_SUCCESS;
}

ommResult fit_device(Baker& b, const ommCpuBakeResultDesc& r, const ommxFitDesc& f, uint8_t* outLevels, ommxDeviceBakeResult* outResult, ommxFitInfo* outInfo, hipStream_t stream)
{
    const ommResult ok = check_coarsen_desc(b.log, r, "ommxFitDesc", f.mixedState, f.flags, f.reserved);
    if (ok != ommResult_SUCCESS) return ok;
    ommxFitInfo info; memset(&info, 0, sizeof info);
    DerivedResult out(b, stream, "fitted", "fit");
    const ommResult done = out.run(outResult, r.indexCount, r.indexFormat, [&] {
        const size_t D = r.descArrayCount;
        PoolBlock levelsBlock;
        if (!out.acquire(levelsBlock, D ? D : 1)) return out.no_memory();
        std::vector<uint8_t> levels(D);
        {
            // the profile, its rows read back as the planner's table, the plan
            ProfileRun p; bool launched;
            if (!p.run(b, profile_args(r, f.devicePrimitiveWeights, nullptr, true), stream, &launched)) return launched ? out.failed() : out.no_memory();
            std::vector<uint32_t> shape(D), known(D * kFitLevels), opaque(D * kFitLevels); std::vector<uint64_t> weight(D);
            if (D) {
                const bool copied = HIP_OK(hipMemcpyAsync(shape.data(), p.a.shape, 4 * D, hipMemcpyDeviceToHost, stream))
                                 && HIP_OK(hipMemcpyAsync(known.data(), p.a.known, 4 * D * kFitLevels, hipMemcpyDeviceToHost, stream))
                                 && HIP_OK(hipMemcpyAsync(opaque.data(), p.a.opaque, 4 * D * kFitLevels, hipMemcpyDeviceToHost, stream))
                                 && HIP_OK(hipMemcpyAsync(weight.data(), p.a.blockWeights, 8 * D, hipMemcpyDeviceToHost, stream))
                                 && HIP_OK(hipStreamSynchronize(stream));
                if (!copied) return out.failed();
            }
            FitTable T; T.count = (uint32_t)D; T.shape = shape.data(); T.known = known.data(); T.opaque = opaque.data(); T.weight = weight.data();
            const FitPlan plan = fit_plan(T, f.maxSubdivisionLevel, !(f.flags & ommxCoarsenFlags_DisableSpecialIndices), f.maxArrayDataSize, levels.data());
            if (!plan.feasible) return out.give_up(b.log.failure("[Failure] - ommxFitDesc.maxArrayDataSize is below what the blocks occupy at their coarsest level (possible only with DisableSpecialIndices); nothing was written"));
            info.unfittedArrayDataSize = plan.unfitted; info.plannedArrayDataSize = plan.planned; info.steps = plan.steps;
        }
        if (D) {
            const bool copied = HIP_OK(hipMemcpyAsync(levelsBlock.p, levels.data(), D, hipMemcpyHostToDevice, stream))
                             && (!outLevels || HIP_OK(hipMemcpyAsync(outLevels, levelsBlock.p, D, hipMemcpyDeviceToDevice, stream)));
            if (!copied) return out.failed();
        }
        // (the plan's levels hold the global cap already; the host vector outlives the upload: every stage below ends with the stream idle)
        const CoarsenArgs a = coarsen_args(r, kRebuildLevels - 1u, D ? (const uint8_t*)levelsBlock.p : nullptr, f.mixedState, f.flags);
        return coarsen_stages(out, a, &info.result);
    });
    if (done == ommResult_SUCCESS && outInfo) *outInfo = info;
    return done;
}
}

OMM_MI355X_API ommResult ommxProfileMicromapLevels(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const float* devicePrimitiveWeights,
                                                   const ommxLevelProfileOutputs* outputs, ommxLevelProfileInfo* outInfo, void* hipStream)
{
    Baker* b = baker_for_device_results(baker);
    if (!b) return ommResult_INVALID_ARGUMENT;
    if (deviceResult == nullptr) return b->log.invalid("[Invalid Arg] - deviceResult was not set");
    if (outputs == nullptr && outInfo == nullptr) return b->log.invalid("[Invalid Arg] - neither outputs nor outInfo was set");
    return guarded(&b->log, [&] { return profile_device(*b, *deviceResult, devicePrimitiveWeights, outputs, outInfo, (hipStream_t)hipStream); });
}

OMM_MI355X_API ommResult ommxFitMicromap(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxFitDesc* desc, uint8_t* outDeviceBlockLevels,
                                         ommxDeviceBakeResult* outResult, ommxFitInfo* outInfo, void* hipStream)
{
    Baker* b = baker_for_device_results(baker);
    if (!b) return ommResult_INVALID_ARGUMENT;
    if (deviceResult == nullptr) return b->log.invalid("[Invalid Arg] - deviceResult was not set");
    if (desc == nullptr) return b->log.invalid("[Invalid Arg] - ommxFitDesc was not set");
    if (outResult == nullptr && outInfo == nullptr && outDeviceBlockLevels == nullptr) return b->log.invalid("[Invalid Arg] - none of outDeviceBlockLevels, outResult and outInfo was set");
    return guarded(&b->log, [&] { return fit_device(*b, *deviceResult, *desc, outDeviceBlockLevels, outResult, outInfo, (hipStream_t)hipStream); });
}

// One conservative result from several device-resident results over the same primitives (include/omm_mi355x_ext.h; kernels in combine_kernels.hip): find
// the distinct tuples of entries, size the per-tuple scratch and the staging arena, join and compare, judge the output's size on the host, then allocate
// the new result's arrays and fill them.
namespace {
ommResult combine_device(Baker& b, const ommCpuBakeResultDesc* const* results, uint32_t count, const ommxCombineDesc& c, ommxDeviceBakeResult* outResult,
                         ommxCombineInfo* outInfo, hipStream_t stream)
{
    if (c.format != (uint32_t)ommFormat_OC1_2_State && c.format != (uint32_t)ommFormat_OC1_4_State) return b.log.invalid("[Invalid Arg] - ommxCombineDesc.format must be OC1_2_State (1) or OC1_4_State (2)");
    if (c.mixedState != 2 && c.mixedState != 3) return b.log.invalid("[Invalid Arg] - ommxCombineDesc.mixedState must be 2 (UnknownTransparent) or 3 (UnknownOpaque)");
    if (c.flags != 0) return b.log.invalid("[Invalid Arg] - ommxCombineDesc.flags must be 0");
    if (c.reserved[0] || c.reserved[1] || c.reserved[2]) return b.log.invalid("[Invalid Arg] - ommxCombineDesc.reserved must be 0");
    ommResult checked = check_source_formats(b.log, results, count);
    if (checked != ommResult_SUCCESS) return checked;
    const uint32_t indexCount = results[0]->indexCount;
    for (uint32_t k = 1; k < count; ++k)
        if (results[k]->indexCount != indexCount) return b.log.invalid("[Invalid Arg] - the sources' indexCount values differ: they must describe the same primitives");
    checked = check_source_arrays(b.log, results, count);
    if (checked != ommResult_SUCCESS) return checked;
    ommxCombineInfo info; memset(&info, 0, sizeof info);
    DerivedResult out(b, stream, "combined", "combine");
    const ommResult done = out.run(outResult, indexCount, ommIndexFormat_UINT_32, [&] {
        CombineArgs a; memset(&a, 0, sizeof a);
        for (uint32_t k = 0; k < count; ++k) a.source[k] = view_of(*results[k]);
        a.sourceCount = count; a.indexCount = indexCount; a.format = c.format; a.mixedState = c.mixedState;
        PoolBlock head, perTuple, staging;
        if (!out.acquire(head, combine_head_bytes(a))) return out.no_memory();
        CombineTuples t;
        if (combine_tuples(a, head.p, &t, stream) != hipSuccess) return out.failed();
        info.combinedTuples = t.tuples; info.skippedPrimitives = t.skipped;
        RebuildCounts n; memset(&n, 0, sizeof n);
        if (t.tuples) {
            if (!out.acquire(perTuple, combine_tuple_bytes(a, t.tuples))) return out.no_memory();
            CombinePlan plan;
            if (combine_plan(a, head.p, perTuple.p, t, &plan, stream) != hipSuccess) return out.failed();
            if (!out.acquire(staging, (size_t)plan.stagingBytes)) return out.no_memory();
            if (combine_join(a, perTuple.p, staging.p, t, plan, &n, stream) != hipSuccess) return out.failed();
            info.refinedTuples = plan.refined; info.uniformBlocks = n.uniform; info.duplicateBlocks = n.duplicate;
        }
        info.arrayDataSize = n.arrayBytes; info.descArrayCount = n.descCount;
        return out.emit(n, [&](const RebuildOutputs& o) { return combine_emit(a, head.p, perTuple.p, staging.p, t, n, o, stream); });
    });
    if (done == ommResult_SUCCESS && outInfo) *outInfo = info;
    return done;
}
}

OMM_MI355X_API ommResult ommxCombineMicromaps(ommBaker baker, const ommCpuBakeResultDesc* const* deviceResults, uint32_t resultCount, const ommxCombineDesc* desc,
                                              ommxDeviceBakeResult* outResult, ommxCombineInfo* outInfo, void* hipStream)
{
    Baker* b = baker_for_device_results(baker);
    if (!b) return ommResult_INVALID_ARGUMENT;
    const ommResult checked = check_result_array(b->log, deviceResults, resultCount, "ommxCombineDesc", desc != nullptr, "OMMX_COMBINE_MAX_SOURCES", OMMX_COMBINE_MAX_SOURCES,
                                                 outResult != nullptr || outInfo != nullptr);
    if (checked != ommResult_SUCCESS) return checked;
    return guarded(&b->log, [&] { return combine_device(*b, deviceResults, resultCount, *desc, outResult, outInfo, (hipStream_t)hipStream); });
}

// The state-by-state difference of two device-resident results over the same primitives (include/omm_mi355x_ext.h; kernels in compare_kernels.hip): find
// the distinct pairs of entries, size the per-pair scratch, stream both sides once per pair, then add up on the device and finish the info here.
namespace {
ommResult compare_device(Baker& b, const ommCpuBakeResultDesc& ra, const ommCpuBakeResultDesc& rb, const ommxCompareDesc& d, const ommxCompareOutputs* outputs,
                         ommxCompareInfo* outInfo, hipStream_t stream)
{
    if ((d.flags & ~(uint32_t)ommxCompareFlags_Force2State) != 0) return b.log.invalid("[Invalid Arg] - ommxCompareDesc.flags has unknown bits");
    if (d.reserved != 0) return b.log.invalid("[Invalid Arg] - ommxCompareDesc.reserved must be 0");
    if (!is_index_format(ra.indexFormat) || !is_index_format(rb.indexFormat)) return b.log.invalid("[Invalid Arg] - a source's indexFormat is not an index format");
    if (ra.indexCount != rb.indexCount) return b.log.invalid("[Invalid Arg] - the sources' indexCount values differ: they must describe the same primitives");
    if (has_null_array(ra) || has_null_array(rb)) return b.log.invalid("[Invalid Arg] - a source has a null array with a non-zero count");
    if (outputs && ((uintptr_t)outputs->confusion & 15u) != 0) return b.log.invalid("[Invalid Arg] - ommxCompareOutputs.confusion is not 16-byte aligned");
    ommxCompareInfo info; memset(&info, 0, sizeof info);
    info.firstConflictPrimitive = 0xFFFFFFFFu;
    if (ra.indexCount != 0) {
        if (!usable_device()) return b.log.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)");
        const DeviceScope onBakersDevice(b.device.load());   // (a baker that has no device yet works on the caller's current one)
        CompareArgs a; memset(&a, 0, sizeof a);
        a.a = view_of(ra); a.b = view_of(rb); a.indexCount = ra.indexCount; a.force2 = d.flags & (uint32_t)ommxCompareFlags_Force2State;
        if (outputs) { a.relations = outputs->relations; a.levels = outputs->levels; a.confusion = outputs->confusion; }
        PoolBlock head, perPair;
        // after a failed launch: the scratch goes back only when nothing can still touch it
        const auto failed = [&] { (void)hipGetLastError(); (void)hipStreamSynchronize(stream); return b.log.failure("[Failure] - the compare kernels could not run"); };
        if (!head.acquire(b.devPool.get(), compare_head_bytes(a))) return b.log.failure("[Failure] - out of device memory for the compare scratch");
        CombineTuples t;
        if (compare_pairs(a, head.p, &t, stream) != hipSuccess) return failed();
        if (t.tuples && !perPair.acquire(b.devPool.get(), compare_pair_bytes(t.tuples))) return b.log.failure("[Failure] - out of device memory for the compare scratch");
        CompareTotals n;
        if (compare_count(a, head.p, perPair.p, t, &n, stream) != hipSuccess) return failed();
        uint32_t byRelation[5] = { n.identical, n.conflict, n.aWeaker, n.bWeaker, n.hint };
        for (uint32_t c = 0; c < 16; ++c) {   // the primitives with two special entries: one field at level 0 each
            info.totals[c >> 2][c & 3] = n.totals[c] + ((uint64_t)n.specialCells[c] << 24);
            const uint32_t r = compare_cell_relation(c >> 2, c & 3);
            if (r == 0) byRelation[0] += n.specialCells[c];
            for (uint32_t bit = 0; bit < 4; ++bit)
                if (r & (1u << bit)) byRelation[1 + bit] += n.specialCells[c];
        }
        info.identicalPrimitives = byRelation[0]; info.conflictPrimitives = byRelation[1]; info.aWeakerPrimitives = byRelation[2];
        info.bWeakerPrimitives = byRelation[3]; info.hintPrimitives = byRelation[4];
        info.skippedPrimitives = t.skipped; info.comparedPairs = t.tuples; info.refinedPairs = n.refined; info.firstConflictPrimitive = n.firstConflict;
    }
    if (outInfo) *outInfo = info;
    return ommResult_SUCCESS;
}
}

OMM_MI355X_API ommResult ommxCompareMicromaps(ommBaker baker, const ommCpuBakeResultDesc* deviceResultA, const ommCpuBakeResultDesc* deviceResultB,
                                              const ommxCompareDesc* desc, const ommxCompareOutputs* outputs, ommxCompareInfo* outInfo, void* hipStream)
{
    Baker* b = baker_for_device_results(baker);
    if (!b) return ommResult_INVALID_ARGUMENT;
    if (deviceResultA == nullptr) return b->log.invalid("[Invalid Arg] - deviceResultA was not set");
    if (deviceResultB == nullptr) return b->log.invalid("[Invalid Arg] - deviceResultB was not set");
    if (desc == nullptr) return b->log.invalid("[Invalid Arg] - ommxCompareDesc was not set");
    if (outputs == nullptr && outInfo == nullptr) return b->log.invalid("[Invalid Arg] - neither outputs nor outInfo was set");
    return guarded(&b->log, [&] { return compare_device(*b, *deviceResultA, *deviceResultB, *desc, outputs, outInfo, (hipStream_t)hipStream); });
}

// One result from chosen primitives of several device-resident results (include/omm_mi355x_ext.h; kernels in gather_kernels.hip): build the source table
// with its scans, mark the descriptors the selection reaches and size the staging arena, copy and compare, judge the output's size on the host, then
// allocate the new result's arrays and fill them.
namespace {
ommResult gather_device(Baker& b, const ommCpuBakeResultDesc* const* results, uint32_t count, const ommxGatherDesc& g, ommxDeviceBakeResult* outResult,
                        ommxGatherInfo* outInfo, hipStream_t stream)
{
    if ((g.flags & ~(uint32_t)(ommxGatherFlags_DisableSpecialIndices | ommxGatherFlags_DisableDuplicateDetection)) != 0) return b.log.invalid("[Invalid Arg] - ommxGatherDesc.flags has unknown bits");
    if (g.reserved != 0) return b.log.invalid("[Invalid Arg] - ommxGatherDesc.reserved must be 0");
    if (g.selection == nullptr && g.selectionCount != 0) return b.log.invalid("[Invalid Arg] - ommxGatherDesc.selection was not set but selectionCount is not 0");
    ommResult checked = check_source_formats(b.log, results, count);
    if (checked == ommResult_SUCCESS) checked = check_source_arrays(b.log, results, count);
    if (checked != ommResult_SUCCESS) return checked;
    std::vector<GatherSource> table(count);
    uint64_t prims = 0, descs = 0;
    for (uint32_t k = 0; k < count; ++k) {
        GatherSource& s = table[k];
        s.view = view_of(*results[k]);
        s.primBase = (uint32_t)prims; s.descBase = (uint32_t)descs;   // (a sum that does not fit is refused below, before the table is used)
        prims += s.view.indexCount; descs += s.view.descCount;
    }
    if (g.selection == nullptr && prims > 0xFFFFFFFFull) return b.log.invalid("[Invalid Arg] - the sources' indexCount values add up to more than 2^32 - 1 primitives");
    if (descs > 0xFFFFFFFFull) return b.log.invalid("[Invalid Arg] - the sources' descArrayCount values add up to more than 2^32 - 1 descriptors");
    const uint32_t primitiveCount = g.selection ? g.selectionCount : (uint32_t)prims;
    ommxGatherInfo info; memset(&info, 0, sizeof info);
    DerivedResult out(b, stream, "gathered", "gather");
    const ommResult done = out.run(outResult, primitiveCount, ommIndexFormat_UINT_32, [&] {
        GatherArgs a; a.sources = table.data(); a.sourceCount = count; a.selection = g.selection; a.primitiveCount = primitiveCount; a.descTotal = (uint32_t)descs; a.flags = g.flags;
        PoolBlock head, staging;
        if (!out.acquire(head, gather_head_bytes(a))) return out.no_memory();
        GatherPlan plan;
        if (gather_plan(a, head.p, &plan, stream) != hipSuccess) return out.failed();
        if (plan.stagingBytes && !out.acquire(staging, (size_t)plan.stagingBytes)) return out.no_memory();
        RebuildCounts n;
        if (gather_stage(a, head.p, staging.p, plan, &n, stream) != hipSuccess) return out.failed();
        info.arrayDataSize = n.arrayBytes; info.descArrayCount = n.descCount; info.primitiveCount = primitiveCount; info.referencedBlocks = plan.referenced;
        info.uniformBlocks = n.uniform; info.duplicateBlocks = n.duplicate; info.skippedPrimitives = plan.skipped;
        return out.emit(n, [&](const RebuildOutputs& o) { return gather_emit(a, head.p, staging.p, n, o, stream); });
    });
    if (done == ommResult_SUCCESS && outInfo) *outInfo = info;
    return done;
}
}

OMM_MI355X_API ommResult ommxGatherMicromaps(ommBaker baker, const ommCpuBakeResultDesc* const* deviceResults, uint32_t resultCount, const ommxGatherDesc* desc,
                                             ommxDeviceBakeResult* outResult, ommxGatherInfo* outInfo, void* hipStream)
{
    Baker* b = baker_for_device_results(baker);
    if (!b) return ommResult_INVALID_ARGUMENT;
    const ommResult checked = check_result_array(b->log, deviceResults, resultCount, "ommxGatherDesc", desc != nullptr, "OMMX_GATHER_MAX_SOURCES", OMMX_GATHER_MAX_SOURCES,
                                                 outResult != nullptr || outInfo != nullptr);
    if (checked != ommResult_SUCCESS) return checked;
    return guarded(&b->log, [&] { return gather_device(*b, deviceResults, resultCount, *desc, outResult, outInfo, (hipStream_t)hipStream); });
}

// A result for the same primitives with their vertices re-ordered (include/omm_mi355x_ext.h; kernels in reorient_kernels.hip): mark the (descriptor,
// orientation) pairs the primitives reach and size the staging arena, permute and compare, judge the output's size on the host, then allocate the new
// result's arrays and fill them.
namespace {
ommResult reorient_device(Baker& b, const ommCpuBakeResultDesc& r, const ommxReorientDesc& d, ommxDeviceBakeResult* outResult, ommxReorientInfo* outInfo, hipStream_t stream)
{
    if ((d.flags & ~(uint32_t)(ommxCoarsenFlags_DisableSpecialIndices | ommxCoarsenFlags_DisableDuplicateDetection)) != 0) return b.log.invalid("[Invalid Arg] - ommxReorientDesc.flags has unknown bits");
    if (d.reserved[0] || d.reserved[1] || d.reserved[2]) return b.log.invalid("[Invalid Arg] - ommxReorientDesc.reserved must be 0");
    if (d.deviceOrientations == nullptr && d.orientation > 5) return b.log.invalid("[Invalid Arg] - ommxReorientDesc.orientation must be 0..5 when deviceOrientations is not set");
    if (!is_index_format(r.indexFormat)) return b.log.invalid("[Invalid Arg] - deviceResult.indexFormat is not an index format");
    if (has_null_array(r)) return b.log.invalid("[Invalid Arg] - deviceResult has a null array with a non-zero count");
    if (d.deviceOrientations != nullptr && r.descArrayCount > 0xFFFFFFFFu / 6u) return b.log.invalid("[Invalid Arg] - deviceResult.descArrayCount is above (2^32 - 1) / 6: six items per descriptor do not fit");
    ommxReorientInfo info; memset(&info, 0, sizeof info);
    DerivedResult out(b, stream, "re-oriented", "re-orientation");
    const ommResult done = out.run(outResult, r.indexCount, ommIndexFormat_UINT_32, [&] {
        ReorientArgs a; a.source = view_of(r); a.orientations = d.deviceOrientations; a.orientation = d.orientation; a.flags = d.flags;
        PoolBlock head, staging;
        if (!out.acquire(head, reorient_head_bytes(a))) return out.no_memory();
        ReorientPlan plan;
        if (reorient_plan(a, head.p, &plan, stream) != hipSuccess) return out.failed();
        if (plan.stagingBytes && !out.acquire(staging, (size_t)plan.stagingBytes)) return out.no_memory();
        RebuildCounts n;
        if (reorient_stage(a, head.p, staging.p, plan, &n, stream) != hipSuccess) return out.failed();
        info.arrayDataSize = n.arrayBytes; info.descArrayCount = n.descCount; info.referencedBlocks = plan.referenced; info.reorientedBlocks = plan.reoriented;
        info.uniformBlocks = n.uniform; info.duplicateBlocks = n.duplicate; info.skippedPrimitives = plan.skipped;
        return out.emit(n, [&](const RebuildOutputs& o) { return reorient_emit(a, head.p, staging.p, n, o, stream); });
    });
    if (done == ommResult_SUCCESS && outInfo) *outInfo = info;
    return done;
}
}

OMM_MI355X_API ommResult ommxReorientMicromap(ommBaker baker, const ommCpuBakeResultDesc* deviceResult, const ommxReorientDesc* desc, ommxDeviceBakeResult* outResult,
                                              ommxReorientInfo* outInfo, void* hipStream)
{
    Baker* b;
    const ommResult checked = check_one_result(baker, deviceResult, "ommxReorientDesc", desc != nullptr, outResult != nullptr || outInfo != nullptr, &b);
    if (checked != ommResult_SUCCESS) return checked;
    return guarded(&b->log, [&] { return reorient_device(*b, *deviceResult, *desc, outResult, outInfo, (hipStream_t)hipStream); });
}

// What ommxResolveHits and ommxRasterizeMicromap ask of the device-resident input desc, from the texture on: it is checked as ommxBakeDevice checks it, so
// a desc that could not have produced the result is refused with the same code.  `entry`: the caller's name for the line about another baker's texture.
namespace {
ommResult check_consumer_desc(Baker& b, ommBaker baker, const ommCpuBakeInputDesc& desc, const char* entry)
{
    if (tag_of(baker) != kCpuBaker) return b.log.invalid("Baker was not created as the right type");
    if (desc.texture == 0) return b.log.invalid("[Invalid Argument] - ommCpuBakeInputDesc has no texture set");
    if (sampler_enums_unknown(desc)) return ommResult_FAILURE;
    ommResult r = validate_desc(b, desc);
    if (r != ommResult_SUCCESS) return r;
    r = scope_fences(b, desc, false);
    if (r != ommResult_SUCCESS) return r;
    if (untag<Texture>(desc.texture)->owner != &b) {
        char buf[160]; snprintf(buf, sizeof buf, "[Invalid Argument] - %s: the texture was created by another baker", entry);
        return b.log.invalid(buf);
    }
    return ommResult_SUCCESS;
}
// mip 0 of the texture, the sampler and the mesh of a desc that passed check_consumer_desc
ResolveParams consumer_params(const ommCpuBakeInputDesc& desc)
{
    const Texture& tex = *untag<Texture>(desc.texture);
    ResolveParams rp; memset(&rp, 0, sizeof rp);
    ClassifyParams& P = rp.tex;
    P.mips[0] = dev_mip(tex.mips[0]);
    P.mipCount = 1; P.pow2Dispatch = P.mips[0].pow2;
    P.texIsFp32 = tex.format == ommCpuTextureFormat_FP32;
    P.addrMode = desc.runtimeSamplerDesc.addressingMode;
    P.filterLinear = desc.runtimeSamplerDesc.filter == ommTextureFilterMode_Linear;
    P.cutoff = desc.alphaCutoff; P.borderAlpha = desc.runtimeSamplerDesc.borderAlpha;
    P.stateGT = desc.alphaCutoffGreater; P.stateLE = desc.alphaCutoffLessEqual;
    rp.texCoords = desc.texCoords; rp.texCoordFormat = desc.texCoordFormat;
    rp.texCoordStride = desc.texCoordStrideInBytes ? desc.texCoordStrideInBytes : (desc.texCoordFormat == ommTexCoordFormat_UV32_FLOAT ? 8u : 4u);
    rp.indices = desc.indexBuffer; rp.indexFormat = desc.indexFormat; rp.numTris = desc.indexCount / 3u;
    return rp;
}
}

// Any-hit resolution of hits against a device-resident result (include/omm_mi355x_ext.h; kernels in lookup_kernels.hip).
OMM_MI355X_API ommResult ommxResolveHits(ommBaker baker, const ommCpuBakeInputDesc* desc, const ommCpuBakeResultDesc* result,
                                         const ommxHit* hits, uint32_t count, uint8_t* out, uint32_t flags, void* hipStream)
{
    if (baker == 0) return ommResult_INVALID_ARGUMENT;
    Baker* b = untag<Baker>(baker);
    if (desc == 0) return b->log.invalid("input desc was not set");
    const ommResult r = check_consumer_desc(*b, baker, *desc, "ommxResolveHits");
    if (r != ommResult_SUCCESS) return r;
    if (result == nullptr) return b->log.invalid("[Invalid Argument] - ommxResolveHits: result is not set");
    if ((flags & ~(uint32_t)(ommxLookupFlags_Force2State | ommxLookupFlags_IgnoreMicromap)) != 0) return b->log.invalid("[Invalid Argument] - ommxResolveHits: unknown flags");
    if (count == 0) return ommResult_SUCCESS;
    if (hits == nullptr || out == nullptr) return b->log.invalid("[Invalid Argument] - ommxResolveHits: hits / out are not set");
    const ResolveParams rp = consumer_params(*desc);
    const DeviceScope onBakersDevice(b->bind_device());
    if (launch_resolve_hits(rp, *result, hits, count, out, flags, (hipStream_t)hipStream) != hipSuccess)
        return b->log.failure("[Failure] - ommxResolveHits: kernel launch failed");
    return ommResult_SUCCESS;
}

// A device-resident result drawn in texture space over its alpha texture (include/omm_mi355x_ext.h; kernels in raster_kernels.hip): the checks in the
// documented order, the primitive range cut to the mesh, one block of scratch from the pool, the passes, then the info from the device's counts.
namespace {
bool finite_f(float x) { return x - x == 0.f; }
ommResult rasterize_device(Baker& b, ommBaker baker, const ommCpuBakeInputDesc& in, const ommCpuBakeResultDesc& r, const ommxRasterDesc& d, const ommxRasterOutputs* outputs,
                           ommxRasterInfo* outInfo, hipStream_t stream)
{
    if ((d.flags & ~(uint32_t)(ommxRasterFlags_NoContour | ommxRasterFlags_MonochromeUnknowns | ommxRasterFlags_HighlightReuse)) != 0) return b.log.invalid("[Invalid Arg] - ommxRasterDesc.flags has unknown bits");
    if (d.reserved[0] || d.reserved[1] || d.reserved[2] || d.reserved[3]) return b.log.invalid("[Invalid Arg] - ommxRasterDesc.reserved must be 0");
    if (d.width == 0 || d.width > OMMX_RASTER_MAX_SIZE || d.height == 0 || d.height > OMMX_RASTER_MAX_SIZE) return b.log.invalid("[Invalid Arg] - ommxRasterDesc.width and height must be 1..OMMX_RASTER_MAX_SIZE (16384)");
    if (!finite_f(d.uvMin[0]) || !finite_f(d.uvMin[1]) || !finite_f(d.uvMax[0]) || !finite_f(d.uvMax[1]) || !(d.uvMin[0] < d.uvMax[0]) || !(d.uvMin[1] < d.uvMax[1]))
        return b.log.invalid("[Invalid Arg] - ommxRasterDesc's viewport must be finite with uvMin < uvMax on both axes");
    if (!is_index_format(r.indexFormat)) return b.log.invalid("[Invalid Arg] - deviceResult.indexFormat is not an index format");
    if (has_null_array(r)) return b.log.invalid("[Invalid Arg] - deviceResult has a null array with a non-zero count");
    if (outputs && ((((uintptr_t)outputs->primitiveIds) | ((uintptr_t)outputs->microTriangles)) & 3u) != 0) return b.log.invalid("[Invalid Arg] - ommxRasterOutputs.primitiveIds and microTriangles must be 4-byte aligned");
    const ommResult checked = check_consumer_desc(b, baker, in, "ommxRasterizeMicromap");
    if (checked != ommResult_SUCCESS) return checked;
    if (!usable_device()) return b.log.failure("[Failure] - no usable HIP device (the MI355X baker has no CPU fallback)");
    RasterArgs a; memset(&a, 0, sizeof a);
    a.mesh = consumer_params(in); a.result = r;
    a.view = raster_view(d.uvMin, d.uvMax, d.width, d.height);
    const uint64_t tris = a.mesh.numTris;
    const uint64_t end = d.primitiveCount == 0xFFFFFFFFu ? tris : std::min<uint64_t>((uint64_t)d.firstPrimitive + d.primitiveCount, tris);
    a.first = d.firstPrimitive; a.count = end > d.firstPrimitive ? (uint32_t)(end - d.firstPrimitive) : 0u;
    a.flags = d.flags;
    if (outputs) { a.primitiveIds = outputs->primitiveIds; a.microTriangles = outputs->microTriangles; a.states = outputs->states; a.alphaTest = outputs->alphaTest; a.rgba = outputs->rgba; }
    const DeviceScope onBakersDevice(b.bind_device());
    PoolBlock scratch;
    if (!scratch.acquire(b.devPool.get(), raster_scratch_bytes(a))) return b.log.failure("[Failure] - out of device memory for the rasterization scratch");
    RasterCounts n;
    if (raster_run(a, scratch.p, &n, stream) != hipSuccess) {   // the scratch goes back only when nothing can still touch it
        (void)hipGetLastError(); (void)hipStreamSynchronize(stream);
        return b.log.failure("[Failure] - the rasterization kernels could not run");
    }
    if (outInfo) {
        ommxRasterInfo info; memset(&info, 0, sizeof info);
        info.coveredPixels = n.covered;
        for (int k = 0; k < 4; ++k) info.pixelsPerState[k] = n.perState[k];
        info.invalidPixels = n.invalid; info.alphaAbovePixels = n.alphaAbove; info.contradictions = n.contradictions;
        info.drawnPrimitives = (uint32_t)n.drawn; info.degeneratePrimitives = (uint32_t)n.degenerate;
        *outInfo = info;
    }
    return ommResult_SUCCESS;
}
}

OMM_MI355X_API ommResult ommxRasterizeMicromap(ommBaker baker, const ommCpuBakeInputDesc* deviceDesc, const ommCpuBakeResultDesc* deviceResult, const ommxRasterDesc* desc,
                                               const ommxRasterOutputs* outputs, ommxRasterInfo* outInfo, void* hipStream)
{
    Baker* b = baker_for_device_results(baker);
    if (!b) return ommResult_INVALID_ARGUMENT;
    if (deviceDesc == nullptr) return b->log.invalid("[Invalid Arg] - deviceDesc was not set");
    if (deviceResult == nullptr) return b->log.invalid("[Invalid Arg] - deviceResult was not set");
    if (desc == nullptr) return b->log.invalid("[Invalid Arg] - ommxRasterDesc was not set");
    if (outputs == nullptr && outInfo == nullptr) return b->log.invalid("[Invalid Arg] - neither outputs nor outInfo was set");
    return guarded(&b->log, [&] { return rasterize_device(*b, baker, *deviceDesc, *deviceResult, *desc, outputs, outInfo, (hipStream_t)hipStream); });
}

OMM_MI355X_API ommResult ommxDebugSaveImagePNG(const char* path, const void* hostRgba8, uint32_t width, uint32_t height, uint32_t rowPitchInBytes)
{
    if (path == nullptr || hostRgba8 == nullptr || width == 0 || height == 0) return ommResult_INVALID_ARGUMENT;
    if (rowPitchInBytes != 0 && (uint64_t)rowPitchInBytes < 4ull * width) return ommResult_INVALID_ARGUMENT;
    FILE* f = fopen(path, "wb");
    if (!f) return ommResult_FAILURE;
    const bool stored = png_store_rgba8(f, (const uint8_t*)hostRgba8, width, height, rowPitchInBytes ? (size_t)rowPitchInBytes : (size_t)4 * width);
    const bool closed = fclose(f) == 0;
    if (stored && closed) return ommResult_SUCCESS;
    (void)remove(path);
    return ommResult_FAILURE;
}

OMM_MI355X_API ommResult ommxSetBakerKnob(ommBaker baker, ommxBakerKnob knob, uint64_t value)
{
    if (baker == 0 || tag_of(baker) != kCpuBaker || (unsigned)knob >= (unsigned)ommxBakerKnob_MAX_NUM) return ommResult_INVALID_ARGUMENT;
    if (knob == ommxBakerKnob_ShardChunkBytes && value != 0 && value < 256) return ommResult_INVALID_ARGUMENT;
    if (knob == ommxBakerKnob_StreamChunks && value > kMaxStreamRanges) return ommResult_INVALID_ARGUMENT;
    if (knob == ommxBakerKnob_GenericPass && value > 2) return ommResult_INVALID_ARGUMENT;
    if (knob == ommxBakerKnob_ResultTransfer && value > (uint64_t)ommxResultTransfer_Compressed) return ommResult_INVALID_ARGUMENT;
    if (knob == ommxBakerKnob_ExpandThreads && value > 64) return ommResult_INVALID_ARGUMENT;
    if (knob == ommxBakerKnob_Devices && value > (uint64_t)kMaxRanks) return ommResult_INVALID_ARGUMENT;
    if (knob == ommxBakerKnob_HelperAffinity && value > 1) return ommResult_INVALID_ARGUMENT;
    if (knob == ommxBakerKnob_ZeroAhead && value > 1) return ommResult_INVALID_ARGUMENT;
    if (knob == ommxBakerKnob_PoisonMemory && value != 0 && (value >> 32) != 1) return ommResult_INVALID_ARGUMENT;   // (off, or bit 32 | a 32-bit word)
    if (knob == ommxBakerKnob_RetainMemory) {
        if (value > 1) return ommResult_INVALID_ARGUMENT;
        Baker* bk = untag<Baker>(baker);
        const bool keep = value == 0;
        bk->hostPool->retain.store(keep); bk->devPool->retain.store(keep); bk->arenas->retain.store(keep);
        if (!keep) { const DeviceScope onBakersDevice(bk->device.load()); bk->hostPool->trim(); bk->devPool->trim(0); bk->arenas->trim(); }
    }
    if (knob == ommxBakerKnob_PoisonMemory) untag<Baker>(baker)->devPool->poison->word.store(value);
    untag<Baker>(baker)->knobs[knob].store(value);
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommxDebugGetPoisonedBytes(ommBaker baker, uint64_t* devicePoolBytes, uint64_t* workingSetBytes)
{
    if (baker == 0 || tag_of(baker) != kCpuBaker) return ommResult_INVALID_ARGUMENT;
    const PoisonFill& p = *untag<Baker>(baker)->devPool->poison;
    if (devicePoolBytes) *devicePoolBytes = p.poolBytes.load();
    if (workingSetBytes) *workingSetBytes = p.workingSetBytes.load();
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommxTrimBaker(ommBaker baker)
{
    if (baker == 0 || tag_of(baker) != kCpuBaker) return ommResult_INVALID_ARGUMENT;
    Baker* b = untag<Baker>(baker);
    const DeviceScope onBakersDevice(b->device.load());
    b->hostPool->trim(); b->devPool->trim(0); b->arenas->trim();
    return ommResult_SUCCESS;
}

OMM_MI355X_API ommResult ommxGetLastBakeTimingsSized(ommBaker baker, void* out, size_t outBytes, size_t* libraryBytes)
{
    if (libraryBytes) *libraryBytes = sizeof(ommxBakeTimings);
    if (baker == 0 || out == nullptr || tag_of(baker) != kCpuBaker) return ommResult_INVALID_ARGUMENT;
    Baker* b = untag<Baker>(baker);
    std::lock_guard<std::mutex> g(b->timingsMu);
    if (!b->haveTimings) return ommResult_FAILURE;
    // the struct only ever grows at its end: a caller built against an older header gets the prefix it knows, one built against a newer header zeros
    const size_t n = outBytes < sizeof(ommxBakeTimings) ? outBytes : sizeof(ommxBakeTimings);
    memcpy(out, &b->timings, n);
    if (outBytes > n) memset((uint8_t*)out + n, 0, outBytes - n);
    return ommResult_SUCCESS;
}
OMM_MI355X_API ommResult ommxGetLastBakeTimings(ommBaker baker, ommxBakeTimings* out)
{
    // The unsized getter is the round-3 symbol: binaries (and ctypes mirrors) built against that header hold a struct that ends in front of
    // streamPreviewMs, so this symbol never writes more than that prefix.  Everything newer is read through ommxGetLastBakeTimingsSized.
    return ommxGetLastBakeTimingsSized(baker, out, offsetof(ommxBakeTimings, streamPreviewMs), nullptr);
}

#include "serialize.inc"
