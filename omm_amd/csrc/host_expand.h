// host_expand.h -- host side of the compressed result of ommCpuBake: the finished arrayData crosses PCIe as a codec stream (tail_kernels.hip "block
// exchange codec": one nibble per 16-byte unit = which state it repeats, or "raw") and a few host threads expand it into the caller's array.
// Plain C++ (no HIP): compiled like host_tail.cpp.
#pragma once
#include <sched.h>
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include "bake_host.h"   // pad256, CarveCursor

namespace ommx {

// CPUs this process can run on at once: scheduler affinity capped by the cgroup CPU quota (cpu.max of cgroup v2, the cfs quota of v1); >= 1
unsigned effective_cpus();

// A baker's helper threads (ommCpuBakeFlags_EnableInternalThreads, omm.h:303: the reference spends that permission on its OpenMP loops).  Threads are
// started on first use and sleep between calls; run() hands out task indices 0 .. tasks-1 to the workers AND the calling thread and returns when all are done.
// One run() at a time (concurrent bakes on one baker take turns).  A thread that cannot be started is simply missing: the caller does the work itself.
class WorkerPool {
public:
    explicit WorkerPool(unsigned workers);
    ~WorkerPool();
    WorkerPool(const WorkerPool&) = delete; WorkerPool& operator=(const WorkerPool&) = delete;
    unsigned workers() const { return (unsigned)threads_.size(); }
    void run(uint32_t tasks, const std::function<void(uint32_t)>& fn);
    // The same tasks on the WORKERS only, in the background: start() returns at once (false: no workers -- nothing was started), wait() returns when every
    // task is done.  Between the two the pool is taken (run() and bind_near() of any thread wait for wait()); whoever owns the started run calls wait() exactly once (any
    // thread) and must not call run() / bind_near() before that.
    bool start(uint32_t tasks, std::function<void(uint32_t)> fn);
    void wait();
    // Moves the workers onto the NUMA node that holds `memory` (the array they are about to fill), each onto its own slice of the node's cores; the calling
    // thread's affinity is not touched.  Best effort: returns the node, or -1 when it could not be found / nothing was changed.
    int bind_near(const void* memory);
private:
    void loop();
    std::vector<std::thread> threads_;
    // one run() / start()..wait() / bind_near() at a time.  Not a plain mutex: wait() may be called by another thread than start() was
    struct Turn {
        std::mutex m; std::condition_variable cv; bool taken = false;
        void take() { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !taken; }); taken = true; }
        void give() { { std::lock_guard<std::mutex> l(m); taken = false; } cv.notify_one(); }
    } turn_;
    struct TurnGuard { Turn& t; explicit TurnGuard(Turn& x) : t(x) { t.take(); } ~TurnGuard() { t.give(); } };
    std::mutex mu_; std::condition_variable wake_, done_;
    const std::function<void(uint32_t)>* fn_ = nullptr;
    std::function<void(uint32_t)> background_; bool backgroundActive_ = false;   // start() / wait()
    uint32_t tasks_ = 0; uint64_t generation_ = 0; unsigned active_ = 0; bool stop_ = false;
    std::atomic<uint32_t> next_{ 0 };
    int boundNode_ = -2;
    cpu_set_t boundMask_;   // the process's affinity mask when the workers were bound (bind_near binds again when it has changed)
};

// Layout of a codec stream (the same arithmetic as tail_kernels.hip: codec_layout): header 16 B | first raw unit of every 256-unit block (uint32, blocks + 1) |
// one nibble per unit (0..3: 16 bytes of 0x00 / 0x55 / 0xAA / 0xFF, 4: raw) | the raw units
struct HostCodecLayout { uint64_t units, blocks, offOfs, offCodes, offRaw; };
HostCodecLayout host_codec_layout(uint64_t paddedBytes);

// ---- the compressed transfer's integer rules (omm_host.cpp: CodecBlock, deliver_compressed; tests/native/result_delivery_check.cpp) ----
// a stream that does not shrink below half of the (padded) array is not sent: the array takes the plain copy
inline uint64_t codec_stream_cap(const HostCodecLayout& L, uint64_t paddedBytes) { return L.offRaw + paddedBytes / 2u + 16u; }
// The device block that holds the codec stream of `arrayBytes` of arrayData: size word (256 B) | scan scratch | [unit codes | block raw counts] | the stream.
// Like carve_bake_tables (bake_host.h): from base 0 `bytes` is what to reserve, from the block's base the pointers are the slots.  The stream slot has
// codec_stream_cap() bytes and ends the block; `withCodes`: a byte per 16-byte unit and a word per codec block (+ 1) for the gather to fill.
struct CodecBlockCarve { uint32_t* sizeWord; uint8_t *scratch, *unitCodes; uint32_t* blockRawCounts; uint8_t* stream; size_t bytes; };
inline CodecBlockCarve carve_codec_block(uintptr_t base, uint64_t arrayBytes, size_t scratchBytes, bool withCodes)
{
    const uint64_t padded = (arrayBytes + 255u) & ~255ull; const HostCodecLayout L = host_codec_layout(padded);
    CodecBlockCarve b = CodecBlockCarve(); CarveCursor c{ base };
    b.sizeWord = c.take<uint32_t>(1); b.scratch = c.take<uint8_t>(scratchBytes);
    if (withCodes) { b.unitCodes = c.take<uint8_t>((size_t)(padded / 16u)); b.blockRawCounts = c.take<uint32_t>((size_t)L.blocks + 1); }
    b.stream = c.take<uint8_t>(0);
    b.bytes = (size_t)(c.at - base) + (size_t)codec_stream_cap(L, padded);
    return b;
}
// The stream crosses the link in kSlices pieces, each the codes of a range of codec blocks and the raw units those blocks point at (both contiguous: `ofs`,
// the stream's table of blocks + 1 first-raw-unit indices, is a prefix sum).  Slice k: blocks [blockCut[k], blockCut[k + 1]), stream bytes [c0, c1) and
// [r0, r1); the last slice's codes end at offRaw (the padding of the code section travels with it).  Empty slices are legal.  `ok` is false when a
// table entry AT A CUT decreases or points beyond streamBytes -- a corrupt table must not turn into a wild copy; entries inside a slice are never read here.
struct CodecSlicePlan {
    static constexpr uint32_t kSlices = 12;
    struct Slice { uint64_t c0, c1, r0, r1; };
    uint64_t blockCut[kSlices + 1]; Slice slice[kSlices]; bool ok;
};
CodecSlicePlan plan_codec_slices(const HostCodecLayout& L, const uint32_t* ofs, uint64_t streamBytes);
// The expansion runs as tasks of kTaskBlocks codec blocks (2 MiB of the array) in block order: task t expands blocks [t kTaskBlocks, s1), s1 cut at L.blocks
constexpr uint64_t kTaskBlocks = 512;
inline uint64_t codec_task_count(const HostCodecLayout& L) { return (L.blocks + kTaskBlocks - 1) / kTaskBlocks; }
inline void codec_task_range(const HostCodecLayout& L, uint64_t t, uint64_t* s0, uint64_t* s1) { *s0 = t * kTaskBlocks; *s1 = *s0 + kTaskBlocks < L.blocks ? *s0 + kTaskBlocks : L.blocks; }
// the last slice a task that ends at block s1 reads from: it may start once slices 0 .. that one are on the host
uint32_t last_slice_needed(const CodecSlicePlan& plan, uint64_t s1);

// Zeroing ahead (omm_host.cpp: ResultArray): while the device bakes, helper threads zero an idle result block of `cap` bytes in pieces of 2 MiB, up to the size of
// the last compressed result (`last`).  The block may then hold a LARGER result (up to `cap`): the last piece ends at `bytes`, not at its 2 MiB boundary, and
// what lies beyond `bytes` is whatever the block held before.
constexpr unsigned kZeroPieceShift = 21;   // 2 MiB pieces
struct ZeroPlan { size_t cap, bytes, pieces; };   // bytes: the zeroed extent, min(last, cap); pieces: ceil(bytes / 2 MiB)
ZeroPlan zero_plan(size_t cap, size_t last);
// bytes [*lo, *hi) of the block that piece j < P.pieces zeroes (the last one is cut at P.bytes)
void zero_piece_range(const ZeroPlan& P, size_t j, size_t* lo, size_t* hi);
// What the expansion may trust: piece j is complete when done[j] is set (after its range was zeroed), and a byte is known to be zero only below `extent`
// in a complete piece.  zeroed_pieces() sets the extent to the plan's bytes; left out, it is unbounded: every complete piece was zeroed in full, or up to
// the end of the destination it is expanded into.
struct ZeroedPieces { const std::atomic<uint8_t>* done; size_t pieces; uint64_t extent = ~(uint64_t)0; };
inline ZeroedPieces zeroed_pieces(const ZeroPlan& P, const std::atomic<uint8_t>* done) { return ZeroedPieces{ done, P.pieces, (uint64_t)P.bytes }; }
inline bool piece_complete(const ZeroedPieces& z, size_t j) { return j < z.pieces && z.done[j].load(std::memory_order_acquire) != 0; }
// bytes [lo, hi) of the block are known to be zero: all below the extent, all in one complete piece
inline bool zeroed_range(const ZeroedPieces& z, uint64_t lo, uint64_t hi)
{
    return lo < hi && hi <= z.extent && (lo >> kZeroPieceShift) == ((hi - 1) >> kZeroPieceShift) && piece_complete(z, (size_t)(lo >> kZeroPieceShift));
}
// the bytes known to be zero (ommxBakeTimings::prefilledBytes): complete pieces, cut at the extent
uint64_t zeroed_bytes(const ZeroedPieces& z);

// Expands codec blocks [b0, b1) of `stream` (layout L) into dst[0 .. dstBytes): block b covers dst bytes [4096 b, 4096 (b + 1)); bytes beyond dstBytes are not
// written (the device pads the array to a multiple of 256 bytes).  Write-only on dst (non-temporal stores when dst is 16-byte aligned).
// `zeroed` (optional): dst is the block that was zeroed ahead (ZeroedPieces); a codec block of 4 KiB that repeats state 0 (a quarter of the blocks of the
// metric configuration), and a 64-byte line of four zero units in a mixed block, are not written again if zeroed_range() holds for all of their bytes.
// *skipped (optional) += the bytes left as they were.
void codec_expand_blocks(uint8_t* dst, uint64_t dstBytes, const uint8_t* stream, const HostCodecLayout& L, uint64_t b0, uint64_t b1,
                         const ZeroedPieces* zeroed = nullptr, uint64_t* skipped = nullptr);
// zero bytes [lo, hi) of a 4 KiB-aligned block with non-temporal stores (the pre-fill itself)
void fill_zero_nt(uint8_t* dst, size_t lo, size_t hi);

// Multi-device ommCpuBake: every device hands its own surviving blocks to the host as ONE codec stream of its contribution (the blocks it owns, back to
// back in the order of the result; all contributions padded to the same size, hence one layout); the host writes every block of the result from its owner's
// stream -- the host form of tail_kernels.hip: shard_scatter_streams.  OMMs [j0, j1) of the result.
struct HostScatter {
    uint32_t world; const uint8_t* stream[16]; bool raw[16];   // raw[r]: rank r's contribution did not shrink and arrived as it is
    HostCodecLayout L;
    const uint8_t *active, *owner, *level; const uint32_t *stateMask, *order, *dstOfs, *sizes; const uint64_t* cofs; int bits;
    uint8_t* arrayData;
};
void codec_scatter_omms(const HostScatter& S, uint32_t j0, uint32_t j1);

} // namespace ommx
