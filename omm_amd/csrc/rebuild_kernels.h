// rebuild_kernels.h -- the tail of an operation that derives a new device-resident result from staged blocks (rebuild_kernels.hip): uniform blocks
// become special indices, equal blocks are merged, the others are ordered by size, then descriptors and arrayData are written.  An item is whatever
// the caller staged a block for: a source descriptor of ommxCoarsenMicromap, a tuple of ommxCombineMicromaps, a (source, descriptor) pair of
// ommxGatherMicromaps, a (descriptor, orientation) pair of ommxReorientMicromap.  The caller stages the blocks, sums their digests and uniformity
// masks (result_words.h) and writes one word per item, into arrays that are laid out here (rebuild_arrays.h); its index kernel takes each output
// entry from the tables of the tail (index_back).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"
#include "rebuild_arrays.h"
#include "result_read.h"

namespace ommx {

constexpr uint32_t kRebuildLevels = 13u;            // 0..12
constexpr uint32_t kRebuildSizeClasses = 23u;       // log2 of a block's size in bytes: 1 byte .. 4 MiB
constexpr uint32_t kRebuildHist = 2 * kRebuildLevels;   // counters of a histogram: (level, format - 1)
constexpr uint32_t kRebuildSlotAlign = 16;          // staging slots: 16-byte reads in the gather, 8-byte writes by the callers

// the launch arithmetic of the tail and of its three callers
constexpr uint32_t kRebuildBlock = 256;
constexpr uint32_t kRebuildMaxGrid = 65536;
inline uint32_t strided_grid(uint64_t items)
{
    const uint64_t blocks = (items + kRebuildBlock - 1u) / kRebuildBlock;
    return (uint32_t)(blocks < kRebuildMaxGrid ? (blocks ? blocks : 1u) : kRebuildMaxGrid);
}
inline uint32_t per_item_grid(uint64_t items) { return (uint32_t)((items + kRebuildBlock - 1u) / kRebuildBlock); }
#define REBUILD_CHECK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

// The word of an item: 0 for an item that stages no block, otherwise the level and the format of its staged block.
constexpr uint32_t kRebuildLive = 0x80000000u;
constexpr uint32_t item_word(uint32_t level, uint32_t bits) { return kRebuildLive | (level << 2) | bits; }
constexpr uint32_t item_level(uint32_t w) { return (w >> 2) & 0xFFu; }
constexpr uint32_t item_bits(uint32_t w) { return w & 3u; }

struct RebuildInputs {             // device memory
    uint32_t items;
    uint32_t flags;                // ommxCoarsenFlags (0: special indices and duplicate detection)
    const uint32_t* item;          // [items] the words above
    const unsigned long long* slotStart;   // [items + 1] offsets into staging, multiples of kRebuildSlotAlign
    const unsigned long long* digest;      // [items] of the live items' staged blocks
    const uint32_t* umask;         // [items] bit s: every field of the staged block is s
    const uint8_t* staging;
    void* scratch;                 // rebuild_bytes(items, flags)
};
struct RebuildCounts {             // after the duplicate search
    uint32_t uniform, duplicate;
    uint32_t classCount[kRebuildSizeClasses];   // output blocks per size class
    uint32_t descCount; uint64_t arrayBytes;    // of the output (sums over the classes)
};
struct RebuildTables {             // what the caller's index kernel reads (per item) and adds to
    const int32_t* special;        // 0, or the special index of a uniform block
    const uint32_t* rep;           // the item whose block stands for this one's
    const uint32_t* newIndex;      // of a representative: its output descriptor (after rebuild_emit)
    uint32_t* indexHist;           // [kRebuildHist]
};
struct RebuildOutputs {            // device memory of the new result; index: in the new result's index format
    uint8_t* arrayData; ommCpuOpacityMicromapDesc* descs; void* index;
    uint32_t* hist;                // host memory, [2][kRebuildLevels][2] = array | index, level, format - 1
};

size_t rebuild_bytes(uint32_t items, uint32_t flags);
// the arrays of `items` items at the cursor: carve_tail_arrays with the scans' temporary storage and rebuild_bytes
TailArrays rebuild_arrays(CarveCursor& c, uint32_t items, uint32_t flags);
inline RebuildInputs tail_inputs(const TailArrays& t, uint32_t items, uint32_t flags, const void* staging)
{
    RebuildInputs in;
    in.items = items; in.flags = flags;
    in.item = t.item; in.slotStart = t.slotStart; in.digest = t.digest; in.umask = t.umask;
    in.staging = (const uint8_t*)staging; in.scratch = t.tailScratch;
    return in;
}
// items > 0.  slotStart and units hold sizes, their element [items] 0: both become offsets in place, slotStart[items] is copied to *stagingBytes and,
// unless totalUnits is null, units[items] to *totalUnits.  Enqueued on `stream`, NOT synchronised: the caller's own read-back and its one wait follow.
hipError_t rebuild_scan(const TailArrays& t, uint32_t items, unsigned long long* stagingBytes, unsigned long long* totalUnits, hipStream_t stream);
RebuildTables rebuild_tables(const RebuildInputs& in);
// classify and resolve on `stream`; the counts copied to the host, the stream synchronised
hipError_t rebuild_count(const RebuildInputs& in, RebuildCounts* out, hipStream_t stream);
// sort, descriptors and arrayData on `stream` (no synchronisation: the caller's index kernel follows)
hipError_t rebuild_emit(const RebuildInputs& in, const RebuildCounts& counts, uint8_t* arrayData, ommCpuOpacityMicromapDesc* descs, hipStream_t stream);
// hist: host memory, [2][kRebuildLevels][2] = array | index, level, format - 1; copied to the host, the stream synchronised
hipError_t rebuild_histograms(const RebuildInputs& in, uint32_t* hist, hipStream_t stream);

// ---- the index back: for the callers' index kernels.  hist: the workgroup's kRebuildHist counters in LDS ----
// the output entry of live item d with word w: its special index, or the output descriptor of its representative, which is then used once more
__device__ __forceinline__ int32_t index_back(const RebuildTables& tail, uint64_t d, uint32_t w, uint32_t* hist)
{
    int32_t v = tail.special[d];
    if (v == 0) {
        v = (int32_t)tail.newIndex[tail.rep[d]];
        atomicAdd(&hist[2u * item_level(w) + item_bits(w) - 1u], 1u);
    }
    return v;
}
// the output entry of primitive p of a source whose descriptors are the items [first, first + descCount): the selection rule of result_read.h behind
// the mark pass -- a special entry passes through, a descriptor with a word (marked: it passed the bounds rule) answers as its item, all else is -4
__device__ __forceinline__ int32_t index_back(const ResultView& s, uint64_t p, const uint32_t* __restrict__ item, uint64_t first, const RebuildTables& tail, uint32_t* hist)
{
    const int32_t e = named_entry(s, p);
    if (e < 0) return e == kSkipped ? -4 : e;
    const uint32_t w = item[first + (uint32_t)e];
    return w ? index_back(tail, first + (uint32_t)e, w, hist) : -4;
}

} // namespace ommx
