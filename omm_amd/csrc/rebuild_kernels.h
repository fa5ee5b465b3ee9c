// rebuild_kernels.h -- the tail of an operation that derives a new device-resident result from staged blocks (rebuild_kernels.hip): uniform blocks
// become special indices, equal blocks are merged, the others are ordered by size, then descriptors and arrayData are written.  An item is whatever
// the caller staged a block for: a source descriptor of ommxCoarsenMicromap, a tuple of ommxCombineMicromaps.  The caller stages the blocks, sums
// their digests and uniformity masks (result_words.h) and writes one word per item; it also writes the index buffer, from the tables of the tail.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"

namespace ommx {

constexpr uint32_t kRebuildLevels = 13u;            // 0..12
constexpr uint32_t kRebuildSizeClasses = 23u;       // log2 of a block's size in bytes: 1 byte .. 4 MiB
constexpr uint32_t kRebuildHist = 2 * kRebuildLevels;   // counters of a histogram: (level, format - 1)
constexpr uint32_t kRebuildSlotAlign = 16;          // staging slots: 16-byte reads in the gather, 8-byte writes by the callers

// the launch arithmetic of the tail and of its two callers
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

size_t rebuild_bytes(uint32_t items, uint32_t flags);
RebuildTables rebuild_tables(const RebuildInputs& in);
// classify and resolve on `stream`; the counts copied to the host, the stream synchronised
hipError_t rebuild_count(const RebuildInputs& in, RebuildCounts* out, hipStream_t stream);
// sort, descriptors and arrayData on `stream` (no synchronisation: the caller's index kernel follows)
hipError_t rebuild_emit(const RebuildInputs& in, const RebuildCounts& counts, uint8_t* arrayData, ommCpuOpacityMicromapDesc* descs, hipStream_t stream);
// hist: host memory, [2][kRebuildLevels][2] = array | index, level, format - 1; copied to the host, the stream synchronised
hipError_t rebuild_histograms(const RebuildInputs& in, uint32_t* hist, hipStream_t stream);

} // namespace ommx
