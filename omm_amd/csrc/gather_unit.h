// gather_unit.h -- one work unit of a block copied, bits unchanged, into its aligned staging slot: the copy of ommxGatherMicromaps (gather_units) and
// the straight path of ommxReorientMicromap (reorient_units).  A unit is 16 KiB of one block, 16 bytes per lane and step, or a whole smaller block;
// a block below 16 bytes is one lane's.  The address arithmetic is gather_copy.h's: the block lies at any byte address and no byte outside it is read.
// The writers sum the digest of the words and AND their uniformity masks into `o` (result_words.h); the caller closes the unit (unit_close).
#pragma once
#include <hip/hip_runtime.h>
#include "gather_copy.h"
#include "result_block.h"
#include "result_words.h"

namespace ommx {

constexpr uint32_t kUnitBytes = 16384;             // a workgroup's unit: four 16-byte vectors per lane of 256
constexpr uint32_t kUnitVectors = kUnitBytes / 16;
// the units of a block of `bytes` bytes
__host__ __device__ inline unsigned long long unit_count(unsigned long long bytes) { return bytes > kUnitBytes ? bytes / kUnitBytes : 1ull; }

// unit `unit` of the block at `block` (level, bits) -> o.dst (the block's slot); every thread of the workgroup of `Threads` calls it
template <uint32_t Threads>
__device__ __forceinline__ void copy_unit(const uint8_t* block, uint32_t level, uint32_t bits, uint64_t unit, UnitOut& o)
{
    const uint32_t t = threadIdx.x;
    const uint64_t bytes = block_bytes(level, bits);
    if (bytes < 16u) {
        if (t == 0u) {
            const uint64_t word = gather_small(block, (uint32_t)bytes, level, bits);
            if (bytes == 8u) *(uint64_t*)o.dst = word;
            else for (uint32_t b = 0; b < (uint32_t)bytes; ++b) o.dst[b] = (uint8_t)(word >> (8u * b));
            const uint32_t used = bits << (2u * level);
            o.digest = word_digest(word, 0u); o.umask = coarsen_word_uniform(word, used < 64u ? used : 64u, bits);
        }
        return;
    }
    const uint64_t first = unit * kUnitVectors;                                     // the unit's first vector within the block
    const uint32_t count = bytes < kUnitBytes ? (uint32_t)(bytes / 16u) : kUnitVectors;
    WordsVec* out = (WordsVec*)o.dst + first;
    if (gather_shift(block) == 0u) {
        const WordsVec* in = (const WordsVec*)block + first;
        #pragma unroll 4
        for (uint32_t v = t; v < count; v += Threads) {
            const WordsVec x = in[v];
            out[v] = x;
            const uint64_t word = 2u * (first + v);
            o.digest += word_digest(x[0], word) + word_digest(x[1], word + 1u);
            o.umask &= coarsen_word_uniform(x[0], 64u, bits) & coarsen_word_uniform(x[1], 64u, bits);
        }
    } else {
        #pragma unroll 4
        for (uint32_t v = t; v < count; v += Threads) {
            const GatherWords x = gather_vector(block, bytes, first + v);
            WordsVec y; y[0] = x.w0; y[1] = x.w1;
            out[v] = y;
            const uint64_t word = 2u * (first + v);
            o.digest += word_digest(x.w0, word) + word_digest(x.w1, word + 1u);
            o.umask &= coarsen_word_uniform(x.w0, 64u, bits) & coarsen_word_uniform(x.w1, 64u, bits);
        }
    }
}

} // namespace ommx
