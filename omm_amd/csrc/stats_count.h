// stats_count.h -- how many micro-triangles of an OMM block are in each of the four states, counted with popcounts on masked words instead of
// a decode per field.  Compiles as HIP device code (stats_kernels.hip) and as plain C++ on the host (tests/native/stats_count_check.cpp), the
// way include/omm_mi355x_lookup.h does, so that the word arithmetic, the masking of a block's unused bits and the head / body / tail split
// of an unaligned byte range are tested without a GPU.
//
// A block is `fieldBits` (1: OC1_2_State, 2: OC1_4_State) bits per micro-triangle, little-endian within bytes, 4^level fields: only the first
// fieldBits * 4^level bits of its ceil(. / 8) bytes count (levels 0 and 1 leave part of their single byte unused).
#pragma once
#include <stdint.h>
#include "result_block.h"

#ifdef __HIPCC__
#define OMMX_STATS_FN __host__ __device__ __forceinline__
#else
#define OMMX_STATS_FN static inline
#endif

namespace ommx {

// work of the block histogram is cut into segments of this many bytes of one block (a level-12 4-state block is 256 of them)
constexpr uint32_t kStatsSegmentBytes = 16384u;

OMMX_STATS_FN uint32_t stats_popc(uint32_t w)
{
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__popc(w);
#else
    return (uint32_t)__builtin_popcount(w);
#endif
}

// Adds the states of the fields in the low `validBits` bits of `w` (a multiple of fieldBits, at most 32) to c[0..3]; the bits above are ignored.
// 1 bit per field: the bit is the state (Transparent / Opaque).  2 bits: with lo = the low bit of every field and hi = the high one,
// state 3 = lo & hi, 1 = lo & ~hi, 2 = hi & ~lo, and state 0 is what remains of the fields.
OMMX_STATS_FN void stats_count_word(uint32_t w, uint32_t validBits, uint32_t fieldBits, uint32_t c[4])
{
    if (validBits < 32u) w &= (1u << validBits) - 1u;
    if (fieldBits == 1u) {
        const uint32_t ones = stats_popc(w);
        c[1] += ones; c[0] += validBits - ones;
    } else {
        const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
        const uint32_t c3 = stats_popc(lo & hi), c1 = stats_popc(lo & ~hi), c2 = stats_popc(hi & ~lo);
        c[1] += c1; c[2] += c2; c[3] += c3; c[0] += (validBits >> 1) - c1 - c2 - c3;
    }
}

// sixteen bytes at a 16-byte aligned address, read as one load
typedef uint32_t StatsVec __attribute__((vector_size(16), may_alias));
OMMX_STATS_FN void stats_count_vec(const StatsVec q, uint32_t fieldBits, uint32_t c[4])
{
    stats_count_word(q[0], 32u, fieldBits, c); stats_count_word(q[1], 32u, fieldBits, c);
    stats_count_word(q[2], 32u, fieldBits, c); stats_count_word(q[3], 32u, fieldBits, c);
}

// The share of lane `lane` of `lanes` in the bytes [begin, end) of one block (offsets relative to the block, end <= its size), added to c[0..3]:
// the sum over all lanes is the histogram of that range.  `block` is the block's first byte, of any alignment.  The range is cut where the
// ADDRESS is a multiple of 16: the aligned middle is read 16 bytes at a time, vector v by lane v mod lanes; the up to 15 bytes in front of it
// and behind it are read one by one, byte j by lane j mod lanes.  Only a single-byte block has unused bits, so a 16-byte read is always all fields.
OMMX_STATS_FN void stats_count_range(const uint8_t* block, uint32_t level, uint32_t fieldBits, uint64_t begin, uint64_t end,
                                     uint32_t lane, uint32_t lanes, uint32_t c[4])
{
    if (begin >= end) return;
    const uint64_t blockBits = (uint64_t)fieldBits << (2u * level);
    const uint8_t* p = block + begin;
    const uint64_t n = end - begin;
    uint64_t head = (uint64_t)(0u - (uint32_t)(uintptr_t)p) & 15u;
    if (head > n) head = n;
    const uint64_t vectors = (n - head) >> 4, tail = n - head - (vectors << 4);
    const uint8_t* body = p + head;
    uint64_t v = lane;
    for (; v + 3u * (uint64_t)lanes < vectors; v += 4u * (uint64_t)lanes) {   // a full segment: four loads in flight per lane before the first count
        const StatsVec q0 = *(const StatsVec*)(body + (v << 4)), q1 = *(const StatsVec*)(body + ((v + lanes) << 4));
        const StatsVec q2 = *(const StatsVec*)(body + ((v + 2u * (uint64_t)lanes) << 4)), q3 = *(const StatsVec*)(body + ((v + 3u * (uint64_t)lanes) << 4));
        stats_count_vec(q0, fieldBits, c); stats_count_vec(q1, fieldBits, c); stats_count_vec(q2, fieldBits, c); stats_count_vec(q3, fieldBits, c);
    }
    for (; v < vectors; v += lanes) stats_count_vec(*(const StatsVec*)(body + (v << 4)), fieldBits, c);
    for (uint64_t j = lane; j < head + tail; j += lanes) {
        const uint64_t at = j < head ? j : (vectors << 4) + j;   // byte offset from p
        const uint64_t bitsLeft = blockBits - ((begin + at) << 3);
        stats_count_word(p[at], bitsLeft < 8u ? (uint32_t)bitsLeft : 8u, fieldBits, c);
    }
}

} // namespace ommx
