// merge_words.h -- the word arithmetic of ommxMergeSimilarMicromaps (include/omm_mi355x_ext.h has the definition): the sampled positions of a round,
// the key of a block's signature, the distance of two words of 4-state fields, their join for either mixedState, and the limit of a level.
// Integers only.  Compiles as HIP device code (merge_kernels.hip) and as plain C++ on the host (tests/native/merge_check.cpp), like compare_count.h.
//
// A word holds 32 fields of two bits, field f in bits [2f, 2f + 2): bit 0 of a field is its side (0 transparent, 1 opaque), bit 1 says "unknown".
#pragma once
#include <stdint.h>
#include "coarsen_reduce.h"   // OMMX_COARSEN_FN

namespace ommx {

constexpr uint32_t kMergeMaxRounds = 32u, kMergeMaxSamples = 28u;
constexpr uint32_t kMergeUnit = 1u << 24;            // 4^12: maxDistance is in units of 4^-12 of a block
constexpr uint64_t kMergeLowBits = 0x5555555555555555ull;

OMMX_COARSEN_FN uint32_t merge_lowbias32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// sample j of round r in a block of level L: a micro-triangle index below 4^L (all arithmetic modulo 2^32)
OMMX_COARSEN_FN uint32_t merge_pos(uint32_t seed, uint32_t L, uint32_t r, uint32_t j)
{
    return merge_lowbias32(seed + 0x9E3779B9u * ((L << 16) | (r << 8) | j)) & ((1u << (2u * L)) - 1u);
}
// the 2-bit state of field `pos` of a 4-state block
OMMX_COARSEN_FN uint32_t merge_state(const uint8_t* block, uint32_t pos) { return ((uint32_t)block[pos >> 2] >> (2u * (pos & 3u))) & 3u; }
// the key: the level above the sampled states, sample j in bits [2j, 2j + 2); samples <= 28
OMMX_COARSEN_FN uint64_t merge_key_begin(uint32_t L) { return (uint64_t)L << 56; }
OMMX_COARSEN_FN uint64_t merge_key_add(uint64_t key, uint32_t j, uint32_t state) { return key | ((uint64_t)state << (2u * j)); }
OMMX_COARSEN_FN uint64_t merge_key(const uint8_t* block, uint32_t L, uint32_t r, uint32_t samples, uint32_t seed)
{
    uint64_t key = merge_key_begin(L);
    for (uint32_t j = 0; j < samples; ++j) key = merge_key_add(key, j, merge_state(block, merge_pos(seed, L, r, j)));
    return key;
}
// the low bit of every field whose two bits differ between a and b
OMMX_COARSEN_FN uint64_t merge_fold(uint64_t a, uint64_t b) { const uint64_t x = a ^ b; return (x | (x >> 1)) & kMergeLowBits; }
// the number of fields of two words whose states differ
OMMX_COARSEN_FN uint32_t merge_distance(uint64_t a, uint64_t b) { return (uint32_t)__builtin_popcountll(merge_fold(a, b)); }
// the join of ommxCombineMicromaps, field by field: sides differ -> mixedState (2 or 3); otherwise side | (either unknown ? 2 : 0)
OMMX_COARSEN_FN uint64_t merge_join(uint64_t a, uint64_t b, uint32_t mixedState)
{
    const uint64_t differ = (a ^ b) & kMergeLowBits;          // the side bit of the fields whose sides differ
    const uint64_t r = a | b | (differ << 1);                  // such a field is now 3; every other field has its side and the OR of the unknown bits
    return mixedState == 2u ? r & ~differ : r;
}
// a block of level L is absorbed iff its distance d has d * 4^(12 - L) <= maxDistance, that is d <= this
OMMX_COARSEN_FN uint32_t merge_limit(uint32_t maxDistance, uint32_t L) { return maxDistance >> (2u * (12u - L)); }

} // namespace ommx
