// coarsen_reduce.h -- the word arithmetic of ommxCoarsenMicromap (include/omm_mi355x_ext.h has the definition): the states of 4^n sibling
// micro-triangles become the one state of their parent, n = 1..3 quad levels up, for 64 fields at a time with shifts and masks.  Compiles as
// HIP device code (coarsen_kernels.hip) and as plain C++ on the host (tests/native/coarsen_check.cpp), the way geometry_cut.h and stats_count.h
// do, so that the masks are tested without a GPU.
//
// 64 fields are held as two bit planes: `lo` has the low bit of every field (the side: 0 transparent, 1 opaque), `hi` the high bit (unknown).
// A 2-state block has no high bits: its words ARE low planes and its high planes are zero.  The rule for a group of covered states: the sides
// differ -> mixedState; otherwise side | (any unknown ? 2 : 0).  With A = AND of the low bits, O = OR of the low bits, U = OR of the high bits
// of the group: mixed = O & ~A, low' = A | (mixed & mixedState.bit0), high' = U | mixed (mixedState is 2 or 3: its high bit is set).
// The rule is associative, so any split of a deep reduction into steps of one to three levels gives the same bits.
#pragma once
#include <stdint.h>
#include "result_block.h"

#ifdef __HIPCC__
#define OMMX_COARSEN_FN __host__ __device__ __forceinline__
#else
#define OMMX_COARSEN_FN static inline
#endif

namespace ommx {

struct CoarsenPlanes { uint64_t lo, hi; };   // field f is bit f of both

// AND / OR over every aligned group of 4^n bits (n = 0..3), left at the group's first bit; the other bits are of no use
OMMX_COARSEN_FN uint64_t coarsen_group_and(uint64_t x, uint32_t n)
{
    if (n >= 1u) { x &= x >> 1; x &= x >> 2; }
    if (n >= 2u) { x &= x >> 4; x &= x >> 8; }
    if (n >= 3u) { x &= x >> 16; x &= x >> 32; }
    return x;
}
OMMX_COARSEN_FN uint64_t coarsen_group_or(uint64_t x, uint32_t n)
{
    if (n >= 1u) { x |= x >> 1; x |= x >> 2; }
    if (n >= 2u) { x |= x >> 4; x |= x >> 8; }
    if (n >= 3u) { x |= x >> 16; x |= x >> 32; }
    return x;
}
// the bits at the multiples of 4^n gathered into the low 64 >> 2n bits
OMMX_COARSEN_FN uint64_t coarsen_compact(uint64_t x, uint32_t n)
{
    if (n == 1u) {
        x &= 0x1111111111111111ull;
        x = (x | (x >> 3)) & 0x0303030303030303ull; x = (x | (x >> 6)) & 0x000f000f000f000full;
        x = (x | (x >> 12)) & 0x000000ff000000ffull; x = (x | (x >> 24)) & 0x000000000000ffffull;
    } else if (n == 2u) {
        x &= 0x0001000100010001ull;
        x = (x | (x >> 15)) & 0x0000000300000003ull; x = (x | (x >> 30)) & 0xfull;
    } else if (n >= 3u) x &= 1ull;
    return x;
}

// 64 fields -> the 64 >> 2n states of their ancestors n levels up (n = 0..3), in the low bits of both planes; the bits above are zero.
// fieldBits 1: the high plane stays zero and a mixed group becomes mixedState & 1.
OMMX_COARSEN_FN CoarsenPlanes coarsen_reduce_planes(CoarsenPlanes p, uint32_t n, uint32_t fieldBits, uint32_t mixedState)
{
    if (n == 0u) return p;
    const uint64_t a = coarsen_group_and(p.lo, n), o = coarsen_group_or(p.lo, n), u = coarsen_group_or(p.hi, n);
    const uint64_t mixed = o & ~a;
    CoarsenPlanes q;
    q.lo = coarsen_compact(a | ((mixedState & 1u) ? mixed : 0ull), n);
    q.hi = fieldBits == 2u ? coarsen_compact(u | mixed, n) : 0ull;
    return q;
}

// bits 0, 2, 4, ... of x gathered into the low 32 bits, and back
OMMX_COARSEN_FN uint64_t coarsen_even_bits(uint64_t x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull; x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull; x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return x;
}
OMMX_COARSEN_FN uint64_t coarsen_spread_bits(uint64_t x)
{
    x &= 0x00000000ffffffffull;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull; x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full; x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
// two consecutive words of a 4-state block (32 fields each) <-> the planes of their 64 fields
OMMX_COARSEN_FN CoarsenPlanes coarsen_split(uint64_t w0, uint64_t w1)
{
    CoarsenPlanes p;
    p.lo = coarsen_even_bits(w0) | (coarsen_even_bits(w1) << 32);
    p.hi = coarsen_even_bits(w0 >> 1) | (coarsen_even_bits(w1 >> 1) << 32);
    return p;
}
OMMX_COARSEN_FN void coarsen_join(CoarsenPlanes p, uint64_t* w0, uint64_t* w1)
{
    *w0 = coarsen_spread_bits(p.lo) | (coarsen_spread_bits(p.hi) << 1);
    *w1 = coarsen_spread_bits(p.lo >> 32) | (coarsen_spread_bits(p.hi >> 32) << 1);
}

// One word of a block reduced by n levels: fieldBits 1: 64 fields, n <= 3; fieldBits 2: 32 fields, n <= 2.  The result is packed like the input.
OMMX_COARSEN_FN uint64_t coarsen_reduce_word(uint64_t w, uint32_t n, uint32_t fieldBits, uint32_t mixedState)
{
    CoarsenPlanes p;
    if (fieldBits == 2u) p = coarsen_split(w, 0ull); else { p.lo = w; p.hi = 0ull; }
    p = coarsen_reduce_planes(p, n, fieldBits, mixedState);
    if (fieldBits == 1u) return p.lo & (n == 0u ? ~0ull : (1ull << (64u >> (2u * n))) - 1ull);
    uint64_t r0, r1;
    coarsen_join(p, &r0, &r1);
    return r0 & (n == 0u ? ~0ull : (1ull << (64u >> (2u * n))) - 1ull);
}

// Which states s have every field in the low validBits bits of w (a multiple of fieldBits, 1..64) equal to s: bit s of the answer.  At most one
// bit is set; AND the answers of a block's words and the block is uniform when a bit survives.
OMMX_COARSEN_FN uint32_t coarsen_word_uniform(uint64_t w, uint32_t validBits, uint32_t fieldBits)
{
    const uint64_t valid = validBits >= 64u ? ~0ull : (1ull << validBits) - 1ull;
    if (fieldBits == 1u) return (((w & valid) == 0ull) ? 1u : 0u) | (((~w & valid) == 0ull) ? 2u : 0u);
    const uint64_t lo = 0x5555555555555555ull, hi = 0xaaaaaaaaaaaaaaaaull;
    return (((w & valid) == 0ull) ? 1u : 0u) | ((((w ^ lo) & valid) == 0ull) ? 2u : 0u) | ((((w ^ hi) & valid) == 0ull) ? 4u : 0u) | (((~w & valid) == 0ull) ? 8u : 0u);
}

} // namespace ommx
