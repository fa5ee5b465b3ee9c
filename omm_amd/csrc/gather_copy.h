// gather_copy.h -- the address and shift arithmetic of ommxGatherMicromaps' copy (include/omm_mi355x_ext.h has the definition): sixteen bytes of a
// block that lies at ANY byte address, read without touching a byte outside the block.  Compiles as HIP device code (gather_kernels.hip) and as plain
// C++ on the host (tests/native/gather_check.cpp, where the block sits in an exact-size allocation under AddressSanitizer), like combine_expand.h.
//
// Output vector j of a block of `bytes` bytes is its bytes [16j, 16j + 16), zeros where the block has ended.  With s = (address of byte 16j) & 15:
//   s == 0   one aligned 16-byte load.
//   s != 0   the aligned vectors L (at address - s) and H (at address - s + 16) hold the sixteen bytes between them: (L >> 8s) | (H << 8(16 - s)) on
//            128 bits.  L of the block's FIRST vector starts in front of the block and H of its LAST vector ends behind it, so those halves are read
//            byte by byte instead; every other L and H lies inside the block.
// The rule is stated for any length (a block of the library is 1, 2, 4, 8 or a multiple of 16 bytes; the native check walks every length): a vector,
// whole or half, is loaded as a vector only if all sixteen bytes of the load lie inside the block.
// Every read goes through gather_aligned or gather_bytes; OMMX_GATHER_READ(p, n), when defined, sees each of them first (the native check's witness).
#pragma once
#include <stdint.h>
#include "coarsen_reduce.h"

#ifndef OMMX_GATHER_READ
#define OMMX_GATHER_READ(p, n) ((void)0)
#endif

namespace ommx {

typedef uint64_t GatherVec __attribute__((vector_size(16), may_alias));   // sixteen bytes at a 16-byte aligned address, as one load

struct GatherWords { uint64_t w0, w1; };   // sixteen bytes, little endian: byte b is bits [8b, 8b + 8) of w0 (b < 8) or of w1

OMMX_COARSEN_FN uint32_t gather_shift(const uint8_t* p) { return (uint32_t)((uintptr_t)p & 15u); }

// n = 0..16 bytes from p, one load each, into the low bytes; the others are zero
OMMX_COARSEN_FN GatherWords gather_bytes(const uint8_t* p, uint32_t n)
{
    GatherWords r; r.w0 = 0ull; r.w1 = 0ull;
    OMMX_GATHER_READ(p, n);
    for (uint32_t b = 0; b < n; ++b) {
        const uint64_t v = (uint64_t)p[b] << (8u * (b & 7u));
        if (b < 8u) r.w0 |= v; else r.w1 |= v;
    }
    return r;
}
// x >> 8n and x << 8n on 128 bits, n = 1..15
OMMX_COARSEN_FN GatherWords gather_down(GatherWords x, uint32_t n)
{
    GatherWords r;
    if (n < 8u) { r.w0 = (x.w0 >> (8u * n)) | (x.w1 << (64u - 8u * n)); r.w1 = x.w1 >> (8u * n); }
    else { r.w0 = x.w1 >> (8u * (n - 8u)); r.w1 = 0ull; }
    return r;
}
OMMX_COARSEN_FN GatherWords gather_up(GatherWords x, uint32_t n)
{
    GatherWords r;
    if (n < 8u) { r.w1 = (x.w1 << (8u * n)) | (x.w0 >> (64u - 8u * n)); r.w0 = x.w0 << (8u * n); }
    else { r.w1 = x.w0 << (8u * (n - 8u)); r.w0 = 0ull; }
    return r;
}
OMMX_COARSEN_FN GatherWords gather_aligned(const uint8_t* p)
{
    OMMX_GATHER_READ(p, 16u);
    const GatherVec v = *(const GatherVec*)p;
    GatherWords r; r.w0 = v[0]; r.w1 = v[1];
    return r;
}

// bytes [16j, 16j + 16) of the block of `bytes` bytes at `block`, 16j < bytes; zeros behind the block's end.  No byte outside the block is read.
OMMX_COARSEN_FN GatherWords gather_vector(const uint8_t* block, uint64_t bytes, uint64_t j)
{
    const uint8_t* a = block + 16u * j;
    const uint64_t avail = bytes - 16u * j;               // >= 1
    const uint32_t want = avail < 16u ? (uint32_t)avail : 16u;
    const uint32_t s = gather_shift(a);
    if (s == 0u) return want == 16u ? gather_aligned(a) : gather_bytes(a, want);
    const uint32_t low = 16u - s;                         // how many of the sixteen bytes L holds
    GatherWords r = j != 0u && avail >= low ? gather_down(gather_aligned(a - s), s) : gather_bytes(a, want < low ? want : low);
    if (want > low) {
        const GatherWords h = gather_up(avail >= low + 16u ? gather_aligned(a + low) : gather_bytes(a + low, want - low), low);
        r.w0 |= h.w0; r.w1 |= h.w1;
    }
    return r;
}

// a block below 16 bytes (1, 2, 4 or 8) as one word: its bytes one by one, the unused bits of a one-byte block cleared
OMMX_COARSEN_FN uint64_t gather_small(const uint8_t* block, uint32_t bytes, uint32_t level, uint32_t fieldBits)
{
    uint64_t w = gather_vector(block, bytes, 0u).w0;
    const uint32_t used = fieldBits << (2u * level);   // level <= 3 here
    if (used < 8u) w &= (1ull << used) - 1ull;
    return w;
}

} // namespace ommx
