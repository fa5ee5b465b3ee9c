// geometry_cut.h -- "the cut of 64", the one routine every tier of ommxExtractMicroGeometry shares (include/omm_mi355x_ext.h has the definition
// of the output).  Compiles as HIP device code (geometry_kernels.hip) and as plain C++ on the host (tests/native/geometry_check.cpp), the way
// stats_count.h does, so that the mask arithmetic is tested without a GPU.
//
// A word is up to 64 sibling subtrees -- the 4^k descendants, k <= 3 quad levels down, of one node of the bird curve, in curve order -- and for
// each of the five classes (output lists 0..3 and "dropped") a 64-bit mask of the entries that are wholly of that class.  An entry without a
// class is in no mask.  The cut decides, with shifts and ANDs on the masks, which nodes of the k levels below the word's own node are emitted
// and what the class of the word's node is.  The same routine serves a lane's 64 micro-triangles, the wave's ballot over its lanes' words,
// and the words of tile summaries above that.
#pragma once
#include <stdint.h>
#include "result_block.h"

#ifdef __HIPCC__
#define OMMX_GEO_FN __host__ __device__ __forceinline__
#define OMMX_GEO_UNROLL _Pragma("unroll")
#else
#define OMMX_GEO_FN static inline
#define OMMX_GEO_UNROLL
#endif

namespace ommx {

constexpr uint32_t kGeoDrop = 4u;        // the class of OMMX_GEOMETRY_DROP (classes 0..3 are the output lists)
constexpr uint32_t kGeoNoClass = 0xFFu;  // a node whose children differ

struct GeoCut {
    uint64_t start[4];   // per list: bit p = a node of that list is emitted whose first entry is entry p of the word (nodes are disjoint: one bit each)
    uint64_t up1, up2;   // of all those bits: the node lies one / two levels above the entries (neither: it is the entry itself)
    uint32_t whole;      // the class of the word's own node (0..4), or kGeoNoClass; that node is never emitted here -- its parent's word decides
};

// m[c]:   entries of class c (bits at or above 4^k are ignored)
// k:      quad levels in the word, 0..3: 4^k entries
// t:      level of the entries minus the emit level E.  Nodes deeper than E (j < t levels above the entries) are not emitted and only hand
//         their uniformity up; a node AT level E (j == t) that has no class gets the class `mixed`.
// mixed:  the class of such a node, 0..4
OMMX_GEO_FN GeoCut geo_cut64(const uint64_t m[5], uint32_t k, int32_t t, uint32_t mixed)
{
    const uint64_t valid = k >= 3u ? ~0ull : (1ull << (1u << (2u * k))) - 1ull;
    const uint64_t P1 = 0x1111111111111111ull, P2 = 0x0001000100010001ull;
    uint64_t q0[5], q1[5], q2[5], q3[5];
    uint64_t any1 = 0ull, any2 = 0ull, any3 = 0ull;
    OMMX_GEO_UNROLL
    for (uint32_t c = 0; c < 5u; ++c) {
        q0[c] = m[c] & valid;
        q1[c] = k >= 1u ? q0[c] & (q0[c] >> 1) & (q0[c] >> 2) & (q0[c] >> 3) & P1 : 0ull;
        any1 |= q1[c];
    }
    if (t == 1 && k >= 1u) {
        const uint64_t none = valid & P1 & ~any1;
        OMMX_GEO_UNROLL
        for (uint32_t c = 0; c < 5u; ++c) q1[c] |= c == mixed ? none : 0ull;
    }
    OMMX_GEO_UNROLL
    for (uint32_t c = 0; c < 5u; ++c) {
        q2[c] = k >= 2u ? q1[c] & (q1[c] >> 4) & (q1[c] >> 8) & (q1[c] >> 12) & P2 : 0ull;
        any2 |= q2[c];
    }
    if (t == 2 && k >= 2u) {
        const uint64_t none = valid & P2 & ~any2;
        OMMX_GEO_UNROLL
        for (uint32_t c = 0; c < 5u; ++c) q2[c] |= c == mixed ? none : 0ull;
    }
    OMMX_GEO_UNROLL
    for (uint32_t c = 0; c < 5u; ++c) {
        q3[c] = k >= 3u ? q2[c] & (q2[c] >> 16) & (q2[c] >> 32) & (q2[c] >> 48) & 1ull : 0ull;
        any3 |= q3[c];
    }
    if (t == 3 && k >= 3u) {
        OMMX_GEO_UNROLL
        for (uint32_t c = 0; c < 5u; ++c) q3[c] |= (c == mixed && !any3) ? 1ull : 0ull;
    }
    GeoCut g;
    g.up1 = 0ull; g.up2 = 0ull; g.whole = kGeoNoClass;
    OMMX_GEO_UNROLL
    for (uint32_t c = 0; c < 5u; ++c) {
        const uint64_t top = k == 0u ? q0[c] : k == 1u ? q1[c] : k == 2u ? q2[c] : q3[c];
        if (top & 1ull) g.whole = c;
        if (c == kGeoDrop) break;
        // a node with a class is emitted where its parent has none; q(j+1) is zero above the word's own level
        const uint64_t e0 = (k >= 1u && t <= 0) ? q0[c] & ~(q1[c] * 0xFull) : 0ull;
        const uint64_t e1 = (k >= 2u && t <= 1) ? q1[c] & ~(q2[c] * 0xFFFFull) : 0ull;
        const uint64_t e2 = (k >= 3u && t <= 2) ? q2[c] & ~(0ull - q3[c]) : 0ull;
        g.start[c] = e0 | e1 | e2;
        g.up1 |= e1; g.up2 |= e2;
    }
    return g;
}

// how many levels above the entries the node emitted at bit p lies
OMMX_GEO_FN uint32_t geo_up(const GeoCut& g, uint32_t p) { return (uint32_t)((g.up1 >> p) & 1ull) + 2u * (uint32_t)((g.up2 >> p) & 1ull); }

// The record of the node emitted at bit p of a word whose entries are the nodes first .. first + 4^k - 1 of `entryLevel`: level << 24 | index
OMMX_GEO_FN uint32_t geo_node(const GeoCut& g, uint32_t p, uint32_t entryLevel, uint32_t first)
{
    const uint32_t up = geo_up(g, p);
    return ((entryLevel - up) << 24) | ((first + p) >> (2u * up));
}

// ---- an OMM block's micro-triangles as class masks ----
// bits 0, 2, 4, ... of x gathered into the low 32 bits
OMMX_GEO_FN uint64_t geo_even_bits(uint64_t x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull; x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull; x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return x;
}

// 64 micro-triangles (w0: the first 64 bits of them, w1: the second 64 bits of an OC1_4_State word) -> m[c] = those whose state maps to class c.
// cls[s] = class of ommOpacityState s (0..4).  fieldBits 1: the bit is the state (Transparent / Opaque); 2: low bit, high bit.
OMMX_GEO_FN void geo_class_masks(uint64_t w0, uint64_t w1, uint32_t fieldBits, const uint8_t cls[4], uint64_t m[5])
{
    uint64_t s[4];
    if (fieldBits == 1u) { s[0] = ~w0; s[1] = w0; s[2] = 0ull; s[3] = 0ull; }
    else {
        const uint64_t lo = geo_even_bits(w0) | (geo_even_bits(w1) << 32), hi = geo_even_bits(w0 >> 1) | (geo_even_bits(w1 >> 1) << 32);
        s[0] = ~lo & ~hi; s[1] = lo & ~hi; s[2] = hi & ~lo; s[3] = lo & hi;
    }
    OMMX_GEO_UNROLL
    for (uint32_t c = 0; c < 5u; ++c) {
        m[c] = 0ull;
        OMMX_GEO_UNROLL
        for (uint32_t k = 0; k < 4u; ++k) m[c] |= cls[k] == c ? s[k] : 0ull;
    }
}

} // namespace ommx
