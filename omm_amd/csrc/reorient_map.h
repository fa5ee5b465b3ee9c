// reorient_map.h -- the index map of ommxReorientMicromap as a digit-by-digit transducer, and a tile of 64 fields moved through it
// (include/omm_mi355x_lookup.h, ommx_reorient_index, states the rule; include/omm_mi355x_ext.h the entry).  Compiles as HIP device code
// (reorient_kernels.hip) and as plain C++ on the host (tests/native/reorient_check.cpp holds it to ommx_reorient_index), like gather_copy.h.
//
// The bird curve splits a triangle into its three corner children and the inverted middle one, and a re-ordering of the vertices maps children to
// children.  So the source index of an output index is found digit by digit from the most significant one: the output digit c' under a node whose
// sub-map is `state` gives the source digit emit(state, c'), and the sub-map below that child is next(state, c').  Only SIX sub-maps occur at any
// depth, and they are the maps of the six orientations themselves: the state is an orientation code, and the walk starts in the call's own.
//     emit   state 0: 0 1 2 3   1: 2 1 3 0   2: 3 1 0 2   3: 0 1 3 2   4: 3 1 2 0   5: 2 1 0 3      (= ommx_reorient_index at level 1)
//     next   state 0: 0 0 0 0   1: 1 2 3 4   2: 4 1 2 3   3: 3 4 1 2   4: 2 3 4 1   5: 5 5 5 5
// Five bits per (state, digit), emit | next << 2, at bit 5 * (4 * (state % 3) + digit) of the constant of states 0..2 or of states 3..5.
// tests/test_reorient.py rebuilds both constants from the forward decode.
//
// A TILE is a node three digits above the fields: 64 fields, one 64-bit word of a 2-state block, one 16-byte vector of a 4-state block.  The walk over
// the digits above the tile gives the source tile and the tile's state; inside the tile the sixteen nodes one digit above the fields (four fields: a
// nibble or a byte) are placed through two small tables per state -- `node`: which source nibble / byte, and in which state; `quad`: that nibble /
// byte with its four fields re-ordered.
#pragma once
#include <stdint.h>
#include "gather_copy.h"   // OMMX_COARSEN_FN, the reads of a source block

namespace ommx {

constexpr uint64_t kReorientCodes012 = 0x720b383d2618820ull;
constexpr uint64_t kReorientCodes345 = 0xbd2b6249ab51e2cull;
constexpr uint32_t kReorientStates = 6;
constexpr uint32_t kReorientTileDepth = 3;
constexpr uint32_t kReorientTileFields = 1u << (2u * kReorientTileDepth);

// emit | next << 2 of output digit c' under `state` (0..5)
OMMX_COARSEN_FN uint32_t reorient_code(uint32_t state, uint32_t digit)
{
    const uint64_t codes = state < 3u ? kReorientCodes012 : kReorientCodes345;
    return (uint32_t)(codes >> (5u * (4u * (state < 3u ? state : state - 3u) + digit))) & 31u;
}
// `digits` digits of `index`, most significant first, from *state on: the source digits; *state <- the state below the last one.  The trip count is
// `digits`, whatever the digits are.
OMMX_COARSEN_FN uint32_t reorient_walk(uint32_t index, uint32_t digits, uint32_t* state)
{
    uint32_t source = 0u, s = *state;
    for (uint32_t i = digits; i-- > 0u;) {
        const uint32_t code = reorient_code(s, (index >> (2u * i)) & 3u);
        source = (source << 2) | (code & 3u);
        s = code >> 2;
    }
    *state = s;
    return source;
}

// ---- the tables of a tile: LDS in the kernel, built once per workgroup ----
struct ReorientTables {
    uint8_t node[kReorientStates][16];    // output node n' (two digits) of a tile in `state`: source node | its state << 4
    uint8_t quad2[kReorientStates][16];   // a nibble of four 1-bit fields under a node in `state`, re-ordered
    uint8_t quad4[kReorientStates][256];  // a byte of four 2-bit fields, re-ordered
};
constexpr uint32_t kReorientTableEntries = (uint32_t)sizeof(ReorientTables);   // 1728
// entry i of the tables, i < kReorientTableEntries: every entry is a function of its own position
OMMX_COARSEN_FN void reorient_tables_fill(ReorientTables* T, uint32_t i)
{
    if (i < 16u * kReorientStates) {
        uint32_t s = i >> 4;
        const uint32_t source = reorient_walk(i & 15u, 2u, &s);
        T->node[i >> 4][i & 15u] = (uint8_t)(source | (s << 4));
        return;
    }
    i -= 16u * kReorientStates;
    const bool two = i < 16u * kReorientStates;
    if (!two) i -= 16u * kReorientStates;
    const uint32_t state = two ? i >> 4 : i >> 8, value = two ? i & 15u : i & 255u, bits = two ? 1u : 2u;
    uint32_t out = 0u;
    for (uint32_t c = 0; c < 4u; ++c) out |= ((value >> (bits * (reorient_code(state, c) & 3u))) & ((1u << bits) - 1u)) << (bits * c);
    if (two) T->quad2[state][value] = (uint8_t)out; else T->quad4[state][value] = (uint8_t)out;
}

// the 64 fields of a tile in `state`: the source tile's word(s) in, the output tile's out
OMMX_COARSEN_FN uint64_t reorient_tile2(const ReorientTables* T, uint32_t state, uint64_t w)
{
    uint64_t out = 0ull;
    for (uint32_t n = 0; n < 16u; ++n) {
        const uint32_t nd = T->node[state][n];
        out |= (uint64_t)T->quad2[nd >> 4][(uint32_t)(w >> (4u * (nd & 15u))) & 15u] << (4u * n);
    }
    return out;
}
OMMX_COARSEN_FN GatherWords reorient_tile4(const ReorientTables* T, uint32_t state, GatherWords w)
{
    GatherWords out; out.w0 = 0ull; out.w1 = 0ull;
    for (uint32_t n = 0; n < 16u; ++n) {
        const uint32_t nd = T->node[state][n], at = nd & 15u;
        const uint64_t b = T->quad4[nd >> 4][(uint32_t)((at < 8u ? w.w0 : w.w1) >> (8u * (at & 7u))) & 255u];
        if (n < 8u) out.w0 |= b << (8u * n); else out.w1 |= b << (8u * (n - 8u));
    }
    return out;
}

// tile `tile` of the source block of `bytes` bytes at `block` (any byte address; nothing outside the block is read): its word in w0 (2-state, bits 1)
// or its two words (4-state, bits 2)
OMMX_COARSEN_FN GatherWords reorient_source_tile(const uint8_t* block, uint64_t bytes, uint32_t bits, uint32_t tile)
{
    if (bits == 2u) return gather_vector(block, bytes, tile);
    GatherWords g = gather_vector(block, bytes, tile >> 1);
    if (tile & 1u) g.w0 = g.w1;
    return g;
}

// a block below a tile (level < 3: at most 16 fields in `word`), field by field through ommx_reorient_index's rule as the walk states it
OMMX_COARSEN_FN uint64_t reorient_small(uint64_t word, uint32_t level, uint32_t bits, uint32_t orientation)
{
    uint64_t out = 0ull;
    for (uint32_t j = 0; j < (1u << (2u * level)); ++j) {
        uint32_t s = orientation;
        const uint32_t source = reorient_walk(j, level, &s);
        out |= ((word >> (bits * source)) & ((1ull << bits) - 1ull)) << (bits * j);
    }
    return out;
}

} // namespace ommx
