// compare_count.h -- the word arithmetic of ommxCompareMicromaps (include/omm_mi355x_ext.h has the definition): the states of two results for the
// same 64 micro-triangles, held as bit planes (coarsen_reduce.h), counted into the 4 x 4 confusion matrix [stateA][stateB], and the relation byte of
// a matrix.  Compiles as HIP device code (compare_kernels.hip) and as plain C++ on the host (tests/native/compare_check.cpp), like combine_expand.h.
//
// Per side the planes become four masks, one per state: mask s has the bit of every field whose state is s.  ANDed with the mask of valid fields,
// the four masks of a side partition the valid fields, so the sixteen popcounts of maskA[sa] & maskB[sb] add up to the number of valid fields
// exactly.  The valid mask matters: the planes of a block of fewer than 64 fields are zero above its last field (result_words.h), and two zeros
// would count as (Transparent, Transparent).
#pragma once
#include <stdint.h>
#include "coarsen_reduce.h"

namespace ommx {

constexpr uint32_t kRelationConflict = 0x01u, kRelationAWeaker = 0x02u, kRelationBWeaker = 0x04u, kRelationHint = 0x08u, kRelationSkipped = 0x80u;

// the low `fields` bits (1..64)
OMMX_COARSEN_FN uint64_t compare_valid_mask(uint32_t fields) { return fields >= 64u ? ~0ull : (1ull << fields) - 1ull; }

struct CompareMasks { uint64_t m[4]; };   // m[s]: the valid fields in state s
// force2: every state s counts as s & 1 (the high plane is ignored)
OMMX_COARSEN_FN CompareMasks compare_state_masks(CoarsenPlanes p, uint64_t valid, uint32_t force2)
{
    const uint64_t hi = force2 ? 0ull : p.hi;
    CompareMasks k;
    k.m[0] = ~p.lo & ~hi & valid; k.m[1] = p.lo & ~hi & valid; k.m[2] = ~p.lo & hi & valid; k.m[3] = p.lo & hi & valid;
    return k;
}
// acc[4 * sa + sb] += the number of valid fields in state sa in `a` and sb in `b`
OMMX_COARSEN_FN void compare_count_add(CoarsenPlanes a, CoarsenPlanes b, uint64_t valid, uint32_t force2, uint32_t acc[16])
{
    const CompareMasks ka = compare_state_masks(a, valid, force2), kb = compare_state_masks(b, ~0ull, force2);
    for (int sa = 0; sa < 4; ++sa)   // (constant bounds: unrolled, acc stays in registers)
        for (int sb = 0; sb < 4; ++sb) acc[4 * sa + sb] += (uint32_t)__builtin_popcountll(ka.m[sa] & kb.m[sb]);
}

// the bit of the off-diagonal cell [sa][sb]; 0 on the diagonal
OMMX_COARSEN_FN uint32_t compare_cell_relation(uint32_t sa, uint32_t sb)
{
    if (sa == sb) return 0u;
    if (sa < 2u) return sb < 2u ? kRelationConflict : kRelationBWeaker;
    return sb < 2u ? kRelationAWeaker : kRelationHint;
}
// the relation of a matrix: the OR of the bits of its non-zero off-diagonal cells
OMMX_COARSEN_FN uint32_t compare_relation(const uint32_t m[16])
{
    uint32_t r = 0u;
    for (uint32_t c = 0; c < 16u; ++c)
        if (m[c]) r |= compare_cell_relation(c >> 2, c & 3u);
    return r;
}

} // namespace ommx
