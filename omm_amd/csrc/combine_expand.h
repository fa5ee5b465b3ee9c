// combine_expand.h -- the word arithmetic of ommxCombineMicromaps (include/omm_mi355x_ext.h has the definition): a coarser block read at a finer
// level, and the states of K sources for the same micro-triangles joined into one.  Compiles as HIP device code (combine_kernels.hip) and as plain
// C++ on the host (tests/native/combine_check.cpp), like coarsen_reduce.h, whose bit planes, plane split and plane join it uses.
//
// Repetition: micro-triangle j of level L covers micro-triangles [j * 4^n, (j + 1) * 4^n) of level L + n (the bird curve is hierarchical), so a
// field read n levels down becomes 4^n equal fields.  For n = 1..3 that stays within a word: the low 64 >> 2n bits of a plane are spread to the
// multiples of 4^n (the inverse of coarsen_compact) and multiplied by 4^n ones.  Above that every output word is one field broadcast.
//
// Join: the rule of coarsen_reduce.h over the K answers for one field instead of over the 4^n fields of a group.  With A = AND of the low planes,
// O = OR of the low planes, U = OR of the high planes: mixed = O & ~A, lo' = A | (mixed & mixedState.bit0), hi' = U | mixed.
#pragma once
#include <stdint.h>
#include "coarsen_reduce.h"

namespace ommx {

// the low 64 >> 2n bits of x (n = 1..3), each repeated 4^n times; the bits above them are ignored
OMMX_COARSEN_FN uint64_t combine_repeat_bits(uint64_t x, uint32_t n)
{
    if (n == 1u) {
        x &= 0x000000000000ffffull;
        x = (x | (x << 24)) & 0x000000ff000000ffull; x = (x | (x << 12)) & 0x000f000f000f000full;
        x = (x | (x << 6)) & 0x0303030303030303ull; x = (x | (x << 3)) & 0x1111111111111111ull;
        return x * 0xfull;
    }
    if (n == 2u) {
        x &= 0xfull;
        x = (x | (x << 30)) & 0x0000000300000003ull; x = (x | (x << 15)) & 0x0001000100010001ull;
        return x * 0xffffull;
    }
    return 0ull - (x & 1ull);
}
// the low 64 >> 2n fields of p (n = 0..3) read n levels down: 64 fields
OMMX_COARSEN_FN CoarsenPlanes combine_repeat_planes(CoarsenPlanes p, uint32_t n)
{
    if (n == 0u) return p;
    CoarsenPlanes q; q.lo = combine_repeat_bits(p.lo, n); q.hi = combine_repeat_bits(p.hi, n);
    return q;
}
// 64 fields of one state 0..3: a special index, or one field read more than three levels down
OMMX_COARSEN_FN CoarsenPlanes combine_broadcast(uint32_t state)
{
    CoarsenPlanes q; q.lo = 0ull - (uint64_t)(state & 1u); q.hi = 0ull - (uint64_t)((state >> 1) & 1u);
    return q;
}

// the join of any number of plane pairs, one at a time and in any order
struct CombineJoin { uint64_t a, o, u; };
OMMX_COARSEN_FN CombineJoin combine_join_begin() { CombineJoin j; j.a = ~0ull; j.o = 0ull; j.u = 0ull; return j; }
OMMX_COARSEN_FN void combine_join_add(CombineJoin& j, CoarsenPlanes p) { j.a &= p.lo; j.o |= p.lo; j.u |= p.hi; }
// 64 joined fields; fieldBits 1: the high plane is zero and a mixed field is mixedState & 1
OMMX_COARSEN_FN CoarsenPlanes combine_join_end(CombineJoin j, uint32_t fieldBits, uint32_t mixedState)
{
    const uint64_t mixed = j.o & ~j.a;
    CoarsenPlanes q;
    q.lo = j.a | ((mixedState & 1u) ? mixed : 0ull);
    q.hi = fieldBits == 2u ? (j.u | mixed) : 0ull;
    return q;
}

} // namespace ommx
