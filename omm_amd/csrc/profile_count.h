// profile_count.h -- one level of ommxProfileMicromapLevels (include/omm_mi355x_ext.h has the definition) on a plane pair: of up to 64 fields, how
// many are known and how many of those are opaque; and the step to the next coarser level, which is the coarsening's own (coarsen_reduce.h) with
// every block read as a 4-state block and a mixed group made unknown.  Compiles as HIP device code (fit_kernels.hip) and as plain C++ on the host
// (tests/native/fit_check.cpp), the way coarsen_reduce.h does.
//
// A field is known when its high bit is clear: its side is then its low bit.  A 2-state block has no high bits, so all its fields are known; after a
// step the high bit of a group is set exactly when the group held both sides (or an unknown field), whatever the format was.  load_fields
// (result_words.h) and the reductions leave zeros above the last field; zeros read as "known transparent", so every count masks them out.
#pragma once
#include <stdint.h>
#include "coarsen_reduce.h"

namespace ommx {

constexpr uint32_t kProfileLevels = 13u;   // OMMX_PROFILE_LEVELS: a row has one count per level 0..12

struct ProfileCount { uint32_t known, opaque; };

// the low `fields` bits (fields <= 64)
OMMX_COARSEN_FN uint64_t profile_valid(uint32_t fields) { return fields >= 64u ? ~0ull : (1ull << fields) - 1ull; }

OMMX_COARSEN_FN uint32_t profile_popcount(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}

// of the first `fields` fields of p
OMMX_COARSEN_FN ProfileCount profile_count(CoarsenPlanes p, uint32_t fields)
{
    const uint64_t known = ~p.hi & profile_valid(fields);
    ProfileCount c; c.known = profile_popcount(known); c.opaque = profile_popcount(p.lo & known);
    return c;
}

// 64 fields -> the 16 states of their parents in the low bits: a parent is known when its four children are known and of one side
OMMX_COARSEN_FN CoarsenPlanes profile_step(CoarsenPlanes p) { return coarsen_reduce_planes(p, 1u, 2u, 3u); }

} // namespace ommx
