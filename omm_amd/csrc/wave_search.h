// wave_search.h -- which owner a work item belongs to, found by a whole wave in an exclusive scan of the owners' item counts (stats_kernels.hip:
// segments of blocks; geometry_kernels.hip: tiles of blocks and of primitives).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ommx {

// The owner of item `seg`: the last d with segStart[d] <= seg (segStart: exclusive scan of the item counts, segStart[0] = 0, so owners without
// items are passed over).  Every lane of the wave gets it.  The 64 lanes probe 64 evenly spaced entries at a time: three dependent loads for
// 2^18 owners where a binary search has eighteen.
__device__ __forceinline__ uint32_t owner_of_segment(const unsigned long long* __restrict__ segStart, uint32_t count, unsigned long long seg)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0u, n = count;
    while (n > 1u) {
        const uint32_t step = (n + 63u) >> 6;
        const uint64_t at = (uint64_t)lane * step;
        const bool le = at < n && segStart[lo + at] <= seg;   // a prefix of the lanes (lane 0 always)
        const uint32_t k = (uint32_t)__popcll(__ballot(le)) - 1u;
        lo += k * step;
        n = n - k * step < step ? n - k * step : step;
    }
    return lo;
}

} // namespace ommx
