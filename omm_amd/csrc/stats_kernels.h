// stats_kernels.h -- ommDebugStats of a result whose arrays are device memory (stats_kernels.hip).  Entry points: ommxDebugGetStatsDevice /
// ommxDebugGetStatsDevice2 (omm_host.cpp owns the baker, its device pool and the argument checks).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"

namespace ommx {

// what the kernels leave for the host: one small copy.  state[] is indexed by ommOpacityState, special[] by -(index + 1).
struct StatsTotals {
    unsigned long long state[4];
    uint32_t special[4];
    uint32_t skipped, pad;
    double knownArea, totalArea;   // fp64 sums over the primitives in a fixed order (0 without areas)
};

struct StatsArgs {
    ommCpuBakeResultDesc result;   // host struct, arrays in device memory; indexFormat already checked
    const float* areas;            // indexCount floats, or null
    uint32_t* stateCounts;         // [descArrayCount][4] of the caller, or null: taken from the scratch block
    uint32_t* referenceCounts;     // [descArrayCount] of the caller, or null: taken from the scratch block
    float* knownFraction;          // [indexCount] of the caller, or null
};

// device scratch of one call (a function of the sizes and of which outputs the caller brought) and the call itself: every launch on `stream`,
// the totals copied to *out, the stream synchronised.  indexCount must be > 0.
size_t stats_scratch_bytes(const StatsArgs& a);
hipError_t launch_stats(const StatsArgs& a, void* scratch, StatsTotals* out, hipStream_t stream);

} // namespace ommx
