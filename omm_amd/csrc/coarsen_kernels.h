// coarsen_kernels.h -- ommxCoarsenMicromap: a device-resident result capped at a subdivision level (coarsen_kernels.hip; the definition is in
// include/omm_mi355x_ext.h).  omm_host.cpp owns the baker, its device pool, the argument checks and the result handle; the three calls below
// are the phases between which the host has to size a block of memory.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"
#include "rebuild_kernels.h"

namespace ommx {

struct CoarsenArgs {
    ommCpuBakeResultDesc result;   // host struct, arrays in device memory; indexFormat already checked
    uint32_t maxLevel;             // clamped to 12
    const uint8_t* blockLevels;    // [descArrayCount] device memory: a cap per source descriptor (>= 12: none), or null (ommxCoarsenMicromap)
    uint32_t mixedState;           // 2 or 3
    uint32_t flags;                // ommxCoarsenFlags
};
struct CoarsenPlan {               // after the index buffer has been read
    uint64_t stagingBytes;         // the arena the reduced blocks are written to before their order is known
    uint32_t skipped, deepBlocks;  // skipped primitives; blocks that need a second reduction pass
    uint32_t referenced, coarsened;   // selected blocks; those above their target
};

size_t coarsen_head_bytes(const CoarsenArgs& a);
// each: every launch on `stream`, the answer copied to the host, the stream synchronised.  indexCount must be > 0.
hipError_t coarsen_plan(const CoarsenArgs& a, void* head, CoarsenPlan* out, hipStream_t stream);
hipError_t coarsen_reduce(const CoarsenArgs& a, void* head, void* staging, const CoarsenPlan& plan, RebuildCounts* out, hipStream_t stream);
hipError_t coarsen_emit(const CoarsenArgs& a, void* head, const void* staging, const RebuildCounts& counts, const RebuildOutputs& o, hipStream_t stream);   // o.index: the source's format

} // namespace ommx
