// gather_kernels.h -- ommxGatherMicromaps: one device-resident result from chosen primitives of up to 4096 results (gather_kernels.hip; the
// definition is in include/omm_mi355x_ext.h).  omm_host.cpp owns the baker, its device pool, the argument checks and the result handle; the three
// calls below are the phases between which the host has to size a block of memory.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"
#include "rebuild_kernels.h"

namespace ommx {

struct GatherSource {              // a row of the source table
    ResultView view;               // (result_read.h)
    uint32_t primBase, descBase;   // exclusive scans of indexCount and descCount over the sources
};
struct GatherArgs {
    const GatherSource* sources;   // HOST memory, sourceCount rows with their scans filled in; uploaded once by gather_plan
    uint32_t sourceCount;          // 1..OMMX_GATHER_MAX_SOURCES
    const ommxPrimitiveRef* selection;   // device memory, or null: the concatenation
    uint32_t primitiveCount;       // of the output, > 0
    uint32_t descTotal;            // the sum of descCount: the items of the tail
    uint32_t flags;                // ommxGatherFlags
};
struct GatherPlan {                // after the selection and the index buffers have been read
    uint64_t stagingBytes;         // the arena the blocks are copied to before their order is known
    uint64_t units;                // work units of the copy
    uint32_t skipped, referenced;  // skipped primitives; distinct accepted (source, descriptor) pairs
};

size_t gather_head_bytes(const GatherArgs& a);
// each: every launch on `stream`, the answer copied to the host, the stream synchronised
hipError_t gather_plan(const GatherArgs& a, void* head, GatherPlan* out, hipStream_t stream);
// staging may be null when plan.units == 0
hipError_t gather_stage(const GatherArgs& a, void* head, void* staging, const GatherPlan& plan, RebuildCounts* out, hipStream_t stream);
hipError_t gather_emit(const GatherArgs& a, void* head, const void* staging, const RebuildCounts& counts, const RebuildOutputs& o, hipStream_t stream);   // o.index: 32-bit entries

} // namespace ommx
