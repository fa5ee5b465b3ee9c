// combine_kernels.h -- ommxCombineMicromaps: one conservative device-resident result from up to 16 results over the same primitives
// (combine_kernels.hip; the definition is in include/omm_mi355x_ext.h).  omm_host.cpp owns the baker, its device pool, the argument checks and
// the result handle; the four calls below are the phases between which the host has to size a block of memory.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"
#include "rebuild_kernels.h"

namespace ommx {

struct CombineArgs {
    ResultView source[OMMX_COMBINE_MAX_SOURCES];   // (result_read.h)
    uint32_t sourceCount;          // 1..16
    uint32_t indexCount;           // of every source, > 0
    uint32_t format;               // of every output block: 1 or 2
    uint32_t mixedState;           // 2 or 3
};
struct CombineTuples {             // after the index buffers have been read
    uint32_t tuples, skipped;      // distinct tuples with a block among their entries; skipped primitives
};
struct CombinePlan {               // after the tuples have been listed
    uint64_t stagingBytes;         // the arena the joined blocks are written to before their order is known
    uint64_t units;                // work units of the streaming pass
    uint32_t refined;              // tuples with a block coarser than their output
};

size_t combine_head_bytes(const CombineArgs& a);                     // scratch per primitive
size_t combine_tuple_bytes(const CombineArgs& a, uint32_t tuples);   // scratch per tuple
// each: every launch on `stream`, the answer copied to the host, the stream synchronised
hipError_t combine_tuples(const CombineArgs& a, void* head, CombineTuples* out, hipStream_t stream);
hipError_t combine_plan(const CombineArgs& a, void* head, void* perTuple, const CombineTuples& t, CombinePlan* out, hipStream_t stream);
hipError_t combine_join(const CombineArgs& a, void* perTuple, void* staging, const CombineTuples& t, const CombinePlan& plan, RebuildCounts* out, hipStream_t stream);
// perTuple and staging may be null when t.tuples == 0; o.index: 32-bit entries
hipError_t combine_emit(const CombineArgs& a, void* head, void* perTuple, const void* staging, const CombineTuples& t, const RebuildCounts& counts,
                        const RebuildOutputs& o, hipStream_t stream);

} // namespace ommx
