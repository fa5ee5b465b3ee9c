// reorient_kernels.h -- ommxReorientMicromap: a device-resident result for triangles whose vertices were re-ordered (reorient_kernels.hip; the
// definition is in include/omm_mi355x_ext.h).  omm_host.cpp owns the baker, its device pool, the argument checks and the result handle; the three
// calls below are the phases between which the host has to size a block of memory, as in gather_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"
#include "rebuild_kernels.h"

namespace ommx {

struct ReorientArgs {
    ResultView source;             // (result_read.h) indexCount > 0
    const uint8_t* orientations;   // device memory, one byte per primitive, or null: `orientation` for every primitive
    uint32_t orientation;          // 0..5
    uint32_t flags;                // ommxCoarsenFlags
};
struct ReorientPlan {              // after the orientations and the index buffer have been read
    uint64_t stagingBytes;         // the arena the blocks are written to before their order is known
    uint64_t units;                // work units of the stage kernel
    uint32_t skipped, referenced, reoriented;   // skipped primitives; distinct accepted (descriptor, orientation) pairs; of those: orientation != 0
};

// the items of the tail: 6 per descriptor, (e, o) at 6e + o; with one orientation for every primitive 1 per descriptor.  The host refuses a source
// whose count does not fit 32 bits.
inline uint64_t reorient_items(const ReorientArgs& a) { return (uint64_t)a.source.descCount * (a.orientations ? 6u : 1u); }
size_t reorient_head_bytes(const ReorientArgs& a);
// each: every launch on `stream`, the answer copied to the host, the stream synchronised
hipError_t reorient_plan(const ReorientArgs& a, void* head, ReorientPlan* out, hipStream_t stream);
// staging may be null when plan.units == 0
hipError_t reorient_stage(const ReorientArgs& a, void* head, void* staging, const ReorientPlan& plan, RebuildCounts* out, hipStream_t stream);
hipError_t reorient_emit(const ReorientArgs& a, void* head, const void* staging, const RebuildCounts& counts, const RebuildOutputs& o, hipStream_t stream);   // o.index: 32-bit entries

} // namespace ommx
