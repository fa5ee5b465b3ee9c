// raster_kernels.h -- ommxRasterizeMicromap: a device-resident result drawn in texture space over its alpha texture (raster_kernels.hip; the rule is
// in include/omm_mi355x_ext.h, its arithmetic in raster_cover.h).  omm_host.cpp owns the baker, its device pool and the argument checks.
#pragma once
#include <hip/hip_runtime.h>
#include "lookup_kernels.h"   // ResolveParams: the texture, the sampler and the mesh, as ommxResolveHits fills them
#include "raster_cover.h"

namespace ommx {

struct RasterArgs {
    ResolveParams mesh;
    ommCpuBakeResultDesc result;   // host struct over device arrays
    RasterView view;
    uint32_t first, count;         // the primitives [first, first + count) after the cut to the mesh; count may be 0
    uint32_t flags;                // ommxRasterFlags
    // device memory of the caller, each or null
    uint32_t *primitiveIds, *microTriangles;
    uint8_t *states, *alphaTest, *rgba;
};
struct RasterCounts {              // what the device counted, in ommxRasterInfo's order
    uint64_t covered, perState[4], invalid, alphaAbove, contradictions, drawn, degenerate;
};

size_t raster_scratch_bytes(const RasterArgs& a);
// every launch on `stream`; the caller's outputs are written, *out is copied to the host and the stream synchronised
hipError_t raster_run(const RasterArgs& a, void* scratch, RasterCounts* out, hipStream_t stream);

} // namespace ommx
