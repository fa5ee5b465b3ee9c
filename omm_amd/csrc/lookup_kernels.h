// lookup_kernels.h -- launches of the two consumers of a baked micromap (lookup_kernels.hip): per-hit OMM state, and the any-hit answer
// that falls back to the alpha texture where the OMM does not decide.  Entry points: ommxLookupOpacity / ommxResolveHits.
#pragma once
#include <hip/hip_runtime.h>
#include "bake_types.h"
#include "../../include/omm_mi355x_ext.h"

namespace ommx {

// What resolve_hits needs of the bake's input desc besides the result: mip 0 of the texture and the sampler (in `tex`: mips[0], mipCount = 1,
// texIsFp32, addrMode, filterLinear, cutoff, borderAlpha, stateGT, stateLE, pow2Dispatch), and the mesh the texture coordinates come from.
struct ResolveParams {
    ClassifyParams tex;
    const void* texCoords; uint32_t texCoordStride; int texCoordFormat;   // ommTexCoordFormat; stride already resolved (never 0)
    const void* indices;   int indexFormat;                               // ommIndexFormat of the input index buffer
    uint32_t    numTris;                                                  // indexCount / 3 of the input desc
};

hipError_t launch_lookup_opacity(const ommCpuBakeResultDesc& result, const ommxHit* hits, uint32_t count, uint8_t* out, uint32_t flags, hipStream_t stream);
hipError_t launch_resolve_hits(const ResolveParams& rp, const ommCpuBakeResultDesc& result, const ommxHit* hits, uint32_t count, uint8_t* out,
                               uint32_t flags, hipStream_t stream);

} // namespace ommx
