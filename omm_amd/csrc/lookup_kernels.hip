// lookup_kernels.hip -- using a baked micromap: the OMM state of a batch of ray hits (lookup_opacity) and the any-hit answer that samples the
// alpha texture only where the OMM leaves the hit unknown (resolve_hits).  The per-hit decode is include/omm_mi355x_lookup.h, the same code the
// host entry point ommxLookupOpacityHost runs; texture coordinates and the sampler are tex_fetch.h (the classifier's own texel addressing and bilinear
// filter), so a resolved hit is sampled the way the bake classified its micro-triangle.
#include <hip/hip_runtime.h>
#include "lookup_kernels.h"
#include "tex_fetch.h"   // fetch_tex_coord, sample_alpha (shared with raster_kernels.hip)
#include "../../include/omm_mi355x_lookup.h"

namespace ommx {

constexpr uint32_t kLookupBlock = 256;
constexpr uint32_t kLookupMaxBlocks = 4096;   // 256 CUs x 16 blocks of 4 waves: more than can be resident; the grid strides over the rest

// The desc's fields as separate kernel arguments would be the same scalar loads; a local copy keeps the decode's pointer argument off the stack.
__device__ __forceinline__ uint32_t hit_state(const ommCpuBakeResultDesc& r, const ommxHit& h, bool force2)
{
    const ommCpuBakeResultDesc rl = r;
    const uint32_t s = ommx_opacity_state(&rl, h.primitiveIndex, h.u, h.v);
    return force2 ? ommx_force_2state(s) : s;
}

// The grid stride without 32-bit wrap-around: a count within one stride of 2^32 would otherwise bring a lane back to hits it has answered, forever.
__device__ __forceinline__ uint32_t next_hit(uint32_t i, uint32_t count)
{
    const uint32_t stride = gridDim.x * kLookupBlock;
    return count - i > stride ? i + stride : count;   // (i < count here)
}

// One hit per lane: index entry -> descriptor -> state byte, three dependent loads.  No LDS, few registers, so that many waves keep loads in flight.
__global__ __launch_bounds__(kLookupBlock) void lookup_opacity(ommCpuBakeResultDesc r, const ommxHit* __restrict__ hits, uint32_t count,
                                                               uint8_t* __restrict__ out, uint32_t force2)
{
    for (uint32_t i = blockIdx.x * kLookupBlock + threadIdx.x; i < count; i = next_hit(i, count)) {
        const ommxHit h = hits[i];
        out[i] = (uint8_t)hit_state(r, h, force2 != 0);
    }
}

// out: bit 0 = opaque, bits 1-2 = OMM state, bit 3 = texture sampled; 0xFF = invalid hit
template <bool FP32>
__global__ __launch_bounds__(kLookupBlock) void resolve_hits(ResolveParams R, ommCpuBakeResultDesc r, const ommxHit* __restrict__ hits, uint32_t count,
                                                             uint8_t* __restrict__ out, uint32_t flags)
{
    for (uint32_t i = blockIdx.x * kLookupBlock + threadIdx.x; i < count; i = next_hit(i, count)) {
        const ommxHit h = hits[i];
        const uint32_t s = hit_state(r, h, (flags & ommxLookupFlags_Force2State) != 0);
        uint32_t o;
        if (s == OMMX_OPACITY_INVALID) o = 0xFFu;
        else if (s < 2u && !(flags & ommxLookupFlags_IgnoreMicromap)) o = s | (s << 1);   // known: the OMM answers, the texture is not touched
        else if (h.primitiveIndex >= R.numTris) o = 0xFFu;
        else {
            const size_t base = 3ull * h.primitiveIndex;
            uint32_t vi[3];
            #pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (R.indexFormat == ommIndexFormat_UINT_8) vi[k] = ((const uint8_t*)R.indices)[base + k];
                else if (R.indexFormat == ommIndexFormat_UINT_16) vi[k] = ((const uint16_t*)R.indices)[base + k];
                else vi[k] = ((const uint32_t*)R.indices)[base + k];
            }
            const V2 t0 = fetch_tex_coord(R, vi[0]), t1 = fetch_tex_coord(R, vi[1]), t2 = fetch_tex_coord(R, vi[2]);
            const float tri[6] = { t0.x, t0.y, t1.x, t1.y, t2.x, t2.y };
            const float alpha = sample_alpha<FP32>(R.tex, bary_point(tri, h.u, h.v));   // weights (1-u-v, u, v)
            const uint32_t st = (uint32_t)(R.tex.cutoff < alpha ? R.tex.stateGT : R.tex.stateLE);
            o = (st & 1u) | (s << 1) | 8u;   // an Unknown* answer counts as its opaque (3) / transparent (2) half
        }
        out[i] = (uint8_t)o;
    }
}

static uint32_t lookup_grid(uint32_t count)
{
    const uint32_t blocks = (count + kLookupBlock - 1u) / kLookupBlock;
    return blocks < kLookupMaxBlocks ? blocks : kLookupMaxBlocks;
}

hipError_t launch_lookup_opacity(const ommCpuBakeResultDesc& result, const ommxHit* hits, uint32_t count, uint8_t* out, uint32_t flags, hipStream_t stream)
{
    lookup_opacity<<<lookup_grid(count), kLookupBlock, 0, stream>>>(result, hits, count, out, flags & ommxLookupFlags_Force2State);
    return hipGetLastError();
}

hipError_t launch_resolve_hits(const ResolveParams& rp, const ommCpuBakeResultDesc& result, const ommxHit* hits, uint32_t count, uint8_t* out,
                               uint32_t flags, hipStream_t stream)
{
    if (rp.tex.texIsFp32) resolve_hits<true><<<lookup_grid(count), kLookupBlock, 0, stream>>>(rp, result, hits, count, out, flags);
    else resolve_hits<false><<<lookup_grid(count), kLookupBlock, 0, stream>>>(rp, result, hits, count, out, flags);
    return hipGetLastError();
}

} // namespace ommx

using namespace ommx;

OMM_MI355X_API ommResult ommxLookupOpacity(const ommCpuBakeResultDesc* result, const ommxHit* hits, uint32_t count, uint8_t* outStates, uint32_t flags,
                                           void* hipStream)
{
    if (result == nullptr || (flags & ~(uint32_t)ommxLookupFlags_Force2State) != 0) return ommResult_INVALID_ARGUMENT;
    if (count == 0) return ommResult_SUCCESS;
    if (hits == nullptr || outStates == nullptr) return ommResult_INVALID_ARGUMENT;
    return launch_lookup_opacity(*result, hits, count, outStates, flags, (hipStream_t)hipStream) == hipSuccess ? ommResult_SUCCESS : ommResult_FAILURE;
}

OMM_MI355X_API ommResult ommxLookupOpacityHost(const ommCpuBakeResultDesc* result, const ommxHit* hits, uint32_t count, uint8_t* outStates, uint32_t flags)
{
    if (result == nullptr || (flags & ~(uint32_t)ommxLookupFlags_Force2State) != 0) return ommResult_INVALID_ARGUMENT;
    if (count == 0) return ommResult_SUCCESS;
    if (hits == nullptr || outStates == nullptr) return ommResult_INVALID_ARGUMENT;
    const bool force2 = (flags & ommxLookupFlags_Force2State) != 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t s = ommx_opacity_state(result, hits[i].primitiveIndex, hits[i].u, hits[i].v);
        outStates[i] = (uint8_t)(force2 ? ommx_force_2state(s) : s);
    }
    return ommResult_SUCCESS;
}
