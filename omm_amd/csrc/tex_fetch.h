// tex_fetch.h -- what the consumers of a bake's input desc read on the device: a vertex's texture coordinate the way the bake's setup reads it, and
// the alpha of mip 0 under the runtime sampler.  Included by lookup_kernels.hip (resolve_hits) and raster_kernels.hip (the texture-space passes), so
// that both sample exactly as the bake classified: texel addressing and the bilinear filter are the classifier's own (classify_device.h).
#pragma once
#include <hip/hip_runtime.h>
#include "lookup_kernels.h"
#include "classify_device.h"

namespace ommx {

// _Float16 -> float is exact (denormals included): the value glm::unpackHalf2x16 gives the bake's setup
__device__ __forceinline__ float half_bits(uint32_t h)
{
    const uint16_t b = (uint16_t)h;
    _Float16 f;
    __builtin_memcpy(&f, &b, 2);
    return (float)f;
}

// texture coordinate of vertex `vi`, read as the bake's setup reads it (setup_fetch)
__device__ __forceinline__ V2 fetch_tex_coord(const ResolveParams& R, uint32_t vi)
{
    const uint8_t* base = (const uint8_t*)R.texCoords + (size_t)R.texCoordStride * vi;
    if (R.texCoordFormat == ommTexCoordFormat_UV32_FLOAT) {
        if (((uintptr_t)base & 3u) == 0) return mk2(((const float*)base)[0], ((const float*)base)[1]);
        uint32_t a = 0, b = 0;
        for (int q = 0; q < 4; ++q) { a |= (uint32_t)base[q] << (8 * q); b |= (uint32_t)base[4 + q] << (8 * q); }
        return mk2(__uint_as_float(a), __uint_as_float(b));
    }
    uint32_t v = 0;
    for (int q = 0; q < 4; ++q) v |= (uint32_t)base[q] << (8 * q);
    if (R.texCoordFormat == ommTexCoordFormat_UV16_UNORM)
        return mk2((float)(v & 0xffffu) * 1.5259021896696421759314870504694e-5f, (float)(v >> 16) * 1.5259021896696421759314870504694e-5f);
    return mk2(half_bits(v & 0xffffu), half_bits(v >> 16));
}

// vertex `k` (0..2) of triangle `prim` in the input desc's index buffer (prim < R.numTris)
__device__ __forceinline__ uint32_t fetch_vertex_index(const ResolveParams& R, uint32_t prim, int k)
{
    const size_t at = 3ull * prim + (size_t)k;
    if (R.indexFormat == ommIndexFormat_UINT_8) return ((const uint8_t*)R.indices)[at];
    if (R.indexFormat == ommIndexFormat_UINT_16) return ((const uint16_t*)R.indices)[at];
    return ((const uint32_t*)R.indices)[at];
}

// alpha of mip 0 at texture coordinate p with the runtime sampler: Linear = the classifier's bilinear(), Nearest = the texel under p
template <bool FP32>
__device__ __forceinline__ float sample_alpha(const ClassifyParams& P, V2 p)
{
    const DevMip& m = P.mips[0];
    TexWindow W; W.tex = nullptr; W.sat = nullptr; W.base = nullptr; W.sx = 0; W.sy = 0; W.w = 0; W.h = 0;   // no LDS window: every fetch reads HBM
    if (P.filterLinear) return bilinear<FP32, ModeDynamic>(P, m, p, W);
    const int x = tex_coord(P.addrMode, P.pow2Dispatch, cvt_trunc_x86(__builtin_floorf(p.x * m.fw)), m.w, m.log2w);
    const int y = tex_coord(P.addrMode, P.pow2Dispatch, cvt_trunc_x86(__builtin_floorf(p.y * m.fh)), m.h, m.log2h);
    return load_texel_border<FP32>(m, x, y, P.borderAlpha, W);
}

} // namespace ommx
