// texture_kernels.hip -- ommxCreateTextureDevice: one channel of an interleaved image that already lives in device memory -> the packed
// row-major texel array of a texture mip (TexMip::texels, omm_host.cpp).  A pure streaming job: every source byte of a row is fetched from
// memory once whatever the kernel does with it (the channel's bytes share their cache lines with the other channels'), so the paths differ in
// instructions per byte, not in bytes.  DESIGN.md section 5.14.
//
// A lane owns a GROUP of G consecutive texels of one row and stores them with aligned 4 / 8 / 16-byte stores.  Groups are laid out from the
// OUTPUT's alignment: row y starts at texel y * w of the packed array, so the first (G - y * w mod G) mod G texels of a row are peeled (lane 0 of
// the row, one texel at a time) and every further group starts on a multiple of G texels of the array.  The source bytes of a full group are
// contiguous (G * stride bytes); where their address is aligned they are read with vector loads, otherwise -- a base or pitch that is only
// channel-aligned, a stride without a wide path -- with one channel-sized load per texel.  Peeled texels and the ragged end of a row always
// take the per-texel loads.  No load starts before the first pixel of a row or ends behind its last one, and only the channel's own bytes
// reach the result.
#include <hip/hip_runtime.h>
#include "texture_kernels.h"

namespace ommx {

// exact fp32 widening of a half, on its bits (independent of the denormal mode; subnormals are normalised, inf / NaN keep their mantissa bits)
__device__ __forceinline__ uint32_t half_to_float_bits(uint32_t h)
{
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 0u) {
        if (m == 0u) return s;
        const uint32_t top = 31u - (uint32_t)__clz((int)m);   // m * 2^-24 = 1.xxx * 2^(top - 24)
        return s | ((103u + top) << 23) | ((m << (23u - top)) & 0x7FFFFFu);
    }
    if (e == 31u) return s | 0x7F800000u | (m << 13);
    return s | ((e + 112u) << 23) | (m << 13);
}

template <int F> __device__ __forceinline__ uint32_t tex_channel(const uint8_t* p)   // the texel's stored value from the channel at p
{
    if (F == kTexGatherUnorm8) return *p;
    if (F == kTexGatherFp16) return half_to_float_bits(*(const uint16_t*)p);
    return *(const uint32_t*)p;
}
template <int F> __device__ __forceinline__ uint32_t tex_from_dword(uint32_t d, uint32_t shift)   // ... from a loaded dword that holds the channel at bit `shift`
{
    if (F == kTexGatherUnorm8) return (d >> shift) & 0xFFu;
    if (F == kTexGatherFp16) return half_to_float_bits((d >> shift) & 0xFFFFu);
    return d;
}
template <int F> __device__ __forceinline__ void tex_store_one(void* dst, uint64_t i, uint32_t v)
{
    if (F == kTexGatherUnorm8) ((uint8_t*)dst)[i] = (uint8_t)v; else ((uint32_t*)dst)[i] = v;
}
// G texels to the array, i a multiple of G: G bytes (UNORM8) or 4 G bytes (fp32 texels) in aligned stores of up to 16 bytes
template <int F, int G> __device__ __forceinline__ void tex_store_group(void* dst, uint64_t i, const uint32_t (&v)[G])
{
    if (F == kTexGatherUnorm8) {
        uint32_t d[G / 4];
        #pragma unroll
        for (int k = 0; k < G / 4; ++k) d[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
        uint8_t* o = (uint8_t*)dst + i;
        if (G == 4) *(uint32_t*)o = d[0];
        else if (G == 8) *(uint2*)o = make_uint2(d[0], d[G / 4 - 1]);
        else *(uint4*)o = make_uint4(d[0], d[(G / 4 > 1) ? 1 : 0], d[(G / 4 > 2) ? 2 : 0], d[(G / 4 > 3) ? 3 : 0]);
    } else {
        uint4* o = (uint4*)((uint32_t*)dst + i);
        #pragma unroll
        for (int k = 0; k < G / 4; ++k) o[k] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    }
}

// STRIDE: the pixel stride when the path is specialised for it, 0 = any (taken from `strideRt`).  WIDE: a full group's G * STRIDE source bytes
// (8, 16 or 32) are read with aligned 8 / 16-byte loads where their address allows it; STRIDE is 1, 2, 4 or 8 then.
template <int F, int STRIDE, int G, bool WIDE>
__global__ __launch_bounds__(256) void texture_gather(const uint8_t* __restrict__ src, uint64_t pitch, uint32_t strideRt, uint32_t off,
                                                      void* __restrict__ dst, int w, int h)
{
    static_assert(G == 4 || G == 8 || G == 16, "group sizes");
    static_assert(!WIDE || ((STRIDE == 1 || STRIDE == 2 || STRIDE == 4 || STRIDE == 8) && (G * STRIDE == 8 || G * STRIDE == 16 || G * STRIDE == 32)), "wide paths");
    const uint32_t stride = STRIDE ? (uint32_t)STRIDE : strideRt;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    for (uint32_t row = blockIdx.y * 4u + threadIdx.y; row < (uint32_t)h; row += gridDim.y * 4u) {
        const uint8_t* rs = src + (uint64_t)row * pitch;
        const uint64_t o = (uint64_t)row * (uint64_t)(uint32_t)w;
        uint32_t lead = (uint32_t)((G - (o & (uint64_t)(G - 1))) & (uint64_t)(G - 1));
        if (lead > (uint32_t)w) lead = (uint32_t)w;
        if (g == 0u) {
            for (uint32_t x = 0; x < lead; ++x) tex_store_one<F>(dst, o + x, tex_channel<F>(rs + (uint64_t)x * stride + off));
            continue;
        }
        const uint64_t x0 = (uint64_t)lead + (uint64_t)(g - 1u) * (uint64_t)G;
        if (x0 >= (uint64_t)(uint32_t)w) continue;
        const uint8_t* p = rs + x0 * stride;
        if (x0 + (uint64_t)G > (uint64_t)(uint32_t)w) {   // the ragged end of the row
            const uint32_t n = (uint32_t)((uint64_t)(uint32_t)w - x0);
            for (uint32_t k = 0; k < n; ++k) tex_store_one<F>(dst, o + x0 + k, tex_channel<F>(p + (uint64_t)k * stride + off));
            continue;
        }
        uint32_t v[G];
        constexpr int NB = WIDE ? G * STRIDE : 16, VEC = NB < 16 ? NB : 16;
        if (WIDE && ((uintptr_t)p & (uintptr_t)(VEC - 1)) == 0) {
            uint32_t buf[NB / 4];
            if (VEC == 8) { const uint2 t = *(const uint2*)p; buf[0] = t.x; buf[1] = t.y; }
            else {
                #pragma unroll
                for (int k = 0; k < NB / 16; ++k) { const uint4 t = ((const uint4*)p)[k]; buf[4 * k] = t.x; buf[4 * k + 1] = t.y; buf[4 * k + 2] = t.z; buf[4 * k + 3] = t.w; }
            }
            #pragma unroll
            for (int j = 0; j < G; ++j) {
                if (STRIDE == 8) v[j] = tex_from_dword<F>(off >= 4u ? buf[(2 * j + 1) % (NB / 4)] : buf[(2 * j) % (NB / 4)], (off & 3u) * 8u);
                else             v[j] = tex_from_dword<F>(buf[((j * STRIDE) >> 2) % (NB / 4)], (uint32_t)((j * STRIDE) & 3) * 8u + off * 8u);
            }
        } else {
            #pragma unroll
            for (int j = 0; j < G; ++j) v[j] = tex_channel<F>(p + (uint64_t)j * stride + off);
        }
        tex_store_group<F, G>(dst, o + x0, v);
    }
}

size_t tex_gather_channel_bytes(int format) { return format == kTexGatherUnorm8 ? 1 : format == kTexGatherFp16 ? 2 : 4; }

template <int F, int STRIDE, int G, bool WIDE>
static int launch_gather(const void* src, size_t pitch, uint32_t stride, uint32_t off, void* dst, int w, int h, hipStream_t stream)
{
    const uint32_t groups = 1u + ((uint32_t)w + (uint32_t)G - 1u) / (uint32_t)G;   // the peeled texels' lane + the groups behind them
    const uint32_t rows4 = ((uint32_t)h + 3u) / 4u;
    const dim3 grid((groups + 63u) / 64u, rows4 < 65535u ? rows4 : 65535u);
    hipLaunchKernelGGL((texture_gather<F, STRIDE, G, WIDE>), grid, dim3(64, 4), 0, stream, (const uint8_t*)src, (uint64_t)pitch, stride, off, dst, w, h);
    return WIDE ? 1 : 0;
}

int launch_texture_gather(const void* src, size_t pitch, uint32_t stride, uint32_t off, int format, void* dst, int w, int h, hipStream_t stream)
{
    if (format == kTexGatherUnorm8) {
        if (stride == 1) return launch_gather<kTexGatherUnorm8, 1, 16, true>(src, pitch, stride, off, dst, w, h, stream);   // a copy: 16 bytes in, 16 out
        if (stride == 2) return launch_gather<kTexGatherUnorm8, 2, 8, true>(src, pitch, stride, off, dst, w, h, stream);
        if (stride == 4) return launch_gather<kTexGatherUnorm8, 4, 4, true>(src, pitch, stride, off, dst, w, h, stream);    // RGBA8: four pixels in, one dword out
        return launch_gather<kTexGatherUnorm8, 0, 4, false>(src, pitch, stride, off, dst, w, h, stream);
    }
    if (format == kTexGatherFp16) {
        if (stride == 2) return launch_gather<kTexGatherFp16, 2, 8, true>(src, pitch, stride, off, dst, w, h, stream);      // a widening: 16 bytes in, 32 out
        if (stride == 4) return launch_gather<kTexGatherFp16, 4, 4, true>(src, pitch, stride, off, dst, w, h, stream);
        if (stride == 8) return launch_gather<kTexGatherFp16, 8, 4, true>(src, pitch, stride, off, dst, w, h, stream);      // RGBA16F
        return launch_gather<kTexGatherFp16, 0, 4, false>(src, pitch, stride, off, dst, w, h, stream);
    }
    if (stride == 4) return launch_gather<kTexGatherFp32, 4, 4, true>(src, pitch, stride, off, dst, w, h, stream);          // a copy
    if (stride == 8) return launch_gather<kTexGatherFp32, 8, 4, true>(src, pitch, stride, off, dst, w, h, stream);
    // RGBA32F: a pixel is a 16-byte vector of which one dword is wanted.  One dword load per pixel touches the same cache lines as a 16-byte
    // load and returns a quarter of the data to the registers, so the per-texel loads ARE the wide path of this layout.
    if (stride == 16) return launch_gather<kTexGatherFp32, 16, 4, false>(src, pitch, stride, off, dst, w, h, stream);
    return launch_gather<kTexGatherFp32, 0, 4, false>(src, pitch, stride, off, dst, w, h, stream);
}

} // namespace ommx
