// block_decode.h -- the alpha of one BC1 / BC2 / BC4-kind block from the 8 bytes that hold it, as ommxCreateTextureBC defines it
// (include/omm_mi355x_ext.h).  Compiles as HIP device code (block_kernels.hip) and as plain C++ on the host
// (tests/native/block_decode_host.cpp), the way stats_count.h does, so that the very code the kernel runs is tested without a GPU.
//
// `q` is the little-endian u64 of the 8 bytes: a whole BC1 or BC4 block, bytes 0..7 of a BC2 or BC3 block, bytes 0..7 or 8..15 of a BC5 block.
// Texel i = 4 * y + x of the block, x, y in 0..3.
//
// The BC4-kind value is ((float)n / (float)D) * (1.f / 255.f): ONE IEEE-correct division and ONE multiplication that must not be fused with or
// reordered against anything.  It depends on the build's -ffp-contract=off and on hipcc's default, correctly rounded fp32 division (no
// -ffast-math, no -fhip-fp32-correctly-rounded-divide-sqrt=off) -- both are set in the Makefile and relied on by the classification already.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define OMMX_BLOCK_FN __host__ __device__ __forceinline__
#else
#define OMMX_BLOCK_FN static inline
#endif

// On the device the finished palette is pinned in its registers: the compiler otherwise moves the selects of block_bc4_select in front of the
// division -- the same values, but 16 divisions per block, one per texel, in place of 8.
#ifdef __HIP_DEVICE_COMPILE__
#define OMMX_BLOCK_KEEP(v) asm volatile("" : "+v"(v))
#else
#define OMMX_BLOCK_KEEP(v) ((void)0)
#endif

namespace ommx {

// BC1: c0 = bits 0..15, c1 = bits 16..31, the 2-bit codes from bit 32.  Row y as 4 packed UNORM8 bytes (x = 0 in the low byte): 0 where the block is
// in punch-through mode (c0 <= c1) and the code is 3, 255 everywhere else.
OMMX_BLOCK_FN uint32_t block_bc1_row(uint64_t q, uint32_t y)
{
    const uint32_t c0 = (uint32_t)q & 0xFFFFu, c1 = ((uint32_t)q >> 16) & 0xFFFFu;
    if (c0 > c1) return 0xFFFFFFFFu;
    const uint32_t codes = ((uint32_t)(q >> 32) >> (8u * y)) & 0xFFu;
    const uint32_t three = codes & (codes >> 1) & 0x55u;                 // bit 2x set where code x is 3
    const uint32_t hole = (three & 1u) | ((three & 4u) << 6) | ((three & 16u) << 12) | ((three & 64u) << 18);   // bit 8x
    return ~(hole * 255u);
}

// BC2: the 4-bit alpha of texel i is bits 4i..4i+3.  Row y as 4 packed UNORM8 bytes, each 17 * a (0x0a -> 0xaa).
OMMX_BLOCK_FN uint32_t block_bc2_row(uint64_t q, uint32_t y)
{
    const uint32_t n = (uint32_t)(q >> (16u * y)) & 0xFFFFu;
    const uint32_t spread = (n & 0xFu) | ((n & 0xF0u) << 4) | ((n & 0xF00u) << 8) | ((n & 0xF000u) << 12);   // nibble x in the low half of byte x
    return spread * 17u;                                                  // (no carries: 17 * 15 = 255)
}

OMMX_BLOCK_FN uint32_t block_float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the one value definition: numerator over denominator "as a float", then the multiplication the classification applies to a UNORM8 byte
OMMX_BLOCK_FN uint32_t block_unorm_bits(uint32_t n, float d) { return block_float_bits(((float)n / d) * (1.f / 255.f)); }

// BC4 kind: a0 = byte 0, a1 = byte 1; the fp32 bit patterns of the 8 palette entries, by code.
OMMX_BLOCK_FN void block_bc4_palette(uint64_t q, uint32_t (&pal)[8])
{
    const uint32_t a0 = (uint32_t)q & 0xFFu, a1 = ((uint32_t)q >> 8) & 0xFFu;
    const bool six = a0 > a1;                                             // 6 interpolated values; otherwise 4 and the constants 0 and 1
    const uint32_t m = six ? 7u : 5u;
    const float d = six ? 7.f : 5.f;
    pal[0] = block_unorm_bits(m * a0, d);
    pal[1] = block_unorm_bits(m * a1, d);
#if defined(__clang__)
    #pragma unroll
#endif
    for (uint32_t k = 2; k < 6; ++k) pal[k] = block_unorm_bits((m + 1u - k) * a0 + (k - 1u) * a1, d);
    pal[6] = block_unorm_bits(six ? 2u * a0 + 5u * a1 : 0u, d);
    pal[7] = block_unorm_bits(six ? a0 + 6u * a1 : 5u * 255u, d);
    OMMX_BLOCK_KEEP(pal[0]); OMMX_BLOCK_KEEP(pal[1]); OMMX_BLOCK_KEEP(pal[2]); OMMX_BLOCK_KEEP(pal[3]);
    OMMX_BLOCK_KEEP(pal[4]); OMMX_BLOCK_KEEP(pal[5]); OMMX_BLOCK_KEEP(pal[6]); OMMX_BLOCK_KEEP(pal[7]);
}

// the palette entry of code k (0..7) by selects: `pal[k]` with a run-time k would put the palette into scratch memory on the device
OMMX_BLOCK_FN uint32_t block_bc4_select(const uint32_t (&pal)[8], uint32_t k)
{
    const uint32_t p01 = (k & 1u) ? pal[1] : pal[0], p23 = (k & 1u) ? pal[3] : pal[2], p45 = (k & 1u) ? pal[5] : pal[4], p67 = (k & 1u) ? pal[7] : pal[6];
    const uint32_t lo = (k & 2u) ? p23 : p01, hi = (k & 2u) ? p67 : p45;
    return (k & 4u) ? hi : lo;
}

// the 3-bit code of texel i (0..15): bits 3i..3i+2 of the 48-bit integer at bytes 2..7
OMMX_BLOCK_FN uint32_t block_bc4_code(uint64_t q, uint32_t i) { return (uint32_t)(q >> (16u + 3u * i)) & 7u; }

} // namespace ommx
