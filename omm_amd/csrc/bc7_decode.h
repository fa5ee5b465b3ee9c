// bc7_decode.h -- the alpha of one BC7 block from its 16 bytes, as ommxCreateTextureBC7 defines it (include/omm_mi355x_ext.h).
// Compiles as HIP device code (bc7_kernels.hip) and as plain C++ on the host (tests/native/bc7_decode_host.cpp), the way block_decode.h does, so that
// the very code the kernel runs is tested without a GPU.
//
// `lo`, `hi` are the little-endian u64 of bytes 0..7 and 8..15: bit b of the block is bit b of lo (b < 64) or bit b - 64 of hi.  Texel i = 4 * y + x.
//
// Lanes of one wave hold blocks of different modes, so the modes with an alpha (4..7) share ONE path: the mode only selects where the two endpoints and
// the indices lie and how wide they are; one extraction and one interpolation follow.  Modes 0..3 (alpha 255) and the reserved byte 0 (alpha 0) leave
// early.  Nothing here is an array indexed at run time but the partition table, which is constant memory, not registers: no scratch on the device.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define OMMX_BC7_FN __host__ __device__ __forceinline__
#else
#define OMMX_BC7_FN static inline
#endif

namespace ommx {

// mode 7, by partition: bits 0..15 the subset of texel i (bit i), bits 16..19 the anchor texel of subset 1 (the one whose index has 1 bit, like texel 0's)
#define OMMX_BC7_P(mask, anchor) (0x##mask##u | ((uint32_t)(anchor) << 16))
static constexpr uint32_t kBc7Partition[64] = {
    OMMX_BC7_P(CCCC, 15), OMMX_BC7_P(8888, 15), OMMX_BC7_P(EEEE, 15), OMMX_BC7_P(ECC8, 15), OMMX_BC7_P(C880, 15), OMMX_BC7_P(FEEC, 15), OMMX_BC7_P(FEC8, 15), OMMX_BC7_P(EC80, 15),
    OMMX_BC7_P(C800, 15), OMMX_BC7_P(FFEC, 15), OMMX_BC7_P(FE80, 15), OMMX_BC7_P(E800, 15), OMMX_BC7_P(FFE8, 15), OMMX_BC7_P(FF00, 15), OMMX_BC7_P(FFF0, 15), OMMX_BC7_P(F000, 15),
    OMMX_BC7_P(F710, 15), OMMX_BC7_P(008E,  2), OMMX_BC7_P(7100,  8), OMMX_BC7_P(08CE,  2), OMMX_BC7_P(008C,  2), OMMX_BC7_P(7310,  8), OMMX_BC7_P(3100,  8), OMMX_BC7_P(8CCE, 15),
    OMMX_BC7_P(088C,  2), OMMX_BC7_P(3110,  8), OMMX_BC7_P(6666,  2), OMMX_BC7_P(366C,  2), OMMX_BC7_P(17E8,  8), OMMX_BC7_P(0FF0,  8), OMMX_BC7_P(718E,  2), OMMX_BC7_P(399C,  2),
    OMMX_BC7_P(AAAA, 15), OMMX_BC7_P(F0F0, 15), OMMX_BC7_P(5A5A,  6), OMMX_BC7_P(33CC,  8), OMMX_BC7_P(3C3C,  2), OMMX_BC7_P(55AA,  8), OMMX_BC7_P(9696, 15), OMMX_BC7_P(A55A, 15),
    OMMX_BC7_P(73CE,  2), OMMX_BC7_P(13C8,  8), OMMX_BC7_P(324C,  2), OMMX_BC7_P(3BDC,  2), OMMX_BC7_P(6996,  2), OMMX_BC7_P(C33C, 15), OMMX_BC7_P(9966, 15), OMMX_BC7_P(0660,  6),
    OMMX_BC7_P(0272,  6), OMMX_BC7_P(04E4,  2), OMMX_BC7_P(4E40,  6), OMMX_BC7_P(2720,  8), OMMX_BC7_P(C936, 15), OMMX_BC7_P(936C, 15), OMMX_BC7_P(39C6,  2), OMMX_BC7_P(639C,  2),
    OMMX_BC7_P(9336, 15), OMMX_BC7_P(9CC6, 15), OMMX_BC7_P(817E, 15), OMMX_BC7_P(E718, 15), OMMX_BC7_P(CCF0, 15), OMMX_BC7_P(0FCC,  2), OMMX_BC7_P(7744,  2), OMMX_BC7_P(EE22, 15),
};
#undef OMMX_BC7_P

// the 64 bits of the block from bit `pos` (0..127) on, zeros beyond bit 127
OMMX_BC7_FN uint64_t bc7_bits(uint64_t lo, uint64_t hi, uint32_t pos)
{
    const uint32_t s = pos & 63u;
    const uint64_t a = pos < 64u ? lo : hi, b = pos < 64u ? hi : 0u;
    return (a >> s) | ((b << 1) << (63u - s));                            // (no shift by 64 at s == 0)
}

// an endpoint of n bits (5..8) widened to 8 by bit replication: n = 5 (v<<3)|(v>>2), 6 (v<<2)|(v>>4), 7 (v<<1)|(v>>6), 8 v
OMMX_BC7_FN uint32_t bc7_widen(uint32_t v, uint32_t n) { return ((v << (8u - n)) | (v >> (2u * n - 8u))) & 0xFFu; }

// The four rows of the block's alpha, row y as 4 packed UNORM8 bytes (x = 0 in the low byte).
OMMX_BC7_FN void bc7_alpha_rows(uint64_t lo, uint64_t hi, uint32_t (&rows)[4])
{
    const uint32_t b0 = (uint32_t)lo & 0xFFu;
    const uint32_t low = b0 & (0u - b0);                                  // 1 << mode; 0 for the reserved byte 0
    if (low < 16u) {                                                      // modes 0..3: no alpha in the block, 255; reserved: 0
        rows[0] = rows[1] = rows[2] = rows[3] = low ? 0xFFFFFFFFu : 0u;
        return;
    }
    const bool m4 = low == 16u, m5 = low == 32u, m6 = low == 64u, m7 = low == 128u;
    // ---- what the mode selects ----
    // rot != 0 (modes 4, 5): the output alpha is colour channel rot - 1 with the colour indices; idxMode (mode 4) swaps the two index sets
    const uint32_t rot = m4 ? (b0 >> 5) & 3u : m5 ? (b0 >> 6) & 3u : 0u;
    const bool three = m4 && (((b0 >> 7) & 1u) == 0u) == (rot == 0u);     // mode 4: the 3-bit set
    // the two endpoints of subset 0: n bits each at ePos and ePos + n; modes 6 and 7 append a P bit
    const uint32_t n = m4 ? (rot ? 5u : 6u) : m5 ? (rot ? 7u : 8u) : m6 ? 7u : 5u;
    const uint32_t ePos = m4 ? (rot ? 10u * rot - 2u : 38u) : m5 ? (rot ? 14u * rot - 6u : 50u) : m6 ? 49u : 74u;
    const uint32_t nP = (m6 || m7) ? 1u : 0u;
    const uint32_t p0 = m6 ? (uint32_t)(lo >> 63) : (uint32_t)(hi >> 30) & 1u, p1 = m6 ? (uint32_t)hi & 1u : (uint32_t)(hi >> 31) & 1u;   // bits 63, 64 / 94, 95
    // the indices: nb bits each from bit iPos, texel 0 with nb - 1
    const uint32_t nb = m6 ? 4u : three ? 3u : 2u;
    const uint32_t iPos = m4 ? (three ? 81u : 50u) : m5 ? (rot ? 66u : 97u) : m6 ? 65u : 98u;
    // ---- one extraction ----
    const uint32_t eMask = (1u << n) - 1u;
    uint32_t e0 = (uint32_t)bc7_bits(lo, hi, ePos) & eMask, e1 = (uint32_t)bc7_bits(lo, hi, ePos + n) & eMask;
    e0 = nP ? (e0 << 1) | p0 : e0; e1 = nP ? (e1 << 1) | p1 : e1;
    e0 = bc7_widen(e0, n + nP); e1 = bc7_widen(e1, n + nP);
    // subset 1 exists in mode 7 only: A at bits 84 and 89, P at bits 96 and 97; every other mode has the empty mask
    const uint32_t f0 = bc7_widen((((uint32_t)(hi >> 20) & 31u) << 1) | ((uint32_t)(hi >> 32) & 1u), 6u);
    const uint32_t f1 = bc7_widen((((uint32_t)(hi >> 25) & 31u) << 1) | ((uint32_t)(hi >> 33) & 1u), 6u);
    const uint32_t entry = kBc7Partition[m7 ? ((uint32_t)lo >> 8) & 63u : 0u];
    const uint32_t mask = m7 ? entry & 0xFFFFu : 0u;
    // the index bits as sixteen fields of nb bits: a zero goes in as the top bit of texel 0 and, in mode 7, of the anchor of subset 1
    uint64_t x = bc7_bits(lo, hi, iPos);
    x = (x & ((1ull << (nb - 1u)) - 1ull)) | ((x >> (nb - 1u)) << nb);
    const uint32_t t = 2u * (entry >> 16) + 1u;                           // (mode 7 has 2-bit indices; t <= 31)
    x = m7 ? (x & ((1ull << t) - 1ull)) | ((x >> t) << (t + 1u)) : x;
    // ---- one interpolation ----
    // weight of index k: (64 k + 1) / 3, (64 k + 3) / 7, (64 k + 7) / 15 in integer division = 0 21 43 64, 0 9 18 27 37 46 55 64, 0 4 9 .. 60 64.  The
    // division is a multiplication by ceil(65536 / d) and a shift: exact while numerator * (ceil(65536 / d) - 65536 / d) < 65536 / d, and the largest
    // numerator is 64 * 15 + 7.
    const uint32_t recip = nb == 2u ? 21846u : nb == 3u ? 9363u : 4370u, half = nb == 2u ? 1u : nb == 3u ? 3u : 7u;
    const uint32_t wMul = 64u * recip, wAdd = half * recip, kMask = (1u << nb) - 1u;
    const int32_t d0 = (int32_t)e1 - (int32_t)e0, d1 = (int32_t)f1 - (int32_t)f0;
    const int32_t base0 = 64 * (int32_t)e0 + 32, base1 = 64 * (int32_t)f0 + 32;
#if defined(__clang__)
    #pragma unroll
#endif
    for (uint32_t y = 0; y < 4u; ++y) {
        uint32_t r = 0;
#if defined(__clang__)
        #pragma unroll
#endif
        for (uint32_t c = 0; c < 4u; ++c) {
            const uint32_t i = 4u * y + c;
            const uint32_t k = (uint32_t)x & kMask;
            x >>= nb;
            const int32_t w = (int32_t)((k * wMul + wAdd) >> 16);
            const bool s = ((mask >> i) & 1u) != 0u;
            const uint32_t v = (uint32_t)((s ? base1 : base0) + w * (s ? d1 : d0)) >> 6;   // ((64 - w) e0 + w e1 + 32) >> 6, never negative
            r |= v << (8u * c);
        }
        rows[y] = r;
    }
}

} // namespace ommx
