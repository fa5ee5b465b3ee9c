/*
 * omm_mi355x_lookup.h -- what a baked opacity micromap says at a ray hit (header-only).
 *
 * GPUs without a ray-tracing unit that reads the OMM array (the MI355X among them) consult a micromap from the any-hit or filter
 * function of their own ray tracer.  This header is that consumer: include it in HIP device code (hipcc) or in plain C++ on the host.
 *
 *   ommx_micro_index(u, v, level)          hit barycentrics -> micro-triangle index on the bird curve, 0 <= index < 4^level
 *   ommx_micro_vertices(index, level, uv)  the way back: the three barycentric vertices of a micro-triangle (or of a merged node)
 *   ommx_opacity_state(result, prim, u, v) the 4-state value (ommOpacityState, 0..3) the result stores there, or OMMX_OPACITY_INVALID
 *   ommx_force_2state(state)               the "force OMM 2-state" ray flag: UnknownTransparent -> Transparent, UnknownOpaque -> Opaque
 *
 * Barycentric convention (DXR / Vulkan): the hit point is (1-u-v) * V0 + u * V1 + v * V2, where V0..V2 are the triangle's vertices in
 * index-buffer order -- the (u, v) a DXR any-hit shader receives as attribs.barycentrics and a Vulkan one as gl_HitAttributeEXT.
 *
 * `result` is an ommCpuBakeResultDesc whose arrays (arrayData, descArray, indexBuffer) are readable where the function runs: host
 * memory on the host, device memory in a kernel.  Its indexCount is one entry per triangle.  Every read stays inside the arrays the
 * desc describes; what does not fit returns OMMX_OPACITY_INVALID instead (see ommx_opacity_state).
 *
 * Exact arithmetic: the mapping below decides on which side of a micro-triangle edge a point lies without rounding error.  It needs
 * IEEE fp32 (no -ffast-math / -ffinite-math-only in the including translation unit).
 */
#ifndef OMM_MI355X_LOOKUP_H
#define OMM_MI355X_LOOKUP_H
#include "omm_mi355x.h"

#ifdef __HIPCC__
#define OMMX_LOOKUP_FN __host__ __device__ __forceinline__
#else
#define OMMX_LOOKUP_FN static inline
#endif

/* returned for a primitive or index entry that the result cannot answer (see ommx_opacity_state) */
#define OMMX_OPACITY_INVALID 0xFFu
#define OMMX_LOOKUP_MAX_LEVEL 12u

/* The bird curve's forward decode (omm_amd/csrc/classify_device.h, micro_triangle) turns index digit i (bits 2i, 2i+1; most significant
 * digit first) into bit i of the discrete barycentrics (iu, iv, iw), with two running parities X, Y of the higher digits:
 *     b0 = digit & 1, b1 = digit >> 1,  X ^= b0,  Y ^= b0 & ~b1,  t = Y ^ b1
 *     iu_i = (X & ~t) | (b0 & ~t) | (~b0 & ~X & t),  iv_i = Y ^ b0,  iw_i = (~X & ~t) | (b0 & ~t) | (~b0 & X & t)
 * For fixed (X, Y) the four digits give four different (iu_i, iv_i, iw_i), so the digit is a function of (X, Y, iu_i, iv_i, iw_i): two
 * bits per 5-bit key, key = X | Y << 1 | iu_i << 2 | iv_i << 3 | iw_i << 4, packed into one 64-bit constant (16 keys occur; the others
 * read 0).  tests/test_lookup.py rebuilds this constant from the forward decode and checks the inverse on every index of every level. */
#define OMMX_BIRD_DIGIT_TABLE 0x5020f008800f0205ull

/* Micro-triangle index of the point (u, v) at `level` (0..12; larger levels are treated as 12).
 *  - a point strictly inside a micro-triangle returns that micro-triangle;
 *  - a point on a shared edge or vertex returns one of the micro-triangles whose closure contains it;
 *  - NaN reads as 0 and u, v are clamped to [0, 1]; a point beyond the edge u + v = 1 is moved onto the row of micro-triangles along that
 *    edge (its discrete barycentric iu is lowered first, then iv).  The result is always a valid index below 4^level. */
OMMX_LOOKUP_FN uint32_t ommx_micro_index(float u, float v, uint32_t level)
{
    if (level == 0u) return 0u;
    if (level > OMMX_LOOKUP_MAX_LEVEL) level = OMMX_LOOKUP_MAX_LEVEL;
    const uint32_t n = 1u << level;
    u = u > 0.f ? (u < 1.f ? u : 1.f) : 0.f;   /* (NaN fails the first comparison) */
    v = v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;
    const float fu = u * (float)n, fv = v * (float)n;   /* exact: scaling by a power of two */
    uint32_t iu = (uint32_t)fu, iv = (uint32_t)fv;      /* floor (both are >= 0) */
    iu = iu < n - 1u ? iu : n - 1u;
    iv = iv < n - 1u ? iv : n - 1u;
    bool upright = true;
    if (iu + iv >= n - 1u) {
        /* on or beyond the edge u + v = 1: the upright cell of that row (a point on the edge lies in its closure) */
        const uint32_t over = iu + iv - (n - 1u);
        const uint32_t du = over < iu ? over : iu;
        iu -= du; iv -= over - du;
    } else {
        /* cell (iu, iv) of the grid: the upright micro-triangle is its half ru + rv < 1, the inverted one the other half.  ru, rv are
           exact; their sum is decided exactly (two-sum error term) so that a point close to the diagonal is not rounded onto it */
        const float ru = fu - (float)iu, rv = fv - (float)iv;
        const float s = ru + rv, bv = s - ru, err = (ru - (s - bv)) + (rv - bv);
        upright = s < 1.f || (s == 1.f && err < 0.f);
    }
    /* discrete barycentrics as the forward decode produces them: iu + iv + iw = n - 1 (upright) or n - 2 (inverted, low corner (iu, iv)) */
    const uint32_t iw = (upright ? n - 1u : n - 2u) - iu - iv;
    uint32_t index = 0u, x = 0u, y = 0u;
    for (uint32_t i = level; i-- > 0u;) {
        const uint32_t key = x | (y << 1) | (((iu >> i) & 1u) << 2) | (((iv >> i) & 1u) << 3) | (((iw >> i) & 1u) << 4);
        const uint32_t digit = (uint32_t)(OMMX_BIRD_DIGIT_TABLE >> (2u * key)) & 3u;
        index = (index << 2) | digit;
        x ^= digit & 1u;
        y ^= digit == 1u ? 1u : 0u;
    }
    return index;
}

/* helpers of the forward decode: bits 0, 2, 4, ... of x gathered into the low half ... */
OMMX_LOOKUP_FN uint32_t ommx_even_bits(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u; x = (x | (x >> 2)) & 0x0f0f0f0fu;
    x = (x | (x >> 4)) & 0x00ff00ffu; x = (x | (x >> 8)) & 0x0000ffffu;
    return x;
}
/* ... and bit i of the result = the xor of the bits >= i of x */
OMMX_LOOKUP_FN uint32_t ommx_prefix_xor(uint32_t x)
{
    x ^= x >> 1; x ^= x >> 2; x ^= x >> 4; x ^= x >> 8; x ^= x >> 16;
    return x;
}

/* The three vertices of micro-triangle `index` at `level` as DXR / Vulkan barycentrics, uv = u0 v0 u1 v1 u2 v2: the bird curve's forward
 * decode (omm_amd/csrc/classify_device.h, micro_triangle), the inverse of ommx_micro_index.
 *  - vertex order is the decode's: (u, v), (u + d, v), (u, v + d) with d = +2^-level for an upright micro-triangle and -2^-level for an
 *    inverted one.  In that order EVERY micro-triangle, upright or inverted, has positive orientation in (u, v) -- the cross product of
 *    its two edges from vertex 0 is d * d > 0 -- so mapped through (1-u-v) * V0 + u * V1 + v * V2 it has the winding of the triangle it
 *    came from;
 *  - every coordinate is k * 2^-level with 0 <= k <= 2^level: exact in fp32;
 *  - the micro-triangles 4j .. 4j+3 of level N + 1 tile micro-triangle j of level N, so the same function is the vertex rule of a merged
 *    node of ommxExtractMicroGeometry: node (level l, index j) is ommx_micro_vertices(j, l);
 *  - levels above 12 are treated as 12 and an index >= 4^level is reduced modulo 4^level, as in ommx_micro_index. */
OMMX_LOOKUP_FN void ommx_micro_vertices(uint32_t index, uint32_t level, float uv[6])
{
    if (level > OMMX_LOOKUP_MAX_LEVEL) level = OMMX_LOOKUP_MAX_LEVEL;
    if (level == 0u) { uv[0] = 0.f; uv[1] = 0.f; uv[2] = 1.f; uv[3] = 0.f; uv[4] = 0.f; uv[5] = 1.f; return; }
    index &= (1u << (2u * level)) - 1u;
    const uint32_t b0 = ommx_even_bits(index), b1 = ommx_even_bits(index >> 1);
    const uint32_t fx = ommx_prefix_xor(b0), fy = ommx_prefix_xor(b0 & ~b1);
    const uint32_t t = fy ^ b1, mask = (1u << level) - 1u;
    uint32_t iu = ((fx & ~t) | (b0 & ~t) | (~b0 & ~fx & t)) & mask;
    uint32_t iv = (fy ^ b0) & mask;
    const uint32_t iw = ((~fx & ~t) | (b0 & ~t) | (~b0 & fx & t)) & mask;
    const bool upright = ((iu ^ iv ^ iw) & 1u) != 0u;
    if (!upright) { iu += 1u; iv += 1u; }
    const float s = 1.f / (float)(1u << level);   /* a power of two: every product and sum below is exact */
    const float d = upright ? s : -s;
    const float u = (float)iu * s, v = (float)iv * s;
    uv[0] = u; uv[1] = v; uv[2] = u + d; uv[3] = v; uv[4] = u; uv[5] = v + d;
}

/* perm_o[k] of ommxReorientMicromap's orientation codes (omm_mi355x_ext.h), two bits each at bit 6o + 2k: new vertex k is old vertex perm_o[k].
 *     o = 0 (0,1,2)   1 (1,2,0)   2 (2,0,1)   3 (0,2,1)   4 (2,1,0)   5 (1,0,2) */
#define OMMX_REORIENT_PERMS 0x846612264ull

/* A triangle's vertices re-ordered by orientation `o`: the micro-triangle of the OLD order that micro-triangle `index` of the NEW order covers,
 * at `level`.  All in integers:
 *   1. (iu', iv', iw') = the forward decode of `index` (the discrete barycentrics of ommx_micro_vertices before its upright / inverted adjustment);
 *   2. t' = (iw', iu', iv'): the weights of new vertices 0, 1, 2;  t[perm_o[k]] = t'[k]: those of the old vertices;
 *   3. the answer is what the digit loop of ommx_micro_index gives for (iu, iv, iw) = (t[1], t[2], t[0]).
 * For a hit (u', v') in the new order, with b' = (1-u'-v', u', v') and b[perm_o[k]] = b'[k]:
 *     ommx_micro_index(b[1], b[2], level) == ommx_reorient_index(ommx_micro_index(u', v', level), level, o)
 * for every point strictly inside a micro-triangle.  For fixed level and o it is a bijection of 0 .. 4^level - 1, and it is hierarchical: the answer
 * for 4j + c at level + 1, shifted right by two, is the answer for j at level.  Orientations 1 and 2 undo each other; 3, 4 and 5 undo themselves.
 *  - levels above 12 are treated as 12 and an index >= 4^level is reduced modulo 4^level, as in ommx_micro_vertices;
 *  - an orientation above 5 returns `index` as it came. */
OMMX_LOOKUP_FN uint32_t ommx_reorient_index(uint32_t index, uint32_t level, uint32_t orientation)
{
    if (orientation > 5u) return index;
    if (level > OMMX_LOOKUP_MAX_LEVEL) level = OMMX_LOOKUP_MAX_LEVEL;
    if (level == 0u) return 0u;
    index &= (1u << (2u * level)) - 1u;
    const uint32_t b0 = ommx_even_bits(index), b1 = ommx_even_bits(index >> 1);
    const uint32_t fx = ommx_prefix_xor(b0), fy = ommx_prefix_xor(b0 & ~b1);
    const uint32_t t = fy ^ b1, mask = (1u << level) - 1u;
    /* the weights of the new vertices 0, 1, 2 ... */
    const uint32_t t0 = ((~fx & ~t) | (b0 & ~t) | (~b0 & fx & t)) & mask;
    const uint32_t t1 = ((fx & ~t) | (b0 & ~t) | (~b0 & ~fx & t)) & mask;
    const uint32_t t2 = (fy ^ b0) & mask;
    /* ... each handed to the old vertex it is (selects, no indexed array: this is device code too) */
    const uint32_t perm = (uint32_t)(OMMX_REORIENT_PERMS >> (6u * orientation)) & 63u;
    const uint32_t p0 = perm & 3u, p1 = (perm >> 2) & 3u;
    const uint32_t iw = p0 == 0u ? t0 : p1 == 0u ? t1 : t2;
    const uint32_t iu = p0 == 1u ? t0 : p1 == 1u ? t1 : t2;
    const uint32_t iv = p0 == 2u ? t0 : p1 == 2u ? t1 : t2;
    uint32_t source = 0u, x = 0u, y = 0u;
    for (uint32_t i = level; i-- > 0u;) {
        const uint32_t key = x | (y << 1) | (((iu >> i) & 1u) << 2) | (((iv >> i) & 1u) << 3) | (((iw >> i) & 1u) << 4);
        const uint32_t digit = (uint32_t)(OMMX_BIRD_DIGIT_TABLE >> (2u * key)) & 3u;
        source = (source << 2) | digit;
        x ^= digit & 1u;
        y ^= digit == 1u ? 1u : 0u;
    }
    return source;
}

/* The state the result stores for triangle `prim` at the hit (u, v): 0..3 (ommOpacityState) or OMMX_OPACITY_INVALID.
 *  - entry e = result->indexBuffer[prim], signed 8-, 16- or 32-bit after result->indexFormat;
 *  - e in -1..-4 is a special index: state -(e + 1);
 *  - e >= 0 selects descArray[e]: state = bit i (OC1_2_State) or bits 2i..2i+1 (OC1_4_State) of the block at arrayData + offset,
 *    little-endian within bytes, i = ommx_micro_index(u, v, subdivisionLevel).
 * OMMX_OPACITY_INVALID, before any read out of range: prim >= indexCount, an unknown indexFormat, e < -4, e >= descArrayCount, a level
 * above 12, a format other than OC1_2_State / OC1_4_State, or a block that does not fit inside arrayDataSize. */
OMMX_LOOKUP_FN uint32_t ommx_opacity_state(const ommCpuBakeResultDesc* r, uint32_t prim, float u, float v)
{
    if (prim >= r->indexCount) return OMMX_OPACITY_INVALID;
    int32_t e;
    switch (r->indexFormat) {
    case ommIndexFormat_UINT_8:  e = ((const int8_t*)r->indexBuffer)[prim]; break;
    case ommIndexFormat_UINT_16: e = ((const int16_t*)r->indexBuffer)[prim]; break;
    case ommIndexFormat_UINT_32: e = ((const int32_t*)r->indexBuffer)[prim]; break;
    default: return OMMX_OPACITY_INVALID;
    }
    if (e < 0) return e >= -4 ? (uint32_t)(-(e + 1)) : OMMX_OPACITY_INVALID;
    if ((uint32_t)e >= r->descArrayCount) return OMMX_OPACITY_INVALID;
    const ommCpuOpacityMicromapDesc d = r->descArray[e];
    const uint32_t level = d.subdivisionLevel, bits = d.format;   /* ommFormat value == bits per micro-triangle */
    if (level > OMMX_LOOKUP_MAX_LEVEL || (bits != 1u && bits != 2u)) return OMMX_OPACITY_INVALID;
    const uint64_t blockBytes = (((uint64_t)bits << (2u * level)) + 7u) >> 3;
    if ((uint64_t)d.offset + blockBytes > (uint64_t)r->arrayDataSize) return OMMX_OPACITY_INVALID;
    const uint32_t bit = ommx_micro_index(u, v, level) * bits;
    const uint32_t byte = ((const uint8_t*)r->arrayData)[(uint64_t)d.offset + (bit >> 3)];
    return (byte >> (bit & 7u)) & ((1u << bits) - 1u);
}

/* ray flag "force OMM 2-state": UnknownTransparent -> Transparent, UnknownOpaque -> Opaque; other values are returned unchanged */
OMMX_LOOKUP_FN uint32_t ommx_force_2state(uint32_t state)
{
    return (state == 2u || state == 3u) ? state - 2u : state;
}

#endif
