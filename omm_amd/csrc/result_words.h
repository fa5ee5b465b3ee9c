// result_words.h -- the device code shared by the kernels that stage the blocks of a new result (coarsen_units, coarsen_deep, combine_units) and by
// the tail that turns staged blocks into a result (rebuild_kernels.hip): a lane's fields of a source block as bit planes, whole output words with
// their digest and uniformity mask, the reduction of those two per workgroup, and a workgroup's counters.  compare_units (ommxCompareMicromaps)
// reads its two sides with load_fields and stages nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "coarsen_reduce.h"

namespace ommx {

typedef uint64_t WordsVec __attribute__((vector_size(16), may_alias));   // sixteen bytes at a 16-byte aligned address, as one load or store

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
// the digest of a block is the sum of these over its 64-bit words (the last one padded with zeros): any partition of the words gives the same sum
__host__ __device__ __forceinline__ uint64_t word_digest(uint64_t w, uint64_t index) { return mix64(w ^ ((index + 1u) * 0x9E3779B97F4A7C15ull)); }
// the hash-table key of a block (its value never shows in a result: equal keys are confirmed by level, format and bytes)
__host__ __device__ __forceinline__ uint64_t block_key(uint64_t digest, uint32_t level, uint32_t bits) { return mix64(digest + (uint64_t)((level << 2) | bits) * 0xD6E8FEB86659FD93ull); }

// a workgroup's counters: zeroed, added to in LDS, then one global atomic per counter that is not zero
template <uint32_t N> __device__ __forceinline__ void counters_begin(uint32_t* s) { if (threadIdx.x < N) s[threadIdx.x] = 0u; __syncthreads(); }
template <uint32_t N> __device__ __forceinline__ void counters_end(const uint32_t* s, uint32_t* global)
{
    __syncthreads();
    if (threadIdx.x < N && s[threadIdx.x]) atomicAdd(&global[threadIdx.x], s[threadIdx.x]);
}

// The fields [first, first + count) of a source block (count a power of four <= 256, first a multiple of it) as plane pairs, 64 fields each, the
// first field in bit 0 of P[0]; bits above the last field are zero.  16-byte loads where the lane's share is 16 bytes or more at a multiple of 16;
// byte by byte where the share is smaller or the block sits at an odd address.
__device__ __forceinline__ void load_fields(const uint8_t* block, uint32_t bits, uint32_t first, uint32_t count, CoarsenPlanes P[4])
{
    const uint32_t firstBit = first * bits, nbits = count * bits;
    const uint8_t* p = block + (firstBit >> 3);
    const uint32_t n = nbits < 8u ? 1u : nbits >> 3;   // 1 .. 64 bytes
    uint64_t w[8];
    #pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = 0ull;
    if (n >= 16u && ((uintptr_t)p & 15u) == 0u) {
        const WordsVec q0 = ((const WordsVec*)p)[0];
        w[0] = q0[0]; w[1] = q0[1];
        if (n >= 32u) { const WordsVec q1 = ((const WordsVec*)p)[1]; w[2] = q1[0]; w[3] = q1[1]; }
        if (n == 64u) {
            const WordsVec q2 = ((const WordsVec*)p)[2], q3 = ((const WordsVec*)p)[3];
            w[4] = q2[0]; w[5] = q2[1]; w[6] = q3[0]; w[7] = q3[1];
        }
    } else {
        #pragma unroll
        for (int i = 0; i < 8; ++i)
            for (uint32_t b = 0; b < 8u; ++b) { const uint32_t at = 8u * (uint32_t)i + b; if (at < n) w[i] |= (uint64_t)p[at] << (8u * b); }
    }
    if (nbits < 64u) w[0] = (w[0] >> (firstBit & 7u)) & ((1ull << nbits) - 1ull);   // (a share below a byte starts inside its byte)
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (bits == 2u) P[i] = coarsen_split(w[2 * i], w[2 * i + 1]);
        else { P[i].lo = w[i]; P[i].hi = 0ull; }
    }
}

struct UnitOut {      // where a unit's output goes and what its writers learn on the way
    uint8_t* dst;             // the block's first output byte
    uint64_t fieldBase;       // the unit's first output field within the block
    uint32_t outFields;       // of the unit
    uint32_t bits;
    uint64_t digest; uint32_t umask;
};
// 64 output fields (or all of a smaller block): plane pair `pair` of the unit
__device__ __forceinline__ void write_pair(UnitOut& o, CoarsenPlanes pl, uint32_t pair)
{
    const uint32_t fieldOff = pair * 64u;
    if (fieldOff >= o.outFields) return;
    const uint32_t nvalid = o.outFields - fieldOff < 64u ? o.outFields - fieldOff : 64u;
    const uint64_t field = o.fieldBase + fieldOff;
    uint64_t w0, w1 = 0ull;
    if (o.bits == 2u) coarsen_join(pl, &w0, &w1); else w0 = pl.lo;
    if (nvalid == 64u) {
        const uint64_t word = o.bits == 2u ? field >> 5 : field >> 6;
        uint64_t* p = (uint64_t*)o.dst + word;
        p[0] = w0;
        o.digest += word_digest(w0, word); o.umask &= coarsen_word_uniform(w0, 64u, o.bits);
        if (o.bits == 2u) { p[1] = w1; o.digest += word_digest(w1, word + 1u); o.umask &= coarsen_word_uniform(w1, 64u, 2u); }
    } else {   // a block of fewer than 64 fields: the unit is the block, the unused bits of its only byte are written as zeros
        const uint32_t vbits = nvalid * o.bits;   // 1 .. 32
        w0 &= (1ull << vbits) - 1ull;
        const uint32_t nbytes = vbits < 8u ? 1u : vbits >> 3;
        for (uint32_t b = 0; b < nbytes; ++b) o.dst[b] = (uint8_t)(w0 >> (8u * b));
        o.digest += word_digest(w0, 0u); o.umask &= coarsen_word_uniform(w0, vbits, o.bits);
    }
}
// What the writers of a unit learned, added to the block's: per wave by shuffle, across the Waves waves through LDS, then one integer atomic each.
// Every thread of the workgroup calls this; the LDS words are free again after the caller's next __syncthreads().
template <uint32_t Waves>
__device__ __forceinline__ void unit_close(UnitOut& o, uint64_t* s_digest, uint32_t* s_umask, unsigned long long* digest, uint32_t* umask)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { o.digest += shfl_xor_u64(o.digest, d); o.umask &= (uint32_t)__shfl_xor((int)o.umask, d); }
    if (lane == 0u) { s_digest[wave] = o.digest; s_umask[wave] = o.umask; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long dg = 0ull; uint32_t um = 0xFu;
        #pragma unroll
        for (uint32_t w2 = 0; w2 < Waves; ++w2) { dg += s_digest[w2]; um &= s_umask[w2]; }
        if (dg) atomicAdd(digest, dg);
        if (um != 0xFu) atomicAnd(umask, um);
    }
}

} // namespace ommx
