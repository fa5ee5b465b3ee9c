// combine_kernels.hip -- ommxCombineMicromaps (include/omm_mi355x_ext.h has the definition): K device-resident results over the same primitives
// joined into one conservative result, then the tail of a bake on the joined blocks.
//
//   combine_entries   one lane per primitive: the K entries under the bounds rule; a primitive with a failing entry is skipped, one with only
//                     special entries is answered here, every other one puts the hash of its tuple into the table (hash_build.h), lowest index wins
//   combine_leaders   one lane per primitive: the lowest primitive with the same tuple (the entries confirm); a scan of the leaders numbers the tuples
//   combine_prepare   one lane per leader: the K normalised entries of its tuple, the level T, the staging slot, the number of work units
//   combine_units     THE pass over the sources' arrayData: one workgroup per unit of 4^8 output micro-triangles, 256 per lane as four plane pairs.
//                     Per source the lane reads the bytes that cover its micro-triangles at the source's own level, repeats them down to T
//                     (combine_expand.h) and adds them to the join; then it writes whole output words, sums their digest and ANDs their
//                     uniformity masks: one integer atomic each per workgroup
//   combine_classify  uniform blocks become special indices; the others enter the hash table under (digest, level)
//   combine_resolve   the lowest tuple under the same key is the candidate; equal level and bytes make it the representative
//   (radix sort)      representatives by size class descending, stable, hence by lowest primitive index ascending within a class
//   combine_descs / combine_gather / combine_index   descriptors and blocks below 16 bytes; the larger blocks 16 bytes per lane; the index buffer
//
// The tail does what coarsen_kernels.hip's does, on tuples instead of source descriptors: those kernels read level and format through the one
// source's descriptor array, so they are not shared.  All counters are integers and every output byte has one writer.
#include <hip/hip_runtime.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include "combine_kernels.h"
#include "combine_expand.h"
#include "hash_build.h"
#include "wave_search.h"

namespace ommx {
namespace {

constexpr uint32_t kCbBlock = 256;
constexpr uint32_t kCbWaves = kCbBlock / 64;
constexpr uint32_t kCbUnitLevel = 8;               // a workgroup's unit: 4^8 output micro-triangles, 256 per lane
constexpr uint32_t kCbUnitFields = 1u << (2 * kCbUnitLevel);
constexpr uint32_t kCbLaneFields = kCbUnitFields / kCbBlock;
constexpr uint32_t kCbMaxGrid = 65536;
constexpr uint32_t kCbSlotAlign = 16;              // staging slots: 16-byte reads in the gather, 8-byte writes in the join
constexpr uint32_t kCbNoClass = 31;                // sort key of a tuple that emits no block
constexpr uint32_t kCbHist = 2 * kCoarsenLevels;   // (level, format - 1)

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

struct CombineHeader {
    uint32_t skipped, refined, uniform, duplicate;
    uint32_t classCount[kCoarsenSizeClasses];
    uint32_t arrayHist[kCbHist], indexHist[kCbHist];
};
struct CombinePlace { uint64_t base[kCoarsenSizeClasses]; uint32_t first[kCoarsenSizeClasses], count[kCoarsenSizeClasses]; };

// A normalised entry, 8 bytes: a block is offset | level << 32 | fieldBits << 40; a special index is state << 48 (fieldBits 0)
__device__ __forceinline__ uint64_t norm_block(const ommCpuOpacityMicromapDesc d) { return (uint64_t)d.offset | ((uint64_t)d.subdivisionLevel << 32) | ((uint64_t)d.format << 40); }
__device__ __forceinline__ uint64_t norm_special(uint32_t state) { return (uint64_t)state << 48; }
__device__ __forceinline__ uint32_t norm_bits(uint64_t n) { return (uint32_t)(n >> 40) & 3u; }
__device__ __forceinline__ uint32_t norm_level(uint64_t n) { return (uint32_t)(n >> 32) & 0xFFu; }
__device__ __forceinline__ uint32_t norm_state(uint64_t n) { return (uint32_t)(n >> 48) & 3u; }

// A descriptor is read ONCE, as one 8-byte load, and judged from registers (a caller's array is only 4-byte aligned: the hardware takes that).
typedef uint32_t CbDescWords __attribute__((vector_size(8), aligned(4), may_alias));
__device__ __forceinline__ ommCpuOpacityMicromapDesc load_desc(const ommCpuOpacityMicromapDesc* p)
{
    const CbDescWords w = *(const CbDescWords*)p;
    ommCpuOpacityMicromapDesc d; d.offset = w[0]; d.subdivisionLevel = (uint16_t)(w[1] & 0xFFFFu); d.format = (uint16_t)(w[1] >> 16);
    return d;
}
// The bounds rule: level <= 12, format 1 or 2, block inside arrayDataSize.
__device__ __forceinline__ bool desc_ok(const ommCpuOpacityMicromapDesc d, uint32_t arrayDataSize)
{
    const uint32_t level = d.subdivisionLevel, bits = d.format;
    if (level > kCoarsenMaxLevel || (bits != 1u && bits != 2u)) return false;
    return (uint64_t)d.offset + coarsen_block_bytes(level, bits) <= (uint64_t)arrayDataSize;
}
__device__ __forceinline__ int32_t index_entry(const void* index, int format, uint64_t i)
{
    if (format == ommIndexFormat_UINT_8) return ((const int8_t*)index)[i];
    if (format == ommIndexFormat_UINT_16) return ((const int16_t*)index)[i];
    return ((const int32_t*)index)[i];
}
// entry e of a source -> false: it fails the rule; otherwise its normalised form
__device__ __forceinline__ bool normalise(const CombineSource& s, int32_t e, uint64_t* out)
{
    if (e < 0) { *out = norm_special((uint32_t)(-(e + 1))); return e >= -4; }
    if ((uint32_t)e >= s.descCount) return false;
    const ommCpuOpacityMicromapDesc d = load_desc(s.descs + e);
    *out = norm_block(d);
    return desc_ok(d, s.arrayDataSize);
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
// the digest of a block is the sum of these over its 64-bit words (the last one padded with zeros): any partition of the words gives the same sum
__device__ __forceinline__ uint64_t word_digest(uint64_t w, uint64_t index) { return mix64(w ^ ((index + 1u) * 0x9E3779B97F4A7C15ull)); }
__device__ __forceinline__ uint64_t block_key(uint64_t digest, uint32_t level) { return mix64(digest + (uint64_t)(level + 1u) * 0xD6E8FEB86659FD93ull); }
__device__ __forceinline__ uint64_t tuple_hash(uint64_t h, int32_t e) { return mix64(h ^ (uint64_t)(uint32_t)e) + 0x9E3779B97F4A7C15ull; }

// a workgroup's counters: zeroed, added to in LDS, then one global atomic per counter that is not zero
template <uint32_t N> __device__ __forceinline__ void counters_begin(uint32_t* s) { if (threadIdx.x < N) s[threadIdx.x] = 0u; __syncthreads(); }
template <uint32_t N> __device__ __forceinline__ void counters_end(const uint32_t* s, uint32_t* global)
{
    __syncthreads();
    if (threadIdx.x < N && s[threadIdx.x]) atomicAdd(&global[threadIdx.x], s[threadIdx.x]);
}

// A. one lane per primitive and turn
__global__ __launch_bounds__(kCbBlock) void combine_entries(CombineArgs a, HashTable table, int32_t* __restrict__ code, unsigned long long* __restrict__ key,
                                                            CombineHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    uint32_t skipped = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kCbBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x; i < a.indexCount; i += stride) {
        bool ok = true, any = false;
        uint32_t allSide = 1u, anySide = 0u, anyUnknown = 0u;
        uint64_t h = 0ull;
        for (uint32_t k = 0; k < a.sourceCount && ok; ++k) {
            const CombineSource& s = a.source[k];
            const int32_t e = index_entry(s.index, s.indexFormat, i);
            uint64_t n = 0ull;
            ok = normalise(s, e, &n);
            if (norm_bits(n)) any = true;
            else { const uint32_t st = norm_state(n); allSide &= st & 1u; anySide |= st & 1u; anyUnknown |= st >> 1; }
            h = tuple_hash(h, e);
        }
        int32_t c = 0;
        if (!ok) { c = -4; skipped++; }
        else if (!any) {
            uint32_t r = anySide != allSide ? a.mixedState : (allSide | (anyUnknown << 1));
            if (a.format == 1u) r &= 1u;
            c = -(int32_t)(r + 1u);
        } else { key[i] = h; hash_put_min(table, h, (uint32_t)i); }
        code[i] = c;
    }
    if (skipped) atomicAdd(&s_n[0], skipped);
    counters_end<1>(s_n, &hdr->skipped);
}

// B. one lane per primitive and one for the scan's closing element
__global__ __launch_bounds__(kCbBlock) void combine_leaders(CombineArgs a, HashTable table, const int32_t* __restrict__ code, const unsigned long long* __restrict__ key,
                                                            uint32_t* __restrict__ leader, uint32_t* __restrict__ isLeader)
{
    const uint64_t i = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x;
    if (i > a.indexCount) return;
    uint32_t f = 0u;
    if (i < a.indexCount && code[i] == 0) {
        uint32_t c = hash_get(table, key[i], (uint32_t)i);
        if (c != (uint32_t)i) {   // (two tuples under one 64-bit hash: the later one is joined on its own, and merged again as a duplicate)
            bool same = true;
            for (uint32_t k = 0; k < a.sourceCount && same; ++k) {
                const CombineSource& s = a.source[k];
                same = index_entry(s.index, s.indexFormat, c) == index_entry(s.index, s.indexFormat, i);
            }
            if (!same) c = (uint32_t)i;
        }
        leader[i] = c;
        f = c == (uint32_t)i ? 1u : 0u;
    }
    isLeader[i] = f;
}

// C. one lane per primitive and one for the scans' closing element; the leaders work
__global__ __launch_bounds__(kCbBlock) void combine_prepare(CombineArgs a, uint32_t tuples, const int32_t* __restrict__ code, const uint32_t* __restrict__ leader,
                                                            const uint32_t* __restrict__ tupleStart, unsigned long long* __restrict__ norm, uint32_t* __restrict__ level,
                                                            unsigned long long* __restrict__ slot, unsigned long long* __restrict__ units,
                                                            unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask, CombineHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const uint64_t i = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x;
    if (i == a.indexCount) { slot[tuples] = 0ull; units[tuples] = 0ull; }
    if (i < a.indexCount && code[i] == 0 && leader[i] == (uint32_t)i) {
        const uint32_t t = tupleStart[i];
        uint32_t top = 0u, low = kCoarsenMaxLevel;
        for (uint32_t k = 0; k < a.sourceCount; ++k) {
            const CombineSource& s = a.source[k];
            uint64_t n = 0ull;
            (void)normalise(s, index_entry(s.index, s.indexFormat, i), &n);   // (it passed in combine_entries)
            norm[(uint64_t)t * a.sourceCount + k] = n;
            if (norm_bits(n)) { const uint32_t l = norm_level(n); top = l > top ? l : top; low = l < low ? l : low; }
        }
        unsigned long long bytes = coarsen_block_bytes(top, a.format);
        bytes = (bytes + kCbSlotAlign - 1u) & ~(unsigned long long)(kCbSlotAlign - 1u);
        level[t] = top; slot[t] = bytes;
        units[t] = top > kCbUnitLevel ? 1ull << (2u * (top - kCbUnitLevel)) : 1ull;
        digest[t] = 0ull; umask[t] = 0xFu;
        if (low < top) atomicAdd(&s_n[0], 1u);
    }
    counters_end<1>(s_n, &hdr->refined);
}

// ---- the join of one unit by one workgroup ----
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

typedef uint64_t CbVec __attribute__((vector_size(16), may_alias));

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
        const CbVec q0 = ((const CbVec*)p)[0];
        w[0] = q0[0]; w[1] = q0[1];
        if (n >= 32u) { const CbVec q1 = ((const CbVec*)p)[1]; w[2] = q1[0]; w[3] = q1[1]; }
        if (n == 64u) {
            const CbVec q2 = ((const CbVec*)p)[2], q3 = ((const CbVec*)p)[3];
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

// D. one unit per workgroup and turn
__global__ __launch_bounds__(kCbBlock) void combine_units(CombineArgs a, uint32_t tuples, const unsigned long long* __restrict__ norm, const uint32_t* __restrict__ level,
                                                          const unsigned long long* __restrict__ unitStart, const unsigned long long* __restrict__ slotStart,
                                                          uint8_t* __restrict__ staging, unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask)
{
    __shared__ uint64_t s_digest[kCbWaves];
    __shared__ uint32_t s_umask[kCbWaves];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned long long total = unitStart[tuples];
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t tup = owner_of_segment(unitStart, tuples, u);
        const uint32_t T = level[tup];
        const uint32_t unit = (uint32_t)(u - unitStart[tup]);
        const uint32_t unitFields = T < kCbUnitLevel ? 1u << (2u * T) : kCbUnitFields;
        const bool active = t * kCbLaneFields < unitFields;
        const uint32_t laneFields = unitFields < kCbLaneFields ? unitFields : kCbLaneFields;   // (of an active lane)
        const uint32_t firstField = unit * kCbUnitFields + t * kCbLaneFields;                   // of the block, at level T
        UnitOut o; o.dst = staging + slotStart[tup]; o.fieldBase = (uint64_t)unit * kCbUnitFields; o.outFields = unitFields; o.bits = a.format; o.digest = 0ull; o.umask = 0xFu;
        if (active) {
            CombineJoin J[4];
            #pragma unroll
            for (int j = 0; j < 4; ++j) J[j] = combine_join_begin();
            for (uint32_t k = 0; k < a.sourceCount; ++k) {
                const uint64_t n = norm[(uint64_t)tup * a.sourceCount + k];
                const uint32_t bits = norm_bits(n);
                if (bits == 0u) {
                    const CoarsenPlanes q = combine_broadcast(norm_state(n));
                    #pragma unroll
                    for (int j = 0; j < 4; ++j) combine_join_add(J[j], q);
                    continue;
                }
                const uint32_t down = T - norm_level(n), shift = 2u * down;   // shift <= 24
                const uint32_t count = (laneFields >> shift) ? laneFields >> shift : 1u;
                CoarsenPlanes P[4];
                load_fields(a.source[k].arrayData + (uint32_t)n, bits, firstField >> shift, count, P);
                if (down == 0u) {
                    #pragma unroll
                    for (int j = 0; j < 4; ++j) combine_join_add(J[j], P[j]);
                } else {
                    // output pair j covers the source fields [j * 64 >> shift, (j + 1) * 64 >> shift) of the lane's share: 16, 4, one, or the one
                    const uint32_t rep = down < 3u ? down : 3u, per = down < 4u ? 64u >> shift : 0u;
                    #pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        CoarsenPlanes q; q.lo = P[0].lo >> (per * (uint32_t)j); q.hi = P[0].hi >> (per * (uint32_t)j);
                        combine_join_add(J[j], combine_repeat_planes(q, rep));
                    }
                }
            }
            #pragma unroll
            for (int j = 0; j < 4; ++j) write_pair(o, combine_join_end(J[j], a.format, a.mixedState), 4u * t + (uint32_t)j);
        }
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { o.digest += shfl_xor_u64(o.digest, d); o.umask &= (uint32_t)__shfl_xor((int)o.umask, d); }
        if (lane == 0u) { s_digest[wave] = o.digest; s_umask[wave] = o.umask; }
        __syncthreads();
        if (t == 0u) {
            unsigned long long dg = 0ull; uint32_t um = 0xFu;
            #pragma unroll
            for (uint32_t w2 = 0; w2 < kCbWaves; ++w2) { dg += s_digest[w2]; um &= s_umask[w2]; }
            if (dg) atomicAdd(digest + tup, dg);
            if (um != 0xFu) atomicAnd(umask + tup, um);
        }
        __syncthreads();   // (the LDS words are the next unit's too)
    }
}

// E1. one lane per tuple: the special index of a uniform block, every other block into the hash table
__global__ __launch_bounds__(kCbBlock) void combine_classify(uint32_t tuples, const uint32_t* __restrict__ level, const unsigned long long* __restrict__ digest,
                                                             const uint32_t* __restrict__ umask, int32_t* __restrict__ special, HashTable table, CombineHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const uint64_t t = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x;
    if (t < tuples) {
        const uint32_t um = umask[t];
        int32_t sp = 0;
        if (um) { sp = -(int32_t)(__ffs((int)um)); atomicAdd(&s_n[0], 1u); }   // bit s -> -(s + 1)
        else hash_put_min(table, block_key(digest[t], level[t]), (uint32_t)t);
        special[t] = sp;
    }
    counters_end<1>(s_n, &hdr->uniform);
}

__device__ __forceinline__ bool same_bytes(const uint8_t* x0, const uint8_t* y0, uint64_t n)
{
    if (n >= 64u) {   // (slots are 16-byte aligned, sizes are powers of two) 64 bytes of each block per turn: eight loads in flight, one branch
        const CbVec* x = (const CbVec*)x0; const CbVec* y = (const CbVec*)y0;
        for (uint64_t i = 0; i < n / 16u; i += 4u) {
            const CbVec d = (x[i] ^ y[i]) | (x[i + 1u] ^ y[i + 1u]) | (x[i + 2u] ^ y[i + 2u]) | (x[i + 3u] ^ y[i + 3u]);
            if (d[0] | d[1]) return false;
        }
        return true;
    }
    if (n >= 8u) {
        const uint64_t* x = (const uint64_t*)x0; const uint64_t* y = (const uint64_t*)y0;
        for (uint64_t i = 0; i < n / 8u; ++i) if (x[i] != y[i]) return false;
        return true;
    }
    for (uint64_t i = 0; i < n; ++i) if (x0[i] != y0[i]) return false;
    return true;
}

// E2. one lane per tuple: its representative, and the sort key of a block that will be emitted
__global__ __launch_bounds__(kCbBlock) void combine_resolve(uint32_t tuples, uint32_t format, const uint32_t* __restrict__ level, const unsigned long long* __restrict__ digest,
                                                            const int32_t* __restrict__ special, HashTable table, const unsigned long long* __restrict__ slotStart,
                                                            const uint8_t* __restrict__ staging, uint32_t* __restrict__ rep, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals, CombineHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1 + kCoarsenSizeClasses];
    counters_begin<1 + kCoarsenSizeClasses>(s_n);
    const uint64_t t = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x;
    if (t < tuples) {
        uint32_t key = kCbNoClass, leader = (uint32_t)t;
        if (special[t] == 0) {
            const uint32_t T = level[t];
            const uint64_t bytes = coarsen_block_bytes(T, format);
            const uint32_t c = hash_get(table, block_key(digest[t], T), (uint32_t)t);
            if (c < t && level[c] == T && same_bytes(staging + slotStart[t], staging + slotStart[c], bytes)) leader = c;
            if (leader == t) {
                const uint32_t cls = 63u - (uint32_t)__clzll((long long)bytes);
                key = kCoarsenSizeClasses - 1u - cls;
                atomicAdd(&s_n[1u + cls], 1u);
            } else atomicAdd(&s_n[0], 1u);
        }
        rep[t] = leader; keys[t] = key; vals[t] = (uint32_t)t;
    }
    counters_end<1 + kCoarsenSizeClasses>(s_n, &hdr->duplicate);
}

// F1. one lane per output descriptor
__global__ __launch_bounds__(kCbBlock) void combine_descs(uint32_t count, uint32_t format, CombinePlace place, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                          const uint32_t* __restrict__ level, const unsigned long long* __restrict__ slotStart,
                                                          const uint8_t* __restrict__ staging, uint8_t* __restrict__ outArray, ommCpuOpacityMicromapDesc* __restrict__ outDescs,
                                                          uint32_t* __restrict__ newIndex, CombineHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[kCbHist];
    counters_begin<kCbHist>(s_n);
    const uint64_t j = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x;
    if (j < count) {
        const uint32_t t = vals[j], cls = kCoarsenSizeClasses - 1u - keys[j], T = level[t];
        const uint64_t off = place.base[cls] + ((uint64_t)(j - place.first[cls]) << cls);
        ommCpuOpacityMicromapDesc o; o.offset = (uint32_t)off; o.subdivisionLevel = (uint16_t)T; o.format = (uint16_t)format;
        outDescs[j] = o;
        newIndex[t] = (uint32_t)j;
        atomicAdd(&s_n[2u * T + format - 1u], 1u);
        if (cls < 4u) { const uint8_t* s = staging + slotStart[t]; for (uint32_t b = 0; b < (1u << cls); ++b) outArray[off + b] = s[b]; }
    }
    counters_end<kCbHist>(s_n, hdr->arrayHist);
}

// F2. the blocks of 16 bytes and more -- a prefix of the output: 16 bytes per lane and turn
__global__ __launch_bounds__(kCbBlock) void combine_gather(uint64_t bigBytes, CombinePlace place, const uint32_t* __restrict__ vals, const unsigned long long* __restrict__ slotStart,
                                                           const uint8_t* __restrict__ staging, uint8_t* __restrict__ outArray)
{
    const uint64_t stride = (uint64_t)gridDim.x * kCbBlock * 16u;
    for (uint64_t pos = ((uint64_t)blockIdx.x * kCbBlock + threadIdx.x) * 16u; pos < bigBytes; pos += stride) {
        uint32_t cls = kCoarsenSizeClasses - 1u;
        while (cls > 4u && pos >= place.base[cls] + ((uint64_t)place.count[cls] << cls)) --cls;
        const uint64_t rel = pos - place.base[cls];
        const uint32_t t = vals[place.first[cls] + (uint32_t)(rel >> cls)];
        *(CbVec*)(outArray + pos) = *(const CbVec*)(staging + slotStart[t] + (rel & ((1ull << cls) - 1ull)));
    }
}

// F3. one lane per primitive and turn
__global__ __launch_bounds__(kCbBlock) void combine_index(uint32_t indexCount, uint32_t format, const int32_t* __restrict__ code, const uint32_t* __restrict__ leader,
                                                          const uint32_t* __restrict__ tupleStart, const uint32_t* __restrict__ level, const int32_t* __restrict__ special,
                                                          const uint32_t* __restrict__ rep, const uint32_t* __restrict__ newIndex, int32_t* __restrict__ outIndex,
                                                          CombineHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[kCbHist];
    counters_begin<kCbHist>(s_n);
    const uint64_t stride = (uint64_t)gridDim.x * kCbBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x; i < indexCount; i += stride) {
        int32_t v = code[i];
        if (v == 0) {
            const uint32_t t = tupleStart[leader[i]];
            v = special[t];
            if (v == 0) {
                v = (int32_t)newIndex[rep[t]];
                atomicAdd(&s_n[2u * level[t] + format - 1u], 1u);
            }
        }
        outIndex[i] = v;
    }
    counters_end<kCbHist>(s_n, hdr->indexHist);
}

struct HeadLayout { size_t header, table, code, key, leader, tupleStart, temp, bytes; size_t tempBytes; uint32_t slots; };
HeadLayout head_layout(const CombineArgs& a)
{
    HeadLayout L; size_t o = 0;
    const size_t N = a.indexCount;
    const auto take = [&o](size_t bytes) { const size_t at = o; o += pad256(bytes); return at; };
    L.header = take(sizeof(CombineHeader));
    L.slots = hash_table_slots(N);
    L.table = take(hash_table_bytes(L.slots));
    L.code = take(4 * N); L.key = take(8 * N); L.leader = take(4 * N); L.tupleStart = take(4 * (N + 1));
    L.tempBytes = 0;
    (void)rocprim::exclusive_scan(nullptr, L.tempBytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, N + 1, rocprim::plus<uint32_t>());
    L.temp = take(L.tempBytes);
    L.bytes = o;
    return L;
}
struct TupleLayout { size_t norm, level, slot, units, digest, umask, special, rep, keys, vals, keysSorted, valsSorted, newIndex, temp, bytes; size_t tempBytes; };
TupleLayout tuple_layout(const CombineArgs& a, uint32_t tuples)
{
    TupleLayout L; size_t o = 0;
    const size_t M = tuples;
    const auto take = [&o](size_t bytes) { const size_t at = o; o += pad256(bytes); return at; };
    L.norm = take(8 * M * a.sourceCount); L.level = take(4 * M);
    L.slot = take(8 * (M + 1)); L.units = take(8 * (M + 1));
    L.digest = take(8 * M); L.umask = take(4 * M); L.special = take(4 * M); L.rep = take(4 * M);
    L.keys = take(4 * M); L.vals = take(4 * M); L.keysSorted = take(4 * M); L.valsSorted = take(4 * M); L.newIndex = take(4 * M);
    size_t scanBytes = 0, sortBytes = 0;
    (void)rocprim::exclusive_scan(nullptr, scanBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, M + 1, rocprim::plus<unsigned long long>());
    if (M) (void)rocprim::radix_sort_pairs(nullptr, sortBytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, M, 0u, 5u);
    L.tempBytes = scanBytes > sortBytes ? scanBytes : sortBytes;
    L.temp = take(L.tempBytes);
    L.bytes = o;
    return L;
}
uint32_t strided_grid(uint64_t items)
{
    const uint64_t blocks = (items + kCbBlock - 1u) / kCbBlock;
    return (uint32_t)(blocks < kCbMaxGrid ? (blocks ? blocks : 1u) : kCbMaxGrid);
}
uint32_t per_item_grid(uint64_t items) { return (uint32_t)((items + kCbBlock - 1u) / kCbBlock); }
CombinePlace place_of(const CombineCounts& c)
{
    CombinePlace p; uint64_t at = 0; uint32_t first = 0;
    for (int cls = (int)kCoarsenSizeClasses - 1; cls >= 0; --cls) {
        p.base[cls] = at; p.first[cls] = first; p.count[cls] = c.classCount[cls];
        at += (uint64_t)c.classCount[cls] << cls; first += c.classCount[cls];
    }
    return p;
}

} // namespace

size_t combine_head_bytes(const CombineArgs& a) { return head_layout(a).bytes; }
size_t combine_tuple_bytes(const CombineArgs& a, uint32_t tuples) { return tuple_layout(a, tuples).bytes; }

#define COMBINE_CHECK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

hipError_t combine_tuples(const CombineArgs& a, void* head, CombineTuples* out, hipStream_t stream)
{
    const HeadLayout L = head_layout(a);
    uint8_t* base = (uint8_t*)head;
    const uint32_t N = a.indexCount;
    CombineHeader* hdr = (CombineHeader*)(base + L.header);
    int32_t* code = (int32_t*)(base + L.code);
    unsigned long long* key = (unsigned long long*)(base + L.key);
    uint32_t* tupleStart = (uint32_t*)(base + L.tupleStart);
    const HashTable table = hash_table_at(base + L.table, L.slots);
    COMBINE_CHECK(hipMemsetAsync(hdr, 0, sizeof(CombineHeader), stream));
    COMBINE_CHECK(hipMemsetAsync(base + L.table, 0xFF, hash_table_bytes(L.slots), stream));
    combine_entries<<<strided_grid(N), kCbBlock, 0, stream>>>(a, table, code, key, hdr);
    COMBINE_CHECK(hipGetLastError());
    combine_leaders<<<per_item_grid((uint64_t)N + 1u), kCbBlock, 0, stream>>>(a, table, code, key, (uint32_t*)(base + L.leader), tupleStart);
    COMBINE_CHECK(hipGetLastError());
    size_t tb = L.tempBytes;   // (in place: every element is read before it is written)
    COMBINE_CHECK(rocprim::exclusive_scan(base + L.temp, tb, tupleStart, tupleStart, 0u, (size_t)N + 1, rocprim::plus<uint32_t>(), stream));
    uint32_t tuples = 0;
    CombineHeader h;
    COMBINE_CHECK(hipMemcpyAsync(&tuples, tupleStart + N, sizeof tuples, hipMemcpyDeviceToHost, stream));
    COMBINE_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    COMBINE_CHECK(hipStreamSynchronize(stream));
    out->tuples = tuples; out->skipped = h.skipped;
    return hipSuccess;
}

hipError_t combine_plan(const CombineArgs& a, void* head, void* perTuple, const CombineTuples& t, CombinePlan* out, hipStream_t stream)
{
    const HeadLayout L = head_layout(a);
    const TupleLayout U = tuple_layout(a, t.tuples);
    uint8_t *base = (uint8_t*)head, *tb = (uint8_t*)perTuple;
    const uint32_t N = a.indexCount, M = t.tuples;
    CombineHeader* hdr = (CombineHeader*)(base + L.header);
    unsigned long long* slot = (unsigned long long*)(tb + U.slot);
    unsigned long long* units = (unsigned long long*)(tb + U.units);
    combine_prepare<<<per_item_grid((uint64_t)N + 1u), kCbBlock, 0, stream>>>(a, M, (const int32_t*)(base + L.code), (const uint32_t*)(base + L.leader),
                                                                             (const uint32_t*)(base + L.tupleStart), (unsigned long long*)(tb + U.norm), (uint32_t*)(tb + U.level),
                                                                             slot, units, (unsigned long long*)(tb + U.digest), (uint32_t*)(tb + U.umask), hdr);
    COMBINE_CHECK(hipGetLastError());
    size_t n = U.tempBytes;   // (in place: every element is read before it is written)
    COMBINE_CHECK(rocprim::exclusive_scan(tb + U.temp, n, slot, slot, 0ull, (size_t)M + 1, rocprim::plus<unsigned long long>(), stream));
    n = U.tempBytes;
    COMBINE_CHECK(rocprim::exclusive_scan(tb + U.temp, n, units, units, 0ull, (size_t)M + 1, rocprim::plus<unsigned long long>(), stream));
    unsigned long long stagingBytes = 0, totalUnits = 0;
    CombineHeader h;
    COMBINE_CHECK(hipMemcpyAsync(&stagingBytes, slot + M, sizeof stagingBytes, hipMemcpyDeviceToHost, stream));
    COMBINE_CHECK(hipMemcpyAsync(&totalUnits, units + M, sizeof totalUnits, hipMemcpyDeviceToHost, stream));
    COMBINE_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    COMBINE_CHECK(hipStreamSynchronize(stream));
    out->stagingBytes = stagingBytes; out->units = totalUnits; out->refined = h.refined;
    return hipSuccess;
}

hipError_t combine_join(const CombineArgs& a, void* head, void* perTuple, void* staging, const CombineTuples& t, const CombinePlan& plan, CombineCounts* out, hipStream_t stream)
{
    const HeadLayout L = head_layout(a);
    const TupleLayout U = tuple_layout(a, t.tuples);
    uint8_t *base = (uint8_t*)head, *tb = (uint8_t*)perTuple;
    const uint32_t M = t.tuples;
    CombineHeader* hdr = (CombineHeader*)(base + L.header);
    const uint32_t* level = (const uint32_t*)(tb + U.level);
    const unsigned long long* slot = (const unsigned long long*)(tb + U.slot);
    unsigned long long* digest = (unsigned long long*)(tb + U.digest);
    uint32_t* umask = (uint32_t*)(tb + U.umask);
    int32_t* special = (int32_t*)(tb + U.special);
    // the table of the tuples has done its work: the blocks use its memory (there are no more tuples than primitives)
    const uint32_t slots = hash_table_slots(M);
    const HashTable table = hash_table_at(base + L.table, slots);
    COMBINE_CHECK(hipMemsetAsync(base + L.table, 0xFF, hash_table_bytes(slots), stream));
    combine_units<<<(uint32_t)(plan.units < kCbMaxGrid ? plan.units : kCbMaxGrid), kCbBlock, 0, stream>>>(a, M, (const unsigned long long*)(tb + U.norm), level,
                                                                                                         (const unsigned long long*)(tb + U.units), slot, (uint8_t*)staging, digest, umask);
    COMBINE_CHECK(hipGetLastError());
    combine_classify<<<per_item_grid(M), kCbBlock, 0, stream>>>(M, level, digest, umask, special, table, hdr);
    COMBINE_CHECK(hipGetLastError());
    combine_resolve<<<per_item_grid(M), kCbBlock, 0, stream>>>(M, a.format, level, digest, special, table, slot, (const uint8_t*)staging, (uint32_t*)(tb + U.rep),
                                                               (uint32_t*)(tb + U.keys), (uint32_t*)(tb + U.vals), hdr);
    COMBINE_CHECK(hipGetLastError());
    CombineHeader h;
    COMBINE_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    COMBINE_CHECK(hipStreamSynchronize(stream));
    memset(out, 0, sizeof *out);
    out->uniform = h.uniform; out->duplicate = h.duplicate;
    for (uint32_t c = 0; c < kCoarsenSizeClasses; ++c) { out->classCount[c] = h.classCount[c]; out->descCount += h.classCount[c]; out->arrayBytes += (uint64_t)h.classCount[c] << c; }
    return hipSuccess;
}

hipError_t combine_emit(const CombineArgs& a, void* head, void* perTuple, const void* staging, const CombineTuples& t, const CombineCounts& counts, const CombineOutputs& o,
                        hipStream_t stream)
{
    const HeadLayout L = head_layout(a);
    const TupleLayout U = tuple_layout(a, t.tuples);
    uint8_t *base = (uint8_t*)head, *tb = (uint8_t*)perTuple;
    const uint32_t M = t.tuples;
    CombineHeader* hdr = (CombineHeader*)(base + L.header);
    if (counts.descCount) {
        const uint32_t* level = (const uint32_t*)(tb + U.level);
        const unsigned long long* slot = (const unsigned long long*)(tb + U.slot);
        const uint32_t* valsSorted = (const uint32_t*)(tb + U.valsSorted);
        const CombinePlace place = place_of(counts);
        size_t n = U.tempBytes;   // stable: equal size classes keep the order of their lowest primitives
        COMBINE_CHECK(rocprim::radix_sort_pairs(tb + U.temp, n, (uint32_t*)(tb + U.keys), (uint32_t*)(tb + U.keysSorted), (uint32_t*)(tb + U.vals), (uint32_t*)(tb + U.valsSorted),
                                                (size_t)M, 0u, 5u, stream));
        combine_descs<<<per_item_grid(counts.descCount), kCbBlock, 0, stream>>>(counts.descCount, a.format, place, (const uint32_t*)(tb + U.keysSorted), valsSorted, level, slot,
                                                                                 (const uint8_t*)staging, o.arrayData, o.descs, (uint32_t*)(tb + U.newIndex), hdr);
        COMBINE_CHECK(hipGetLastError());
        const uint64_t big = place.base[3];   // the blocks of 16 bytes and more end where the 8-byte blocks begin
        if (big) {
            combine_gather<<<strided_grid(big / 16u), kCbBlock, 0, stream>>>(big, place, valsSorted, slot, (const uint8_t*)staging, o.arrayData);
            COMBINE_CHECK(hipGetLastError());
        }
    }
    combine_index<<<strided_grid(a.indexCount), kCbBlock, 0, stream>>>(a.indexCount, a.format, (const int32_t*)(base + L.code), (const uint32_t*)(base + L.leader),
                                                                       (const uint32_t*)(base + L.tupleStart), M ? (const uint32_t*)(tb + U.level) : nullptr,
                                                                       M ? (const int32_t*)(tb + U.special) : nullptr, M ? (const uint32_t*)(tb + U.rep) : nullptr,
                                                                       M ? (const uint32_t*)(tb + U.newIndex) : nullptr, o.index, hdr);
    COMBINE_CHECK(hipGetLastError());
    CombineHeader h;
    COMBINE_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    COMBINE_CHECK(hipStreamSynchronize(stream));
    memcpy(o.hist, h.arrayHist, sizeof h.arrayHist);
    memcpy(o.hist + kCbHist, h.indexHist, sizeof h.indexHist);
    return hipSuccess;
}

} // namespace ommx
