// coarsen_kernels.hip -- ommxCoarsenMicromap (include/omm_mi355x_ext.h has the definition): the blocks of a device-resident result reduced to a
// maximum subdivision level, then the tail of a bake on what is left -- uniform blocks to special indices, equal blocks merged, blocks ordered
// by size, descriptors, index buffer and histograms rebuilt.
//
//   coarsen_mark      the index buffer once: which descriptors are selected (and pass the bounds rule), how many primitives are skipped
//   coarsen_prepare   per selected descriptor: the size of its slot in the staging arena, its number of work units, its place in the deep list
//   coarsen_units     THE pass over arrayData: one workgroup per unit of 4^8 micro-triangles; 256 of them per lane as bit planes in registers
//                     (coarsen_reduce.h), four levels in the lane, up to three across the lanes of the wave by ballot, one across the waves in
//                     LDS.  A block above level 8 has several units whose outputs must be whole words, so such a block is reduced by at most five
//                     levels here and, if it has further to go, once more by coarsen_deep (the rule is associative).  The writers of the output
//                     words also sum a digest of them and AND the "all fields equal s" masks: one integer atomic each per workgroup.
//   coarsen_classify  uniform blocks become special indices; the others enter the hash table (hash_build.h) under (digest, level, format)
//   coarsen_resolve   the lowest source index under the same key is the candidate; equal level, format and bytes make it the representative
//   (radix sort)      representatives by size class descending, stable, hence by source index ascending within a class
//   coarsen_descs / coarsen_gather / coarsen_index   descriptors and blocks below 16 bytes; the larger blocks 16 bytes per lane; the index buffer
//
// All counters are integers and every output byte has one writer, so the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include "coarsen_kernels.h"
#include "coarsen_reduce.h"
#include "hash_build.h"
#include "wave_search.h"

namespace ommx {

constexpr uint32_t kCoBlock = 256;
constexpr uint32_t kCoWaves = kCoBlock / 64;
constexpr uint32_t kCoUnitLevel = 8;              // a workgroup's unit: 4^8 micro-triangles, 256 per lane
constexpr uint32_t kCoUnitFields = 1u << (2 * kCoUnitLevel);
constexpr uint32_t kCoFirstPassLevels = 5;        // of a block with several units: every unit then still writes 64 fields or more
constexpr uint32_t kCoMaxGrid = 65536;
constexpr uint32_t kCoSlotAlign = 16;             // staging slots: 16-byte reads in the gather, 8-byte writes in the reduction
constexpr uint32_t kCoNoClass = 31;               // sort key of a descriptor that emits no block
constexpr uint32_t kCoHist = 2 * kCoarsenLevels;  // (level, format - 1)

static inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

struct CoarsenHeader {
    uint32_t skipped, deepBlocks, referenced, coarsened, uniform, duplicate;
    uint32_t classCount[kCoarsenSizeClasses];
    uint32_t arrayHist[kCoHist], indexHist[kCoHist];
};
struct CoarsenPlace { uint64_t base[kCoarsenSizeClasses]; uint32_t first[kCoarsenSizeClasses], count[kCoarsenSizeClasses]; };

// what becomes of a source block
struct BlockPlan {
    uint32_t level, bits, target, firstPass;   // firstPass: levels taken off by coarsen_units
    bool deep;                                 // coarsen_deep takes off the rest
};
__device__ __forceinline__ BlockPlan plan_block(const ommCpuOpacityMicromapDesc d, uint32_t maxLevel)
{
    BlockPlan p;
    p.level = d.subdivisionLevel; p.bits = d.format;
    p.target = p.level < maxLevel ? p.level : maxLevel;
    const uint32_t k = p.level - p.target;
    const bool several = p.level > kCoUnitLevel;
    p.firstPass = several && k > kCoFirstPassLevels ? kCoFirstPassLevels : k;
    p.deep = p.firstPass != k;
    return p;
}

// A descriptor is read ONCE, as one 8-byte load, and judged from registers (a caller's array is only 4-byte aligned: the hardware takes that).
typedef uint32_t CoDescWords __attribute__((vector_size(8), aligned(4), may_alias));
__device__ __forceinline__ ommCpuOpacityMicromapDesc load_desc(const ommCpuOpacityMicromapDesc* p)
{
    const CoDescWords w = *(const CoDescWords*)p;
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
__device__ __forceinline__ void index_store(void* index, int format, uint64_t i, int32_t v)
{
    if (format == ommIndexFormat_UINT_8) ((int8_t*)index)[i] = (int8_t)v;
    else if (format == ommIndexFormat_UINT_16) ((int16_t*)index)[i] = (int16_t)v;
    else ((int32_t*)index)[i] = v;
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
__device__ __forceinline__ uint64_t block_key(uint64_t digest, uint32_t level, uint32_t bits) { return mix64(digest + (uint64_t)((level << 2) | bits) * 0xD6E8FEB86659FD93ull); }

// a workgroup's counters: zeroed, added to in LDS, then one global atomic per counter that is not zero
template <uint32_t N> __device__ __forceinline__ void counters_begin(uint32_t* s) { if (threadIdx.x < N) s[threadIdx.x] = 0u; __syncthreads(); }
template <uint32_t N> __device__ __forceinline__ void counters_end(const uint32_t* s, uint32_t* global)
{
    __syncthreads();
    if (threadIdx.x < N && s[threadIdx.x]) atomicAdd(&global[threadIdx.x], s[threadIdx.x]);
}

// A. one lane per primitive and turn
__global__ __launch_bounds__(kCoBlock) void coarsen_mark(ommCpuBakeResultDesc r, uint32_t* __restrict__ ref, CoarsenHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    uint32_t skipped = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kCoBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kCoBlock + threadIdx.x; i < r.indexCount; i += stride) {
        const int32_t e = index_entry(r.indexBuffer, (int)r.indexFormat, i);
        if (e < 0) { skipped += e < -4 ? 1u : 0u; continue; }
        bool ok = (uint32_t)e < r.descArrayCount;
        if (ok) ok = desc_ok(load_desc(r.descArray + e), r.arrayDataSize);
        if (ok) atomicOr(&ref[e], 1u); else skipped++;
    }
    if (skipped) atomicAdd(&s_n[0], skipped);
    counters_end<1>(s_n, &hdr->skipped);
}

// B. one lane per descriptor and one for the scans' closing element
__global__ __launch_bounds__(kCoBlock) void coarsen_prepare(ommCpuBakeResultDesc r, uint32_t maxLevel, const uint32_t* __restrict__ ref, unsigned long long* __restrict__ slot,
                                                            unsigned long long* __restrict__ units, unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask,
                                                            uint32_t* __restrict__ deepList, CoarsenHeader* __restrict__ hdr)
{
    const uint64_t d = (uint64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (d > r.descArrayCount) return;
    unsigned long long bytes = 0ull, n = 0ull;
    if (d < r.descArrayCount && ref[d]) {
        const BlockPlan p = plan_block(load_desc(r.descArray + d), maxLevel);
        bytes = coarsen_block_bytes(p.level - p.firstPass, p.bits);
        bytes = (bytes + kCoSlotAlign - 1u) & ~(unsigned long long)(kCoSlotAlign - 1u);
        n = p.level > kCoUnitLevel ? 1ull << (2u * (p.level - kCoUnitLevel)) : 1ull;
        if (p.deep) deepList[atomicAdd(&hdr->deepBlocks, 1u)] = (uint32_t)d;
        digest[d] = 0ull; umask[d] = 0xFu;
    }
    slot[d] = bytes; units[d] = n;
}

// ---- the reduction of one unit by one workgroup ----
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

typedef uint64_t CoVec __attribute__((vector_size(16), may_alias));

// src: the unit's first byte; unitLevel <= 8: the unit holds 4^unitLevel fields; r <= unitLevel levels are taken off.  Every thread of the
// workgroup calls this with the same arguments.  Reads are complete before the first write (src may be dst).
__device__ __forceinline__ void reduce_unit(const uint8_t* src, uint32_t unitLevel, uint32_t bits, uint32_t r, uint32_t mixedState, uint8_t* dst, uint64_t fieldBase,
                                            bool final, unsigned long long* digest, uint32_t* umask, uint64_t (*s_planes)[2], uint64_t* s_digest, uint32_t* s_umask)
{
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t fields = 1u << (2u * unitLevel);
    const uint32_t laneBytes = 32u * bits;
    const uint32_t unitBytes = (fields * bits + 7u) >> 3;
    const bool active = (t << 8) < fields;
    CoarsenPlanes P[4];
    {
        uint64_t w[8];
        #pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = 0ull;
        if (active) {
            const uint8_t* p = src + (size_t)t * laneBytes;
            const uint32_t left = unitBytes - t * laneBytes, n = left < laneBytes ? left : laneBytes;
            if (n == laneBytes && ((uintptr_t)p & 15u) == 0u) {
                const CoVec q0 = ((const CoVec*)p)[0], q1 = ((const CoVec*)p)[1];
                w[0] = q0[0]; w[1] = q0[1]; w[2] = q1[0]; w[3] = q1[1];
                if (bits == 2u) {
                    const CoVec q2 = ((const CoVec*)p)[2], q3 = ((const CoVec*)p)[3];
                    w[4] = q2[0]; w[5] = q2[1]; w[6] = q3[0]; w[7] = q3[1];
                }
            } else {   // a block at an odd address, or one smaller than a lane's share: byte by byte
                #pragma unroll
                for (int i = 0; i < 8; ++i)
                    for (uint32_t b = 0; b < 8u; ++b) { const uint32_t at = 8u * (uint32_t)i + b; if (at < n) w[i] |= (uint64_t)p[at] << (8u * b); }
            }
        }
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (bits == 2u) P[i] = coarsen_split(w[2 * i], w[2 * i + 1]);
            else { P[i].lo = w[i]; P[i].hi = 0ull; }
        }
    }
    __syncthreads();
    UnitOut o; o.dst = dst; o.fieldBase = fieldBase; o.outFields = fields >> (2u * r); o.bits = bits; o.digest = 0ull; o.umask = 0xFu;
    if (r == 0u) {
        if (active) {
            #pragma unroll
            for (int i = 0; i < 4; ++i) write_pair(o, P[i], 4u * t + (uint32_t)i);
        }
    } else {
        // in the lane: up to three levels on each of the four plane pairs, their results side by side, a fourth level on those
        const uint32_t n = r < 3u ? r : 3u, nf = 64u >> (2u * n);
        CoarsenPlanes cat; cat.lo = 0ull; cat.hi = 0ull;
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
            const CoarsenPlanes q = coarsen_reduce_planes(P[i], n, bits, mixedState);
            cat.lo |= q.lo << (nf * (uint32_t)i); cat.hi |= q.hi << (nf * (uint32_t)i);
        }
        if (r <= 3u) {
            // 64, 16 or 4 fields per lane: groups of 1, 4 or 16 lanes put theirs side by side with a butterfly of ORs
            const uint32_t n1 = 4u * nf, group = 64u / n1, sub = lane & (group - 1u);
            cat.lo <<= n1 * sub; cat.hi <<= n1 * sub;
            for (uint32_t d = 1; d < group; d <<= 1) { cat.lo |= shfl_xor_u64(cat.lo, (int)d); cat.hi |= shfl_xor_u64(cat.hi, (int)d); }
            if (sub == 0u) write_pair(o, cat, t / group);
        } else {
            cat = coarsen_reduce_planes(cat, 1u, bits, mixedState);
            // one field per lane: the wave's 64 by ballot
            CoarsenPlanes wv; wv.lo = __ballot((int)(cat.lo & 1ull)); wv.hi = __ballot((int)(cat.hi & 1ull));
            if (r == 4u) { if (lane == 0u) write_pair(o, wv, wave); }
            else {
                const uint32_t n2 = r - 4u < 3u ? r - 4u : 3u, nw = 64u >> (2u * n2);
                const CoarsenPlanes q = coarsen_reduce_planes(wv, n2, bits, mixedState);
                if (lane == 0u) { s_planes[wave][0] = q.lo; s_planes[wave][1] = q.hi; }
                __syncthreads();
                if (t == 0u) {
                    CoarsenPlanes all; all.lo = 0ull; all.hi = 0ull;
                    #pragma unroll
                    for (uint32_t w2 = 0; w2 < kCoWaves; ++w2) { all.lo |= s_planes[w2][0] << (nw * w2); all.hi |= s_planes[w2][1] << (nw * w2); }
                    if (r == 8u) all = coarsen_reduce_planes(all, 1u, bits, mixedState);
                    write_pair(o, all, 0u);
                }
            }
        }
    }
    if (final) {
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { o.digest += shfl_xor_u64(o.digest, d); o.umask &= (uint32_t)__shfl_xor((int)o.umask, d); }
        if (lane == 0u) { s_digest[wave] = o.digest; s_umask[wave] = o.umask; }
        __syncthreads();
        if (t == 0u) {
            unsigned long long dg = 0ull; uint32_t um = 0xFu;
            #pragma unroll
            for (uint32_t w2 = 0; w2 < kCoWaves; ++w2) { dg += s_digest[w2]; um &= s_umask[w2]; }
            if (dg) atomicAdd(digest, dg);
            if (um != 0xFu) atomicAnd(umask, um);
        }
    }
    __syncthreads();   // (the LDS words are the next unit's too)
}

// C. one unit per workgroup and turn
__global__ __launch_bounds__(kCoBlock) void coarsen_units(ommCpuBakeResultDesc r, uint32_t maxLevel, uint32_t mixedState, const unsigned long long* __restrict__ unitStart,
                                                          const unsigned long long* __restrict__ slotStart, uint8_t* __restrict__ staging,
                                                          unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask)
{
    __shared__ uint64_t s_planes[kCoWaves][2];
    __shared__ uint64_t s_digest[kCoWaves];
    __shared__ uint32_t s_umask[kCoWaves];
    const unsigned long long total = unitStart[r.descArrayCount];
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t d = owner_of_segment(unitStart, r.descArrayCount, u);
        const ommCpuOpacityMicromapDesc desc = load_desc(r.descArray + d);   // (has units, so a primitive selects it and it passed the bounds rule)
        const BlockPlan p = plan_block(desc, maxLevel);
        const uint64_t unit = u - unitStart[d];
        const uint32_t unitLevel = p.level < kCoUnitLevel ? p.level : kCoUnitLevel;
        const uint8_t* src = (const uint8_t*)r.arrayData + desc.offset + unit * (uint64_t)(kCoUnitFields / 8u * p.bits);
        reduce_unit(src, unitLevel, p.bits, p.firstPass, mixedState, staging + slotStart[d], unit * (uint64_t)(kCoUnitFields >> (2u * p.firstPass)),
                    !p.deep, digest + d, umask + d, s_planes, s_digest, s_umask);
    }
}

// C'. blocks above level 8 that lose more than five levels: the rest, in place in the staging slot (at most 4^7 fields: one unit)
__global__ __launch_bounds__(kCoBlock) void coarsen_deep(ommCpuBakeResultDesc r, uint32_t maxLevel, uint32_t mixedState, const uint32_t* __restrict__ deepList,
                                                         const unsigned long long* __restrict__ slotStart, uint8_t* __restrict__ staging,
                                                         unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask)
{
    __shared__ uint64_t s_planes[kCoWaves][2];
    __shared__ uint64_t s_digest[kCoWaves];
    __shared__ uint32_t s_umask[kCoWaves];
    const uint32_t d = deepList[blockIdx.x];
    const BlockPlan p = plan_block(load_desc(r.descArray + d), maxLevel);
    uint8_t* at = staging + slotStart[d];
    const uint32_t level = p.level - p.firstPass;
    reduce_unit(at, level, p.bits, level - p.target, mixedState, at, 0ull, true, digest + d, umask + d, s_planes, s_digest, s_umask);
}

// D1. one lane per descriptor: the counts of the info, the special index of a uniform block, every other block into the hash table
__global__ __launch_bounds__(kCoBlock) void coarsen_classify(ommCpuBakeResultDesc r, uint32_t maxLevel, uint32_t flags, const uint32_t* __restrict__ ref,
                                                             const unsigned long long* __restrict__ digest, const uint32_t* __restrict__ umask, int32_t* __restrict__ special,
                                                             HashTable table, CoarsenHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[3];
    counters_begin<3>(s_n);
    const uint64_t d = (uint64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (d < r.descArrayCount) {
        int32_t sp = 0;
        if (ref[d]) {
            const BlockPlan p = plan_block(load_desc(r.descArray + d), maxLevel);
            const uint32_t um = umask[d];
            atomicAdd(&s_n[0], 1u);
            if (p.level > p.target) atomicAdd(&s_n[1], 1u);
            if (um) atomicAdd(&s_n[2], 1u);
            if (um && !(flags & ommxCoarsenFlags_DisableSpecialIndices)) sp = -(int32_t)(__ffs((int)um));   // bit s -> -(s + 1)
            else if (!(flags & ommxCoarsenFlags_DisableDuplicateDetection)) hash_put_min(table, block_key(digest[d], p.target, p.bits), (uint32_t)d);
        }
        special[d] = sp;
    }
    counters_end<3>(s_n, &hdr->referenced);
}

__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint64_t n)
{
    if (n >= 8u) {   // (slots are 16-byte aligned)
        const uint64_t* x = (const uint64_t*)a; const uint64_t* y = (const uint64_t*)b;
        for (uint64_t i = 0; i < n / 8u; ++i) if (x[i] != y[i]) return false;
        return true;
    }
    for (uint64_t i = 0; i < n; ++i) if (a[i] != b[i]) return false;
    return true;
}

// D2. one lane per descriptor: its representative, and the sort key of a block that will be emitted
__global__ __launch_bounds__(kCoBlock) void coarsen_resolve(ommCpuBakeResultDesc r, uint32_t maxLevel, uint32_t flags, const uint32_t* __restrict__ ref,
                                                            const unsigned long long* __restrict__ digest, const int32_t* __restrict__ special, HashTable table,
                                                            const unsigned long long* __restrict__ slotStart, const uint8_t* __restrict__ staging,
                                                            uint32_t* __restrict__ rep, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, CoarsenHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1 + kCoarsenSizeClasses];
    counters_begin<1 + kCoarsenSizeClasses>(s_n);
    const uint64_t d = (uint64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (d < r.descArrayCount) {
        uint32_t key = kCoNoClass, leader = (uint32_t)d;
        if (ref[d] && special[d] == 0) {
            const BlockPlan p = plan_block(load_desc(r.descArray + d), maxLevel);
            const uint64_t bytes = coarsen_block_bytes(p.target, p.bits);
            if (!(flags & ommxCoarsenFlags_DisableDuplicateDetection)) {
                const uint32_t c = hash_get(table, block_key(digest[d], p.target, p.bits), (uint32_t)d);
                if (c < d) {
                    const BlockPlan q = plan_block(load_desc(r.descArray + c), maxLevel);
                    if (q.target == p.target && q.bits == p.bits && same_bytes(staging + slotStart[d], staging + slotStart[c], bytes)) leader = c;
                }
            }
            if (leader == d) {
                const uint32_t cls = 63u - (uint32_t)__clzll((long long)bytes);
                key = kCoarsenSizeClasses - 1u - cls;
                atomicAdd(&s_n[1u + cls], 1u);
            } else atomicAdd(&s_n[0], 1u);
        }
        rep[d] = leader; keys[d] = key; vals[d] = (uint32_t)d;
    }
    counters_end<1 + kCoarsenSizeClasses>(s_n, &hdr->duplicate);
}

// F1. one lane per output descriptor
__global__ __launch_bounds__(kCoBlock) void coarsen_descs(ommCpuBakeResultDesc r, uint32_t maxLevel, uint32_t count, CoarsenPlace place, const uint32_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ vals, const unsigned long long* __restrict__ slotStart, const uint8_t* __restrict__ staging,
                                                          uint8_t* __restrict__ outArray, ommCpuOpacityMicromapDesc* __restrict__ outDescs, uint32_t* __restrict__ newIndex,
                                                          CoarsenHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[kCoHist];
    counters_begin<kCoHist>(s_n);
    const uint64_t j = (uint64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (j < count) {
        const uint32_t d = vals[j], cls = kCoarsenSizeClasses - 1u - keys[j];
        const BlockPlan p = plan_block(load_desc(r.descArray + d), maxLevel);
        const uint64_t off = place.base[cls] + ((uint64_t)(j - place.first[cls]) << cls);
        ommCpuOpacityMicromapDesc o; o.offset = (uint32_t)off; o.subdivisionLevel = (uint16_t)p.target; o.format = (uint16_t)p.bits;
        outDescs[j] = o;
        newIndex[d] = (uint32_t)j;
        atomicAdd(&s_n[2u * p.target + p.bits - 1u], 1u);
        if (cls < 4u) { const uint8_t* s = staging + slotStart[d]; for (uint32_t b = 0; b < (1u << cls); ++b) outArray[off + b] = s[b]; }
    }
    counters_end<kCoHist>(s_n, hdr->arrayHist);
}

// F2. the blocks of 16 bytes and more -- a prefix of the output: 16 bytes per lane and turn
__global__ __launch_bounds__(kCoBlock) void coarsen_gather(uint64_t bigBytes, CoarsenPlace place, const uint32_t* __restrict__ vals, const unsigned long long* __restrict__ slotStart,
                                                           const uint8_t* __restrict__ staging, uint8_t* __restrict__ outArray)
{
    const uint64_t stride = (uint64_t)gridDim.x * kCoBlock * 16u;
    for (uint64_t pos = ((uint64_t)blockIdx.x * kCoBlock + threadIdx.x) * 16u; pos < bigBytes; pos += stride) {
        uint32_t cls = kCoarsenSizeClasses - 1u;
        while (cls > 4u && pos >= place.base[cls] + ((uint64_t)place.count[cls] << cls)) --cls;
        const uint64_t rel = pos - place.base[cls];
        const uint32_t d = vals[place.first[cls] + (uint32_t)(rel >> cls)];
        *(CoVec*)(outArray + pos) = *(const CoVec*)(staging + slotStart[d] + (rel & ((1ull << cls) - 1ull)));
    }
}

// F3. one lane per primitive and turn
__global__ __launch_bounds__(kCoBlock) void coarsen_index(ommCpuBakeResultDesc r, uint32_t maxLevel, const uint32_t* __restrict__ ref, const int32_t* __restrict__ special,
                                                          const uint32_t* __restrict__ rep, const uint32_t* __restrict__ newIndex, void* __restrict__ outIndex,
                                                          CoarsenHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[kCoHist];
    counters_begin<kCoHist>(s_n);
    const uint64_t stride = (uint64_t)gridDim.x * kCoBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kCoBlock + threadIdx.x; i < r.indexCount; i += stride) {
        const int32_t e = index_entry(r.indexBuffer, (int)r.indexFormat, i);
        int32_t v = -4;
        if (e < 0) v = e >= -4 ? e : -4;
        else if ((uint32_t)e < r.descArrayCount && ref[e]) {   // (marked: it passed the bounds rule)
            v = special[e];
            if (v == 0) {
                const BlockPlan p = plan_block(load_desc(r.descArray + e), maxLevel);
                v = (int32_t)newIndex[rep[e]];
                atomicAdd(&s_n[2u * p.target + p.bits - 1u], 1u);
            }
        }
        index_store(outIndex, (int)r.indexFormat, i, v);
    }
    counters_end<kCoHist>(s_n, hdr->indexHist);
}

namespace {
struct CoarsenLayout {
    size_t header, ref, slot, units, digest, umask, deepList, special, rep, keys, vals, keysSorted, valsSorted, newIndex, table, temp, bytes;
    size_t tempBytes; uint32_t slots;
};
CoarsenLayout coarsen_layout(const CoarsenArgs& a)
{
    CoarsenLayout L; size_t o = 0;
    const size_t D = a.result.descArrayCount;
    const auto take = [&o](size_t bytes) { const size_t at = o; o += pad256(bytes); return at; };
    L.header = take(sizeof(CoarsenHeader));
    L.ref = take(4 * D);
    L.slot = take(8 * (D + 1)); L.units = take(8 * (D + 1));
    L.digest = take(8 * D); L.umask = take(4 * D); L.deepList = take(4 * D); L.special = take(4 * D); L.rep = take(4 * D);
    L.keys = take(4 * D); L.vals = take(4 * D); L.keysSorted = take(4 * D); L.valsSorted = take(4 * D); L.newIndex = take(4 * D);
    L.slots = (a.flags & ommxCoarsenFlags_DisableDuplicateDetection) || !D ? 0u : hash_table_slots(D);
    L.table = take(L.slots ? hash_table_bytes(L.slots) : 0);
    size_t scanBytes = 0, sortBytes = 0;
    if (D) {
        (void)rocprim::exclusive_scan(nullptr, scanBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, D + 1, rocprim::plus<unsigned long long>());
        (void)rocprim::radix_sort_pairs(nullptr, sortBytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, D, 0u, 5u);
    }
    L.tempBytes = scanBytes > sortBytes ? scanBytes : sortBytes;
    L.temp = take(L.tempBytes);
    L.bytes = o;
    return L;
}
uint32_t strided_grid(uint64_t items)
{
    const uint64_t blocks = (items + kCoBlock - 1u) / kCoBlock;
    return (uint32_t)(blocks < kCoMaxGrid ? (blocks ? blocks : 1u) : kCoMaxGrid);
}
uint32_t per_item_grid(uint64_t items) { return (uint32_t)((items + kCoBlock - 1u) / kCoBlock); }
CoarsenPlace place_of(const CoarsenCounts& c)
{
    CoarsenPlace p; uint64_t at = 0; uint32_t first = 0;
    for (int cls = (int)kCoarsenSizeClasses - 1; cls >= 0; --cls) {
        p.base[cls] = at; p.first[cls] = first; p.count[cls] = c.classCount[cls];
        at += (uint64_t)c.classCount[cls] << cls; first += c.classCount[cls];
    }
    return p;
}
} // namespace

size_t coarsen_head_bytes(const CoarsenArgs& a) { return coarsen_layout(a).bytes; }

#define COARSEN_CHECK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

hipError_t coarsen_plan(const CoarsenArgs& a, void* head, CoarsenPlan* out, hipStream_t stream)
{
    const CoarsenLayout L = coarsen_layout(a);
    uint8_t* base = (uint8_t*)head;
    const ommCpuBakeResultDesc& r = a.result;
    const uint32_t D = r.descArrayCount;
    CoarsenHeader* hdr = (CoarsenHeader*)(base + L.header);
    uint32_t* ref = (uint32_t*)(base + L.ref);
    unsigned long long* slot = (unsigned long long*)(base + L.slot);
    unsigned long long* units = (unsigned long long*)(base + L.units);
    COARSEN_CHECK(hipMemsetAsync(hdr, 0, sizeof(CoarsenHeader), stream));
    if (D) COARSEN_CHECK(hipMemsetAsync(ref, 0, 4 * (size_t)D, stream));
    coarsen_mark<<<strided_grid(r.indexCount), kCoBlock, 0, stream>>>(r, ref, hdr);
    COARSEN_CHECK(hipGetLastError());
    unsigned long long stagingBytes = 0;
    if (D) {
        coarsen_prepare<<<per_item_grid((uint64_t)D + 1u), kCoBlock, 0, stream>>>(r, a.maxLevel, ref, slot, units, (unsigned long long*)(base + L.digest),
                                                                                 (uint32_t*)(base + L.umask), (uint32_t*)(base + L.deepList), hdr);
        COARSEN_CHECK(hipGetLastError());
        size_t tb = L.tempBytes;   // (in place: every element is read before it is written)
        COARSEN_CHECK(rocprim::exclusive_scan(base + L.temp, tb, slot, slot, 0ull, (size_t)D + 1, rocprim::plus<unsigned long long>(), stream));
        tb = L.tempBytes;
        COARSEN_CHECK(rocprim::exclusive_scan(base + L.temp, tb, units, units, 0ull, (size_t)D + 1, rocprim::plus<unsigned long long>(), stream));
        COARSEN_CHECK(hipMemcpyAsync(&stagingBytes, slot + D, sizeof stagingBytes, hipMemcpyDeviceToHost, stream));
    }
    CoarsenHeader h;
    COARSEN_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    COARSEN_CHECK(hipStreamSynchronize(stream));
    out->stagingBytes = stagingBytes; out->skipped = h.skipped; out->deepBlocks = h.deepBlocks;
    return hipSuccess;
}

hipError_t coarsen_reduce(const CoarsenArgs& a, void* head, void* staging, const CoarsenPlan& plan, CoarsenCounts* out, hipStream_t stream)
{
    const CoarsenLayout L = coarsen_layout(a);
    uint8_t* base = (uint8_t*)head;
    const ommCpuBakeResultDesc& r = a.result;
    const uint32_t D = r.descArrayCount;
    CoarsenHeader* hdr = (CoarsenHeader*)(base + L.header);
    memset(out, 0, sizeof *out);
    if (D) {
        const uint32_t* ref = (const uint32_t*)(base + L.ref);
        const unsigned long long* slot = (const unsigned long long*)(base + L.slot);
        const unsigned long long* units = (const unsigned long long*)(base + L.units);
        unsigned long long* digest = (unsigned long long*)(base + L.digest);
        uint32_t* umask = (uint32_t*)(base + L.umask);
        int32_t* special = (int32_t*)(base + L.special);
        uint32_t *keys = (uint32_t*)(base + L.keys), *vals = (uint32_t*)(base + L.vals);
        HashTable table; memset(&table, 0, sizeof table);
        if (L.slots) {
            table = hash_table_at(base + L.table, L.slots);
            COARSEN_CHECK(hipMemsetAsync(base + L.table, 0xFF, hash_table_bytes(L.slots), stream));
        }
        // no read-back to size the grid: blocks that do not overlap have at most this many units, and the kernel strides over any more
        const uint64_t bound = (uint64_t)r.arrayDataSize / (kCoUnitFields / 8u) + D;
        coarsen_units<<<(uint32_t)(bound < kCoMaxGrid ? bound : kCoMaxGrid), kCoBlock, 0, stream>>>(r, a.maxLevel, a.mixedState, units, slot, (uint8_t*)staging, digest, umask);
        COARSEN_CHECK(hipGetLastError());
        if (plan.deepBlocks) {
            coarsen_deep<<<plan.deepBlocks, kCoBlock, 0, stream>>>(r, a.maxLevel, a.mixedState, (const uint32_t*)(base + L.deepList), slot, (uint8_t*)staging, digest, umask);
            COARSEN_CHECK(hipGetLastError());
        }
        coarsen_classify<<<per_item_grid(D), kCoBlock, 0, stream>>>(r, a.maxLevel, a.flags, ref, digest, umask, special, table, hdr);
        COARSEN_CHECK(hipGetLastError());
        coarsen_resolve<<<per_item_grid(D), kCoBlock, 0, stream>>>(r, a.maxLevel, a.flags, ref, digest, special, table, slot, (const uint8_t*)staging,
                                                                   (uint32_t*)(base + L.rep), keys, vals, hdr);
        COARSEN_CHECK(hipGetLastError());
        size_t tb = L.tempBytes;   // stable: equal size classes keep their source order
        COARSEN_CHECK(rocprim::radix_sort_pairs(base + L.temp, tb, keys, (uint32_t*)(base + L.keysSorted), vals, (uint32_t*)(base + L.valsSorted), (size_t)D, 0u, 5u, stream));
    }
    CoarsenHeader h;
    COARSEN_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    COARSEN_CHECK(hipStreamSynchronize(stream));
    out->referenced = h.referenced; out->coarsened = h.coarsened; out->uniform = h.uniform; out->duplicate = h.duplicate;
    for (uint32_t c = 0; c < kCoarsenSizeClasses; ++c) { out->classCount[c] = h.classCount[c]; out->descCount += h.classCount[c]; out->arrayBytes += (uint64_t)h.classCount[c] << c; }
    return hipSuccess;
}

hipError_t coarsen_emit(const CoarsenArgs& a, void* head, const void* staging, const CoarsenCounts& counts, const CoarsenOutputs& o, hipStream_t stream)
{
    const CoarsenLayout L = coarsen_layout(a);
    uint8_t* base = (uint8_t*)head;
    const ommCpuBakeResultDesc& r = a.result;
    CoarsenHeader* hdr = (CoarsenHeader*)(base + L.header);
    const unsigned long long* slot = (const unsigned long long*)(base + L.slot);
    const uint32_t* valsSorted = (const uint32_t*)(base + L.valsSorted);
    uint32_t* newIndex = (uint32_t*)(base + L.newIndex);
    const CoarsenPlace place = place_of(counts);
    if (counts.descCount) {
        coarsen_descs<<<per_item_grid(counts.descCount), kCoBlock, 0, stream>>>(r, a.maxLevel, counts.descCount, place, (const uint32_t*)(base + L.keysSorted), valsSorted, slot,
                                                                                 (const uint8_t*)staging, o.arrayData, o.descs, newIndex, hdr);
        COARSEN_CHECK(hipGetLastError());
        const uint64_t big = place.base[3];   // the blocks of 16 bytes and more end where the 8-byte blocks begin
        if (big) {
            coarsen_gather<<<strided_grid(big / 16u), kCoBlock, 0, stream>>>(big, place, valsSorted, slot, (const uint8_t*)staging, o.arrayData);
            COARSEN_CHECK(hipGetLastError());
        }
    }
    coarsen_index<<<strided_grid(r.indexCount), kCoBlock, 0, stream>>>(r, a.maxLevel, (const uint32_t*)(base + L.ref), (const int32_t*)(base + L.special),
                                                                       (const uint32_t*)(base + L.rep), newIndex, o.index, hdr);
    COARSEN_CHECK(hipGetLastError());
    CoarsenHeader h;
    COARSEN_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    COARSEN_CHECK(hipStreamSynchronize(stream));
    memcpy(o.hist, h.arrayHist, sizeof h.arrayHist);
    memcpy(o.hist + kCoHist, h.indexHist, sizeof h.indexHist);
    return hipSuccess;
}

} // namespace ommx
