// coarsen_kernels.hip -- ommxCoarsenMicromap and ommxCoarsenMicromapLevels (include/omm_mi355x_ext.h has the definition): the blocks of a device-resident result reduced to a
// maximum subdivision level, then the tail of a bake on what is left (rebuild_kernels.hip) -- uniform blocks to special indices, equal blocks
// merged, blocks ordered by size, descriptors and histograms rebuilt -- and the index buffer.
//
//   coarsen_mark      the index buffer once: which descriptors are selected (and pass the bounds rule), how many primitives are skipped
//   coarsen_prepare   per selected descriptor: the size of its slot in the staging arena, its number of work units, its place in the deep list,
//                     and its word for the tail (the level and format of its output block)
//   coarsen_units     THE pass over arrayData: one workgroup per unit of 4^8 micro-triangles; 256 of them per lane as bit planes in registers
//                     (coarsen_reduce.h), four levels in the lane, up to three across the lanes of the wave by ballot, one across the waves in
//                     LDS.  A block above level 8 has several units whose outputs must be whole words, so such a block is reduced by at most five
//                     levels here and, if it has further to go, once more by coarsen_deep (the rule is associative).  The writers of the output
//                     words also sum a digest of them and AND the "all fields equal s" masks (result_words.h): one integer atomic each per workgroup.
//   (the tail)        items are source descriptors, so representatives within a size class are ordered by source index ascending
//   coarsen_index     the index buffer, in the source's index format
//
// All counters are integers and every output byte has one writer, so the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <string.h>
#include "coarsen_kernels.h"
#include "coarsen_reduce.h"
#include "result_read.h"
#include "result_words.h"
#include "wave_search.h"

namespace ommx {
namespace {

constexpr uint32_t kCoBlock = kRebuildBlock;
constexpr uint32_t kCoWaves = kCoBlock / 64;
constexpr uint32_t kCoUnitLevel = 8;              // a workgroup's unit: 4^8 micro-triangles, 256 per lane
constexpr uint32_t kCoUnitFields = 1u << (2 * kCoUnitLevel);
constexpr uint32_t kCoFirstPassLevels = 5;        // of a block with several units: every unit then still writes 64 fields or more

struct CoarsenHeader { uint32_t skipped, deepBlocks, referenced, coarsened; };

// what becomes of a source block
struct BlockPlan {
    uint32_t level, bits, target, firstPass;   // firstPass: levels taken off by coarsen_units
    bool deep;                                 // coarsen_deep takes off the rest
};
// blockLevels: a cap per source descriptor (ommxCoarsenMicromapLevels), or null
__device__ __forceinline__ BlockPlan plan_block(const ommCpuOpacityMicromapDesc d, uint32_t maxLevel, const uint8_t* __restrict__ blockLevels, uint64_t index)
{
    BlockPlan p;
    p.level = d.subdivisionLevel; p.bits = d.format;
    p.target = p.level < maxLevel ? p.level : maxLevel;
    if (blockLevels) { const uint32_t own = blockLevels[index]; p.target = own < p.target ? own : p.target; }
    const uint32_t k = p.level - p.target;
    const bool several = p.level > kCoUnitLevel;
    p.firstPass = several && k > kCoFirstPassLevels ? kCoFirstPassLevels : k;
    p.deep = p.firstPass != k;
    return p;
}

// A. one lane per primitive and turn
__global__ __launch_bounds__(kCoBlock) void coarsen_mark(ommCpuBakeResultDesc r, uint32_t* __restrict__ ref, CoarsenHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const ResultView s = view_of(r);
    uint32_t skipped = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kCoBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kCoBlock + threadIdx.x; i < s.indexCount; i += stride) skipped += mark_selected(s, i, ref);
    if (skipped) atomicAdd(&s_n[0], skipped);
    counters_end<1>(s_n, &hdr->skipped);
}

// B. one lane per descriptor and one for the scans' closing element
__global__ __launch_bounds__(kCoBlock) void coarsen_prepare(ommCpuBakeResultDesc r, uint32_t maxLevel, const uint8_t* __restrict__ blockLevels, const uint32_t* __restrict__ ref, uint32_t* __restrict__ item,
                                                            unsigned long long* __restrict__ slot, unsigned long long* __restrict__ units,
                                                            unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask, uint32_t* __restrict__ deepList,
                                                            CoarsenHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[2];
    counters_begin<2>(s_n);
    const uint64_t d = (uint64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (d <= r.descArrayCount) {
        unsigned long long bytes = 0ull, n = 0ull;
        if (d < r.descArrayCount) {
            uint32_t w = 0u;
            if (ref[d]) {
                const BlockPlan p = plan_block(load_desc(r.descArray + d), maxLevel, blockLevels, d);
                bytes = block_bytes(p.level - p.firstPass, p.bits);
                bytes = (bytes + kRebuildSlotAlign - 1u) & ~(unsigned long long)(kRebuildSlotAlign - 1u);
                n = p.level > kCoUnitLevel ? 1ull << (2u * (p.level - kCoUnitLevel)) : 1ull;
                if (p.deep) deepList[atomicAdd(&hdr->deepBlocks, 1u)] = (uint32_t)d;
                digest[d] = 0ull; umask[d] = 0xFu;
                w = item_word(p.target, p.bits);
                atomicAdd(&s_n[0], 1u);
                if (p.level > p.target) atomicAdd(&s_n[1], 1u);
            }
            item[d] = w;
        }
        slot[d] = bytes; units[d] = n;
    }
    counters_end<2>(s_n, &hdr->referenced);
}

// ---- the reduction of one unit by one workgroup ----
// src: the unit's first byte; unitLevel <= 8: the unit holds 4^unitLevel fields; r <= unitLevel levels are taken off.  Every thread of the
// workgroup calls this with the same arguments.  Reads are complete before the first write (src may be dst).
__device__ __forceinline__ void reduce_unit(const uint8_t* src, uint32_t unitLevel, uint32_t bits, uint32_t r, uint32_t mixedState, uint8_t* dst, uint64_t fieldBase,
                                            bool final, unsigned long long* digest, uint32_t* umask, uint64_t (*s_planes)[2], uint64_t* s_digest, uint32_t* s_umask)
{
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t fields = 1u << (2u * unitLevel);
    const bool active = (t << 8) < fields;
    CoarsenPlanes P[4];
    if (active) load_fields(src, bits, t << 8, fields < 256u ? fields : 256u, P);
    else {
        #pragma unroll
        for (int i = 0; i < 4; ++i) { P[i].lo = 0ull; P[i].hi = 0ull; }
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
    if (final) unit_close<kCoWaves>(o, s_digest, s_umask, digest, umask);
    __syncthreads();   // (the LDS words are the next unit's too)
}

// C. one unit per workgroup and turn
__global__ __launch_bounds__(kCoBlock) void coarsen_units(ommCpuBakeResultDesc r, uint32_t maxLevel, const uint8_t* __restrict__ blockLevels, uint32_t mixedState, const unsigned long long* __restrict__ unitStart,
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
        const BlockPlan p = plan_block(desc, maxLevel, blockLevels, d);
        const uint64_t unit = u - unitStart[d];
        const uint32_t unitLevel = p.level < kCoUnitLevel ? p.level : kCoUnitLevel;
        const uint8_t* src = (const uint8_t*)r.arrayData + desc.offset + unit * (uint64_t)(kCoUnitFields / 8u * p.bits);
        reduce_unit(src, unitLevel, p.bits, p.firstPass, mixedState, staging + slotStart[d], unit * (uint64_t)(kCoUnitFields >> (2u * p.firstPass)),
                    !p.deep, digest + d, umask + d, s_planes, s_digest, s_umask);
    }
}

// C'. blocks above level 8 that lose more than five levels: the rest, in place in the staging slot (at most 4^7 fields: one unit)
__global__ __launch_bounds__(kCoBlock) void coarsen_deep(ommCpuBakeResultDesc r, uint32_t maxLevel, const uint8_t* __restrict__ blockLevels, uint32_t mixedState, const uint32_t* __restrict__ deepList,
                                                         const unsigned long long* __restrict__ slotStart, uint8_t* __restrict__ staging,
                                                         unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask)
{
    __shared__ uint64_t s_planes[kCoWaves][2];
    __shared__ uint64_t s_digest[kCoWaves];
    __shared__ uint32_t s_umask[kCoWaves];
    const uint32_t d = deepList[blockIdx.x];
    const BlockPlan p = plan_block(load_desc(r.descArray + d), maxLevel, blockLevels, d);
    uint8_t* at = staging + slotStart[d];
    const uint32_t level = p.level - p.firstPass;
    reduce_unit(at, level, p.bits, level - p.target, mixedState, at, 0ull, true, digest + d, umask + d, s_planes, s_digest, s_umask);
}

// F3. one lane per primitive and turn
__global__ __launch_bounds__(kCoBlock) void coarsen_index(ommCpuBakeResultDesc r, const uint32_t* __restrict__ item, RebuildTables tail, void* __restrict__ outIndex)
{
    __shared__ uint32_t s_n[kRebuildHist];
    counters_begin<kRebuildHist>(s_n);
    const ResultView s = view_of(r);
    const uint64_t stride = (uint64_t)gridDim.x * kCoBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kCoBlock + threadIdx.x; i < s.indexCount; i += stride)
        index_store(outIndex, s.indexFormat, i, index_back(s, i, item, 0u, tail, s_n));
    counters_end<kRebuildHist>(s_n, tail.indexHist);
}

// the call's scratch: the header and the marks behind it (ONE memset clears both), the deep list, the arrays of the tail
struct CoarsenScratch { CoarsenHeader* hdr; uint32_t *ref, *deepList; TailArrays t; size_t bytes; };
CoarsenScratch coarsen_scratch(const CoarsenArgs& a, void* base)
{
    CoarsenScratch s; CarveCursor c{ (uintptr_t)base };
    const size_t D = a.result.descArrayCount;
    s.hdr = c.take<CoarsenHeader>(1); s.ref = c.take<uint32_t>(D);
    s.deepList = c.take<uint32_t>(D);
    s.t = rebuild_arrays(c, a.result.descArrayCount, a.flags);
    s.bytes = (size_t)(c.at - (uintptr_t)base);
    return s;
}

} // namespace

size_t coarsen_head_bytes(const CoarsenArgs& a) { return coarsen_scratch(a, nullptr).bytes; }

hipError_t coarsen_plan(const CoarsenArgs& a, void* head, CoarsenPlan* out, hipStream_t stream)
{
    const CoarsenScratch s = coarsen_scratch(a, head);
    const ommCpuBakeResultDesc& r = a.result;
    const uint32_t D = r.descArrayCount;
    REBUILD_CHECK(hipMemsetAsync(s.hdr, 0, (size_t)((uint8_t*)s.ref - (uint8_t*)s.hdr) + 4 * (size_t)D, stream));   // (the header and the marks behind it)
    coarsen_mark<<<strided_grid(r.indexCount), kCoBlock, 0, stream>>>(r, s.ref, s.hdr);
    REBUILD_CHECK(hipGetLastError());
    unsigned long long stagingBytes = 0;
    if (D) {
        coarsen_prepare<<<per_item_grid((uint64_t)D + 1u), kCoBlock, 0, stream>>>(r, a.maxLevel, a.blockLevels, s.ref, s.t.item, s.t.slotStart, s.t.units, s.t.digest, s.t.umask, s.deepList, s.hdr);
        REBUILD_CHECK(hipGetLastError());
        REBUILD_CHECK(rebuild_scan(s.t, D, &stagingBytes, nullptr, stream));   // (the units' sum is not read back: coarsen_reduce sizes its grid from a bound)
    }
    CoarsenHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&h, s.hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    out->stagingBytes = stagingBytes; out->skipped = h.skipped; out->deepBlocks = h.deepBlocks; out->referenced = h.referenced; out->coarsened = h.coarsened;
    return hipSuccess;
}

hipError_t coarsen_reduce(const CoarsenArgs& a, void* head, void* staging, const CoarsenPlan& plan, RebuildCounts* out, hipStream_t stream)
{
    const CoarsenScratch s = coarsen_scratch(a, head);
    const ommCpuBakeResultDesc& r = a.result;
    const uint32_t D = r.descArrayCount;
    if (D) {
        // no read-back to size the grid: blocks that do not overlap have at most this many units, and the kernel strides over any more
        const uint64_t bound = (uint64_t)r.arrayDataSize / (kCoUnitFields / 8u) + D;
        coarsen_units<<<(uint32_t)(bound < kRebuildMaxGrid ? bound : kRebuildMaxGrid), kCoBlock, 0, stream>>>(r, a.maxLevel, a.blockLevels, a.mixedState, s.t.units, s.t.slotStart, (uint8_t*)staging,
                                                                                                            s.t.digest, s.t.umask);
        REBUILD_CHECK(hipGetLastError());
        if (plan.deepBlocks) {
            coarsen_deep<<<plan.deepBlocks, kCoBlock, 0, stream>>>(r, a.maxLevel, a.blockLevels, a.mixedState, s.deepList, s.t.slotStart, (uint8_t*)staging, s.t.digest, s.t.umask);
            REBUILD_CHECK(hipGetLastError());
        }
    }
    return rebuild_count(tail_inputs(s.t, D, a.flags, staging), out, stream);
}

hipError_t coarsen_emit(const CoarsenArgs& a, void* head, const void* staging, const RebuildCounts& counts, const RebuildOutputs& o, hipStream_t stream)
{
    const RebuildInputs in = tail_inputs(coarsen_scratch(a, head).t, a.result.descArrayCount, a.flags, staging);
    REBUILD_CHECK(rebuild_emit(in, counts, o.arrayData, o.descs, stream));
    coarsen_index<<<strided_grid(a.result.indexCount), kCoBlock, 0, stream>>>(a.result, in.item, rebuild_tables(in), o.index);
    REBUILD_CHECK(hipGetLastError());
    return rebuild_histograms(in, o.hist, stream);
}

} // namespace ommx
