// combine_kernels.hip -- ommxCombineMicromaps (include/omm_mi355x_ext.h has the definition): K device-resident results over the same primitives
// joined into one conservative result, then the tail of a bake on the joined blocks (rebuild_kernels.hip) and the index buffer.
//
//   combine_entries, combine_leaders   the front that finds the distinct tuples (combine_front.h, shared with ommxCompareMicromaps)
//   combine_prepare   one lane per leader: the K normalised entries of its tuple, the level T, the staging slot, the number of work units, and the
//                     tuple's word for the tail (T and the output format)
//   combine_units     THE pass over the sources' arrayData: one workgroup per unit of 4^8 output micro-triangles, 256 per lane as four plane pairs.
//                     Per source the lane reads the bytes that cover its micro-triangles at the source's own level, repeats them down to T
//                     (combine_expand.h) and adds them to the join; then it writes whole output words, sums their digest and ANDs their
//                     uniformity masks (result_words.h): one integer atomic each per workgroup
//   (the tail)        items are tuples, numbered by their lowest primitive, so representatives within a size class are ordered by that primitive
//   combine_index     the index buffer, 32-bit entries, through code / leader / tupleStart
//
// All counters are integers and every output byte has one writer.
#include <hip/hip_runtime.h>
#include <string.h>
#include "combine_kernels.h"
#include "combine_front.h"
#include "combine_expand.h"
#include "wave_search.h"

namespace ommx {
namespace {

// C. one lane per primitive and one for the scans' closing element; the leaders work
__global__ __launch_bounds__(kCbBlock) void combine_prepare(CombineArgs a, uint32_t tuples, const int32_t* __restrict__ code, const uint32_t* __restrict__ leader,
                                                            const uint32_t* __restrict__ tupleStart, unsigned long long* __restrict__ norm, uint32_t* __restrict__ item,
                                                            unsigned long long* __restrict__ slot, unsigned long long* __restrict__ units,
                                                            unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask, CombineHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const uint64_t i = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x;
    if (i == a.indexCount) { slot[tuples] = 0ull; units[tuples] = 0ull; }
    if (i < a.indexCount && code[i] == 0 && leader[i] == (uint32_t)i) {
        const uint32_t t = tupleStart[i];
        uint32_t top = 0u, low = kResultMaxLevel;
        for (uint32_t k = 0; k < a.sourceCount; ++k) {
            const ResultView& s = a.source[k];
            uint64_t n = 0ull;
            (void)normalise(s, index_entry(s.index, s.indexFormat, i), &n);   // (it passed in combine_entries)
            norm[(uint64_t)t * a.sourceCount + k] = n;
            if (norm_bits(n)) { const uint32_t l = norm_level(n); top = l > top ? l : top; low = l < low ? l : low; }
        }
        unsigned long long bytes = block_bytes(top, a.format);
        bytes = (bytes + kRebuildSlotAlign - 1u) & ~(unsigned long long)(kRebuildSlotAlign - 1u);
        item[t] = item_word(top, a.format); slot[t] = bytes;
        units[t] = top > kCbUnitLevel ? 1ull << (2u * (top - kCbUnitLevel)) : 1ull;
        digest[t] = 0ull; umask[t] = 0xFu;
        if (low < top) atomicAdd(&s_n[0], 1u);
    }
    counters_end<1>(s_n, &hdr->refined);
}

// D. the join of one unit per workgroup and turn
__global__ __launch_bounds__(kCbBlock) void combine_units(CombineArgs a, uint32_t tuples, const unsigned long long* __restrict__ norm, const uint32_t* __restrict__ item,
                                                          const unsigned long long* __restrict__ unitStart, const unsigned long long* __restrict__ slotStart,
                                                          uint8_t* __restrict__ staging, unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask)
{
    __shared__ uint64_t s_digest[kCbWaves];
    __shared__ uint32_t s_umask[kCbWaves];
    const uint32_t t = threadIdx.x;
    const unsigned long long total = unitStart[tuples];
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t tup = owner_of_segment(unitStart, tuples, u);
        const uint32_t T = item_level(item[tup]);
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
        unit_close<kCbWaves>(o, s_digest, s_umask, digest + tup, umask + tup);
        __syncthreads();   // (the LDS words are the next unit's too)
    }
}

// F3. one lane per primitive and turn
__global__ __launch_bounds__(kCbBlock) void combine_index(uint32_t indexCount, const int32_t* __restrict__ code, const uint32_t* __restrict__ leader,
                                                          const uint32_t* __restrict__ tupleStart, const uint32_t* __restrict__ item, RebuildTables tail,
                                                          int32_t* __restrict__ outIndex)
{
    __shared__ uint32_t s_n[kRebuildHist];
    counters_begin<kRebuildHist>(s_n);
    const uint64_t stride = (uint64_t)gridDim.x * kCbBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x; i < indexCount; i += stride) {
        int32_t v = code[i];
        if (v == 0) {
            const uint32_t t = tupleStart[leader[i]];
            v = index_back(tail, t, item[t], s_n);
        }
        outIndex[i] = v;
    }
    counters_end<kRebuildHist>(s_n, tail.indexHist);   // (without tuples nothing was counted and nothing is added)
}

// the scratch per tuple: the normalised entries, the arrays of the tail
struct TupleScratch { unsigned long long* norm; TailArrays t; size_t bytes; };
TupleScratch tuple_scratch(const CombineArgs& a, uint32_t tuples, void* base)
{
    TupleScratch s; CarveCursor c{ (uintptr_t)base };
    s.norm = c.take<unsigned long long>((size_t)tuples * a.sourceCount);
    s.t = rebuild_arrays(c, tuples, 0u);
    s.bytes = (size_t)(c.at - (uintptr_t)base);
    return s;
}

} // namespace

size_t combine_head_bytes(const CombineArgs& a) { return head_layout(a).bytes; }
size_t combine_tuple_bytes(const CombineArgs& a, uint32_t tuples) { return tuple_scratch(a, tuples, nullptr).bytes; }

hipError_t combine_tuples(const CombineArgs& a, void* head, CombineTuples* out, hipStream_t stream) { return front_tuples(a, head, out, stream); }

hipError_t combine_plan(const CombineArgs& a, void* head, void* perTuple, const CombineTuples& t, CombinePlan* out, hipStream_t stream)
{
    const HeadLayout L = head_layout(a);
    const TupleScratch U = tuple_scratch(a, t.tuples, perTuple);
    uint8_t* base = (uint8_t*)head;
    const uint32_t N = a.indexCount, M = t.tuples;
    CombineHeader* hdr = (CombineHeader*)(base + L.header);
    combine_prepare<<<per_item_grid((uint64_t)N + 1u), kCbBlock, 0, stream>>>(a, M, (const int32_t*)(base + L.code), (const uint32_t*)(base + L.leader),
                                                                             (const uint32_t*)(base + L.tupleStart), U.norm, U.t.item, U.t.slotStart, U.t.units, U.t.digest, U.t.umask, hdr);
    REBUILD_CHECK(hipGetLastError());
    unsigned long long stagingBytes = 0, totalUnits = 0;
    REBUILD_CHECK(rebuild_scan(U.t, M, &stagingBytes, &totalUnits, stream));
    CombineHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    out->stagingBytes = stagingBytes; out->units = totalUnits; out->refined = h.refined;
    return hipSuccess;
}

hipError_t combine_join(const CombineArgs& a, void* perTuple, void* staging, const CombineTuples& t, const CombinePlan& plan, RebuildCounts* out, hipStream_t stream)
{
    const TupleScratch U = tuple_scratch(a, t.tuples, perTuple);
    combine_units<<<(uint32_t)(plan.units < kRebuildMaxGrid ? plan.units : kRebuildMaxGrid), kCbBlock, 0, stream>>>(a, t.tuples, U.norm, U.t.item, U.t.units, U.t.slotStart, (uint8_t*)staging,
                                                                                                                   U.t.digest, U.t.umask);
    REBUILD_CHECK(hipGetLastError());
    return rebuild_count(tail_inputs(U.t, t.tuples, 0u, staging), out, stream);
}

hipError_t combine_emit(const CombineArgs& a, void* head, void* perTuple, const void* staging, const CombineTuples& t, const RebuildCounts& counts, const RebuildOutputs& o,
                        hipStream_t stream)
{
    const HeadLayout L = head_layout(a);
    uint8_t* base = (uint8_t*)head;
    RebuildInputs in; memset(&in, 0, sizeof in);
    RebuildTables tail; memset(&tail, 0, sizeof tail);
    if (t.tuples) {
        in = tail_inputs(tuple_scratch(a, t.tuples, perTuple).t, t.tuples, 0u, staging);
        tail = rebuild_tables(in);
        REBUILD_CHECK(rebuild_emit(in, counts, o.arrayData, o.descs, stream));
    }
    combine_index<<<strided_grid(a.indexCount), kCbBlock, 0, stream>>>(a.indexCount, (const int32_t*)(base + L.code), (const uint32_t*)(base + L.leader),
                                                                       (const uint32_t*)(base + L.tupleStart), in.item, tail, (int32_t*)o.index);
    REBUILD_CHECK(hipGetLastError());
    return t.tuples ? rebuild_histograms(in, o.hist, stream) : hipStreamSynchronize(stream);   // (hist: the caller's zeros stand)
}

} // namespace ommx
