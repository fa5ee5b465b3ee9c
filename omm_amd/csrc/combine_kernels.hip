// combine_kernels.hip -- ommxCombineMicromaps (include/omm_mi355x_ext.h has the definition): K device-resident results over the same primitives
// joined into one conservative result, then the tail of a bake on the joined blocks (rebuild_kernels.hip) and the index buffer.
//
//   combine_entries   one lane per primitive: the K entries under the bounds rule; a primitive with a failing entry is skipped, one with only
//                     special entries is answered here, every other one puts the hash of its tuple into the table (hash_build.h), lowest index wins
//   combine_leaders   one lane per primitive: the lowest primitive with the same tuple (the entries confirm); a scan of the leaders numbers the tuples
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
#include <rocprim/rocprim.hpp>
#include "combine_kernels.h"
#include "combine_expand.h"
#include "result_read.h"
#include "result_words.h"
#include "hash_build.h"
#include "bake_host.h"   // pad256
#include "wave_search.h"

namespace ommx {
namespace {

constexpr uint32_t kCbBlock = kRebuildBlock;
constexpr uint32_t kCbWaves = kCbBlock / 64;
constexpr uint32_t kCbUnitLevel = 8;               // a workgroup's unit: 4^8 output micro-triangles, 256 per lane
constexpr uint32_t kCbUnitFields = 1u << (2 * kCbUnitLevel);
constexpr uint32_t kCbLaneFields = kCbUnitFields / kCbBlock;

struct CombineHeader { uint32_t skipped, refined; };

// A normalised entry, 8 bytes: a block is offset | level << 32 | fieldBits << 40; a special index is state << 48 (fieldBits 0)
__device__ __forceinline__ uint64_t norm_block(const ommCpuOpacityMicromapDesc d) { return (uint64_t)d.offset | ((uint64_t)d.subdivisionLevel << 32) | ((uint64_t)d.format << 40); }
__device__ __forceinline__ uint64_t norm_special(uint32_t state) { return (uint64_t)state << 48; }
__device__ __forceinline__ uint32_t norm_bits(uint64_t n) { return (uint32_t)(n >> 40) & 3u; }
__device__ __forceinline__ uint32_t norm_level(uint64_t n) { return (uint32_t)(n >> 32) & 0xFFu; }
__device__ __forceinline__ uint32_t norm_state(uint64_t n) { return (uint32_t)(n >> 48) & 3u; }

// entry e of a source -> false: it fails the rule; otherwise its normalised form
__device__ __forceinline__ bool normalise(const ResultView& s, int32_t e, uint64_t* out)
{
    if (e < 0) { *out = norm_special((uint32_t)(-(e + 1))); return e >= -4; }
    if ((uint32_t)e >= s.descCount) return false;
    const ommCpuOpacityMicromapDesc d = load_desc(s.descs + e);
    *out = norm_block(d);
    return desc_ok(d, s.arrayDataSize);
}
__device__ __forceinline__ uint64_t tuple_hash(uint64_t h, int32_t e) { return mix64(h ^ (uint64_t)(uint32_t)e) + 0x9E3779B97F4A7C15ull; }

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
            const ResultView& s = a.source[k];
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
                const ResultView& s = a.source[k];
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
    REBUILD_CHECK(hipMemsetAsync(hdr, 0, sizeof(CombineHeader), stream));
    REBUILD_CHECK(hipMemsetAsync(base + L.table, 0xFF, hash_table_bytes(L.slots), stream));
    combine_entries<<<strided_grid(N), kCbBlock, 0, stream>>>(a, table, code, key, hdr);
    REBUILD_CHECK(hipGetLastError());
    combine_leaders<<<per_item_grid((uint64_t)N + 1u), kCbBlock, 0, stream>>>(a, table, code, key, (uint32_t*)(base + L.leader), tupleStart);
    REBUILD_CHECK(hipGetLastError());
    size_t tb = L.tempBytes;   // (in place: every element is read before it is written)
    REBUILD_CHECK(rocprim::exclusive_scan(base + L.temp, tb, tupleStart, tupleStart, 0u, (size_t)N + 1, rocprim::plus<uint32_t>(), stream));
    uint32_t tuples = 0;
    CombineHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&tuples, tupleStart + N, sizeof tuples, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    out->tuples = tuples; out->skipped = h.skipped;
    return hipSuccess;
}

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
