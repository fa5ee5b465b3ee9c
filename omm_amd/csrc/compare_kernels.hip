// compare_kernels.hip -- ommxCompareMicromaps (include/omm_mi355x_ext.h has the definition): two device-resident results over the same primitives
// read side by side, a 4 x 4 confusion matrix [stateA][stateB] per primitive, and exact integer totals.  Nothing is written but counts.
//
//   combine_entries, combine_leaders   the front of ommxCombineMicromaps with two sources (combine_front.h): the distinct pairs of entries, numbered by
//                     their lowest primitive.  A pair that loses its hash slot is its own leader and is streamed on its own: no answer depends on it
//   compare_prepare   one lane per primitive: the references of its pair (one atomic per distinct pair of a wave); the leaders write the two
//                     normalised entries, the level T, the pair's lowest primitive and its number of work units
//   compare_units     THE pass over both arrayData: one workgroup per unit of 4^8 level-T micro-triangles, 256 per lane as four plane pairs per side.
//                     Each side is read at its own level (load_fields) and repeated down to T (combine_expand.h); sixteen AND + popcount sums per
//                     plane pair (compare_count.h) go to sixteen 32-bit accumulators per lane; per wave by shuffle, across waves through LDS, then
//                     one integer atomic per non-zero cell and unit (a pair of one unit stores)
//   compare_relations one lane per pair: the relation byte of its matrix
//   compare_totals    one lane per pair: matrix * references * 4^(12 - T) into the totals, the references into the primitive counts, atomicMin of
//                     the lowest primitive of a pair with CONFLICT -- in LDS, then one atomic per counter and workgroup
//   compare_scatter   four lanes per primitive: relation, level and the matrix (one 16-byte store per lane) to the caller's arrays; a primitive with
//                     two special entries is answered here without a pair, a skipped one gets 0x80, 0xFF and zeros
//
// All counters are integers: any order of the atomics gives the same bytes.
#include <hip/hip_runtime.h>
#include <string.h>
#include "compare_kernels.h"
#include "compare_count.h"
#include "combine_front.h"
#include "combine_expand.h"
#include "wave_search.h"

namespace ommx {
namespace {

constexpr uint32_t kCmpMaxLevel = 12;
constexpr uint32_t kCmpUnitGrid = 4096;   // compare_units strides over the units: their number stays on the device

typedef uint32_t CellRow __attribute__((vector_size(16), may_alias));   // four cells at a 16-byte aligned address, as one load or store

struct PairScratch {
    unsigned long long* norm;         // [2 * pairs] the normalised entries of A and B
    uint32_t *level, *first, *refs;   // [pairs] T; the lowest primitive; the primitives with this pair
    uint8_t* relation;                // [pairs]
    unsigned long long* unitStart;    // [pairs + 1] units, then (scanned in place) their offsets
    uint32_t* matrix;                 // [pairs][16]
    uint8_t* temp; size_t tempBytes;  // of the scan
    size_t bytes;
};
PairScratch pair_scratch(uint32_t pairs, void* base)
{
    PairScratch s; CarveCursor c{ (uintptr_t)base };
    const size_t M = pairs;
    s.norm = c.take<unsigned long long>(2 * M);
    s.level = c.take<uint32_t>(M); s.first = c.take<uint32_t>(M); s.refs = c.take<uint32_t>(M);
    s.relation = c.take<uint8_t>(M);
    s.unitStart = c.take<unsigned long long>(M + 1);
    s.matrix = c.take<uint32_t>(16 * M);
    s.tempBytes = 0;
    (void)rocprim::exclusive_scan(nullptr, s.tempBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, M + 1, rocprim::plus<unsigned long long>());
    s.temp = c.take<uint8_t>(s.tempBytes);
    s.bytes = (size_t)(c.at - (uintptr_t)base);
    return s;
}

CombineArgs front_args(const CompareArgs& a)
{
    CombineArgs f; memset(&f, 0, sizeof f);
    f.source[0] = a.a; f.source[1] = a.b;
    f.sourceCount = 2; f.indexCount = a.indexCount;
    f.format = 2; f.mixedState = 3;   // (of the front's answer for two special entries, which is not used here)
    return f;
}
__device__ __forceinline__ const ResultView& side(const CompareArgs& a, uint32_t k) { return k ? a.b : a.a; }

// C. one lane per primitive and one for the scan's closing element
__global__ __launch_bounds__(kCbBlock) void compare_prepare(CompareArgs a, uint32_t pairs, const int32_t* __restrict__ code, const uint32_t* __restrict__ leader,
                                                            const uint32_t* __restrict__ tupleStart, unsigned long long* __restrict__ norm, uint32_t* __restrict__ level,
                                                            uint32_t* __restrict__ first, uint32_t* __restrict__ refs, unsigned long long* __restrict__ units,
                                                            CompareTotals* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const uint64_t i = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    if (i == a.indexCount) units[pairs] = 0ull;
    const bool has = i < a.indexCount && code[i] == 0;
    const uint32_t lead = has ? leader[i] : 0u, t = has ? tupleStart[lead] : 0u;
    // the references: one atomic per distinct pair among the wave's lanes
    for (uint64_t pending = __ballot(has); pending; ) {
        const int from = __ffsll((unsigned long long)pending) - 1;
        const uint32_t tf = (uint32_t)__shfl((int)t, from);
        const uint64_t same = __ballot(has && t == tf);
        if ((int)lane == from) atomicAdd(&refs[tf], (uint32_t)__popcll(same));
        pending &= ~same;
    }
    if (has && lead == (uint32_t)i) {
        uint32_t top = 0u, low = kCmpMaxLevel, blocks = 0u;
        for (uint32_t k = 0; k < 2u; ++k) {
            const ResultView& s = side(a, k);
            uint64_t n = 0ull;
            (void)normalise(s, index_entry(s.index, s.indexFormat, i), &n);   // (it passed in combine_entries)
            norm[2ull * t + k] = n;
            if (norm_bits(n)) { const uint32_t l = norm_level(n); top = l > top ? l : top; low = l < low ? l : low; blocks++; }
        }
        level[t] = top; first[t] = (uint32_t)i;
        units[t] = top > kCbUnitLevel ? 1ull << (2u * (top - kCbUnitLevel)) : 1ull;
        if (low < top || blocks < 2u) atomicAdd(&s_n[0], 1u);
    }
    counters_end<1>(s_n, &hdr->refined);
}

// 256 (or all) fields of one side of a pair at level T as four plane pairs: a special entry is broadcast, a block is read at its own level and
// repeated down to T
__device__ __forceinline__ void side_planes(const uint8_t* arrayData, uint64_t n, uint32_t T, uint32_t laneFields, uint32_t firstField, CoarsenPlanes Q[4])
{
    const uint32_t bits = norm_bits(n);
    if (bits == 0u) {
        const CoarsenPlanes q = combine_broadcast(norm_state(n));
        #pragma unroll
        for (int j = 0; j < 4; ++j) Q[j] = q;
        return;
    }
    const uint32_t down = T - norm_level(n), shift = 2u * down;   // shift <= 24
    const uint32_t count = (laneFields >> shift) ? laneFields >> shift : 1u;
    CoarsenPlanes P[4];
    load_fields(arrayData + (uint32_t)n, bits, firstField >> shift, count, P);
    if (down == 0u) {
        #pragma unroll
        for (int j = 0; j < 4; ++j) Q[j] = P[j];
        return;
    }
    // plane pair j covers the source fields [j * 64 >> shift, (j + 1) * 64 >> shift) of the lane's share: 16, 4, one, or the one
    const uint32_t rep = down < 3u ? down : 3u, per = down < 4u ? 64u >> shift : 0u;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
        CoarsenPlanes q; q.lo = P[0].lo >> (per * (uint32_t)j); q.hi = P[0].hi >> (per * (uint32_t)j);
        Q[j] = combine_repeat_planes(q, rep);
    }
}

// D. one unit per workgroup and turn
__global__ __launch_bounds__(kCbBlock) void compare_units(CompareArgs a, uint32_t pairs, const unsigned long long* __restrict__ norm, const uint32_t* __restrict__ level,
                                                          const unsigned long long* __restrict__ unitStart, uint32_t* __restrict__ matrix)
{
    __shared__ uint32_t s_acc[kCbWaves][16];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const unsigned long long total = unitStart[pairs];
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t pair = owner_of_segment(unitStart, pairs, u);
        const uint32_t T = level[pair];
        const unsigned long long start = unitStart[pair];
        const uint32_t unit = (uint32_t)(u - start);
        const bool single = unitStart[pair + 1u] - start == 1ull;
        const uint32_t unitFields = T < kCbUnitLevel ? 1u << (2u * T) : kCbUnitFields;
        const bool active = t * kCbLaneFields < unitFields;
        const uint32_t laneFields = unitFields < kCbLaneFields ? unitFields : kCbLaneFields;   // (of an active lane)
        const uint32_t firstField = unit * kCbUnitFields + t * kCbLaneFields;                   // of the pair, at level T
        uint32_t acc[16];
        #pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = 0u;
        if (active) {
            CoarsenPlanes A[4], B[4];
            side_planes(a.a.arrayData, norm[2ull * pair], T, laneFields, firstField, A);
            side_planes(a.b.arrayData, norm[2ull * pair + 1u], T, laneFields, firstField, B);
            compare_count_add(A[0], B[0], compare_valid_mask(laneFields), a.force2, acc);   // (a lane's share below 64 fields is in the first plane pair)
            if (laneFields == kCbLaneFields) {
                #pragma unroll
                for (int j = 1; j < 4; ++j) compare_count_add(A[j], B[j], ~0ull, a.force2, acc);
            }
        }
        #pragma unroll
        for (int c = 0; c < 16; ++c) {
            #pragma unroll
            for (int d = 32; d >= 1; d >>= 1) acc[c] += (uint32_t)__shfl_xor((int)acc[c], d);
        }
        if (lane == 0u) {
            #pragma unroll
            for (int c = 0; c < 16; ++c) s_acc[wave][c] = acc[c];
        }
        __syncthreads();
        if (t < 16u) {
            uint32_t n = 0u;
            #pragma unroll
            for (uint32_t w = 0; w < kCbWaves; ++w) n += s_acc[w][t];
            if (single) matrix[16ull * pair + t] = n;
            else if (n) atomicAdd(&matrix[16ull * pair + t], n);
        }
        __syncthreads();   // (the LDS words are the next unit's too)
    }
}

// E. one lane per pair
__global__ __launch_bounds__(kCbBlock) void compare_relations(uint32_t pairs, const uint32_t* __restrict__ matrix, uint8_t* __restrict__ relation)
{
    const uint32_t p = blockIdx.x * kCbBlock + threadIdx.x;
    if (p >= pairs) return;
    uint32_t m[16];
    #pragma unroll
    for (int q = 0; q < 4; ++q) { const CellRow r = ((const CellRow*)matrix)[4ull * p + q]; m[4 * q] = r[0]; m[4 * q + 1] = r[1]; m[4 * q + 2] = r[2]; m[4 * q + 3] = r[3]; }
    relation[p] = (uint8_t)compare_relation(m);
}

// F. one lane per pair
__global__ __launch_bounds__(kCbBlock) void compare_totals(uint32_t pairs, const uint32_t* __restrict__ matrix, const uint8_t* __restrict__ relation,
                                                           const uint32_t* __restrict__ level, const uint32_t* __restrict__ first, const uint32_t* __restrict__ refs,
                                                           CompareTotals* __restrict__ hdr)
{
    __shared__ unsigned long long s_total[16];
    __shared__ uint32_t s_n[5], s_first;
    if (threadIdx.x < 16u) s_total[threadIdx.x] = 0ull;
    if (threadIdx.x < 5u) s_n[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) s_first = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t p = blockIdx.x * kCbBlock + threadIdx.x;
    if (p < pairs) {
        const uint32_t r = relation[p], n = refs[p];
        const unsigned long long weight = (unsigned long long)n << (2u * (kCmpMaxLevel - level[p]));   // <= 2^32 * 2^24 with the cell
        #pragma unroll
        for (int q = 0; q < 4; ++q) {
            const CellRow row = ((const CellRow*)matrix)[4ull * p + q];
            #pragma unroll
            for (int k = 0; k < 4; ++k)
                if (row[k]) atomicAdd(&s_total[4 * q + k], row[k] * weight);
        }
        if (r == 0u) atomicAdd(&s_n[0], n);
        #pragma unroll
        for (uint32_t b = 0; b < 4u; ++b)
            if (r & (1u << b)) atomicAdd(&s_n[1u + b], n);
        if (r & kRelationConflict) atomicMin(&s_first, first[p]);
    }
    __syncthreads();
    if (threadIdx.x < 16u && s_total[threadIdx.x]) atomicAdd((unsigned long long*)&hdr->totals[threadIdx.x], s_total[threadIdx.x]);
    if (threadIdx.x < 5u && s_n[threadIdx.x]) atomicAdd(&hdr->identical + threadIdx.x, s_n[threadIdx.x]);
    if (threadIdx.x == 0u && s_first != 0xFFFFFFFFu) atomicMin(&hdr->firstConflict, s_first);
}

// G. four lanes per primitive and turn: lane q has the row [q][0..3] of the matrix
__global__ __launch_bounds__(kCbBlock) void compare_scatter(CompareArgs a, const int32_t* __restrict__ code, const uint32_t* __restrict__ leader,
                                                            const uint32_t* __restrict__ tupleStart, const uint32_t* __restrict__ matrix,
                                                            const uint8_t* __restrict__ relation, const uint32_t* __restrict__ level, CompareTotals* __restrict__ hdr)
{
    __shared__ uint32_t s_cells[16], s_first;
    if (threadIdx.x < 16u) s_cells[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) s_first = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kCbBlock, lanes = 4ull * a.indexCount;
    for (uint64_t g = (uint64_t)blockIdx.x * kCbBlock + threadIdx.x; g < lanes; g += stride) {
        const uint64_t i = g >> 2;
        const uint32_t q = (uint32_t)g & 3u;
        uint32_t rel = kRelationSkipped, lvl = 0xFFu;
        CellRow row = { 0u, 0u, 0u, 0u };
        if (code[i] == 0) {
            const uint32_t p = tupleStart[leader[i]];
            rel = relation[p]; lvl = level[p];
            row = ((const CellRow*)matrix)[4ull * p + q];
        } else {
            const int32_t ea = index_entry(a.a.index, a.a.indexFormat, i), eb = index_entry(a.b.index, a.b.indexFormat, i);
            if (ea < 0 && ea >= -4 && eb < 0 && eb >= -4) {   // two special entries: one field at level 0
                uint32_t sa = (uint32_t)(-(ea + 1)), sb = (uint32_t)(-(eb + 1));
                if (a.force2) { sa &= 1u; sb &= 1u; }
                rel = compare_cell_relation(sa, sb); lvl = 0u;
                if (sa == q) row[sb] = 1u;
                if (q == 0u) {
                    atomicAdd(&s_cells[4u * sa + sb], 1u);
                    if (rel & kRelationConflict) atomicMin(&s_first, (uint32_t)i);
                }
            }
        }
        if (q == 0u) {
            if (a.relations) a.relations[i] = (uint8_t)rel;
            if (a.levels) a.levels[i] = (uint8_t)lvl;
        }
        if (a.confusion) ((CellRow*)a.confusion)[g] = row;
    }
    __syncthreads();
    if (threadIdx.x < 16u && s_cells[threadIdx.x]) atomicAdd(&hdr->specialCells[threadIdx.x], s_cells[threadIdx.x]);
    if (threadIdx.x == 0u && s_first != 0xFFFFFFFFu) atomicMin(&hdr->firstConflict, s_first);
}

} // namespace

size_t compare_head_bytes(const CompareArgs& a) { return head_layout(front_args(a)).bytes + pad256(sizeof(CompareTotals)); }
size_t compare_pair_bytes(uint32_t pairs) { return pair_scratch(pairs, nullptr).bytes; }

hipError_t compare_pairs(const CompareArgs& a, void* head, CombineTuples* out, hipStream_t stream) { return front_tuples(front_args(a), head, out, stream); }

hipError_t compare_count(const CompareArgs& a, void* head, void* perPair, const CombineTuples& t, CompareTotals* out, hipStream_t stream)
{
    const CombineArgs f = front_args(a);
    const HeadLayout L = head_layout(f);
    uint8_t* base = (uint8_t*)head;
    const uint32_t N = a.indexCount, M = t.tuples;
    const int32_t* code = (const int32_t*)(base + L.code);
    const uint32_t *leader = (const uint32_t*)(base + L.leader), *tupleStart = (const uint32_t*)(base + L.tupleStart);
    CompareTotals* hdr = (CompareTotals*)(base + L.bytes);
    REBUILD_CHECK(hipMemsetAsync(hdr, 0, sizeof(CompareTotals), stream));
    REBUILD_CHECK(hipMemsetAsync(&hdr->firstConflict, 0xFF, sizeof hdr->firstConflict, stream));
    PairScratch U; memset(&U, 0, sizeof U);
    if (M) {
        U = pair_scratch(M, perPair);
        REBUILD_CHECK(hipMemsetAsync(U.refs, 0, sizeof(uint32_t) * (size_t)M, stream));
        REBUILD_CHECK(hipMemsetAsync(U.matrix, 0, sizeof(uint32_t) * 16 * (size_t)M, stream));
        compare_prepare<<<per_item_grid((uint64_t)N + 1u), kCbBlock, 0, stream>>>(a, M, code, leader, tupleStart, U.norm, U.level, U.first, U.refs, U.unitStart, hdr);
        REBUILD_CHECK(hipGetLastError());
        size_t tb = U.tempBytes;   // (in place: every element is read before it is written)
        REBUILD_CHECK(rocprim::exclusive_scan(U.temp, tb, U.unitStart, U.unitStart, 0ull, (size_t)M + 1, rocprim::plus<unsigned long long>(), stream));
        const uint64_t most = (uint64_t)M << (2u * (kCmpMaxLevel - kCbUnitLevel));   // units, at most
        compare_units<<<(uint32_t)(most < kCmpUnitGrid ? most : kCmpUnitGrid), kCbBlock, 0, stream>>>(a, M, U.norm, U.level, U.unitStart, U.matrix);
        REBUILD_CHECK(hipGetLastError());
        compare_relations<<<per_item_grid(M), kCbBlock, 0, stream>>>(M, U.matrix, U.relation);
        REBUILD_CHECK(hipGetLastError());
        compare_totals<<<per_item_grid(M), kCbBlock, 0, stream>>>(M, U.matrix, U.relation, U.level, U.first, U.refs, hdr);
        REBUILD_CHECK(hipGetLastError());
    }
    compare_scatter<<<strided_grid(4ull * N), kCbBlock, 0, stream>>>(a, code, leader, tupleStart, U.matrix, U.relation, U.level, hdr);
    REBUILD_CHECK(hipGetLastError());
    REBUILD_CHECK(hipMemcpyAsync(out, hdr, sizeof *out, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

} // namespace ommx
