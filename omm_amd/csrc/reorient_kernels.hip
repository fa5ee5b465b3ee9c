// reorient_kernels.hip -- ommxReorientMicromap (include/omm_mi355x_ext.h has the definition): a result for the same primitives with their vertices
// re-ordered.  The blocks the primitives select are written, fields permuted, into aligned staging slots; then the tail of a bake runs on them
// (rebuild_kernels.hip) and the index buffer is written.  The phases are those of gather_kernels.hip.
//
//   reorient_mark     one lane per primitive: its orientation byte, the selection rule (result_read.h); the (descriptor, orientation) pair is marked, a
//                     primitive that fails the rule or whose byte is above 5 is counted
//   reorient_prepare  one lane per item (6e + o; e alone when the call has one orientation for every primitive): for a marked one its word for the
//                     tail (level and format, unchanged), the address of its block, the size of its staging slot and its number of work units
//   reorient_units    THE permutation: one workgroup per unit of 16 KiB of one output block and turn.  A lane takes a tile of 64 output fields -- one
//                     word of a 2-state block, one 16-byte vector of a 4-state block: the transducer of reorient_map.h over the digits above the tile
//                     gives the source tile and the tile's state (as many steps in every lane as the block has digits above a tile), the source
//                     tile is read with the address arithmetic of gather_copy.h, its sixteen nibbles / bytes are placed through the tables of the
//                     state in LDS, and the word(s) are stored whole.  Orientation 0 is the gather's copy (gather_unit.h); a block below a tile is
//                     one lane's, field by field.  Digest and uniformity mask as in result_words.h.
//   (the tail)        items are (descriptor, orientation) pairs in lexicographic order
//   reorient_index    one lane per primitive: the index buffer, 32-bit entries
//
// All counters are integers and every output byte has one writer, so the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <string.h>
#include "reorient_kernels.h"
#include "reorient_map.h"
#include "gather_unit.h"
#include "result_read.h"
#include "result_words.h"
#include "wave_search.h"

namespace ommx {
namespace {

constexpr uint32_t kRoBlock = kRebuildBlock;
constexpr uint32_t kRoWaves = kRoBlock / 64;

struct ReorientHeader { uint32_t skipped, referenced, reoriented; };

// how the items of a call are numbered: (e, o) -> 6e + o, or e when every primitive has the call's one orientation
struct ItemRule {
    const uint8_t* orientations; uint32_t orientation;
    __device__ __forceinline__ uint32_t of_primitive(uint64_t p) const { return orientations ? orientations[p] : orientation; }
    __device__ __forceinline__ uint64_t item(uint32_t e, uint32_t o) const { return orientations ? 6ull * e + o : e; }
    __device__ __forceinline__ uint32_t descriptor(uint64_t d) const { return (uint32_t)(orientations ? d / 6u : d); }
    __device__ __forceinline__ uint32_t of_item(uint64_t d) const { return orientations ? (uint32_t)(d % 6u) : orientation; }
};

// A. one lane per primitive and turn
__global__ __launch_bounds__(kRoBlock) void reorient_mark(ResultView src, ItemRule rule, uint32_t* __restrict__ ref, ReorientHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    uint32_t skipped = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kRoBlock;
    for (uint64_t p = (uint64_t)blockIdx.x * kRoBlock + threadIdx.x; p < src.indexCount; p += stride) {
        const uint32_t o = rule.of_primitive(p);
        uint32_t skip = 1u;                                        // (a byte above 5: nothing is read through the primitive's descriptor)
        if (o <= 5u) {
            const int32_t e = select_entry(src, p);
            if (e >= 0) atomicOr(&ref[rule.item((uint32_t)e, o)], 1u);
            skip = e == kSkipped ? 1u : 0u;
        }
        skipped += skip;
    }
    if (skipped) atomicAdd(&s_n[0], skipped);
    counters_end<1>(s_n, &hdr->skipped);
}

// B. one lane per item and one for the scans' closing element
__global__ __launch_bounds__(kRoBlock) void reorient_prepare(ResultView src, ItemRule rule, uint32_t items, const uint32_t* __restrict__ ref, uint32_t* __restrict__ item,
                                                             unsigned long long* __restrict__ slot, unsigned long long* __restrict__ units,
                                                             unsigned long long* __restrict__ srcAddr, unsigned long long* __restrict__ digest,
                                                             uint32_t* __restrict__ umask, ReorientHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[2];
    counters_begin<2>(s_n);
    const uint64_t d = (uint64_t)blockIdx.x * kRoBlock + threadIdx.x;
    if (d <= items) {
        unsigned long long bytes = 0ull, n = 0ull;
        if (d < items) {
            uint32_t w = 0u;
            if (ref[d]) {
                const ommCpuOpacityMicromapDesc desc = load_desc(src.descs + rule.descriptor(d));   // (marked: it passed the bounds rule)
                bytes = block_bytes(desc.subdivisionLevel, desc.format);
                n = unit_count(bytes);
                srcAddr[d] = (unsigned long long)(uintptr_t)(src.arrayData + desc.offset);
                bytes = (bytes + kRebuildSlotAlign - 1u) & ~(unsigned long long)(kRebuildSlotAlign - 1u);
                digest[d] = 0ull; umask[d] = 0xFu;
                w = item_word(desc.subdivisionLevel, desc.format);
                atomicAdd(&s_n[0], 1u);
                if (rule.of_item(d) != 0u) atomicAdd(&s_n[1], 1u);
            }
            item[d] = w;
        }
        slot[d] = bytes; units[d] = n;
    }
    counters_end<2>(s_n, &hdr->referenced);   // (referenced, reoriented: neighbours in the header)
}

// C. one unit per workgroup and turn
__global__ __launch_bounds__(kRoBlock) void reorient_units(ItemRule rule, uint32_t items, const uint32_t* __restrict__ item, const unsigned long long* __restrict__ srcAddr,
                                                           const unsigned long long* __restrict__ unitStart, const unsigned long long* __restrict__ slotStart,
                                                           uint8_t* __restrict__ staging, unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask)
{
    __shared__ ReorientTables s_tables;
    __shared__ uint64_t s_digest[kRoWaves];
    __shared__ uint32_t s_umask[kRoWaves];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < kReorientTableEntries; i += kRoBlock) reorient_tables_fill(&s_tables, i);
    __syncthreads();
    const unsigned long long total = unitStart[items];
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t d = owner_of_segment(unitStart, items, u);
        const uint32_t w = item[d], level = item_level(w), bits = item_bits(w), orientation = rule.of_item(d);
        const uint8_t* block = (const uint8_t*)(uintptr_t)srcAddr[d];
        const uint64_t unit = u - unitStart[d];
        UnitOut o; o.dst = staging + slotStart[d]; o.fieldBase = 0ull; o.outFields = 0u; o.bits = bits; o.digest = 0ull; o.umask = 0xFu;
        if (orientation == 0u) {
            copy_unit<kRoBlock>(block, level, bits, unit, o);
        } else if (level < kReorientTileDepth) {                  // 1, 2 or 4 bytes
            if (t == 0u) {
                const uint32_t bytes = (uint32_t)block_bytes(level, bits), used = bits << (2u * level);
                const uint64_t word = reorient_small(gather_small(block, bytes, level, bits), level, bits, orientation);
                for (uint32_t b = 0; b < bytes; ++b) o.dst[b] = (uint8_t)(word >> (8u * b));
                o.digest = word_digest(word, 0u); o.umask = coarsen_word_uniform(word, used, bits);
            }
        } else {
            const uint64_t bytes = block_bytes(level, bits);
            const uint32_t digits = level - kReorientTileDepth;   // above a tile: the same in every lane
            const uint32_t tiles = 1u << (2u * digits), perUnit = kUnitBytes / (8u * bits);
            const uint32_t first = (uint32_t)unit * perUnit, count = tiles < perUnit ? tiles : perUnit;
            for (uint32_t v = t; v < count; v += kRoBlock) {
                const uint32_t tile = first + v;
                uint32_t state = orientation;
                const uint32_t from = reorient_walk(tile, digits, &state);
                const GatherWords x = reorient_source_tile(block, bytes, bits, from);
                if (bits == 2u) {
                    const GatherWords y = reorient_tile4(&s_tables, state, x);
                    WordsVec out; out[0] = y.w0; out[1] = y.w1;
                    ((WordsVec*)o.dst)[tile] = out;
                    const uint64_t word = 2ull * tile;
                    o.digest += word_digest(y.w0, word) + word_digest(y.w1, word + 1u);
                    o.umask &= coarsen_word_uniform(y.w0, 64u, 2u) & coarsen_word_uniform(y.w1, 64u, 2u);
                } else {
                    const uint64_t y = reorient_tile2(&s_tables, state, x.w0);
                    ((uint64_t*)o.dst)[tile] = y;
                    o.digest += word_digest(y, tile);
                    o.umask &= coarsen_word_uniform(y, 64u, 1u);
                }
            }
        }
        unit_close<kRoWaves>(o, s_digest, s_umask, digest + d, umask + d);
        __syncthreads();   // (the LDS words are the next unit's too)
    }
}

// F3. one lane per primitive and turn
__global__ __launch_bounds__(kRoBlock) void reorient_index(ResultView src, ItemRule rule, const uint32_t* __restrict__ item, RebuildTables tail, int32_t* __restrict__ outIndex)
{
    __shared__ uint32_t s_n[kRebuildHist];
    counters_begin<kRebuildHist>(s_n);
    const uint64_t stride = (uint64_t)gridDim.x * kRoBlock;
    for (uint64_t p = (uint64_t)blockIdx.x * kRoBlock + threadIdx.x; p < src.indexCount; p += stride) {
        const uint32_t o = rule.of_primitive(p);
        int32_t v = -4;
        if (o <= 5u) {
            const int32_t e = named_entry(src, p);
            if (e < 0) v = e == kSkipped ? -4 : e;
            else {
                const uint64_t d = rule.item((uint32_t)e, o);
                const uint32_t w = item[d];                        // (a word: the pair was marked, so it passed the bounds rule)
                if (w) v = index_back(tail, d, w, s_n);
            }
        }
        outIndex[p] = v;
    }
    counters_end<kRebuildHist>(s_n, tail.indexHist);
}

// the call's scratch: the header and the marks behind it (ONE memset clears both), the blocks' addresses, the arrays of the tail
struct ReorientScratch { ReorientHeader* hdr; uint32_t* ref; unsigned long long* srcAddr; TailArrays t; size_t bytes; };
ReorientScratch reorient_scratch(const ReorientArgs& a, void* base)
{
    ReorientScratch s; CarveCursor c{ (uintptr_t)base };
    const uint32_t items = (uint32_t)reorient_items(a);
    s.hdr = c.take<ReorientHeader>(1); s.ref = c.take<uint32_t>(items);
    s.srcAddr = c.take<unsigned long long>(items);
    s.t = rebuild_arrays(c, items, a.flags);
    s.bytes = (size_t)(c.at - (uintptr_t)base);
    return s;
}
ItemRule item_rule(const ReorientArgs& a) { ItemRule r; r.orientations = a.orientations; r.orientation = a.orientation; return r; }

} // namespace

size_t reorient_head_bytes(const ReorientArgs& a) { return reorient_scratch(a, nullptr).bytes; }

hipError_t reorient_plan(const ReorientArgs& a, void* head, ReorientPlan* out, hipStream_t stream)
{
    const ReorientScratch s = reorient_scratch(a, head);
    const uint32_t items = (uint32_t)reorient_items(a);
    REBUILD_CHECK(hipMemsetAsync(s.hdr, 0, (size_t)((uint8_t*)s.ref - (uint8_t*)s.hdr) + 4 * (size_t)items, stream));   // (the header and the marks behind it)
    reorient_mark<<<strided_grid(a.source.indexCount), kRoBlock, 0, stream>>>(a.source, item_rule(a), s.ref, s.hdr);
    REBUILD_CHECK(hipGetLastError());
    unsigned long long stagingBytes = 0, totalUnits = 0;
    if (items) {
        reorient_prepare<<<per_item_grid((uint64_t)items + 1u), kRoBlock, 0, stream>>>(a.source, item_rule(a), items, s.ref, s.t.item, s.t.slotStart, s.t.units, s.srcAddr,
                                                                                        s.t.digest, s.t.umask, s.hdr);
        REBUILD_CHECK(hipGetLastError());
        REBUILD_CHECK(rebuild_scan(s.t, items, &stagingBytes, &totalUnits, stream));
    }
    ReorientHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&h, s.hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    out->stagingBytes = stagingBytes; out->units = totalUnits; out->skipped = h.skipped; out->referenced = h.referenced; out->reoriented = h.reoriented;
    return hipSuccess;
}

hipError_t reorient_stage(const ReorientArgs& a, void* head, void* staging, const ReorientPlan& plan, RebuildCounts* out, hipStream_t stream)
{
    const ReorientScratch s = reorient_scratch(a, head);
    const uint32_t items = (uint32_t)reorient_items(a);
    if (plan.units) {
        reorient_units<<<(uint32_t)(plan.units < kRebuildMaxGrid ? plan.units : kRebuildMaxGrid), kRoBlock, 0, stream>>>(item_rule(a), items, s.t.item, s.srcAddr, s.t.units,
                                                                                                                       s.t.slotStart, (uint8_t*)staging, s.t.digest, s.t.umask);
        REBUILD_CHECK(hipGetLastError());
    }
    return rebuild_count(tail_inputs(s.t, items, a.flags, staging), out, stream);
}

hipError_t reorient_emit(const ReorientArgs& a, void* head, const void* staging, const RebuildCounts& counts, const RebuildOutputs& o, hipStream_t stream)
{
    const ReorientScratch s = reorient_scratch(a, head);
    const RebuildInputs in = tail_inputs(s.t, (uint32_t)reorient_items(a), a.flags, staging);
    REBUILD_CHECK(rebuild_emit(in, counts, o.arrayData, o.descs, stream));
    reorient_index<<<strided_grid(a.source.indexCount), kRoBlock, 0, stream>>>(a.source, item_rule(a), in.item, rebuild_tables(in), (int32_t*)o.index);
    REBUILD_CHECK(hipGetLastError());
    return rebuild_histograms(in, o.hist, stream);
}

} // namespace ommx
