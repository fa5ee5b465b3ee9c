// gather_kernels.hip -- ommxGatherMicromaps (include/omm_mi355x_ext.h has the definition): chosen primitives of K device-resident results become one
// result.  The blocks they select are copied, bits unchanged, into aligned staging slots; then the tail of a bake runs on them (rebuild_kernels.hip)
// -- uniform blocks to special indices, equal blocks merged, blocks ordered by size, descriptors and histograms rebuilt -- and the index buffer is
// written.  The K sources do not fit in kernel arguments: their table lies in the call's scratch, uploaded once.
//
//   gather_mark       one lane per output primitive: its (source, primitive) from the selection or from the scan of the sources' indexCount, the
//                     index entry in the source's width, the bounds rule; the selected descriptor is marked, a primitive that fails is counted
//   gather_prepare    one lane per descriptor of the concatenated descriptor arrays: for a marked one its word for the tail (level and format,
//                     unchanged), the address of its block, the size of its staging slot and its number of work units
//   gather_units      THE copy (copy_unit in gather_unit.h): one workgroup per unit of 16 KiB of one block and turn, 16 bytes per lane and step.  The block lies at any byte
//                     address (gather_copy.h): an aligned one is a plain vector copy, any other reads aligned vectors and shifts two neighbours
//                     into place, with the block's first and last partial vector read byte by byte -- no byte outside the block is read.  The
//                     writers sum the digest of the words and AND their uniformity masks (result_words.h): one integer atomic each per workgroup.
//                     A block below 16 bytes is one lane's.
//   (the tail)        items are (source, descriptor) pairs in lexicographic order, so representatives within a size class are ordered that way
//   gather_index      one lane per output primitive: the index buffer, 32-bit entries
//
// All counters are integers and every output byte has one writer, so the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <string.h>
#include "gather_kernels.h"
#include "gather_unit.h"
#include "result_read.h"
#include "result_words.h"
#include "wave_search.h"

namespace ommx {
namespace {

constexpr uint32_t kGaBlock = kRebuildBlock;
constexpr uint32_t kGaWaves = kGaBlock / 64;

struct GatherHeader { uint32_t skipped, referenced; };

// the last row k with base(row k) <= x (base(row 0) is 0); rows without items share their base with the next row and are passed over.  The steps are
// the powers of two below `rows`, the same for every lane: the lanes of a wave stay together whatever rows they find.
template <typename Base>
__device__ __forceinline__ uint32_t row_of(uint32_t rows, uint64_t x, Base base)
{
    uint32_t lo = 0u;
    for (uint32_t step = 1u << (31u - (uint32_t)__clz((int)rows)); step; step >>= 1) {
        const uint32_t at = lo + step;
        if (at < rows && base(at) <= x) lo = at;
    }
    return lo;
}
// output primitive i -> (source, primitive); false: it names no primitive of a source
__device__ __forceinline__ bool resolve(const GatherSource* __restrict__ table, uint32_t sources, const ommxPrimitiveRef* __restrict__ selection, uint64_t i,
                                        uint32_t* k, uint32_t* p)
{
    if (selection) {
        *k = selection[i].source; *p = selection[i].primitive;
        return *k < sources && *p < table[*k].view.indexCount;
    }
    *k = row_of(sources, i, [table](uint32_t r) { return (uint64_t)table[r].primBase; });
    *p = (uint32_t)(i - table[*k].primBase);   // (i < the sum of indexCount, so p < indexCount of that row)
    return true;
}

// A. one lane per output primitive and turn
__global__ __launch_bounds__(kGaBlock) void gather_mark(const GatherSource* __restrict__ table, uint32_t sources, const ommxPrimitiveRef* __restrict__ selection,
                                                        uint32_t primitives, uint32_t* __restrict__ ref, GatherHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    uint32_t skipped = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kGaBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kGaBlock + threadIdx.x; i < primitives; i += stride) {
        uint32_t k, p, skip = 1u;                                  // (a primitive that names none is skipped like an entry below -4)
        if (resolve(table, sources, selection, i, &k, &p)) {
            const GatherSource s = table[k];
            skip = mark_selected(s.view, p, ref + s.descBase);
        }
        skipped += skip;
    }
    if (skipped) atomicAdd(&s_n[0], skipped);
    counters_end<1>(s_n, &hdr->skipped);
}

// B. one lane per descriptor of the concatenation and one for the scans' closing element
__global__ __launch_bounds__(kGaBlock) void gather_prepare(const GatherSource* __restrict__ table, uint32_t sources, uint32_t descTotal, const uint32_t* __restrict__ ref,
                                                           uint32_t* __restrict__ item, unsigned long long* __restrict__ slot, unsigned long long* __restrict__ units,
                                                           unsigned long long* __restrict__ srcAddr, unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask,
                                                           GatherHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const uint64_t d = (uint64_t)blockIdx.x * kGaBlock + threadIdx.x;
    if (d <= descTotal) {
        unsigned long long bytes = 0ull, n = 0ull;
        if (d < descTotal) {
            uint32_t w = 0u;
            if (ref[d]) {
                const GatherSource s = table[row_of(sources, d, [table](uint32_t r) { return (uint64_t)table[r].descBase; })];
                const ommCpuOpacityMicromapDesc desc = load_desc(s.view.descs + (d - s.descBase));   // (marked: it passed the bounds rule)
                bytes = block_bytes(desc.subdivisionLevel, desc.format);
                n = unit_count(bytes);
                srcAddr[d] = (unsigned long long)(uintptr_t)(s.view.arrayData + desc.offset);
                bytes = (bytes + kRebuildSlotAlign - 1u) & ~(unsigned long long)(kRebuildSlotAlign - 1u);
                digest[d] = 0ull; umask[d] = 0xFu;
                w = item_word(desc.subdivisionLevel, desc.format);
                atomicAdd(&s_n[0], 1u);
            }
            item[d] = w;
        }
        slot[d] = bytes; units[d] = n;
    }
    counters_end<1>(s_n, &hdr->referenced);
}

// C. one unit per workgroup and turn
__global__ __launch_bounds__(kGaBlock) void gather_units(uint32_t descTotal, const uint32_t* __restrict__ item, const unsigned long long* __restrict__ srcAddr,
                                                         const unsigned long long* __restrict__ unitStart, const unsigned long long* __restrict__ slotStart,
                                                         uint8_t* __restrict__ staging, unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask)
{
    __shared__ uint64_t s_digest[kGaWaves];
    __shared__ uint32_t s_umask[kGaWaves];
    const unsigned long long total = unitStart[descTotal];
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t d = owner_of_segment(unitStart, descTotal, u);
        const uint32_t w = item[d], level = item_level(w), bits = item_bits(w);
        const uint8_t* block = (const uint8_t*)(uintptr_t)srcAddr[d];
        uint8_t* dst = staging + slotStart[d];
        UnitOut o; o.dst = dst; o.fieldBase = 0ull; o.outFields = 0u; o.bits = bits; o.digest = 0ull; o.umask = 0xFu;
        copy_unit<kGaBlock>(block, level, bits, u - unitStart[d], o);
        unit_close<kGaWaves>(o, s_digest, s_umask, digest + d, umask + d);
        __syncthreads();   // (the LDS words are the next unit's too)
    }
}

// F3. one lane per output primitive and turn
__global__ __launch_bounds__(kGaBlock) void gather_index(const GatherSource* __restrict__ table, uint32_t sources, const ommxPrimitiveRef* __restrict__ selection,
                                                         uint32_t primitives, const uint32_t* __restrict__ item, RebuildTables tail, int32_t* __restrict__ outIndex)
{
    __shared__ uint32_t s_n[kRebuildHist];
    counters_begin<kRebuildHist>(s_n);
    const uint64_t stride = (uint64_t)gridDim.x * kGaBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kGaBlock + threadIdx.x; i < primitives; i += stride) {
        int32_t v = -4;
        uint32_t k, p;
        if (resolve(table, sources, selection, i, &k, &p)) {
            const GatherSource s = table[k];
            v = index_back(s.view, p, item, s.descBase, tail, s_n);
        }
        outIndex[i] = v;
    }
    counters_end<kRebuildHist>(s_n, tail.indexHist);
}

// the call's scratch: the header and the marks behind it (ONE memset clears both), the source table, the blocks' addresses, the arrays of the tail
struct GatherScratch { GatherHeader* hdr; uint32_t* ref; GatherSource* table; unsigned long long* srcAddr; TailArrays t; size_t bytes; };
GatherScratch gather_scratch(const GatherArgs& a, void* base)
{
    GatherScratch s; CarveCursor c{ (uintptr_t)base };
    s.hdr = c.take<GatherHeader>(1); s.ref = c.take<uint32_t>(a.descTotal);
    s.table = c.take<GatherSource>(a.sourceCount); s.srcAddr = c.take<unsigned long long>(a.descTotal);
    s.t = rebuild_arrays(c, a.descTotal, a.flags);   // (ommxGatherFlags have the values of ommxCoarsenFlags)
    s.bytes = (size_t)(c.at - (uintptr_t)base);
    return s;
}

} // namespace

size_t gather_head_bytes(const GatherArgs& a) { return gather_scratch(a, nullptr).bytes; }

hipError_t gather_plan(const GatherArgs& a, void* head, GatherPlan* out, hipStream_t stream)
{
    const GatherScratch s = gather_scratch(a, head);
    const uint32_t D = a.descTotal, K = a.sourceCount;
    REBUILD_CHECK(hipMemsetAsync(s.hdr, 0, (size_t)((uint8_t*)s.ref - (uint8_t*)s.hdr) + 4 * (size_t)D, stream));   // (the header and the marks behind it)
    REBUILD_CHECK(hipMemcpyAsync(s.table, a.sources, sizeof(GatherSource) * (size_t)K, hipMemcpyHostToDevice, stream));
    gather_mark<<<strided_grid(a.primitiveCount), kGaBlock, 0, stream>>>(s.table, K, a.selection, a.primitiveCount, s.ref, s.hdr);
    REBUILD_CHECK(hipGetLastError());
    unsigned long long stagingBytes = 0, totalUnits = 0;
    if (D) {
        gather_prepare<<<per_item_grid((uint64_t)D + 1u), kGaBlock, 0, stream>>>(s.table, K, D, s.ref, s.t.item, s.t.slotStart, s.t.units, s.srcAddr, s.t.digest, s.t.umask, s.hdr);
        REBUILD_CHECK(hipGetLastError());
        REBUILD_CHECK(rebuild_scan(s.t, D, &stagingBytes, &totalUnits, stream));
    }
    GatherHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&h, s.hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    out->stagingBytes = stagingBytes; out->units = totalUnits; out->skipped = h.skipped; out->referenced = h.referenced;
    return hipSuccess;
}

hipError_t gather_stage(const GatherArgs& a, void* head, void* staging, const GatherPlan& plan, RebuildCounts* out, hipStream_t stream)
{
    const GatherScratch s = gather_scratch(a, head);
    if (plan.units) {
        gather_units<<<(uint32_t)(plan.units < kRebuildMaxGrid ? plan.units : kRebuildMaxGrid), kGaBlock, 0, stream>>>(a.descTotal, s.t.item, s.srcAddr, s.t.units, s.t.slotStart,
                                                                                                                     (uint8_t*)staging, s.t.digest, s.t.umask);
        REBUILD_CHECK(hipGetLastError());
    }
    return rebuild_count(tail_inputs(s.t, a.descTotal, a.flags, staging), out, stream);
}

hipError_t gather_emit(const GatherArgs& a, void* head, const void* staging, const RebuildCounts& counts, const RebuildOutputs& o, hipStream_t stream)
{
    const GatherScratch s = gather_scratch(a, head);
    const RebuildInputs in = tail_inputs(s.t, a.descTotal, a.flags, staging);
    REBUILD_CHECK(rebuild_emit(in, counts, o.arrayData, o.descs, stream));
    gather_index<<<strided_grid(a.primitiveCount), kGaBlock, 0, stream>>>(s.table, a.sourceCount, a.selection, a.primitiveCount, in.item, rebuild_tables(in), (int32_t*)o.index);
    REBUILD_CHECK(hipGetLastError());
    return rebuild_histograms(in, o.hist, stream);
}

} // namespace ommx
