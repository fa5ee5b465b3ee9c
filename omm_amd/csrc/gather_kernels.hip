// gather_kernels.hip -- ommxGatherMicromaps (include/omm_mi355x_ext.h has the definition): chosen primitives of K device-resident results become one
// result.  The blocks they select are copied, bits unchanged, into aligned staging slots; then the tail of a bake runs on them (rebuild_kernels.hip)
// -- uniform blocks to special indices, equal blocks merged, blocks ordered by size, descriptors and histograms rebuilt -- and the index buffer is
// written.  The K sources do not fit in kernel arguments: their table lies in the call's scratch, uploaded once.
//
//   gather_mark       one lane per output primitive: its (source, primitive) from the selection or from the scan of the sources' indexCount, the
//                     index entry in the source's width, the bounds rule; the selected descriptor is marked, a primitive that fails is counted
//   gather_prepare    one lane per descriptor of the concatenated descriptor arrays: for a marked one its word for the tail (level and format,
//                     unchanged), the address of its block, the size of its staging slot and its number of work units
//   gather_units      THE copy: one workgroup per unit of 16 KiB of one block and turn, 16 bytes per lane and step.  The block lies at any byte
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
#include <rocprim/rocprim.hpp>
#include "gather_kernels.h"
#include "gather_copy.h"
#include "result_read.h"
#include "result_words.h"
#include "bake_host.h"   // pad256
#include "wave_search.h"

namespace ommx {
namespace {

constexpr uint32_t kGaBlock = kRebuildBlock;
constexpr uint32_t kGaWaves = kGaBlock / 64;
constexpr uint32_t kGaUnitBytes = 16384;             // a workgroup's unit: four 16-byte vectors per lane
constexpr uint32_t kGaUnitVectors = kGaUnitBytes / 16;

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
        return *k < sources && *p < table[*k].indexCount;
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
        uint32_t k = 0u, p = 0u;
        int32_t e = -5;                                        // (a primitive that names none is skipped like an entry below -4)
        bool ok = false;
        if (resolve(table, sources, selection, i, &k, &p)) {
            const GatherSource s = table[k];
            e = index_entry(s.index, s.indexFormat, p);
            if (e >= 0 && (uint32_t)e < s.descCount && desc_ok(load_desc(s.descs + e), s.arrayDataSize)) {
                ok = true;
                atomicOr(&ref[(uint64_t)s.descBase + (uint32_t)e], 1u);
            }
        }
        skipped += e < -4 || (e >= 0 && !ok) ? 1u : 0u;
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
                const ommCpuOpacityMicromapDesc desc = load_desc(s.descs + (d - s.descBase));   // (marked: it passed the bounds rule)
                bytes = block_bytes(desc.subdivisionLevel, desc.format);
                n = bytes > kGaUnitBytes ? bytes / kGaUnitBytes : 1ull;
                srcAddr[d] = (unsigned long long)(uintptr_t)(s.arrayData + desc.offset);
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
    const uint32_t t = threadIdx.x;
    const unsigned long long total = unitStart[descTotal];
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t d = owner_of_segment(unitStart, descTotal, u);
        const uint32_t w = item[d], level = item_level(w), bits = item_bits(w);
        const uint64_t bytes = block_bytes(level, bits);
        const uint8_t* block = (const uint8_t*)(uintptr_t)srcAddr[d];
        uint8_t* dst = staging + slotStart[d];
        UnitOut o; o.dst = dst; o.fieldBase = 0ull; o.outFields = 0u; o.bits = bits; o.digest = 0ull; o.umask = 0xFu;
        if (bytes < 16u) {
            if (t == 0u) {
                const uint64_t word = gather_small(block, (uint32_t)bytes, level, bits);
                if (bytes == 8u) *(uint64_t*)dst = word;
                else for (uint32_t b = 0; b < (uint32_t)bytes; ++b) dst[b] = (uint8_t)(word >> (8u * b));
                const uint32_t used = bits << (2u * level);
                o.digest = word_digest(word, 0u); o.umask = coarsen_word_uniform(word, used < 64u ? used : 64u, bits);
            }
        } else {
            const uint64_t first = (u - unitStart[d]) * kGaUnitVectors;                 // the unit's first vector within the block
            const uint32_t count = bytes < kGaUnitBytes ? (uint32_t)(bytes / 16u) : kGaUnitVectors;
            WordsVec* out = (WordsVec*)dst + first;
            if (gather_shift(block) == 0u) {
                const WordsVec* in = (const WordsVec*)block + first;
                #pragma unroll 4
                for (uint32_t v = t; v < count; v += kGaBlock) {
                    const WordsVec x = in[v];
                    out[v] = x;
                    const uint64_t word = 2u * (first + v);
                    o.digest += word_digest(x[0], word) + word_digest(x[1], word + 1u);
                    o.umask &= coarsen_word_uniform(x[0], 64u, bits) & coarsen_word_uniform(x[1], 64u, bits);
                }
            } else {
                #pragma unroll 4
                for (uint32_t v = t; v < count; v += kGaBlock) {
                    const GatherWords x = gather_vector(block, bytes, first + v);
                    WordsVec y; y[0] = x.w0; y[1] = x.w1;
                    out[v] = y;
                    const uint64_t word = 2u * (first + v);
                    o.digest += word_digest(x.w0, word) + word_digest(x.w1, word + 1u);
                    o.umask &= coarsen_word_uniform(x.w0, 64u, bits) & coarsen_word_uniform(x.w1, 64u, bits);
                }
            }
        }
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
            const int32_t e = index_entry(s.index, s.indexFormat, p);
            uint32_t w;
            if (e < 0) v = e >= -4 ? e : -4;
            else if ((uint32_t)e < s.descCount && (w = item[(uint64_t)s.descBase + (uint32_t)e]) != 0u) {   // (marked: it passed the bounds rule)
                const uint64_t d = (uint64_t)s.descBase + (uint32_t)e;
                v = tail.special[d];
                if (v == 0) {
                    v = (int32_t)tail.newIndex[tail.rep[d]];
                    atomicAdd(&s_n[2u * item_level(w) + item_bits(w) - 1u], 1u);
                }
            }
        }
        outIndex[i] = v;
    }
    counters_end<kRebuildHist>(s_n, tail.indexHist);
}

struct GatherLayout { size_t header, ref, table, item, slot, units, srcAddr, digest, umask, temp, tail, bytes; size_t tempBytes; };
GatherLayout gather_layout(const GatherArgs& a)
{
    GatherLayout L; size_t o = 0;
    const size_t D = a.descTotal;
    const auto take = [&o](size_t bytes) { const size_t at = o; o += pad256(bytes); return at; };
    L.header = take(sizeof(GatherHeader));
    L.ref = take(4 * D); L.table = take(sizeof(GatherSource) * (size_t)a.sourceCount); L.item = take(4 * D);
    L.slot = take(8 * (D + 1)); L.units = take(8 * (D + 1)); L.srcAddr = take(8 * D);
    L.digest = take(8 * D); L.umask = take(4 * D);
    L.tempBytes = 0;
    if (D) (void)rocprim::exclusive_scan(nullptr, L.tempBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, D + 1, rocprim::plus<unsigned long long>());
    L.temp = take(L.tempBytes);
    L.tail = take(rebuild_bytes(a.descTotal, a.flags));
    L.bytes = o;
    return L;
}
RebuildInputs tail_inputs(const GatherArgs& a, const GatherLayout& L, uint8_t* base, const void* staging)
{
    RebuildInputs in;
    in.items = a.descTotal; in.flags = a.flags;   // (ommxGatherFlags have the values of ommxCoarsenFlags)
    in.item = (const uint32_t*)(base + L.item); in.slotStart = (const unsigned long long*)(base + L.slot);
    in.digest = (const unsigned long long*)(base + L.digest); in.umask = (const uint32_t*)(base + L.umask);
    in.staging = (const uint8_t*)staging; in.scratch = base + L.tail;
    return in;
}

} // namespace

size_t gather_head_bytes(const GatherArgs& a) { return gather_layout(a).bytes; }

hipError_t gather_plan(const GatherArgs& a, void* head, GatherPlan* out, hipStream_t stream)
{
    const GatherLayout L = gather_layout(a);
    uint8_t* base = (uint8_t*)head;
    const uint32_t D = a.descTotal, K = a.sourceCount;
    GatherHeader* hdr = (GatherHeader*)(base + L.header);
    uint32_t* ref = (uint32_t*)(base + L.ref);
    const GatherSource* table = (const GatherSource*)(base + L.table);
    unsigned long long* slot = (unsigned long long*)(base + L.slot);
    unsigned long long* units = (unsigned long long*)(base + L.units);
    REBUILD_CHECK(hipMemsetAsync(hdr, 0, L.ref - L.header + 4 * (size_t)D, stream));   // (the header and the marks behind it)
    REBUILD_CHECK(hipMemcpyAsync(base + L.table, a.sources, sizeof(GatherSource) * (size_t)K, hipMemcpyHostToDevice, stream));
    gather_mark<<<strided_grid(a.primitiveCount), kGaBlock, 0, stream>>>(table, K, a.selection, a.primitiveCount, ref, hdr);
    REBUILD_CHECK(hipGetLastError());
    unsigned long long stagingBytes = 0, totalUnits = 0;
    if (D) {
        gather_prepare<<<per_item_grid((uint64_t)D + 1u), kGaBlock, 0, stream>>>(table, K, D, ref, (uint32_t*)(base + L.item), slot, units, (unsigned long long*)(base + L.srcAddr),
                                                                                (unsigned long long*)(base + L.digest), (uint32_t*)(base + L.umask), hdr);
        REBUILD_CHECK(hipGetLastError());
        size_t tb = L.tempBytes;   // (in place: every element is read before it is written)
        REBUILD_CHECK(rocprim::exclusive_scan(base + L.temp, tb, slot, slot, 0ull, (size_t)D + 1, rocprim::plus<unsigned long long>(), stream));
        tb = L.tempBytes;
        REBUILD_CHECK(rocprim::exclusive_scan(base + L.temp, tb, units, units, 0ull, (size_t)D + 1, rocprim::plus<unsigned long long>(), stream));
        REBUILD_CHECK(hipMemcpyAsync(&stagingBytes, slot + D, sizeof stagingBytes, hipMemcpyDeviceToHost, stream));
        REBUILD_CHECK(hipMemcpyAsync(&totalUnits, units + D, sizeof totalUnits, hipMemcpyDeviceToHost, stream));
    }
    GatherHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    out->stagingBytes = stagingBytes; out->units = totalUnits; out->skipped = h.skipped; out->referenced = h.referenced;
    return hipSuccess;
}

hipError_t gather_stage(const GatherArgs& a, void* head, void* staging, const GatherPlan& plan, RebuildCounts* out, hipStream_t stream)
{
    const GatherLayout L = gather_layout(a);
    uint8_t* base = (uint8_t*)head;
    const RebuildInputs in = tail_inputs(a, L, base, staging);
    if (plan.units) {
        gather_units<<<(uint32_t)(plan.units < kRebuildMaxGrid ? plan.units : kRebuildMaxGrid), kGaBlock, 0, stream>>>(a.descTotal, in.item, (const unsigned long long*)(base + L.srcAddr),
                                                                                                                     (const unsigned long long*)(base + L.units), in.slotStart, (uint8_t*)staging,
                                                                                                                     (unsigned long long*)(base + L.digest), (uint32_t*)(base + L.umask));
        REBUILD_CHECK(hipGetLastError());
    }
    return rebuild_count(in, out, stream);
}

hipError_t gather_emit(const GatherArgs& a, void* head, const void* staging, const RebuildCounts& counts, const GatherOutputs& o, hipStream_t stream)
{
    const GatherLayout L = gather_layout(a);
    uint8_t* base = (uint8_t*)head;
    const RebuildInputs in = tail_inputs(a, L, base, staging);
    REBUILD_CHECK(rebuild_emit(in, counts, o.arrayData, o.descs, stream));
    gather_index<<<strided_grid(a.primitiveCount), kGaBlock, 0, stream>>>((const GatherSource*)(base + L.table), a.sourceCount, a.selection, a.primitiveCount, in.item,
                                                                          rebuild_tables(in), o.index);
    REBUILD_CHECK(hipGetLastError());
    return rebuild_histograms(in, o.hist, stream);
}

} // namespace ommx
