// rebuild_kernels.hip -- staged blocks with a digest and a uniformity mask become a result: the tail of a bake, for ommxCoarsenMicromap,
// ommxCombineMicromaps and ommxGatherMicromaps (rebuild_kernels.h says what an item is and what the caller brings).
//
//   (two scans)       for the caller, before it stages: sizes of slots and numbers of work units become offsets (rebuild_scan)
//   rebuild_classify  one lane per item: uniform blocks become special indices; the others enter the hash table (hash_build.h) under (digest, level, format)
//   rebuild_resolve   one lane per item: the lowest item under the same key is the candidate; equal level, format and bytes make it the representative
//   (radix sort)      representatives by size class descending, stable, hence by item ascending within a class
//   rebuild_descs / rebuild_gather   descriptors and blocks below 16 bytes; the larger blocks 16 bytes per lane
//
// All counters are integers and every output byte has one writer, so the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include "rebuild_kernels.h"
#include "result_words.h"
#include "hash_build.h"
#include "bake_host.h"   // CarveCursor

namespace ommx {
namespace {

constexpr uint32_t kNoClass = 31;   // sort key of an item that emits no block

struct RebuildHeader {
    uint32_t uniform, duplicate;
    uint32_t classCount[kRebuildSizeClasses];
    uint32_t arrayHist[kRebuildHist], indexHist[kRebuildHist];
};
struct Place { uint64_t base[kRebuildSizeClasses]; uint32_t first[kRebuildSizeClasses], count[kRebuildSizeClasses]; };

// E1. the special index of a uniform block, every other block into the hash table
__global__ __launch_bounds__(kRebuildBlock) void rebuild_classify(uint32_t items, uint32_t flags, const uint32_t* __restrict__ item, const unsigned long long* __restrict__ digest,
                                                                  const uint32_t* __restrict__ umask, int32_t* __restrict__ special, HashTable table,
                                                                  RebuildHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const uint64_t t = (uint64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (t < items) {
        const uint32_t w = item[t];
        int32_t sp = 0;
        if (w) {
            const uint32_t um = umask[t];
            if (um) atomicAdd(&s_n[0], 1u);
            if (um && !(flags & ommxCoarsenFlags_DisableSpecialIndices)) sp = -(int32_t)(__ffs((int)um));   // bit s -> -(s + 1)
            else if (!(flags & ommxCoarsenFlags_DisableDuplicateDetection)) hash_put_min(table, block_key(digest[t], item_level(w), item_bits(w)), (uint32_t)t);
        }
        special[t] = sp;
    }
    counters_end<1>(s_n, &hdr->uniform);
}

__device__ __forceinline__ bool same_bytes(const uint8_t* x0, const uint8_t* y0, uint64_t n)
{
    if (n >= 64u) {   // (slots are 16-byte aligned, sizes are powers of two) 64 bytes of each block per turn: eight loads in flight, one branch
        const WordsVec* x = (const WordsVec*)x0; const WordsVec* y = (const WordsVec*)y0;
        for (uint64_t i = 0; i < n / 16u; i += 4u) {
            const WordsVec d = (x[i] ^ y[i]) | (x[i + 1u] ^ y[i + 1u]) | (x[i + 2u] ^ y[i + 2u]) | (x[i + 3u] ^ y[i + 3u]);
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

// E2. the item's representative, and the sort key of a block that will be emitted
__global__ __launch_bounds__(kRebuildBlock) void rebuild_resolve(uint32_t items, uint32_t flags, const uint32_t* __restrict__ item, const unsigned long long* __restrict__ digest,
                                                                 const int32_t* __restrict__ special, HashTable table, const unsigned long long* __restrict__ slotStart,
                                                                 const uint8_t* __restrict__ staging, uint32_t* __restrict__ rep, uint32_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ vals, RebuildHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1 + kRebuildSizeClasses];
    counters_begin<1 + kRebuildSizeClasses>(s_n);
    const uint64_t t = (uint64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (t < items) {
        uint32_t key = kNoClass, leader = (uint32_t)t;
        const uint32_t w = item[t];
        if (w && special[t] == 0) {
            const uint64_t bytes = block_bytes(item_level(w), item_bits(w));
            if (!(flags & ommxCoarsenFlags_DisableDuplicateDetection)) {
                const uint32_t c = hash_get(table, block_key(digest[t], item_level(w), item_bits(w)), (uint32_t)t);
                if (c < t && item[c] == w && same_bytes(staging + slotStart[t], staging + slotStart[c], bytes)) leader = c;
            }
            if (leader == t) {
                const uint32_t cls = 63u - (uint32_t)__clzll((long long)bytes);
                key = kRebuildSizeClasses - 1u - cls;
                atomicAdd(&s_n[1u + cls], 1u);
            } else atomicAdd(&s_n[0], 1u);
        }
        rep[t] = leader; keys[t] = key; vals[t] = (uint32_t)t;
    }
    counters_end<1 + kRebuildSizeClasses>(s_n, &hdr->duplicate);
}

// F1. one lane per output descriptor
__global__ __launch_bounds__(kRebuildBlock) void rebuild_descs(uint32_t count, Place place, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                               const uint32_t* __restrict__ item, const unsigned long long* __restrict__ slotStart,
                                                               const uint8_t* __restrict__ staging, uint8_t* __restrict__ outArray, ommCpuOpacityMicromapDesc* __restrict__ outDescs,
                                                               uint32_t* __restrict__ newIndex, RebuildHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[kRebuildHist];
    counters_begin<kRebuildHist>(s_n);
    const uint64_t j = (uint64_t)blockIdx.x * kRebuildBlock + threadIdx.x;
    if (j < count) {
        const uint32_t t = vals[j], cls = kRebuildSizeClasses - 1u - keys[j], w = item[t];
        const uint64_t off = place.base[cls] + ((uint64_t)(j - place.first[cls]) << cls);
        ommCpuOpacityMicromapDesc o; o.offset = (uint32_t)off; o.subdivisionLevel = (uint16_t)item_level(w); o.format = (uint16_t)item_bits(w);
        outDescs[j] = o;
        newIndex[t] = (uint32_t)j;
        atomicAdd(&s_n[2u * item_level(w) + item_bits(w) - 1u], 1u);
        if (cls < 4u) { const uint8_t* s = staging + slotStart[t]; for (uint32_t b = 0; b < (1u << cls); ++b) outArray[off + b] = s[b]; }
    }
    counters_end<kRebuildHist>(s_n, hdr->arrayHist);
}

// F2. the blocks of 16 bytes and more -- a prefix of the output: 16 bytes per lane and turn
__global__ __launch_bounds__(kRebuildBlock) void rebuild_gather(uint64_t bigBytes, Place place, const uint32_t* __restrict__ vals, const unsigned long long* __restrict__ slotStart,
                                                                const uint8_t* __restrict__ staging, uint8_t* __restrict__ outArray)
{
    const uint64_t stride = (uint64_t)gridDim.x * kRebuildBlock * 16u;
    for (uint64_t pos = ((uint64_t)blockIdx.x * kRebuildBlock + threadIdx.x) * 16u; pos < bigBytes; pos += stride) {
        uint32_t cls = kRebuildSizeClasses - 1u;
        while (cls > 4u && pos >= place.base[cls] + ((uint64_t)place.count[cls] << cls)) --cls;
        const uint64_t rel = pos - place.base[cls];
        const uint32_t t = vals[place.first[cls] + (uint32_t)(rel >> cls)];
        *(WordsVec*)(outArray + pos) = *(const WordsVec*)(staging + slotStart[t] + (rel & ((1ull << cls) - 1ull)));
    }
}

struct Carve {
    RebuildHeader* header; int32_t* special; uint32_t *rep, *keys, *vals, *keysSorted, *valsSorted, *newIndex;
    uint8_t *table, *temp; size_t tempBytes, bytes; uint32_t slots;
};
Carve carve(uintptr_t base, uint32_t items, uint32_t flags)
{
    Carve c; CarveCursor at{ base }; const size_t n = items;
    c.header = at.take<RebuildHeader>(1);
    c.special = at.take<int32_t>(n); c.rep = at.take<uint32_t>(n);
    c.keys = at.take<uint32_t>(n); c.vals = at.take<uint32_t>(n); c.keysSorted = at.take<uint32_t>(n); c.valsSorted = at.take<uint32_t>(n);
    c.newIndex = at.take<uint32_t>(n);
    c.slots = (flags & ommxCoarsenFlags_DisableDuplicateDetection) || !n ? 0u : hash_table_slots(n);
    c.table = at.take<uint8_t>(c.slots ? hash_table_bytes(c.slots) : 0);
    c.tempBytes = 0;
    if (n) (void)rocprim::radix_sort_pairs(nullptr, c.tempBytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, 5u);
    c.temp = at.take<uint8_t>(c.tempBytes);
    c.bytes = (size_t)(at.at - base);
    return c;
}
Carve carve(const RebuildInputs& in) { return carve((uintptr_t)in.scratch, in.items, in.flags); }

Place place_of(const RebuildCounts& c)
{
    Place p; uint64_t at = 0; uint32_t first = 0;
    for (int cls = (int)kRebuildSizeClasses - 1; cls >= 0; --cls) {
        p.base[cls] = at; p.first[cls] = first; p.count[cls] = c.classCount[cls];
        at += (uint64_t)c.classCount[cls] << cls; first += c.classCount[cls];
    }
    return p;
}

} // namespace

size_t rebuild_bytes(uint32_t items, uint32_t flags) { return carve(0, items, flags).bytes; }

TailArrays rebuild_arrays(CarveCursor& c, uint32_t items, uint32_t flags)
{
    size_t tempBytes = 0;
    if (items) (void)rocprim::exclusive_scan(nullptr, tempBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, (size_t)items + 1, rocprim::plus<unsigned long long>());
    return carve_tail_arrays(c, items, tempBytes, rebuild_bytes(items, flags));
}

hipError_t rebuild_scan(const TailArrays& t, uint32_t items, unsigned long long* stagingBytes, unsigned long long* totalUnits, hipStream_t stream)
{
    size_t tb = t.tempBytes;   // (in place: every element is read before it is written)
    REBUILD_CHECK(rocprim::exclusive_scan(t.temp, tb, t.slotStart, t.slotStart, 0ull, (size_t)items + 1, rocprim::plus<unsigned long long>(), stream));
    tb = t.tempBytes;
    REBUILD_CHECK(rocprim::exclusive_scan(t.temp, tb, t.units, t.units, 0ull, (size_t)items + 1, rocprim::plus<unsigned long long>(), stream));
    REBUILD_CHECK(hipMemcpyAsync(stagingBytes, t.slotStart + items, sizeof *stagingBytes, hipMemcpyDeviceToHost, stream));
    if (totalUnits) REBUILD_CHECK(hipMemcpyAsync(totalUnits, t.units + items, sizeof *totalUnits, hipMemcpyDeviceToHost, stream));
    return hipSuccess;
}

RebuildTables rebuild_tables(const RebuildInputs& in)
{
    const Carve c = carve(in);
    RebuildTables t; t.special = c.special; t.rep = c.rep; t.newIndex = c.newIndex; t.indexHist = c.header->indexHist;
    return t;
}

hipError_t rebuild_count(const RebuildInputs& in, RebuildCounts* out, hipStream_t stream)
{
    const Carve c = carve(in);
    REBUILD_CHECK(hipMemsetAsync(c.header, 0, sizeof(RebuildHeader), stream));
    if (in.items) {
        HashTable table; memset(&table, 0, sizeof table);
        if (c.slots) {
            table = hash_table_at(c.table, c.slots);
            REBUILD_CHECK(hipMemsetAsync(c.table, 0xFF, hash_table_bytes(c.slots), stream));
        }
        rebuild_classify<<<per_item_grid(in.items), kRebuildBlock, 0, stream>>>(in.items, in.flags, in.item, in.digest, in.umask, c.special, table, c.header);
        REBUILD_CHECK(hipGetLastError());
        rebuild_resolve<<<per_item_grid(in.items), kRebuildBlock, 0, stream>>>(in.items, in.flags, in.item, in.digest, c.special, table, in.slotStart, in.staging, c.rep, c.keys,
                                                                              c.vals, c.header);
        REBUILD_CHECK(hipGetLastError());
    }
    RebuildHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&h, c.header, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    memset(out, 0, sizeof *out);
    out->uniform = h.uniform; out->duplicate = h.duplicate;
    for (uint32_t k = 0; k < kRebuildSizeClasses; ++k) { out->classCount[k] = h.classCount[k]; out->descCount += h.classCount[k]; out->arrayBytes += (uint64_t)h.classCount[k] << k; }
    return hipSuccess;
}

hipError_t rebuild_emit(const RebuildInputs& in, const RebuildCounts& counts, uint8_t* arrayData, ommCpuOpacityMicromapDesc* descs, hipStream_t stream)
{
    if (!counts.descCount) return hipSuccess;
    const Carve c = carve(in);
    const Place place = place_of(counts);
    size_t tb = c.tempBytes;   // stable: equal size classes keep the order of their items
    REBUILD_CHECK(rocprim::radix_sort_pairs(c.temp, tb, c.keys, c.keysSorted, c.vals, c.valsSorted, (size_t)in.items, 0u, 5u, stream));
    rebuild_descs<<<per_item_grid(counts.descCount), kRebuildBlock, 0, stream>>>(counts.descCount, place, c.keysSorted, c.valsSorted, in.item, in.slotStart, in.staging, arrayData, descs,
                                                                                 c.newIndex, c.header);
    REBUILD_CHECK(hipGetLastError());
    const uint64_t big = place.base[3];   // the blocks of 16 bytes and more end where the 8-byte blocks begin
    if (big) {
        rebuild_gather<<<strided_grid(big / 16u), kRebuildBlock, 0, stream>>>(big, place, c.valsSorted, in.slotStart, in.staging, arrayData);
        REBUILD_CHECK(hipGetLastError());
    }
    return hipSuccess;
}

hipError_t rebuild_histograms(const RebuildInputs& in, uint32_t* hist, hipStream_t stream)
{
    const Carve c = carve(in);
    RebuildHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&h, c.header, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    memcpy(hist, h.arrayHist, sizeof h.arrayHist);
    memcpy(hist + kRebuildHist, h.indexHist, sizeof h.indexHist);
    return hipSuccess;
}

} // namespace ommx
