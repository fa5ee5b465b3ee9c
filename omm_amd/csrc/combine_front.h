// combine_front.h -- the front of the entries that read several device-resident results primitive by primitive (ommxCombineMicromaps in
// combine_kernels.hip, ommxCompareMicromaps in compare_kernels.hip): the normalised entry, the two kernels that find the distinct tuples of entries
// with their lowest primitive, the layout of the scratch per primitive, and the host call that runs them.
//
//   combine_entries   one lane per primitive: the K entries under the bounds rule; a primitive with a failing entry is skipped, one with only
//                     special entries is answered here, every other one puts the hash of its tuple into the table (hash_build.h), lowest index wins
//   combine_leaders   one lane per primitive: the lowest primitive with the same tuple (the entries confirm); a scan of the leaders numbers the tuples
//
// Each file that includes this compiles kernels of its own (they are in an anonymous namespace): include it from a .hip file only.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "combine_kernels.h"
#include "result_read.h"
#include "result_words.h"
#include "hash_build.h"
#include "bake_host.h"   // pad256

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

// the scratch per primitive.  After front_tuples: code[i] is 0 for a primitive with a tuple, -4 for a skipped one (combine's answer for a primitive
// with only special entries can be -4 too); leader[i] is the lowest primitive with the same tuple; tupleStart[leader] numbers the tuples
struct HeadLayout { size_t header, table, code, key, leader, tupleStart, temp, bytes; size_t tempBytes; uint32_t slots; };
inline HeadLayout head_layout(const CombineArgs& a)
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

// A, B and the scan on `stream`; the number of tuples and of skipped primitives copied to the host, the stream synchronised
inline hipError_t front_tuples(const CombineArgs& a, void* head, CombineTuples* out, hipStream_t stream)
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

} // namespace
} // namespace ommx
