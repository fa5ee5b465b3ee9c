// bake_host.h -- the host-side rules of a bake that need no device: flag bits, index formats, the raw triangle upload, histogram lists, the result descriptor
// the carve of the working set, and the decisions and layouts of bake_core's stages that follow from a bake's counters alone (rank ranges, streamed result or
// not, deferred generic pass, the states arena, the read-back slots) and of the sharded bake (stride, chunks, exchange arena, host scatter).  Plain C++ (no HIP): omm_host.cpp calls each directly, tests/native/bake_host_check.cpp
// runs them under sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/omm_mi355x.h"

namespace ommx {
struct SetupCounters;   // bake_kernels.h (only pointed at here)

// constants of the kernel headers, restated so that this header stands alone; omm_host.cpp asserts each against its origin
constexpr int kBakeLevels = 13;                 // kNumLevels
constexpr size_t kBakeFineWords = 256 * 16;     // kFineSlots * kFineStride
constexpr size_t kBakeMaxRanks = 16, kBakePreviewSlotBytes = 256, kBakeStreamCtlWords = 100;   // kMaxRanks, kPreviewSlotBytes, kStreamCtlWords
constexpr size_t kBakeCountersSlot = 256;       // arena slot of SetupCounters: BakeHead (omm_host.cpp) fills it and the digest table behind it in ONE copy
inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- bake flags: bits 0-6 by their public ommCpuBakeFlags_* names, the internal ones (bake_cpu_impl.cpp:43-48) named here ----
constexpr uint32_t kBakeFlag_EnableAABBTesting = 1u << 7;              // bake_cpu_impl.cpp:43
constexpr uint32_t kBakeFlag_DisableLevelLineIntersection = 1u << 8;   // bake_cpu_impl.cpp:44
constexpr uint32_t kBakeFlag_DisableFineClassification = 1u << 9;      // bake_cpu_impl.cpp:45
constexpr uint32_t kBakeFlag_NearDuplicateBruteForce = 1u << 10;       // bake_cpu_impl.cpp:46
constexpr uint32_t kBakeFlag_EnableEdgeHeuristic = 1u << 11;           // bake_cpu_impl.cpp:48
inline bool has_flag(uint32_t flags, uint32_t bit) { return (flags & bit) != 0; }
// near-duplicate merging / a size budget: the reference's serial reducers, run on the host over the classified states (host_tail.cpp)
inline bool wants_host_tail(const ommCpuBakeInputDesc& d)
{
    return has_flag((uint32_t)d.bakeFlags, ommCpuBakeFlags_EnableNearDuplicateDetection | kBakeFlag_NearDuplicateBruteForce) || d.maxArrayDataSize != 0xFFFFFFFFu;
}
// no fine pass with the 2-state format: unresolved micro-triangles keep UnknownOpaque (3), which has no 1-bit form (bake_cpu_impl.cpp:1811)
inline bool no_fine_two_state(const ommCpuBakeInputDesc& d) { return has_flag((uint32_t)d.bakeFlags, kBakeFlag_DisableFineClassification) && d.format == ommFormat_OC1_2_State; }

// ---- index formats: the result's depends on the triangle count alone, the reference narrows int32 to int8 / int16 (bake_cpu_impl.cpp:1872-1902) ----
inline ommIndexFormat index_format_for(uint32_t numTris, uint32_t flags)
{
    if (has_flag(flags, ommCpuBakeFlags_Force32BitIndices)) return ommIndexFormat_UINT_32;
    if (has_flag(flags, ommCpuBakeFlags_Allow8BitIndices) && numTris <= INT8_MAX) return ommIndexFormat_UINT_8;
    return numTris <= INT16_MAX ? ommIndexFormat_UINT_16 : ommIndexFormat_UINT_32;
}
inline size_t index_bytes(ommIndexFormat f) { return f == ommIndexFormat_UINT_8 ? 1 : (f == ommIndexFormat_UINT_16 ? 2 : 4); }

// ---- the caller's raw triangle data as one device block: texture coordinates | indices | per-triangle levels, each from a 256-byte boundary ----
inline size_t uv_element_bytes(ommTexCoordFormat f) { return f == ommTexCoordFormat_UV32_FLOAT ? 8 : 4; }
inline uint32_t uv_stride(const ommCpuBakeInputDesc& d) { return d.texCoordStrideInBytes ? d.texCoordStrideInBytes : (uint32_t)uv_element_bytes(d.texCoordFormat); }
struct RawInputLayout { size_t uvBytes, idxBytes, lvlBytes, offUv, offIdx, offLvl, total; };   // total: with 256 bytes of slack behind the last region
// (the C ABI gives no vertex count: it is max(index) + 1, as serialize_impl.cpp:60-79)
inline RawInputLayout raw_input_layout(const ommCpuBakeInputDesc& d, uint32_t numTris, uint32_t maxIndex)
{
    RawInputLayout L;
    L.uvBytes = numTris ? (size_t)uv_stride(d) * maxIndex + uv_element_bytes(d.texCoordFormat) : 0;
    L.idxBytes = index_bytes(d.indexFormat) * 3 * (size_t)numTris;
    L.lvlBytes = d.subdivisionLevels ? numTris : 0;
    L.offUv = 0; L.offIdx = pad256(L.uvBytes); L.offLvl = L.offIdx + pad256(L.idxBytes);
    L.total = L.offLvl + pad256(L.lvlBytes) + 256;
    return L;
}

// ---- histograms: format {2-state, 4-state} x level ascending, non-zero entries only (bake_cpu_impl.cpp:1833-1850); one global format per bake ----
// hist: kBakeLevels counts of the OMM array, then kBakeLevels of the index buffer; the lists hold up to 2 * kBakeLevels entries
inline void compact_histograms(const uint32_t* hist, int bits, ommCpuOpacityMicromapUsageCount* outArray, ommCpuOpacityMicromapUsageCount* outIndex, uint32_t* nArray, uint32_t* nIndex)
{
    *nArray = 0; *nIndex = 0;
    for (int l = 0; l < kBakeLevels; ++l) {
        if (hist[l]) outArray[(*nArray)++] = ommCpuOpacityMicromapUsageCount{ hist[l], (uint16_t)l, (uint16_t)bits };
        if (hist[kBakeLevels + l]) outIndex[(*nIndex)++] = ommCpuOpacityMicromapUsageCount{ hist[kBakeLevels + l], (uint16_t)l, (uint16_t)bits };
    }
}
inline uint32_t clamp_hist_count(size_t n) { return n < 2 * (size_t)kBakeLevels ? (uint32_t)n : 2u * (uint32_t)kBakeLevels; }
// The one place that writes an ommCpuBakeResultDesc.  A bake without OMMs reports null arrays of size zero whatever the caller holds; the histogram
// lists are the caller's arrays of 2 * kBakeLevels entries: their counts are clamped to that.
inline void fill_result_desc(ommCpuBakeResultDesc* out, const void* arrayData, uint64_t arrayDataSize, const ommCpuOpacityMicromapDesc* descs, uint32_t numDescs,
                             const void* indexBuffer, uint32_t numTris, ommIndexFormat indexFormat,
                             const ommCpuOpacityMicromapUsageCount* arrayHist, size_t numArrayHist, const ommCpuOpacityMicromapUsageCount* indexHist, size_t numIndexHist)
{
    out->arrayData = numDescs ? arrayData : nullptr; out->arrayDataSize = numDescs ? (uint32_t)arrayDataSize : 0;
    out->descArray = numDescs ? descs : nullptr; out->descArrayCount = numDescs;
    out->descArrayHistogram = arrayHist; out->descArrayHistogramCount = clamp_hist_count(numArrayHist);
    out->indexBuffer = indexBuffer; out->indexCount = numTris; out->indexFormat = indexFormat;
    out->indexHistogram = indexHist; out->indexHistogramCount = clamp_hist_count(numIndexHist);
}
// micro-triangles of a bake: 4^level per work item (levelCount: SetupCounters)
inline uint64_t micro_triangles_of(const uint32_t* levelCount) { uint64_t n = 0; for (int l = 0; l < kBakeLevels; ++l) n += (uint64_t)levelCount[l] << (2 * l); return n; }

// ---- the working set of a bake (worst case: every triangle is its own work item) ----
// ONE function walks the slots in order over a bump cursor: from base 0 it gives the bytes to reserve (`bytes`; the pointers are then offsets), from the arena's
// base the pointers.  Two contracts rest on the order: `uniformDigest` lies kBakeCountersSlot behind `counters` (one host-to-device copy fills both), and
// `arrayHist`, `indexHist`, `err`, `fine` are consecutive (one device-to-host copy reads them back).
struct BakeTables {
    float* uv; uint8_t *level, *degen, *active; uint64_t *stateOfs, *digests; uint32_t *itemIds, *activeIds; int32_t *triToItem, *index;
    uint32_t *mask, *known; int32_t* special; uint32_t *rep, *order, *dstOfs, *sizes; int32_t* itemValue; float* triArea;
    SetupCounters* counters; uint64_t* uniformDigest; uint32_t *arrayHist, *indexHist, *err; unsigned long long* fine;   // fine: striped statistic counter (bake_types.h)
    uint8_t* scratch; size_t scratchBytes;   // setup / tail / stream scratch
    uint32_t* meta; uint8_t* owner; uint64_t *cofs, *totals;   // sharded bake: metadata words of the active items, owner rank, offsets in the contributions, bytes per rank
    // streamed result: placed offset per item, cursor + control words; preview: collapsed UVs, 256-byte state slots, offsets, masks, early flags
    uint64_t* placed; unsigned long long* cursor; uint32_t* streamCtl;
    float* uv2; uint8_t* states2; uint64_t* ofs2; uint32_t* mask2; uint8_t* early; uint32_t *earlyList, *earlyLead; unsigned long long* fine2;
    size_t bytes;   // end of the last slot, from the base
    size_t readback_bytes() const { return (size_t)((uintptr_t)fine - (uintptr_t)arrayHist) + kBakeFineWords * sizeof(unsigned long long); }   // [arrayHist, end of fine)
};
struct CarveCursor {   // (an integer, not a pointer: the sizing pass has no memory to point into)
    uintptr_t at;
    template <class T> T* take(size_t count) { T* p = reinterpret_cast<T*>(at); at += pad256(count * sizeof(T)); return p; }
};
inline BakeTables carve_bake_tables(uintptr_t base, uint32_t maxItems, size_t scratchBytes, bool sharded, bool streamed)
{
    BakeTables t = BakeTables(); CarveCursor c{ base }; const size_t n = maxItems;
    t.uv = c.take<float>(n * 6);
    t.level = c.take<uint8_t>(n); t.degen = c.take<uint8_t>(n); t.active = c.take<uint8_t>(n);
    t.stateOfs = c.take<uint64_t>(n); t.digests = c.take<uint64_t>(n);
    t.itemIds = c.take<uint32_t>(n); t.activeIds = c.take<uint32_t>(n);
    t.triToItem = c.take<int32_t>(n); t.index = c.take<int32_t>(n);
    t.mask = c.take<uint32_t>(n); t.known = c.take<uint32_t>(n);
    t.special = c.take<int32_t>(n); t.rep = c.take<uint32_t>(n);
    t.order = c.take<uint32_t>(n); t.dstOfs = c.take<uint32_t>(n);
    t.sizes = c.take<uint32_t>(n); t.itemValue = c.take<int32_t>(n);
    t.triArea = c.take<float>(n);
    t.counters = reinterpret_cast<SetupCounters*>(c.take<uint8_t>(kBakeCountersSlot));
    t.uniformDigest = c.take<uint64_t>((size_t)kBakeLevels * 4);
    t.arrayHist = c.take<uint32_t>(kBakeLevels); t.indexHist = c.take<uint32_t>(kBakeLevels); t.err = c.take<uint32_t>(1);
    t.fine = c.take<unsigned long long>(kBakeFineWords);
    t.scratch = c.take<uint8_t>(scratchBytes); t.scratchBytes = scratchBytes;
    if (sharded) { t.meta = c.take<uint32_t>(n * 4); t.owner = c.take<uint8_t>(n); t.cofs = c.take<uint64_t>(n); t.totals = c.take<uint64_t>(kBakeMaxRanks); }
    if (streamed) {
        t.placed = c.take<uint64_t>(n); t.cursor = c.take<unsigned long long>(1); t.streamCtl = c.take<uint32_t>(kBakeStreamCtlWords);
        t.uv2 = c.take<float>(n * 6); t.states2 = c.take<uint8_t>(n * kBakePreviewSlotBytes); t.ofs2 = c.take<uint64_t>(n);
        t.mask2 = c.take<uint32_t>(n); t.early = c.take<uint8_t>(n); t.earlyList = c.take<uint32_t>(n); t.earlyLead = c.take<uint32_t>(n); t.fine2 = c.take<unsigned long long>(kBakeFineWords);
    }
    t.bytes = (size_t)(c.at - base);
    return t;
}

// ---- the decisions of a bake that follow from its counters alone (SetupCounters after the triage): bake_core's stages call them (omm_host.cpp) ----
// rank ranges of the per-level active lists: rank r owns [b[l][r], b[l][r + 1]) of level l (single GPU: world 1, every range is the whole level group)
inline void rank_ranges(const uint32_t* activeStart, uint32_t rank, uint32_t world, uint32_t (*b)[kBakeMaxRanks + 1], uint32_t* first, uint32_t* count)
{
    for (int l = 0; l < kBakeLevels; ++l) {
        const uint64_t a = activeStart[l], cnt = activeStart[l + 1] - activeStart[l];
        for (uint32_t r = 0; r <= world; ++r) b[l][r] = (uint32_t)(a + cnt * r / world);
        first[l] = b[l][rank]; count[l] = b[l][rank + 1] - b[l][rank];
    }
}

// The classification time is estimated from the two quantities that drive it: micro-triangles (sub-texel ones, mostly culled: 2.5e-10 ms each -- 27 ms for
// 6.5e10, 128 ms for 6.0e11 measured) and texels under the triangles' boxes (micro-triangles of several texels walk them: 4e-9 ms each -- 55 ms for 1.4e10
// measured on asset-sized cards, where streaming the 0.28 GB result made the bake 10 ms SLOWER).
constexpr double kMsPerMicroTriangle = 2.5e-10, kMsPerWorkloadTexel = 4e-9;
inline double classify_estimate_ms(double microTriangles, uint64_t workload) { return kMsPerMicroTriangle * microTriangles + kMsPerWorkloadTexel * (double)workload; }
constexpr uint64_t kStreamMinStateBytes = 64ull << 20;   // a streamed result from 64 MiB of packed states on ...
constexpr int kStreamRangeShift = 25;                    // ... one range per 32 MiB ...
constexpr uint32_t kBakeMaxStreamRanges = 32;            // ... at most kMaxStreamRanges (round 3, classification-bound, at 1.27 GB: 8 / 16 / 24 / 32 ranges = 38.4 / 36.7 / 36.2 / 36.2 ms;
                                                         //     round 4, copy-bound: 12 / 16 / 24 / 32 ranges = 32.4 / 31.8 / 31.0 / 30.9 ms)
constexpr double kLinkBytesPerMs = 57e6;                 // ~57 GB/s over PCIe
constexpr double kStreamClassifyShare = 0.25;            // streaming costs the classification about a quarter of its time (5 instead of 6 workgroups per CU, the placement kernels next to it)
// the streamed against the compressed transfer (round 5: the codec stream over the link, expanded by the helper threads AFTER the bake), both priced from the same two
// quantities, with this round's rates (1.35e-10 ms per micro-triangle: 8.8 ms for 6.5e10, 88 for 6.0e11) and 65 % of the packed states as the result (what is left
// after promotion and dedup at the metric configuration):
//     streamed    6 + max(1.15 classification + 2.7 (preview), result / 57 GB/s)       c2: 28.3 (29.4 measured)   configs[4]: 110 (was 118 at 95 ms)
//     compressed  3.3 + classification + result / 150 GB/s + codec (0.63 ms per GB)       c2: 18.4 (17 - 20)         configs[4]: 117 (124)
// -- a long classification hides the whole copy, a short one is better off with every workgroup on the chip and the expansion behind it.
constexpr double kPricedMsPerMicroTriangle = 1.35e-10, kResultShareOfStates = 0.65;
constexpr double kStreamedFixedMs = 6.0, kStreamedClassifyFactor = 1.15, kStreamedPreviewMs = 2.7;
constexpr double kCompressedFixedMs = 3.3, kCompressedBytesPerMs = 150e6, kCodecMsPerByte = 0.63e-9;
// Ranges of a streamed result (0: not streamed) for a bake that is eligible for one.  Worth it when the packed states are large enough for the copy to matter,
// only when the copy is worth hiding (it saves at most the copy), and, when the compressed transfer is on offer too, only when streaming wins.  A forced count
// (the knob) is only clamped.
inline uint32_t stream_range_count(uint64_t stateBytes, double microTriangles, uint64_t workload, bool compressedAvailable, bool forced, uint32_t chunksWanted)
{
    uint32_t k = chunksWanted;
    if (!forced) {
        k = stateBytes >= kStreamMinStateBytes ? (uint32_t)(stateBytes >> kStreamRangeShift) : 0u; if (k > kBakeMaxStreamRanges) k = kBakeMaxStreamRanges;
        const double classifyMs = classify_estimate_ms(microTriangles, workload), copyMs = (double)stateBytes / kLinkBytesPerMs;
        if (copyMs <= kStreamClassifyShare * classifyMs) k = 0;
        if (k && compressedAvailable) {
            const double cMs = kPricedMsPerMicroTriangle * microTriangles + kMsPerWorkloadTexel * (double)workload, resultBytes = kResultShareOfStates * (double)stateBytes;
            const double streamedMs = kStreamedFixedMs + std::max(kStreamedClassifyFactor * cMs + kStreamedPreviewMs, resultBytes / kLinkBytesPerMs), compressedMs = kCompressedFixedMs + cMs + resultBytes / kCompressedBytesPerMs + resultBytes * kCodecMsPerByte;
            if (compressedMs <= streamedMs) k = 0;
        }
    }
    return k > kBakeMaxStreamRanges ? kBakeMaxStreamRanges : k;
}
// how long the placement stream waits for a range before it gives the stream up: 100 x the estimate of the whole classification, never below 4 s
inline double stream_wait_seconds(double microTriangles, uint64_t workload) { return 4.0 + 100.0 * 1e-3 * classify_estimate_ms(microTriangles, workload); }

// Deferred generic pass (bake_kernels.hip: classify_generic): for bakes whose cost is in the texels under their micro-triangles, not in their number -- the
// same two terms as above.  mode: ommxBakerKnob_GenericPass (0 = by cost, 1 = never, 2 = always).
inline bool generic_pass_wanted(uint64_t mode, double microTriangles, uint64_t workload)
{
    return mode == 2 || (mode == 0 && kMsPerWorkloadTexel * (double)workload > kMsPerMicroTriangle * microTriangles);
}
constexpr uint64_t kGenericMaxEntries = 256ull << 20;   // at most 2 GB of entries (a tile that finds no room walks its micro-triangles itself)
inline uint64_t generic_pass_capacity(uint64_t stateBytes, int storeBits)
{
    const uint64_t n = stateBytes * 8ull / (uint64_t)storeBits;   // every micro-triangle of every active item ...
    return n > kGenericMaxEntries ? kGenericMaxEntries : n;       // ... up to the cap
}

// stride that interleaves a level's active list of cnt >= 3 items across the ranks (tail_kernels.hip: shard_interleave): golden-ratio start, the next number
// coprime to cnt (cnt - 1 always is: terminates), already reduced % cnt
inline uint32_t interleave_stride(uint32_t cnt)
{
    uint32_t stride = (uint32_t)((double)cnt * 0.6180339887498949); if (stride < 1) stride = 1;
    auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t t = x % y; x = y; y = t; } return x; };
    while (gcd(stride, cnt) != 1) ++stride;
    return stride % cnt;
}

// ---- the sharded bake's rules (omm_host.cpp: "multi-GPU sharded bake") ----
inline bool rank_in_world(uint32_t rank, uint32_t worldSize) { return worldSize >= 1 && worldSize <= kBakeMaxRanks && rank < worldSize; }
// bytes between the ranks' contributions in a gathered buffer: the largest of the per-rank totals, padded to 256, never 0
inline uint64_t contribution_stride(const uint64_t* totals, uint32_t world)
{
    uint64_t mx = 0; for (uint32_t r = 0; r < world; ++r) mx = totals[r] > mx ? totals[r] : mx;
    const uint64_t stride = (mx + 255) & ~255ull;
    return stride ? stride : 256;
}
// The all-gather of the block contributions moves in chunks of <= 64 MiB per rank (at most 8 chunks, multiples of 256 bytes), so that the scatter of one
// chunk overlaps the transfer of the next.  knob: ommxBakerKnob_ShardChunkBytes overrides the chunk size (tests use tiny chunks to force blocks across
// chunk boundaries); 0 = unset.
constexpr uint64_t kShardChunkBytes = 64ull << 20, kShardMaxChunks = 8;
inline uint64_t shard_chunk_bytes(uint64_t strideBytes, uint64_t knob)
{
    const uint64_t want = knob ? knob : kShardChunkBytes;
    uint64_t chunks = (strideBytes + want - 1) / want; if (chunks > kShardMaxChunks) chunks = kShardMaxChunks; if (chunks < 1) chunks = 1;
    return ((((strideBytes + chunks - 1) / chunks) + 255) & ~255ull);
}
// the chunks [lo, hi) of [0, strideBytes) in order: `for (ShardChunks w(stride, knob); w.next();)`; a block that straddles a boundary is placed in pieces
struct ShardChunks {
    uint64_t strideBytes, chunkBytes, lo = 0, hi = 0;
    ShardChunks(uint64_t strideBytes_, uint64_t knob) : strideBytes(strideBytes_), chunkBytes(shard_chunk_bytes(strideBytes_, knob)) {}
    bool next() { lo = hi; hi = lo + chunkBytes < strideBytes ? lo + chunkBytes : strideBytes; return lo < hi; }   // false: the first empty chunk
};
// The exchange arena of a sharded bake: this rank's contribution, and for the one-call form (async) the gather staging of all ranks' raw chunks, this rank's
// codec stream of at most half the contribution, the gathered streams, the stream's size word and the codec's count / scan scratch (it grows with the
// contribution -- a word per 4 KiB of it plus rocPRIM's -- while the bake's own scratch is sized from the triangle count: a few large blocks need more).
// Sized and carved by ONE traversal, like the tables above; `bytes` includes a slack of 256 bytes (async: 1 KiB) behind the last slot.
struct ExchangeArena {
    uint8_t *contrib, *gathered, *comp, *gatherComp; uint32_t* compSize; uint8_t* codecScratch;   // all but contrib: null in the synchronous form
    size_t compCap, codecScratchBytes;   // of comp (gatherComp: x world), of codecScratch
    size_t bytes;                        // to reserve, from the base
};
inline ExchangeArena carve_exchange_arena(uintptr_t base, uint64_t strideBytes, uint32_t world, bool async, size_t codecScratchWanted)
{
    ExchangeArena x = ExchangeArena(); CarveCursor c{ base };
    x.contrib = c.take<uint8_t>((size_t)strideBytes);
    if (async) {
        x.compCap = pad256((size_t)(strideBytes / 2) + 4096); x.codecScratchBytes = pad256(codecScratchWanted);
        x.gathered = c.take<uint8_t>((size_t)strideBytes * world + 4096);
        x.comp = c.take<uint8_t>(x.compCap); x.gatherComp = c.take<uint8_t>(x.compCap * world);
        x.compSize = c.take<uint32_t>(1); x.codecScratch = c.take<uint8_t>(x.codecScratchBytes);
    }
    x.bytes = (size_t)(c.at - base) + (async ? 1024 : 256);
    return x;
}
// rank r's share [lo, hi) of the `words` metadata words that N ranks sum through host memory (ommCpuBake over several devices)
inline void meta_sum_share(size_t words, uint32_t r, uint32_t N, size_t* lo, size_t* hi) { *lo = words * r / N; *hi = words * (r + 1) / N; }
// what a rank of that bake sends over its link: its codec stream, or -- when the stream did not shrink below `cap`, or holds no more than its `offRaw`
// bytes of tables -- the blocks of its contribution as they are
struct RankSend { bool raw; uint64_t bytes; };
inline RankSend rank_send(uint64_t streamBytes, uint64_t cap, uint64_t offRaw, uint64_t contributionBytes)
{
    const bool raw = streamBytes > cap || streamBytes < offRaw;
    return RankSend{ raw, raw ? contributionBytes : streamBytes };
}
// the host scatter's ranges of OMMs for the helper threads: range t = [cut[t], cut[t + 1]), each of at least 2 MiB of blocks but the last; first cut 0, last cut E
constexpr uint64_t kScatterRangeBytes = 2ull << 20;
inline std::vector<uint32_t> scatter_cuts(const uint32_t* sizes, uint32_t E)
{
    std::vector<uint32_t> cut; cut.push_back(0);
    uint64_t acc = 0; for (uint32_t j = 0; j < E; ++j) { acc += sizes[j]; if (acc >= kScatterRangeBytes) { cut.push_back(j + 1); acc = 0; } }
    if (cut.back() != E) cut.push_back(E);
    return cut;
}

// ---- the states arena of a bake: packed states of the active items | queue of open tiles | its control words | staging copy of a streamed result |
//      deferred generic pass: count word (256 B), then the entries (8 bytes each).  Sized and carved by ONE traversal, like the tables above. ----
constexpr size_t kBakeClassifyCtlWords = 512;   // kClassifyCtlWords
struct BakeStates {
    uint8_t *states, *tileQueue; uint32_t* queueCtl; uint8_t *stage, *genericCount; uint64_t* genericEntries;   // stage / generic*: null when absent
    size_t stateBytes;   // of `states` (and of `stage`): at least 256
    size_t bytes;        // end of the last slot, from the base
};
inline BakeStates carve_bake_states(uintptr_t base, uint64_t packedStateBytes, size_t queueBytes, bool streamed, uint64_t genericCapacity)
{
    BakeStates s = BakeStates(); CarveCursor c{ base };
    s.stateBytes = pad256(packedStateBytes ? (size_t)packedStateBytes : 256);
    s.states = c.take<uint8_t>(s.stateBytes);
    s.tileQueue = c.take<uint8_t>(queueBytes);
    s.queueCtl = c.take<uint32_t>(kBakeClassifyCtlWords);
    if (streamed) s.stage = c.take<uint8_t>(s.stateBytes);
    if (genericCapacity) { s.genericCount = c.take<uint8_t>(256); s.genericEntries = c.take<uint64_t>((size_t)genericCapacity); }
    s.bytes = (size_t)(c.at - base);
    return s;
}

// ---- the final read-backs in the arena's pinned host block: [0, 256) counters, [256, 512) tail summary, from 1 KiB the span [arrayHist, end of fine), the
//      classification's control words, the three words of the generic pass.  !fits: they go to pageable memory instead. ----
constexpr size_t kBakeHostBlockBytes = 64u << 10;   // kHostBlockBytes
constexpr size_t kGenericReadbackBytes = 3 * sizeof(unsigned long long);   // reservations (incl. null padding), the pass's cursor, micro-triangles it classified
struct ReadbackSlots { size_t spanAt, ctlAt, genAt; bool fits; };
inline ReadbackSlots readback_slots(size_t spanBytes, size_t blockBytes = kBakeHostBlockBytes)
{
    ReadbackSlots s; s.spanAt = 1024; s.ctlAt = s.spanAt + pad256(spanBytes); s.genAt = s.ctlAt + sizeof(uint32_t) * kBakeClassifyCtlWords;
    s.fits = s.genAt + kGenericReadbackBytes <= blockBytes;
    return s;
}

// classify_tiles launches: one per level below 5, one for level 5, ONE for all levels >= 6 (bake_kernels.hip)
inline uint32_t classify_launches(const uint32_t* activeStart)
{
    uint32_t n = 0; bool big = false;
    for (int l = 0; l < kBakeLevels; ++l) { const bool any = activeStart[l + 1] != activeStart[l]; if (l < 6) n += any; else big = big || any; }
    return n + big;
}
// every work item outside the active lists is uniform, and uniform items of one level and state share a digest: at most 13 x 4 of those
inline uint32_t max_distinct_digests(uint32_t activeItems) { return activeItems + 64u; }
} // namespace ommx
