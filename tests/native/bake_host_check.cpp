// The host-side rules of a bake (omm_amd/csrc/bake_host.h) at the smallest cases at which each can go wrong; built with AddressSanitizer and UBSan by
// tests/test_bake_host.py.  Prints "ok <number of checks>".
#include "bake_host.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ommx;

static long g_checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } ++g_checks; } while (0)

static size_t p256(size_t b) { return (b + 255) / 256 * 256; }   // (written differently from the header's on purpose)

static void index_formats()
{
    const uint32_t T[6] = { 0, 1, 127, 128, 32767, 32768 };
    const ommIndexFormat I8 = ommIndexFormat_UINT_8, I16 = ommIndexFormat_UINT_16, I32 = ommIndexFormat_UINT_32;
    // per triangle count: plain | Allow8BitIndices | Force32BitIndices | both
    const ommIndexFormat want[6][4] = {
        { I16, I8, I32, I32 },    // 0
        { I16, I8, I32, I32 },    // 1
        { I16, I8, I32, I32 },    // 127: the last count an int8 index holds
        { I16, I16, I32, I32 },   // 128
        { I16, I16, I32, I32 },   // 32767: the last count an int16 index holds
        { I32, I32, I32, I32 },   // 32768
    };
    for (int t = 0; t < 6; ++t)
        for (int k = 0; k < 4; ++k) {
            const uint32_t flags = ((k & 1) ? (uint32_t)ommCpuBakeFlags_Allow8BitIndices : 0u) | ((k & 2) ? (uint32_t)ommCpuBakeFlags_Force32BitIndices : 0u)
                                 | (uint32_t)ommCpuBakeFlags_EnableInternalThreads | kBakeFlag_EnableEdgeHeuristic;   // (unrelated bits must not matter)
            CHECK(index_format_for(T[t], flags) == want[t][k], "T=%u case %d", T[t], k);
        }
    CHECK(index_bytes(I8) == 1 && index_bytes(I16) == 2 && index_bytes(I32) == 4, "bytes per index");
    // the flag names are the bits the reference uses (omm.h:298-334, bake_cpu_impl.cpp:43-48)
    CHECK(ommCpuBakeFlags_Force32BitIndices == 4 && ommCpuBakeFlags_Allow8BitIndices == 64 && kBakeFlag_EnableAABBTesting == 128 && kBakeFlag_DisableLevelLineIntersection == 256 &&
          kBakeFlag_DisableFineClassification == 512 && kBakeFlag_NearDuplicateBruteForce == 1024 && kBakeFlag_EnableEdgeHeuristic == 2048, "flag bits");
}

struct Entry { uint32_t count; int level; };
static void histogram_case(const uint32_t* hist, const std::vector<Entry>& wantArray, const std::vector<Entry>& wantIndex)
{
    for (int bits = 1; bits <= 2; ++bits) {
        ommCpuOpacityMicromapUsageCount a[2 * kBakeLevels + 1], x[2 * kBakeLevels + 1];
        memset(a, 0xEE, sizeof a); memset(x, 0xEE, sizeof x);
        uint32_t nA = 99, nI = 99;
        compact_histograms(hist, bits, a, x, &nA, &nI);
        CHECK(nA == wantArray.size() && nI == wantIndex.size(), "counts %u %u", nA, nI);
        for (size_t k = 0; k < wantArray.size(); ++k)
            CHECK(a[k].count == wantArray[k].count && a[k].subdivisionLevel == wantArray[k].level && a[k].format == bits, "array entry %zu", k);
        for (size_t k = 0; k < wantIndex.size(); ++k)
            CHECK(x[k].count == wantIndex[k].count && x[k].subdivisionLevel == wantIndex[k].level && x[k].format == bits, "index entry %zu", k);
        CHECK(a[nA].count == 0xEEEEEEEEu && x[nI].count == 0xEEEEEEEEu, "nothing is written behind the lists");
    }
}
static void histograms()
{
    uint32_t h[2 * kBakeLevels];
    memset(h, 0, sizeof h);
    histogram_case(h, {}, {});                                             // all zero
    h[5] = 7; h[kBakeLevels + 3] = 9;
    histogram_case(h, { { 7, 5 } }, { { 9, 3 } });                         // one level
    memset(h, 0, sizeof h);
    h[0] = 1; h[12] = 2; h[kBakeLevels + 0] = 3; h[kBakeLevels + 12] = 0xFFFFFFFFu;
    histogram_case(h, { { 1, 0 }, { 2, 12 } }, { { 3, 0 }, { 0xFFFFFFFFu, 12 } });   // the first and the last level only
    std::vector<Entry> allA, allI;
    for (int l = 0; l < kBakeLevels; ++l) { h[l] = 100u + (uint32_t)l; h[kBakeLevels + l] = 200u + (uint32_t)l; allA.push_back({ 100u + (uint32_t)l, l }); allI.push_back({ 200u + (uint32_t)l, l }); }
    histogram_case(h, allA, allI);                                         // every level, ascending
    uint32_t lc[kBakeLevels]; memset(lc, 0, sizeof lc);
    CHECK(micro_triangles_of(lc) == 0, "no items");
    lc[0] = 3; lc[1] = 2; lc[12] = 0xFFFFFFFFu;
    CHECK(micro_triangles_of(lc) == 3ull + 8ull + 0xFFFFFFFFull * 16777216ull, "4^level per item, in 64 bits");
}

static void result_descs()
{
    ommCpuOpacityMicromapUsageCount ah[2 * kBakeLevels], ih[2 * kBakeLevels];
    ommCpuOpacityMicromapDesc descs[2]; uint8_t array[64]; int32_t index[4];
    const size_t lists[4] = { 0, 13, 26, 27 }, wantCount[4] = { 0, 13, 26, 26 };   // 27 entries do not fit the lists: clamped
    for (int omms = 0; omms < 2; ++omms)
        for (int k = 0; k < 4; ++k) {
            ommCpuBakeResultDesc d; memset(&d, 0xEE, sizeof d);
            fill_result_desc(&d, array, 64, descs, omms ? 2u : 0u, index, 4, ommIndexFormat_UINT_16, ah, lists[k], ih, lists[3 - k]);
            CHECK(d.arrayData == (omms ? array : nullptr) && d.arrayDataSize == (omms ? 64u : 0u), "array of a bake with%s OMMs", omms ? "" : "out");
            CHECK(d.descArray == (omms ? descs : nullptr) && d.descArrayCount == (omms ? 2u : 0u), "descriptors");
            CHECK(d.indexBuffer == index && d.indexCount == 4 && d.indexFormat == ommIndexFormat_UINT_16, "index buffer");
            CHECK(d.descArrayHistogram == ah && d.descArrayHistogramCount == wantCount[k], "array histogram of %zu entries", lists[k]);
            CHECK(d.indexHistogram == ih && d.indexHistogramCount == wantCount[3 - k], "index histogram of %zu entries", lists[3 - k]);
        }
}

static void raw_inputs()
{
    struct Uv { ommTexCoordFormat format; uint32_t stride, wantStride; size_t element; };
    const Uv uvs[10] = {
        { ommTexCoordFormat_UV32_FLOAT, 0, 8, 8 }, { ommTexCoordFormat_UV32_FLOAT, 8, 8, 8 }, { ommTexCoordFormat_UV32_FLOAT, 12, 12, 8 }, { ommTexCoordFormat_UV32_FLOAT, 9, 9, 8 },
        { ommTexCoordFormat_UV16_UNORM, 0, 4, 4 }, { ommTexCoordFormat_UV16_UNORM, 4, 4, 4 }, { ommTexCoordFormat_UV16_UNORM, 6, 6, 4 },
        { ommTexCoordFormat_UV16_FLOAT, 0, 4, 4 }, { ommTexCoordFormat_UV16_FLOAT, 4, 4, 4 }, { ommTexCoordFormat_UV16_FLOAT, 6, 6, 4 },
    };
    struct Ix { ommIndexFormat format; size_t bytes; };
    const Ix ixs[3] = { { ommIndexFormat_UINT_8, 1 }, { ommIndexFormat_UINT_16, 2 }, { ommIndexFormat_UINT_32, 4 } };
    struct Mesh { uint32_t tris, maxIndex; };
    const Mesh meshes[3] = { { 0, 0 }, { 1, 2 }, { 100, 255 } };   // (the last: regions longer than one 256-byte unit)
    const uint8_t levels[100] = { 0 };
    for (const Uv& u : uvs) for (const Ix& x : ixs) for (const Mesh& m : meshes) for (int withLevels = 0; withLevels < 2; ++withLevels) {
        ommCpuBakeInputDesc d; memset(&d, 0, sizeof d);
        d.texCoordFormat = u.format; d.texCoordStrideInBytes = u.stride; d.indexFormat = x.format; d.indexCount = 3 * m.tris; d.subdivisionLevels = withLevels ? levels : nullptr;
        CHECK(uv_stride(d) == u.wantStride, "stride %u of format %d", u.stride, (int)u.format);
        const RawInputLayout L = raw_input_layout(d, m.tris, m.maxIndex);
        CHECK(L.uvBytes == (m.tris ? (size_t)u.wantStride * m.maxIndex + u.element : 0), "uvBytes %zu", L.uvBytes);
        CHECK(L.idxBytes == x.bytes * 3 * m.tris && L.lvlBytes == (withLevels ? m.tris : 0u), "idxBytes %zu lvlBytes %zu", L.idxBytes, L.lvlBytes);
        CHECK(L.offUv % 256 == 0 && L.offIdx % 256 == 0 && L.offLvl % 256 == 0, "offsets are multiples of 256");
        CHECK(L.offUv == 0 && L.offUv + L.uvBytes <= L.offIdx && L.offIdx + L.idxBytes <= L.offLvl && L.offLvl + L.lvlBytes + 256 <= L.total, "regions are disjoint, slack behind the last");
        CHECK(L.total == p256(L.uvBytes) + p256(L.idxBytes) + p256(L.lvlBytes) + 256, "total %zu", L.total);
    }
}

struct Region { const char* name; uintptr_t at; size_t bytes; };
static std::vector<Region> regions_of(const BakeTables& t, size_t n, bool sharded, bool streamed)
{
    std::vector<Region> r;
#define REGION(field, count) r.push_back(Region{ #field, (uintptr_t)t.field, (size_t)(count) * sizeof(*t.field) })
    REGION(uv, n * 6); REGION(level, n); REGION(degen, n); REGION(active, n); REGION(stateOfs, n); REGION(digests, n); REGION(itemIds, n); REGION(activeIds, n);
    REGION(triToItem, n); REGION(index, n); REGION(mask, n); REGION(known, n); REGION(special, n); REGION(rep, n); REGION(order, n); REGION(dstOfs, n); REGION(sizes, n);
    REGION(itemValue, n); REGION(triArea, n);
    r.push_back(Region{ "counters", (uintptr_t)t.counters, kBakeCountersSlot });
    REGION(uniformDigest, kBakeLevels * 4); REGION(arrayHist, kBakeLevels); REGION(indexHist, kBakeLevels); REGION(err, 1); REGION(fine, kBakeFineWords); REGION(scratch, t.scratchBytes);
    if (sharded) { REGION(meta, n * 4); REGION(owner, n); REGION(cofs, n); REGION(totals, kBakeMaxRanks); }
    if (streamed) {
        REGION(placed, n); REGION(cursor, 1); REGION(streamCtl, kBakeStreamCtlWords); REGION(uv2, n * 6); REGION(states2, n * kBakePreviewSlotBytes); REGION(ofs2, n);
        REGION(mask2, n); REGION(early, n); REGION(earlyList, n); REGION(earlyLead, n); REGION(fine2, kBakeFineWords);
    }
#undef REGION
    return r;
}
static void carve()
{
    const uint32_t items[5] = { 1, 255, 256, 257, 4097 };
    const size_t scratches[2] = { 1000, (size_t)1 << 20 };
    for (uint32_t n : items) for (size_t scratch : scratches) for (int sharded = 0; sharded < 2; ++sharded) for (int streamed = 0; streamed < 2; ++streamed) {
        const BakeTables sized = carve_bake_tables(0, n, scratch, sharded, streamed);   // the sizing pass: offsets from a null base
        uint8_t* block = (uint8_t*)aligned_alloc(256, sized.bytes);                      // (exact size: a slot that runs over is the sanitizer's to report)
        CHECK(block != nullptr, "allocation of %zu bytes", sized.bytes);
        const BakeTables t = carve_bake_tables((uintptr_t)block, n, scratch, sharded, streamed);
        CHECK(t.bytes == sized.bytes && t.scratchBytes == scratch, "both passes agree on the size");
        std::vector<Region> r = regions_of(t, n, sharded, streamed);
        const std::vector<Region> offsets = regions_of(sized, n, sharded, streamed);
        for (size_t k = 0; k < r.size(); ++k) {
            CHECK(r[k].at % 256 == 0, "%s is 256-aligned", r[k].name);
            CHECK(r[k].at - (uintptr_t)block == offsets[k].at, "%s: the sizing pass walks the same offsets", r[k].name);
            CHECK(r[k].at >= (uintptr_t)block && r[k].at + r[k].bytes <= (uintptr_t)block + t.bytes, "%s lies inside the reservation", r[k].name);
            memset((void*)r[k].at, (int)k, r[k].bytes);
        }
        std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.at < b.at; });
        for (size_t k = 0; k + 1 < r.size(); ++k) CHECK(r[k].at + r[k].bytes <= r[k + 1].at, "%s and %s are disjoint", r[k].name, r[k + 1].name);
        CHECK(r.back().at + p256(r.back().bytes) == (uintptr_t)block + t.bytes, "the last slot (%s) ends at the byte count of the sizing pass", r.back().name);
        if (!sharded) CHECK(!t.meta && !t.owner && !t.cofs && !t.totals, "no sharded tables");
        if (!streamed) CHECK(!t.placed && !t.cursor && !t.streamCtl && !t.uv2 && !t.states2 && !t.ofs2 && !t.mask2 && !t.early && !t.earlyList && !t.earlyLead && !t.fine2, "no streamed tables");
        // one copy fills the counters and the digest table behind them
        CHECK((uintptr_t)t.uniformDigest == (uintptr_t)t.counters + 256, "uniformDigest == counters + 256");
        // one copy reads back [arrayHist, end of fine)
        CHECK((uintptr_t)t.indexHist == (uintptr_t)t.arrayHist + 256 && (uintptr_t)t.err == (uintptr_t)t.indexHist + 256 && (uintptr_t)t.fine == (uintptr_t)t.err + 256, "arrayHist, indexHist, err, fine are consecutive");
        CHECK(t.readback_bytes() == 768 + kBakeFineWords * 8 && (uintptr_t)t.arrayHist + t.readback_bytes() <= (uintptr_t)block + t.bytes, "the read-back span ends inside the carve");
        // the hand-written sum that carve_bake_tables replaced (bake_core in omm_host.cpp at c66820b): the reservation never grows
        const size_t maxItems = n, i32 = p256(maxItems * 4), i64 = p256(maxItems * 8);
        const size_t shardBytes = sharded ? p256(maxItems * 16) + p256(maxItems) + i64 + p256(8 * 16) : 0;
        const size_t streamBytes = streamed ? i64 + 512 + p256(maxItems * 24) + p256(maxItems * 256) + i64 + i32 * 3 + p256(maxItems) + p256(8 * 256 * 16) : 0;
        const size_t need = p256(maxItems * 24) + 3 * p256(maxItems) + i64 * 2 + i32 * 13 + 256 + 4096 + p256(8 * 256 * 16) + p256(scratch) + shardBytes + streamBytes;
        CHECK(t.bytes <= need, "%zu bytes reserved, %zu before", t.bytes, need);
        free(block);
    }
}

// ---- the decisions and layouts of bake_core's stages: each held to the expression it had inline in bake_core (omm_host.cpp at a8c6db0), restated verbatim ----
static void rank_range_rules()
{
    const uint32_t worlds[5] = { 1, 2, 3, 8, 16 };
    for (uint32_t world : worlds) {
        const uint32_t counts[5] = { 0, 1, world - 1, world + 1, 1000003 };
        uint32_t activeStart[kBakeLevels + 1]; activeStart[0] = 7;   // (the lists need not start at zero for the rule to hold)
        for (int l = 0; l < kBakeLevels; ++l) activeStart[l + 1] = activeStart[l] + counts[(l + world) % 5];
        uint32_t end[kBakeLevels];
        for (int l = 0; l < kBakeLevels; ++l) end[l] = activeStart[l];
        for (uint32_t rank = 0; rank < world; ++rank) {
            uint32_t b[kBakeLevels][kBakeMaxRanks + 1], first[kBakeLevels], count[kBakeLevels];
            uint32_t wantB[kBakeLevels][kBakeMaxRanks + 1], lvlFirst[kBakeLevels], lvlCount[kBakeLevels];
            memset(b, 0, sizeof b); memset(wantB, 0, sizeof wantB);
            rank_ranges(activeStart, rank, world, b, first, count);
            for (int l = 0; l < kBakeLevels; ++l) {
                const uint64_t a = activeStart[l], cnt = activeStart[l + 1] - activeStart[l];
                for (uint32_t r = 0; r <= world; ++r) wantB[l][r] = (uint32_t)(a + cnt * r / world);
                lvlFirst[l] = wantB[l][rank]; lvlCount[l] = wantB[l][rank + 1] - wantB[l][rank];
            }
            CHECK(memcmp(b, wantB, sizeof b) == 0, "bounds of world %u as seen by rank %u", world, rank);
            CHECK(memcmp(first, lvlFirst, sizeof first) == 0 && memcmp(count, lvlCount, sizeof count) == 0, "range of rank %u of %u", rank, world);
            for (int l = 0; l < kBakeLevels; ++l) { CHECK(first[l] == end[l], "level %d: rank %u of %u starts where the rank before it ends", l, rank, world); end[l] = first[l] + count[l]; }
        }
        for (int l = 0; l < kBakeLevels; ++l) CHECK(end[l] == activeStart[l + 1], "level %d: the last rank of %u ends with the list", l, world);
    }
}

static uint32_t parent_stream_chunks(uint64_t stateBytes, double microAll, uint64_t workload, bool compressedAvailable, bool forced, uint32_t chunksWanted)
{
    const uint32_t kMaxStreamRanges = 32;
    uint32_t k = chunksWanted;
    if (!forced) {
        k = stateBytes >= (64ull << 20) ? (uint32_t)(stateBytes >> 25) : 0u; if (k > kMaxStreamRanges) k = kMaxStreamRanges;
        const double classifyMs = 2.5e-10 * microAll + 4e-9 * (double)workload, copyMs = (double)stateBytes / 57e6;
        if (copyMs <= 0.25 * classifyMs) k = 0;
        if (k && compressedAvailable) {
            const double cMs = 1.35e-10 * microAll + 4e-9 * (double)workload, resultBytes = 0.65 * (double)stateBytes;
            const double streamedMs = 6.0 + std::max(1.15 * cMs + 2.7, resultBytes / 57e6), compressedMs = 3.3 + cMs + resultBytes / 150e6 + resultBytes * 0.63e-9;
            if (compressedMs <= streamedMs) k = 0;
        }
    }
    if (k > kMaxStreamRanges) k = kMaxStreamRanges;
    return k;
}
// the integers around a real workload (none when it is not a workload at all)
static void around(double w, std::vector<uint64_t>& out) { if (w >= 2.0 && w < 1e18) for (int k = -1; k <= 2; ++k) out.push_back((uint64_t)w + (uint64_t)(int64_t)k); }
static void stream_range_rules()
{
    std::vector<uint64_t> states = { 0, (64ull << 20) - 1, 64ull << 20, (64ull << 20) + 1, 1270000000ull, 5400000000ull };   // (the last two: the sizes of the two anchors below)
    for (uint64_t k = 3; k <= 34; ++k) states.push_back(k << 25);   // 32 MiB multiples, up to beyond 32 ranges
    const double micros[3] = { 0.0, 6.5e10, 6.0e11 };
    long copyFlips = 0, priceFlips = 0;
    for (uint64_t sb : states) for (double micro : micros) for (int comp = 0; comp < 2; ++comp) {
        std::vector<uint64_t> workloads = { 0, 14000000000ull };
        // copyMs == 0.25 * classifyMs
        const double copyMs = (double)sb / 57e6;
        const size_t copyAt = workloads.size();
        around((4.0 * copyMs - 2.5e-10 * micro) / 4e-9, workloads);
        // compressedMs == streamedMs, on either branch of the max: 0.15 cMs == X - 5.4 (the classification hides the copy) | cMs == 2.7 + copy - X (it does not)
        const double r = 0.65 * (double)sb, X = r / 150e6 + r * 0.63e-9;
        const size_t priceAt = workloads.size();
        around(((X - 5.4) / 0.15 - 1.35e-10 * micro) / 4e-9, workloads);
        around((2.7 + r / 57e6 - X - 1.35e-10 * micro) / 4e-9, workloads);
        long wrong = 0;
        for (uint64_t w : workloads) wrong += stream_range_count(sb, micro, w, comp != 0, false, 0) != parent_stream_chunks(sb, micro, w, comp != 0, false, 0);
        CHECK(wrong == 0, "%ld of %zu workloads at %llu bytes of states, %g micro-triangles, compressed transfer %d", wrong, workloads.size(), (unsigned long long)sb, micro, comp);
        // (the points do straddle the thresholds: the decision differs between the two sides at some of them)
        if (priceAt - copyAt == 4 && !comp) copyFlips += stream_range_count(sb, micro, workloads[copyAt], false, false, 0) != stream_range_count(sb, micro, workloads[copyAt + 3], false, false, 0);
        for (size_t at = priceAt; at + 4 <= workloads.size() && comp; at += 4) priceFlips += stream_range_count(sb, micro, workloads[at], true, false, 0) != stream_range_count(sb, micro, workloads[at + 3], true, false, 0);
    }
    CHECK(copyFlips > 0, "no grid point straddles copyMs == 0.25 classifyMs");
    CHECK(priceFlips > 0, "no grid point straddles compressedMs == streamedMs");
    const uint32_t forcedValues[3] = { 1, 3, 32 };
    for (uint32_t f : forcedValues) for (uint64_t sb : states)
        CHECK(stream_range_count(sb, 6.5e10, 0, true, true, f) == f && parent_stream_chunks(sb, 6.5e10, 0, true, true, f) == f, "%u forced ranges at %llu bytes", f, (unsigned long long)sb);
    CHECK(stream_range_count(256, 0.0, 0, false, true, 33) == 32 && parent_stream_chunks(256, 0.0, 0, false, true, 33) == 32, "a forced count is clamped");
    // the two anchors of the pricing (bake_host.h): the metric configuration takes the compressed transfer, a classification of 100 ms streams
    CHECK(stream_range_count(1270000000ull, 6.5e10, 0, true, false, 0) == 0, "c2-like: 6.5e10 micro-triangles, 1.27 GB, compressed transfer on offer");
    CHECK(stream_range_count(5400000000ull, 6.0e11, 1750000000ull, true, false, 0) > 1, "configs[4]-like: 6.0e11 micro-triangles");
}

static void generic_pass_rules()
{
    const double micros[2] = { 6.5e10, 6.0e11 };
    for (uint64_t mode = 0; mode < 3; ++mode) for (double microAll : micros) {
        std::vector<uint64_t> workloads = { 0, 14000000000ull };
        around(2.5e-10 * microAll / 4e-9, workloads);   // both sides of 4e-9 * workload > 2.5e-10 * micro
        CHECK(workloads.size() == 6, "four workloads around the threshold");
        for (uint64_t workload : workloads) {
            const bool wanted = mode == 2 || (mode == 0 && 4e-9 * (double)workload > 2.5e-10 * microAll);
            CHECK(generic_pass_wanted(mode, microAll, workload) == wanted, "mode %llu, %g micro-triangles, workload %llu", (unsigned long long)mode, microAll, (unsigned long long)workload);
        }
    }
    CHECK(!generic_pass_wanted(0, 6.5e10, 0) && generic_pass_wanted(0, 6.5e10, 14000000000ull), "by cost: texels under the micro-triangles against their number");
    CHECK(!generic_pass_wanted(1, 6.5e10, 14000000000ull) && generic_pass_wanted(2, 6.5e10, 0), "never / always");
    for (int storeBits = 1; storeBits <= 2; ++storeBits) {
        const uint64_t onCap = (32ull << 20) * (uint64_t)storeBits;   // bytes of states whose micro-triangles are exactly 256 Mi
        const uint64_t states[7] = { 0, 256, 1ull << 20, onCap - 1, onCap, onCap + 1, 1270000000ull };
        for (uint64_t stateBytes : states) {
            uint64_t genericCapacity = stateBytes * 8ull / (uint64_t)storeBits;
            if (genericCapacity > (256ull << 20)) genericCapacity = 256ull << 20;
            CHECK(generic_pass_capacity(stateBytes, storeBits) == genericCapacity, "%llu bytes of %d-bit states", (unsigned long long)stateBytes, storeBits);
        }
        CHECK(generic_pass_capacity(onCap - 1, storeBits) < (256ull << 20), "below the cap");
        CHECK(generic_pass_capacity(onCap, storeBits) == (256ull << 20), "on the cap");
        CHECK(generic_pass_capacity(onCap + 1, storeBits) == (256ull << 20), "the first size with entries above the cap");
    }
}

static uint32_t gcd_of(uint32_t x, uint32_t y) { while (y) { const uint32_t t = x % y; x = y; y = t; } return x; }
static void interleave_rules()
{
    std::vector<uint32_t> counts;
    for (uint32_t cnt = 3; cnt <= 4096; ++cnt) counts.push_back(cnt);
    const uint32_t large[9] = { 65521u, 1000003u, 16777213u, 2147483647u, 4294967291u, 1u << 16, 1u << 20, 1u << 24, 1u << 31 };   // primes, powers of two
    counts.insert(counts.end(), large, large + 9);
    std::vector<uint8_t> hit;
    for (uint32_t cnt : counts) {
        uint32_t stride = (uint32_t)((double)cnt * 0.6180339887498949); if (stride < 1) stride = 1;
        auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t t = x % y; x = y; y = t; } return x; };
        while (gcd(stride, cnt) != 1) ++stride;
        const uint32_t got = interleave_stride(cnt);
        CHECK(got == stride % cnt, "cnt %u: %u, %u before", cnt, got, stride % cnt);
        CHECK(gcd_of(got, cnt) == 1, "cnt %u: stride %u is not coprime", cnt, got);
        CHECK(got >= 1 && got < cnt, "cnt %u: stride %u", cnt, got);
        if (cnt > 4096) continue;
        hit.assign(cnt, 0);
        for (uint32_t p = 0; p < cnt; ++p) hit[(size_t)((uint64_t)p * got % cnt)]++;
        CHECK(std::count(hit.begin(), hit.end(), 1) == (long)cnt, "cnt %u: p -> p * %u %% cnt is no permutation", cnt, got);
    }
}

static void states_carve()
{
    const uint64_t states[3] = { 256, 1ull << 20, 1270000000ull };
    const size_t queues[3] = { 16, 1000 * 112 + 16, 300000 * 112 + 16 };   // records of kTileRecordBytes + 16
    const uint64_t generics[3] = { 0, 1, 256ull << 20 };
    for (uint64_t hcStateBytes : states) for (size_t queueRaw : queues) for (int streamChunks = 0; streamChunks < 2; ++streamChunks) for (uint64_t genericCapacity : generics) {
        const BakeStates sized = carve_bake_states(0, hcStateBytes, queueRaw, streamChunks != 0, genericCapacity);
        // what bake_core summed by hand
        const size_t stateBytes = p256(hcStateBytes ? (size_t)hcStateBytes : 256), ctlBytes = p256(sizeof(uint32_t) * 512), queueBytes = p256(queueRaw);
        const size_t genericBytes = genericCapacity ? p256((size_t)genericCapacity * 8) + 256 : 0;
        const size_t total = stateBytes + queueBytes + ctlBytes + (streamChunks ? stateBytes : 0) + genericBytes;
        const size_t dTileQueue = stateBytes, dQueueCtl = stateBytes + queueBytes, dStage = stateBytes + queueBytes + ctlBytes, dGeneric = stateBytes + queueBytes + ctlBytes + (streamChunks ? stateBytes : 0);
        CHECK(sized.states == nullptr && (size_t)sized.tileQueue == dTileQueue && (size_t)sized.queueCtl == dQueueCtl && sized.stateBytes == stateBytes && sized.bytes == total &&
              (!streamChunks || (size_t)sized.stage == dStage) && (!genericCapacity || (size_t)sized.genericCount == dGeneric), "offsets and total %zu, %zu before", sized.bytes, total);
        CHECK((sized.stage != nullptr) == (streamChunks != 0), "a staging copy for a streamed result only");
        if (genericCapacity) CHECK((uintptr_t)sized.genericEntries == (uintptr_t)sized.genericCount + 256, "the count word lies 256 bytes before the entries");
        else CHECK(!sized.genericCount && !sized.genericEntries, "no generic pass");
        std::vector<Region> r = { { "states", (uintptr_t)sized.states, sized.stateBytes }, { "tileQueue", (uintptr_t)sized.tileQueue, queueRaw }, { "queueCtl", (uintptr_t)sized.queueCtl, 4 * 512 } };
        if (streamChunks) r.push_back(Region{ "stage", (uintptr_t)sized.stage, sized.stateBytes });
        if (genericCapacity) { r.push_back(Region{ "genericCount", (uintptr_t)sized.genericCount, 256 }); r.push_back(Region{ "genericEntries", (uintptr_t)sized.genericEntries, (size_t)genericCapacity * 8 }); }
        bool apart = r.back().at + p256(r.back().bytes) == sized.bytes;   // (the slots are in carve order: each ends before the next, the last with the reservation)
        for (size_t k = 0; k < r.size(); ++k) apart = apart && r[k].at % 256 == 0 && (k + 1 == r.size() || r[k].at + r[k].bytes <= r[k + 1].at);
        CHECK(apart, "slots are aligned, disjoint and end with the reservation");
        if (sized.bytes > ((size_t)32 << 20)) continue;
        uint8_t* block = (uint8_t*)aligned_alloc(256, sized.bytes);   // (exact size: a slot that runs over is the sanitizer's to report)
        const BakeStates s = carve_bake_states((uintptr_t)block, hcStateBytes, queueRaw, streamChunks != 0, genericCapacity);
        memset(s.states, 1, s.stateBytes); memset(s.tileQueue, 2, queueRaw); memset(s.queueCtl, 3, 4 * 512);
        if (s.stage) memset(s.stage, 4, s.stateBytes);
        if (s.genericCount) { memset(s.genericCount, 5, 256); memset(s.genericEntries, 6, (size_t)genericCapacity * 8); }
        CHECK(block != nullptr && s.states == block && s.bytes == sized.bytes && s.tileQueue == block + dTileQueue && (uint8_t*)s.queueCtl == block + dQueueCtl && s.states[s.stateBytes - 1] == 1 && s.tileQueue[0] == 2,
              "both passes agree, every slot was written end to end");
        free(block);
    }
}

static void readback_and_small_rules()
{
    const size_t actual = 768 + kBakeFineWords * 8;   // BakeTables::readback_bytes
    const size_t spans[6] = { 0, 1, 256, actual, 62208, 62209 };
    for (size_t spanBytes : spans) {
        const size_t spanAt = 1024, ctlAt = spanAt + p256(spanBytes), genAt = ctlAt + sizeof(uint32_t[512]);
        const bool pinnedBack = genAt + sizeof(unsigned long long[3]) <= ((size_t)64u << 10);
        const ReadbackSlots s = readback_slots(spanBytes);
        CHECK(s.spanAt == spanAt && s.ctlAt == ctlAt && s.genAt == genAt && s.fits == pinnedBack, "read-back slots of a span of %zu bytes", spanBytes);
    }
    const ReadbackSlots s = readback_slots(actual);
    CHECK(readback_slots(actual, s.genAt + 24).fits, "the last word ends with the block");
    CHECK(!readback_slots(actual, s.genAt + 23).fits, "the last word ends one byte behind the block");
    CHECK(readback_slots(62208).fits && readback_slots(62208).genAt + 24 + 232 == ((size_t)64 << 10), "the longest span the 64 KiB block takes");
    CHECK(!readback_slots(62209).fits, "one byte more");
    uint32_t activeStart[kBakeLevels + 1];
    for (int only = -1; only <= kBakeLevels; ++only) {   // no level | one level | every level
        activeStart[0] = 5;
        for (int l = 0; l < kBakeLevels; ++l) activeStart[l + 1] = activeStart[l] + ((l == only || only == kBakeLevels) ? 3u : 0u);
        uint32_t classifyLaunches = 0; bool big = false;
        for (int l = 0; l < kBakeLevels; ++l) { const bool any = activeStart[l + 1] != activeStart[l]; if (l < 6) classifyLaunches += any; else big = big || any; }
        classifyLaunches += big;
        CHECK(classify_launches(activeStart) == classifyLaunches, "launches with level %d active", only);
        if (only == -1) CHECK(classifyLaunches == 0, "nothing to classify");
        if (only == 9) CHECK(classifyLaunches == 1, "the levels from 6 on share ONE launch");
        if (only == kBakeLevels) CHECK(classifyLaunches == 7, "six launches below level 6 and the persistent one");
    }
    const double micros[3] = { 0.0, 6.5e10, 6.0e11 }; const uint64_t workloads[2] = { 0, 14000000000ull };
    for (double microAll : micros) for (uint64_t workload : workloads)
        CHECK(stream_wait_seconds(microAll, workload) == 4.0 + 100.0 * 1e-3 * (2.5e-10 * microAll + 4e-9 * (double)workload), "wait for %g micro-triangles, workload %llu", microAll, (unsigned long long)workload);
    CHECK(stream_wait_seconds(0.0, 0) == 4.0, "never below 4 s");
    const uint32_t actives[3] = { 0u, 1u, 0xFFFFFFBFu };
    for (uint32_t active : actives) CHECK(max_distinct_digests(active) == active + 64u, "%u active items", active);
}

// ---- the sharded bake's rules: each held to the expression it had inline in the sharded section of omm_host.cpp (at 01c096a), restated ----
static void shard_rank_and_stride_rules()
{
    for (uint32_t worldSize = 0; worldSize < 18; ++worldSize) for (uint32_t rank = 0; rank < 18; ++rank)
        CHECK(rank_in_world(rank, worldSize) == !(worldSize == 0 || worldSize > 16u || rank >= worldSize), "rank %u of %u", rank, worldSize);
    CHECK(rank_in_world(15, 16) && !rank_in_world(16, 16) && !rank_in_world(0, 17), "at most 16 ranks");
    CHECK(!rank_in_world(0xFFFFFFFFu, 16) && !rank_in_world(0, 0xFFFFFFFFu) && !rank_in_world(0, 0), "far out of range");
    const uint64_t maxima[6] = { 0, 1, 255, 256, 257, (1ull << 32) + 1 }, strides[6] = { 256, 256, 256, 256, 512, (1ull << 32) + 256 };
    const uint32_t worlds[5] = { 1, 2, 3, 8, 16 };
    for (int m = 0; m < 6; ++m) {
        for (uint32_t world : worlds) {
            uint64_t totals[kBakeMaxRanks];
            for (uint32_t r = 0; r < kBakeMaxRanks; ++r) totals[r] = r < world ? maxima[m] / 2 : ~0ull;   // (ranks outside the world must not count)
            totals[(m + world / 2) % world] = maxima[m];
            uint64_t mx = 0; for (uint32_t r = 0; r < world; ++r) mx = totals[r] > mx ? totals[r] : mx;
            uint64_t strideBytes = (mx + 255) & ~255ull; if (strideBytes == 0) strideBytes = 256;
            CHECK(contribution_stride(totals, world) == strideBytes, "largest total %llu of %u ranks", (unsigned long long)maxima[m], world);
        }
        CHECK(contribution_stride(&maxima[m], 1) == strides[m], "a total of %llu bytes", (unsigned long long)maxima[m]);
    }
}

static uint64_t parent_chunk_bytes(uint64_t knob, uint64_t strideBytes)
{
    uint64_t want = 64ull << 20;
    if (const uint64_t v = knob) want = v;
    uint64_t chunks = (strideBytes + want - 1) / want; if (chunks > 8) chunks = 8; if (chunks < 1) chunks = 1;
    return ((((strideBytes + chunks - 1) / chunks) + 255) & ~255ull);
}
struct Chunk { uint64_t lo, hi; };
static void shard_chunk_rules()
{
    const uint64_t M = 64ull << 20;
    const uint64_t strides[7] = { 256, 512, M - 256, M, M + 256, 8 * M, 8 * M + 256 }, knobs[3] = { 0, 256, 4352 };
    for (uint64_t strideBytes : strides) for (uint64_t knob : knobs) {
        const uint64_t chunkBytes = parent_chunk_bytes(knob, strideBytes);
        CHECK(shard_chunk_bytes(strideBytes, knob) == chunkBytes, "chunk size of a stride of %llu, knob %llu", (unsigned long long)strideBytes, (unsigned long long)knob);
        std::vector<Chunk> got;
        for (ShardChunks w(strideBytes, knob); w.next();) got.push_back(Chunk{ w.lo, w.hi });
        // the two loops the walk replaced: the four-phase finish ...
        std::vector<Chunk> finish, rccl;
        for (uint64_t lo = 0; lo < strideBytes; lo += chunkBytes) finish.push_back(Chunk{ lo, lo + chunkBytes < strideBytes ? lo + chunkBytes : strideBytes });
        // ... and the raw exchange of the one-call form
        uint64_t chunks = (strideBytes + chunkBytes - 1) / chunkBytes;
        for (uint64_t k = 0; k < chunks; ++k) {
            const uint64_t lo = k * chunkBytes, hi = lo + chunkBytes < strideBytes ? lo + chunkBytes : strideBytes;
            if (lo >= hi) { chunks = k; break; }
            rccl.push_back(Chunk{ lo, hi });
        }
        bool same = got.size() == finish.size() && got.size() == rccl.size();
        for (size_t k = 0; same && k < got.size(); ++k) same = got[k].lo == finish[k].lo && got[k].hi == finish[k].hi && got[k].lo == rccl[k].lo && got[k].hi == rccl[k].hi;
        CHECK(same, "%zu chunks, %zu and %zu before", got.size(), finish.size(), rccl.size());
        bool tiles = !got.empty() && got.front().lo == 0 && got.back().hi == strideBytes, whole = true;
        for (size_t k = 0; k < got.size(); ++k) {
            tiles = tiles && got[k].lo < got[k].hi && (k == 0 || got[k].lo == got[k - 1].hi);
            whole = whole && (k + 1 == got.size() || (got[k].hi - got[k].lo) % 256 == 0);
        }
        CHECK(tiles, "the chunks tile [0, %llu) without gap or overlap", (unsigned long long)strideBytes);
        CHECK(whole, "every chunk but the last is a multiple of 256 bytes");
        CHECK(got.size() <= kShardMaxChunks, "%zu chunks (one event each)", got.size());
    }
    CHECK(shard_chunk_bytes(M, 0) == M && shard_chunk_bytes(M + 256, 0) == M / 2 + 256, "one chunk up to 64 MiB, two from there");
    CHECK(shard_chunk_bytes(8 * M, 0) == M && shard_chunk_bytes(8 * M + 256, 0) == M + 256, "eight chunks of 64 MiB, then eight larger ones");
    CHECK(shard_chunk_bytes(4352 * 3, 4352) == 4352 && shard_chunk_bytes(4352 * 3, 256) == 1792, "the knob sets the size, the eight chunks bound it");
}

static void exchange_arena()
{
    const uint32_t worlds[3] = { 1, 2, 16 };
    const uint64_t strides[2] = { 256, 1ull << 20 };
    for (int asyncBegin = 0; asyncBegin < 2; ++asyncBegin) for (uint32_t world : worlds) for (uint64_t strideBytes : strides) {
        const size_t scratchWanted = 4 * (size_t)(strideBytes / 4096) + 1234;   // (stands for shard_codec_scratch_bytes: no multiple of 256)
        const ExchangeArena sized = carve_exchange_arena(0, strideBytes, world, asyncBegin != 0, scratchWanted);
        // what sharded_tail summed by hand, and where its six takes landed
        const size_t gatherBytes = asyncBegin ? (size_t)strideBytes * world + 4096 : 0;
        const size_t compCap = asyncBegin ? p256((size_t)(strideBytes / 2) + 4096) : 0;
        const size_t codecScratchBytes = asyncBegin ? p256(scratchWanted) : 0;
        const size_t codecBytes = asyncBegin ? compCap * (world + 1) + 1024 + codecScratchBytes : 0;
        CHECK(sized.bytes == (size_t)strideBytes + 256 + gatherBytes + codecBytes, "%zu bytes reserved, %zu before", sized.bytes, (size_t)strideBytes + 256 + gatherBytes + codecBytes);
        const size_t dGathered = p256((size_t)strideBytes), dComp = dGathered + p256(gatherBytes), dGatherComp = dComp + p256(compCap), dCompSize = dGatherComp + p256(compCap * world), dCodecScratch = dCompSize + 256;
        if (asyncBegin) CHECK(sized.contrib == nullptr && (size_t)sized.gathered == dGathered && (size_t)sized.comp == dComp && (size_t)sized.gatherComp == dGatherComp && (size_t)sized.compSize == dCompSize &&
                              (size_t)sized.codecScratch == dCodecScratch && sized.compCap == compCap && sized.codecScratchBytes == codecScratchBytes, "the offsets of the six takes");
        else CHECK(!sized.contrib && !sized.gathered && !sized.comp && !sized.gatherComp && !sized.compSize && !sized.codecScratch && !sized.compCap && !sized.codecScratchBytes, "the synchronous form has the contribution only");
        uint8_t* block = (uint8_t*)aligned_alloc(256, sized.bytes);   // (exact size: a slot that runs over is the sanitizer's to report)
        const ExchangeArena x = carve_exchange_arena((uintptr_t)block, strideBytes, world, asyncBegin != 0, scratchWanted);
        CHECK(block != nullptr && x.contrib == block && x.bytes == sized.bytes && x.compCap == sized.compCap && x.codecScratchBytes == sized.codecScratchBytes &&
              (!asyncBegin || (x.gathered == block + dGathered && x.comp == block + dComp && x.gatherComp == block + dGatherComp && (uint8_t*)x.compSize == block + dCompSize && x.codecScratch == block + dCodecScratch)),
              "both passes agree");
        std::vector<Region> r = { { "contrib", (uintptr_t)x.contrib, (size_t)strideBytes } };
        if (asyncBegin) {
            r.push_back(Region{ "gathered", (uintptr_t)x.gathered, gatherBytes }); r.push_back(Region{ "comp", (uintptr_t)x.comp, compCap }); r.push_back(Region{ "gatherComp", (uintptr_t)x.gatherComp, compCap * world });
            r.push_back(Region{ "compSize", (uintptr_t)x.compSize, 4 }); r.push_back(Region{ "codecScratch", (uintptr_t)x.codecScratch, codecScratchBytes });
        }
        bool apart = r.back().at + p256(r.back().bytes) + (asyncBegin ? 1024 : 256) == (uintptr_t)block + x.bytes;   // (the slots are in carve order; the arena's slack lies behind the last)
        for (size_t k = 0; k < r.size(); ++k) { apart = apart && r[k].at % 256 == 0 && (k + 1 == r.size() || r[k].at + r[k].bytes <= r[k + 1].at); memset((void*)r[k].at, (int)k + 1, r[k].bytes); }
        CHECK(apart, "slots are aligned, disjoint and end the reservation's slack before its end");
        CHECK(x.contrib[strideBytes - 1] == 1 && (!asyncBegin || (x.gathered[gatherBytes - 1] == 2 && x.codecScratch[codecScratchBytes - 1] == 6)), "every slot was written end to end");
        free(block);
    }
}

static void meta_share_and_send_rules()
{
    const size_t wordCounts[5] = { 0, 1, 4, 7, 4 * (size_t)1000003 };
    const uint32_t worlds[5] = { 1, 2, 3, 8, 16 };
    for (size_t metaWords : wordCounts) for (uint32_t N : worlds) {
        size_t end = 0;
        for (uint32_t r = 0; r < N; ++r) {
            size_t lo = 99, hi = 99; meta_sum_share(metaWords, r, N, &lo, &hi);
            CHECK(lo == metaWords * r / N && hi == metaWords * (r + 1) / N && lo == end && hi >= lo, "share of rank %u of %u in %zu words", r, N, metaWords);
            end = hi;
        }
        CHECK(end == metaWords, "the shares of %u ranks tile [0, %zu)", N, metaWords);
    }
    // a rank's stream of cap 1000 whose tables end at byte 100, next to a contribution of 777 bytes
    const uint64_t sizes[6] = { 0, 99, 100, 101, 1000, 1001 };
    for (uint64_t streamBytes : sizes) {
        const uint64_t cap = 1000, offRaw = 100, total = 777;
        const bool raw = streamBytes > cap || streamBytes < offRaw;
        const uint64_t take = raw ? total : streamBytes;
        const RankSend s = rank_send(streamBytes, cap, offRaw, total);
        CHECK(s.raw == raw && s.bytes == take && s.raw == (streamBytes < 100 || streamBytes > 1000), "a stream of %llu bytes", (unsigned long long)streamBytes);
    }
}

static void scatter_cut_case(const std::vector<uint32_t>& hSizes, const std::vector<uint32_t>& want)
{
    const uint32_t E = (uint32_t)hSizes.size();
    std::vector<uint32_t> cut; cut.push_back(0);
    uint64_t acc = 0; for (uint32_t j = 0; j < E; ++j) { acc += hSizes[j]; if (acc >= ((uint64_t)2 << 20)) { cut.push_back(j + 1); acc = 0; } }
    if (cut.back() != E) cut.push_back(E);
    const std::vector<uint32_t> got = scatter_cuts(hSizes.data(), E);
    CHECK(got == cut, "%u blocks: %zu cuts, %zu before", E, got.size(), cut.size());
    CHECK(got == want, "%u blocks: %zu cuts, %zu expected", E, got.size(), want.size());
    bool sound = got.front() == 0 && got.back() == E && (E ? got.size() >= 2 : got.size() == 1);
    for (size_t t = 0; t + 1 < got.size(); ++t) {
        uint64_t bytes = 0; for (uint32_t j = got[t]; j < got[t + 1]; ++j) bytes += hSizes[j];
        sound = sound && got[t] < got[t + 1] && (t + 2 == got.size() || bytes >= (2u << 20));
    }
    CHECK(sound, "%u blocks: first cut 0, last cut E, no empty range, at least 2 MiB in every range but the last", E);
}
static void scatter_cut_rules()
{
    const uint32_t K = 512u << 10;
    scatter_cut_case({}, { 0 });
    scatter_cut_case({ 16 }, { 0, 1 });
    scatter_cut_case({ 4u << 20 }, { 0, 1 });
    scatter_cut_case(std::vector<uint32_t>(1000, 16u), { 0, 1000 });
    scatter_cut_case({ K, K, K, K }, { 0, 4 });                   // 2 MiB exactly on the last block: no empty range behind it
    scatter_cut_case({ K, K, K, K, K, K, K, K }, { 0, 4, 8 });
    scatter_cut_case({ K, K, K, K - 16, 16, K }, { 0, 5, 6 });
}

int main()
{
    index_formats();
    histograms();
    result_descs();
    raw_inputs();
    carve();
    rank_range_rules();
    stream_range_rules();
    generic_pass_rules();
    interleave_rules();
    states_carve();
    readback_and_small_rules();
    shard_rank_and_stride_rules();
    shard_chunk_rules();
    exchange_arena();
    meta_share_and_send_rules();
    scatter_cut_rules();
    printf("ok %ld\n", g_checks);
    return 0;
}
