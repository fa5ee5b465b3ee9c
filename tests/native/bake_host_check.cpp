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

int main()
{
    index_formats();
    histograms();
    result_descs();
    raw_inputs();
    carve();
    printf("ok %ld\n", g_checks);
    return 0;
}
