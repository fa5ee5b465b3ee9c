// geometry_kernels.hip -- triangles from a micromap.  ommxExtractMicroGeometry cuts every OMM block of a device-resident result into the maximal
// nodes of the bird curve whose micro-triangles all go to one output list (include/omm_mi355x_ext.h has the definition); ommxExpandMicroNodes
// turns such nodes into barycentrics and positions.  The cut is tiered: geo_cut64 (geometry_cut.h) on a lane's 64 micro-triangles, on the wave's
// ballot of the lanes whose word is uniform (a tile: 4096 micro-triangles), and twice more on the tiles' summaries (geo_blocks), which makes the
// twelve quad levels of the largest block.  Tiers are anchored at the micro-triangles, so a block whose level is no multiple of three has its
// partial word at the top.  All counters are integers and every record's place is a prefix sum over a fixed order: nothing depends on arrival.
#include <hip/hip_runtime.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include "geometry_kernels.h"
#include "geometry_cut.h"
#include "result_read.h"
#include "bake_host.h"   // pad256
#include "wave_search.h"
#include "../../include/omm_mi355x_lookup.h"

namespace ommx {

constexpr uint32_t kGeoBlock = 256;
constexpr uint32_t kGeoWaves = kGeoBlock / 64;
constexpr uint32_t kGeoMaxGrid = 1u << 20;       // the wave-per-item kernels stride over what is beyond
constexpr uint32_t kGeoRun = 4;                  // consecutive tiles per wave and turn: one owner search while they stay inside one block
constexpr uint32_t kGeoTileLevels = 6;           // a tile is 4^6 micro-triangles: 64 lanes x 64
constexpr uint32_t kGeoAncestor = 0x80000000u;   // tileAnc: this bit | list << 28 | node

typedef uint32_t GeoVec __attribute__((vector_size(16), may_alias));
typedef uint64_t GeoWord __attribute__((may_alias));

__device__ __forceinline__ unsigned long long shfl_up_ull(unsigned long long v, uint32_t d)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}
// inclusive prefix sum over the wave's lanes in lane order
__device__ __forceinline__ unsigned long long wave_scan_ull(unsigned long long v)
{
    const uint32_t lane = threadIdx.x & 63u;
    #pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) { const unsigned long long t = shfl_up_ull(v, d); if (lane >= d) v += t; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_last_ull(unsigned long long v)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, 63), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

// class of ommOpacityState s (a run-time s: no indexing into the kernel's arguments)
__device__ __forceinline__ uint32_t class_of_state(const GeoArgs& P, uint32_t s)
{
    const uint32_t packed = P.cls[0] | ((uint32_t)P.cls[1] << 8) | ((uint32_t)P.cls[2] << 16) | ((uint32_t)P.cls[3] << 24);
    return (packed >> (8u * s)) & 0xFFu;
}

// the first `n` <= 16 bytes at p, little-endian, by byte loads
__device__ __forceinline__ void load_bytes(const uint8_t* p, uint32_t n, uint64_t* w0, uint64_t* w1)
{
    uint64_t a = 0ull, b = 0ull;
    #pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) { if (j < n) a |= (uint64_t)p[j] << (8u * j); }
    #pragma unroll
    for (uint32_t j = 8; j < 16u; ++j) { if (j < n) b |= (uint64_t)p[j] << (8u * (j - 8u)); }
    *w0 = a; *w1 = b;
}

// One tile of one block, cut by one wave: the lane's word (up to 64 micro-triangles: one 16-byte load in OC1_4_State, 8 bytes in OC1_2_State) and
// the wave's word over the lanes.  tile `tib` of a block of level L is node tib of level L - kl, kl = min(L, 6).
struct TileCut { GeoCut lane, wave; uint32_t k1, k2; };
__device__ __forceinline__ TileCut tile_cut(const GeoArgs& P, const ommCpuOpacityMicromapDesc desc, uint32_t tib)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t L = desc.subdivisionLevel, bits = desc.format;
    const uint32_t kl = L < kGeoTileLevels ? L : kGeoTileLevels, k1 = L < 3u ? L : 3u, k2 = kl - k1;
    const int32_t E = (int32_t)(L < P.emitLevel ? L : P.emitLevel);
    const uint8_t* block = (const uint8_t*)P.result.arrayData + desc.offset;
    TileCut T; T.k1 = k1; T.k2 = k2;
    #pragma unroll
    for (int c = 0; c < 4; ++c) T.lane.start[c] = 0ull;
    T.lane.up1 = 0ull; T.lane.up2 = 0ull; T.lane.whole = kGeoNoClass;
    const bool active = lane < (1u << (2u * k2));
    uint64_t w0 = 0ull, w1 = 0ull;
    bool plain = true; uint32_t state = 0u;
    if (active) {
        if (L >= 3u) {
            const uint32_t wordBytes = 8u * bits;
            const uint8_t* p = block + (uint64_t)((tib << (2u * k2)) + lane) * wordBytes;
            if (bits == 2u && ((uintptr_t)p & 15u) == 0u) { const GeoVec q = *(const GeoVec*)p; w0 = q[0] | ((uint64_t)q[1] << 32); w1 = q[2] | ((uint64_t)q[3] << 32); }
            else if (bits == 1u && ((uintptr_t)p & 7u) == 0u) { w0 = *(const GeoWord*)p; w1 = 0ull; }
            else load_bytes(p, wordBytes, &w0, &w1);
        } else load_bytes(block, ((bits << (2u * L)) + 7u) >> 3, &w0, &w1);   // (a one-byte block's unused bits fall outside the word's 4^k1 entries)
        // a full word in one state (most words of a real result) needs no cut: its class is the state's, whatever the emit level
        const uint64_t rep = bits == 2u ? (w0 & 3ull) * 0x5555555555555555ull : 0ull - (w0 & 1ull);
        plain = L >= 3u && w0 == rep && (bits == 1u || w1 == rep);
        state = (uint32_t)w0 & (bits == 2u ? 3u : 1u);
    }
    if (__ballot(!plain) == 0ull) {          // (the same branch for the whole wave)
        if (active) T.lane.whole = class_of_state(P, state);
    } else if (active) {
        uint64_t m[5];
        geo_class_masks(w0, w1, bits, P.cls, m);
        T.lane = geo_cut64(m, k1, (int32_t)L - E, P.mixed);
    }
    uint64_t mb[5];
    #pragma unroll
    for (uint32_t c = 0; c < 5u; ++c) mb[c] = __ballot(T.lane.whole == c);
    T.wave = geo_cut64(mb, k2, (int32_t)(L - k1) - E, P.mixed);
    return T;
}

// records per list of this lane's share of a tile, 16 bits each (a tile has at most 4096): its own word's and the wave's node that starts at it
__device__ __forceinline__ unsigned long long tile_lane_counts(const TileCut& T)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long packed = 0ull;
    #pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) packed |= (unsigned long long)((uint32_t)__popcll(T.lane.start[c]) + (uint32_t)((T.wave.start[c] >> lane) & 1ull)) << (16u * c);
    return packed;
}

// One lane per descriptor (and one for the scan's closing element): how many tiles the block is cut into -- 0 for a descriptor that fails the bounds
// rule of include/omm_mi355x_lookup.h, which therefore is never read through.
__global__ __launch_bounds__(kGeoBlock) void geo_prepare(ommCpuBakeResultDesc r, unsigned long long* __restrict__ tileStart)
{
    const uint64_t d = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x;
    if (d > r.descArrayCount) return;
    unsigned long long tiles = 0ull;
    if (d < r.descArrayCount) {
        const ommCpuOpacityMicromapDesc desc = r.descArray[d];
        const uint32_t level = desc.subdivisionLevel;
        if (desc_ok(desc, r.arrayDataSize)) tiles = level > kGeoTileLevels ? 1ull << (2u * (level - kGeoTileLevels)) : 1ull;
    }
    tileStart[d] = tiles;
}

// One wave per tile: its per-list record counts and its class.  A block that is one tile is finished here, root included.
__global__ __launch_bounds__(kGeoBlock) void geo_tiles(GeoArgs P, const unsigned long long* __restrict__ tileStart, unsigned long long* __restrict__ tileCounts,
                                                       uint8_t* __restrict__ tileClass, uint32_t* __restrict__ tileOff, uint32_t* __restrict__ tileAnc,
                                                       uint32_t* __restrict__ blockCounts)
{
    const uint32_t D = P.result.descArrayCount, lane = threadIdx.x & 63u;
    const unsigned long long total = tileStart[D];
    uint32_t d = 0u;
    ommCpuOpacityMicromapDesc desc = {};
    const unsigned long long turn = (unsigned long long)gridDim.x * kGeoWaves * kGeoRun;
    for (unsigned long long w0 = ((unsigned long long)blockIdx.x * kGeoWaves + (threadIdx.x >> 6)) * kGeoRun; w0 < total; w0 += turn)
    for (unsigned long long w = w0, end = 0ull, first = 0ull; w < w0 + kGeoRun && w < total; ++w) {
        if (w >= end) { d = owner_of_segment(tileStart, D, w); first = tileStart[d]; end = tileStart[d + 1]; desc = P.result.descArray[d]; }   // (has tiles: it passed the bounds rule)
        const TileCut T = tile_cut(P, desc, (uint32_t)(w - first));
        const unsigned long long sum = wave_last_ull(wave_scan_ull(tile_lane_counts(T)));
        if (lane == 0) {
            tileCounts[w] = sum;
            tileClass[w] = (uint8_t)T.wave.whole;
            if (desc.subdivisionLevel <= kGeoTileLevels) {
                const uint32_t root = T.wave.whole;
                #pragma unroll
                for (uint32_t c = 0; c < 4u; ++c) { blockCounts[4ull * d + c] = (uint32_t)((sum >> (16u * c)) & 0xFFFFu) + (root == c ? 1u : 0u); tileOff[4ull * w + c] = 0u; }
                tileAnc[w] = root < 4u ? kGeoAncestor | (root << 28) : 0u;
            }
        }
    }
}

// One wave per block of more than one tile: the tiers above the tiles (entries: the tiles' classes, nodes of level L - 6), every tile's offset among
// the block's records per list, the node above the tiles that starts at a tile (at most one: a tile swallowed by a uniform ancestor has no records
// of its own and carries the ancestor where it is the ancestor's first tile), and the block's counts.
__global__ __launch_bounds__(kGeoBlock) void geo_blocks(GeoArgs P, const unsigned long long* __restrict__ tileStart, const unsigned long long* __restrict__ tileCounts,
                                                        const uint8_t* __restrict__ tileClass, uint32_t* __restrict__ tileOff, uint32_t* __restrict__ tileAnc,
                                                        uint32_t* __restrict__ blockCounts)
{
    const uint32_t D = P.result.descArrayCount, lane = threadIdx.x & 63u;
    for (uint64_t d = (uint64_t)blockIdx.x * kGeoWaves + (threadIdx.x >> 6); d < D; d += (uint64_t)gridDim.x * kGeoWaves) {
        const unsigned long long t0 = tileStart[d];
        if (tileStart[d + 1] - t0 <= 1ull) continue;
        const uint32_t L = P.result.descArray[d].subdivisionLevel;
        const uint32_t ku = L - kGeoTileLevels, k2 = ku < 3u ? ku : 3u, k1 = ku - k2, n = 1u << (2u * k1);   // up to 64 tiles: one per lane, cut by the ballot
        const int32_t E = (int32_t)(L < P.emitLevel ? L : P.emitLevel);
        const bool active = lane < (1u << (2u * k2));
        const unsigned long long mine = t0 + (unsigned long long)lane * n;
        GeoCut lc;
        #pragma unroll
        for (int c = 0; c < 4; ++c) lc.start[c] = 0ull;
        lc.up1 = 0ull; lc.up2 = 0ull; lc.whole = kGeoNoClass;
        if (active) {
            uint64_t m[5] = { 0ull, 0ull, 0ull, 0ull, 0ull };
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t cl = tileClass[mine + i];
                #pragma unroll
                for (uint32_t c = 0; c < 5u; ++c) m[c] |= cl == c ? 1ull << i : 0ull;
            }
            lc = geo_cut64(m, k1, (int32_t)ku - E, P.mixed);
        }
        uint64_t mb[5];
        #pragma unroll
        for (uint32_t c = 0; c < 5u; ++c) mb[c] = __ballot(lc.whole == c);
        const GeoCut wc = geo_cut64(mb, k2, (int32_t)(ku - k1) - E, P.mixed);
        const uint32_t root = wc.whole;
        // the lane's records per list: its tiles', its word's nodes, the wave's node that starts at it, the root
        uint32_t tot[4];
        #pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) tot[c] = (uint32_t)__popcll(lc.start[c]) + (uint32_t)((wc.start[c] >> lane) & 1ull) + ((lane == 0u && root == c) ? 1u : 0u);
        if (active) for (uint32_t i = 0; i < n; ++i) {
            const unsigned long long tc = tileCounts[mine + i];
            #pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) tot[c] += (uint32_t)((tc >> (16u * c)) & 0xFFFFu);
        }
        const unsigned long long in01 = wave_scan_ull(tot[0] | ((unsigned long long)tot[1] << 32)), in23 = wave_scan_ull(tot[2] | ((unsigned long long)tot[3] << 32));
        uint32_t run[4] = { (uint32_t)in01 - tot[0], (uint32_t)(in01 >> 32) - tot[1], (uint32_t)in23 - tot[2], (uint32_t)(in23 >> 32) - tot[3] };
        const unsigned long long all01 = wave_last_ull(in01), all23 = wave_last_ull(in23);
        if (lane == 0) {
            blockCounts[4ull * d + 0] = (uint32_t)all01; blockCounts[4ull * d + 1] = (uint32_t)(all01 >> 32);
            blockCounts[4ull * d + 2] = (uint32_t)all23; blockCounts[4ull * d + 3] = (uint32_t)(all23 >> 32);
        }
        if (active) for (uint32_t i = 0; i < n; ++i) {
            const unsigned long long tc = tileCounts[mine + i];
            uint32_t anc = 0u;
            #pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) {
                if (lane == 0u && i == 0u && root == c) anc = kGeoAncestor | (c << 28);                                            // node (0, 0)
                else if (i == 0u && ((wc.start[c] >> lane) & 1ull)) anc = kGeoAncestor | (c << 28) | geo_node(wc, lane, ku - k1, 0u);
                else if ((lc.start[c] >> i) & 1ull) anc = kGeoAncestor | (c << 28) | geo_node(lc, i, ku, lane * n);
            }
            tileAnc[mine + i] = anc;
            #pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) {
                tileOff[4ull * (mine + i) + c] = run[c];
                run[c] += (uint32_t)((tc >> (16u * c)) & 0xFFFFu) + ((anc && ((anc >> 28) & 3u) == c) ? 1u : 0u);
            }
        }
    }
}

// One lane per primitive (and one for the scans' closing elements): its record counts per list -- its block's, or one node for a special index --
// and, for the emission, how many tiles its block has.  Primitives that no block answers are counted as skipped.
__global__ __launch_bounds__(kGeoBlock) void geo_primitives(GeoArgs P, const unsigned long long* __restrict__ tileStart, const uint32_t* __restrict__ blockCounts,
                                                            unsigned long long* __restrict__ primCounts, unsigned long long* __restrict__ primTiles,
                                                            GeoTotals* __restrict__ tot)
{
    const uint64_t T = P.result.indexCount, i = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x;
    uint32_t cnt[4] = { 0u, 0u, 0u, 0u };
    unsigned long long tiles = 0ull;
    bool skipped = false;
    if (i < T) {
        const int32_t e = index_entry(P.result.indexBuffer, (int)P.result.indexFormat, i);
        if (e < 0) {
            if (e >= -4) {
                const uint32_t cl = class_of_state(P, (uint32_t)(-(e + 1)));
                #pragma unroll
                for (uint32_t c = 0; c < 4u; ++c) cnt[c] = cl == c ? 1u : 0u;
            } else skipped = true;
        } else if ((uint32_t)e < P.result.descArrayCount && (tiles = tileStart[e + 1] - tileStart[e]) != 0ull) {
            #pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) cnt[c] = blockCounts[4ull * (uint32_t)e + c];
        } else skipped = true;
    }
    const uint32_t nSkipped = (uint32_t)__popcll(__ballot(skipped));
    if ((threadIdx.x & 63u) == 0u && nSkipped) atomicAdd(&tot->skipped, nSkipped);
    if (i > T) return;
    #pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) primCounts[c * (T + 1u) + i] = cnt[c];
    primTiles[i] = tiles;
}

// after the scans: the closing elements are the totals
__global__ void geo_totals(uint64_t T, const unsigned long long* __restrict__ primOff, const unsigned long long* __restrict__ primTileStart, uint32_t withTiles,
                           GeoTotals* __restrict__ tot)
{
    if (threadIdx.x < 4u) tot->counts[threadIdx.x] = primOff[threadIdx.x * (T + 1u) + T];
    if (threadIdx.x == 4u) tot->primTiles = withTiles ? primTileStart[T] : 0ull;
}

struct GeoLists { ommxMicroNode* nodes[4]; };

__device__ __forceinline__ void put_record(ommxMicroNode* list, unsigned long long at, uint32_t prim, uint32_t node)
{
    list[at].primitiveIndex = prim; list[at].node = node;   // (a caller's array is only 4-byte aligned)
}

// the one node (level 0, index 0) of every primitive with a special index
__global__ __launch_bounds__(kGeoBlock) void geo_emit_specials(GeoArgs P, const unsigned long long* __restrict__ primOff, GeoLists out)
{
    const uint64_t T = P.result.indexCount, stride = (uint64_t)gridDim.x * kGeoBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x; i < T; i += stride) {
        const int32_t e = index_entry(P.result.indexBuffer, (int)P.result.indexFormat, i);
        if (e >= 0 || e < -4) continue;
        const uint32_t cl = class_of_state(P, (uint32_t)(-(e + 1)));
        #pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) if (cl == c && out.nodes[c]) put_record(out.nodes[c], primOff[c * (T + 1u) + i], (uint32_t)i, 0u);
    }
}

// One wave per (primitive, tile of its block): the tile's cut again, every record at primitive offset + tile offset + rank in the wave (lane order,
// then entry order within the lane: the order of the first covered micro-triangle).  A tile without records of its own is not read again.
__global__ __launch_bounds__(kGeoBlock) void geo_emit_tiles(GeoArgs P, const unsigned long long* __restrict__ tileStart, const unsigned long long* __restrict__ tileCounts,
                                                            const uint32_t* __restrict__ tileOff, const uint32_t* __restrict__ tileAnc,
                                                            const unsigned long long* __restrict__ primOff, const unsigned long long* __restrict__ primTileStart,
                                                            unsigned long long total, GeoLists out)
{
    const uint64_t T = P.result.indexCount;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long turn = (unsigned long long)gridDim.x * kGeoWaves * kGeoRun;
    uint32_t prim = 0u, d = 0u;
    for (unsigned long long w0 = ((unsigned long long)blockIdx.x * kGeoWaves + (threadIdx.x >> 6)) * kGeoRun; w0 < total; w0 += turn)
    for (unsigned long long w = w0, end = 0ull, first = 0ull, firstTile = 0ull; w < w0 + kGeoRun && w < total; ++w) {
        if (w >= end) {
            prim = owner_of_segment(primTileStart, (uint32_t)T, w); first = primTileStart[prim]; end = primTileStart[prim + 1];
            d = (uint32_t)index_entry(P.result.indexBuffer, (int)P.result.indexFormat, prim);   // (has tiles: a block that passed the bounds rule)
            firstTile = tileStart[d];
        }
        const uint32_t tib = (uint32_t)(w - first);
        const unsigned long long tile = firstTile + tib;
        const uint32_t anc = tileAnc[tile];
        if (anc) {
            const uint32_t c = (anc >> 28) & 3u;
            if (lane == 0 && out.nodes[c]) put_record(out.nodes[c], primOff[c * (T + 1u) + prim] + tileOff[4ull * tile + c], prim, anc & 0x0FFFFFFFu);
            continue;
        }
        if (tileCounts[tile] == 0ull) continue;
        const ommCpuOpacityMicromapDesc desc = P.result.descArray[d];
        const TileCut C = tile_cut(P, desc, tib);
        const unsigned long long own = tile_lane_counts(C), before = wave_scan_ull(own) - own;
        const uint32_t L = desc.subdivisionLevel, laneWord = (tib << (2u * C.k2)) + lane;
        #pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
            if (!out.nodes[c]) continue;
            unsigned long long at = primOff[c * (T + 1u) + prim] + tileOff[4ull * tile + c] + ((before >> (16u * c)) & 0xFFFFull);
            if ((C.wave.start[c] >> lane) & 1ull) put_record(out.nodes[c], at++, prim, geo_node(C.wave, lane, L - C.k1, tib << (2u * C.k2)));
            for (uint64_t s = C.lane.start[c]; s; s &= s - 1ull)
                put_record(out.nodes[c], at++, prim, geo_node(C.lane, (uint32_t)__builtin_ctzll(s), L, laneWord << (2u * C.k1)));
        }
    }
}

// ---- ommxExpandMicroNodes ----
struct ExpandMesh { const uint8_t* positions; uint32_t stride; const void* indices; int indexFormat; uint32_t triangleCount; uint32_t present; };

__global__ __launch_bounds__(kGeoBlock) void expand_micro_nodes(const ommxMicroNode* __restrict__ nodes, uint64_t count, ExpandMesh M,
                                                                float* __restrict__ outBary, float* __restrict__ outPos)
{
    const uint64_t stride = (uint64_t)gridDim.x * kGeoBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x; i < count; i += stride) {
        const uint32_t prim = nodes[i].primitiveIndex, node = nodes[i].node;
        const uint32_t level = node >> 24, index = node & 0xFFFFFFu;
        const bool ok = level <= OMMX_LOOKUP_MAX_LEVEL && index < (1u << (2u * level)) && (!M.present || prim < M.triangleCount);
        float uv[6];
        const float nan = __uint_as_float(0x7FC00000u);
        if (ok) ommx_micro_vertices(index, level, uv);
        else { uv[0] = uv[1] = uv[2] = uv[3] = uv[4] = uv[5] = nan; }
        if (outBary) {
            #pragma unroll
            for (int k = 0; k < 6; ++k) outBary[6ull * i + k] = uv[k];
        }
        if (!outPos) continue;
        float V[3][3];
        if (ok) {
            #pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint64_t at = 3ull * prim + k;
                uint32_t vi;
                if (M.indexFormat == ommIndexFormat_UINT_8) vi = ((const uint8_t*)M.indices)[at];
                else if (M.indexFormat == ommIndexFormat_UINT_16) vi = ((const uint16_t*)M.indices)[at];
                else vi = ((const uint32_t*)M.indices)[at];
                const float* p = (const float*)(M.positions + (uint64_t)M.stride * vi);
                V[k][0] = p[0]; V[k][1] = p[1]; V[k][2] = p[2];
            }
        }
        #pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float u = uv[2 * k], v = uv[2 * k + 1], w = (1.f - u) - v;
            #pragma unroll
            for (int c = 0; c < 3; ++c) outPos[9ull * i + 3 * k + c] = ok ? (V[0][c] * w + V[1][c] * u) + V[2][c] * v : nan;
        }
    }
}

// ---- host side ----
namespace {
struct HeadLayout { size_t totals, tileStart, blockCounts, primCounts, primTiles, scanTemp, scanTempBytes, bytes; };
HeadLayout head_layout(const GeoArgs& a)
{
    HeadLayout L; size_t o = 0;
    const size_t D = a.result.descArrayCount, T = a.result.indexCount;
    L.totals = o; o += pad256(sizeof(GeoTotals));
    L.tileStart = o; o += pad256(sizeof(unsigned long long) * (D + 1));
    L.blockCounts = o; o += pad256(sizeof(uint32_t) * 4 * D);
    L.primCounts = o; o += pad256(sizeof(unsigned long long) * 4 * (T + 1));
    L.primTiles = o; o += pad256(sizeof(unsigned long long) * (T + 1));
    L.scanTempBytes = 0;
    (void)rocprim::exclusive_scan(nullptr, L.scanTempBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, (D > T ? D : T) + 1, rocprim::plus<unsigned long long>());
    L.scanTemp = o; o += pad256(L.scanTempBytes);
    L.bytes = o;
    return L;
}
struct TileLayout { size_t counts, off, anc, cls, bytes; };
TileLayout tile_layout(unsigned long long n)
{
    TileLayout L; size_t o = 0;
    L.counts = o; o += pad256(sizeof(unsigned long long) * (size_t)n);
    L.off = o; o += pad256(sizeof(uint32_t) * 4 * (size_t)n);
    L.anc = o; o += pad256(sizeof(uint32_t) * (size_t)n);
    L.cls = o; o += pad256((size_t)n);
    L.bytes = o;
    return L;
}
uint32_t lane_grid(uint64_t items)
{
    return (uint32_t)((items + kGeoBlock - 1u) / kGeoBlock);
}
uint32_t wave_grid(unsigned long long items)
{
    const unsigned long long blocks = (items + kGeoWaves - 1u) / kGeoWaves;
    return (uint32_t)(blocks < kGeoMaxGrid ? (blocks ? blocks : 1u) : kGeoMaxGrid);
}
hipError_t scan_in_place(const HeadLayout& L, uint8_t* base, unsigned long long* data, size_t n, hipStream_t stream)
{
    size_t tb = L.scanTempBytes;   // (in place: every element is read before it is written)
    return rocprim::exclusive_scan(base + L.scanTemp, tb, data, data, 0ull, n, rocprim::plus<unsigned long long>(), stream);
}
} // namespace

size_t geo_head_bytes(const GeoArgs& a) { return head_layout(a).bytes; }
size_t geo_tile_bytes(unsigned long long tileCount) { return tile_layout(tileCount).bytes; }

#define GEO_CHECK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

hipError_t geo_count_tiles(const GeoArgs& a, void* head, unsigned long long* tileCount, hipStream_t stream)
{
    const HeadLayout L = head_layout(a);
    uint8_t* base = (uint8_t*)head;
    const uint32_t D = a.result.descArrayCount;
    GEO_CHECK(hipMemsetAsync(base + L.totals, 0, sizeof(GeoTotals), stream));
    *tileCount = 0ull;
    if (!D) return hipStreamSynchronize(stream);
    unsigned long long* tileStart = (unsigned long long*)(base + L.tileStart);
    geo_prepare<<<lane_grid((uint64_t)D + 1u), kGeoBlock, 0, stream>>>(a.result, tileStart);
    GEO_CHECK(hipGetLastError());
    GEO_CHECK(scan_in_place(L, base, tileStart, (size_t)D + 1, stream));
    GEO_CHECK(hipMemcpyAsync(tileCount, tileStart + D, sizeof *tileCount, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t geo_count(const GeoArgs& a, void* head, void* tiles, unsigned long long tileCount, bool wantEmit, GeoTotals* out, hipStream_t stream)
{
    const HeadLayout L = head_layout(a);
    const TileLayout TL = tile_layout(tileCount);
    uint8_t* base = (uint8_t*)head; uint8_t* tb = (uint8_t*)tiles;
    const uint32_t D = a.result.descArrayCount;
    const uint64_t T = a.result.indexCount;
    unsigned long long* tileStart = (unsigned long long*)(base + L.tileStart);
    uint32_t* blockCounts = (uint32_t*)(base + L.blockCounts);
    unsigned long long* primCounts = (unsigned long long*)(base + L.primCounts);
    unsigned long long* primTiles = (unsigned long long*)(base + L.primTiles);
    GeoTotals* tot = (GeoTotals*)(base + L.totals);
    if (tileCount) {
        geo_tiles<<<wave_grid((tileCount + kGeoRun - 1u) / kGeoRun), kGeoBlock, 0, stream>>>(a, tileStart, (unsigned long long*)(tb + TL.counts), tb + TL.cls, (uint32_t*)(tb + TL.off),
                                                                 (uint32_t*)(tb + TL.anc), blockCounts);
        GEO_CHECK(hipGetLastError());
        geo_blocks<<<wave_grid(D), kGeoBlock, 0, stream>>>(a, tileStart, (const unsigned long long*)(tb + TL.counts), tb + TL.cls, (uint32_t*)(tb + TL.off),
                                                          (uint32_t*)(tb + TL.anc), blockCounts);
        GEO_CHECK(hipGetLastError());
    }
    geo_primitives<<<lane_grid(T + 1u), kGeoBlock, 0, stream>>>(a, tileStart, blockCounts, primCounts, primTiles, tot);
    GEO_CHECK(hipGetLastError());
    for (uint32_t c = 0; c < 4u; ++c) GEO_CHECK(scan_in_place(L, base, primCounts + c * (T + 1u), (size_t)T + 1, stream));
    if (wantEmit) GEO_CHECK(scan_in_place(L, base, primTiles, (size_t)T + 1, stream));
    geo_totals<<<1, 64, 0, stream>>>(T, primCounts, primTiles, wantEmit ? 1u : 0u, tot);
    GEO_CHECK(hipGetLastError());
    GEO_CHECK(hipMemcpyAsync(out, tot, sizeof(GeoTotals), hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

hipError_t geo_emit(const GeoArgs& a, const void* head, const void* tiles, unsigned long long tileCount, const GeoTotals& totals, const ommxMicroGeometryOutputs& o,
                    hipStream_t stream)
{
    const HeadLayout L = head_layout(a);
    const TileLayout TL = tile_layout(tileCount);
    const uint8_t* base = (const uint8_t*)head; const uint8_t* tb = (const uint8_t*)tiles;
    const uint64_t T = a.result.indexCount;
    const unsigned long long* primOff = (const unsigned long long*)(base + L.primCounts);
    GeoLists lists; bool any = false;
    for (uint32_t c = 0; c < 4u; ++c) {
        lists.nodes[c] = totals.counts[c] ? o.nodes[c] : nullptr;
        any = any || lists.nodes[c] != nullptr;
        if (o.primitiveOffsets[c]) GEO_CHECK(hipMemcpyAsync(o.primitiveOffsets[c], primOff + c * (T + 1u), sizeof(unsigned long long) * (T + 1u), hipMemcpyDeviceToDevice, stream));
    }
    if (any) {
        const uint64_t blocks = (T + kGeoBlock - 1u) / kGeoBlock;
        geo_emit_specials<<<(uint32_t)(blocks < kGeoMaxGrid ? blocks : kGeoMaxGrid), kGeoBlock, 0, stream>>>(a, primOff, lists);
        GEO_CHECK(hipGetLastError());
        if (totals.primTiles) {
            geo_emit_tiles<<<wave_grid((totals.primTiles + kGeoRun - 1u) / kGeoRun), kGeoBlock, 0, stream>>>(a, (const unsigned long long*)(base + L.tileStart), (const unsigned long long*)(tb + TL.counts),
                                                                                  (const uint32_t*)(tb + TL.off), (const uint32_t*)(tb + TL.anc), primOff,
                                                                                  (const unsigned long long*)(base + L.primTiles), totals.primTiles, lists);
            GEO_CHECK(hipGetLastError());
        }
    }
    return hipStreamSynchronize(stream);
}

} // namespace ommx

using namespace ommx;

OMM_MI355X_API ommResult ommxExpandMicroNodes(const ommxMicroNode* nodes, uint64_t count, const ommxMicroMeshDesc* mesh, float* outBarycentrics, float* outPositions,
                                              void* hipStream)
{
    if (outPositions != nullptr && mesh == nullptr) return ommResult_INVALID_ARGUMENT;
    ExpandMesh M; memset(&M, 0, sizeof M);
    if (mesh) {
        if (mesh->indexFormat != ommIndexFormat_UINT_8 && mesh->indexFormat != ommIndexFormat_UINT_16 && mesh->indexFormat != ommIndexFormat_UINT_32) return ommResult_INVALID_ARGUMENT;
        const uint32_t stride = mesh->positionStrideInBytes ? mesh->positionStrideInBytes : 12u;
        if (stride < 12u || (stride & 3u) != 0u) return ommResult_INVALID_ARGUMENT;
        if (mesh->triangleCount && outPositions && (mesh->positions == nullptr || mesh->indexBuffer == nullptr)) return ommResult_INVALID_ARGUMENT;
        M.positions = (const uint8_t*)mesh->positions; M.stride = stride; M.indices = mesh->indexBuffer; M.indexFormat = (int)mesh->indexFormat;
        M.triangleCount = mesh->triangleCount; M.present = 1u;
    }
    if (count == 0 || (outBarycentrics == nullptr && outPositions == nullptr)) return ommResult_SUCCESS;
    if (nodes == nullptr) return ommResult_INVALID_ARGUMENT;
    const uint64_t blocks = (count + kGeoBlock - 1u) / kGeoBlock;
    expand_micro_nodes<<<(uint32_t)(blocks < 65536u ? blocks : 65536u), kGeoBlock, 0, (hipStream_t)hipStream>>>(nodes, count, M, outBarycentrics, outPositions);
    return hipGetLastError() == hipSuccess ? ommResult_SUCCESS : ommResult_FAILURE;
}
