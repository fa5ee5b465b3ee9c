// raster_kernels.hip -- ommxRasterizeMicromap (include/omm_mi355x_ext.h): a coverage pass that finds the owner of every pixel, the lowest covering
// primitive, and a shading pass that looks up the owner's state, samples the alpha texture and writes and counts.  The arithmetic of the rule is
// raster_cover.h (also host C++); texture coordinates and the sampler are tex_fetch.h, the resolve kernel's; the state is omm_mi355x_lookup.h.
//
// Coverage.  A primitive is tested against the pixels of its clipped bounding box only, never primitives x pixels, in three shapes of work by the box's
// size, as in the bake's texel walk:
//   raster_cover_small   a lane per primitive.  It fetches the triangle, makes the box and, where the box has at most kRasterLaneBox pixels, walks it
//                        itself.  Preferred over a lane per pixel of one primitive: the triangle (six fp64 values and the box) is then in the lane's own
//                        registers, no cross-lane traffic and no LDS, and with a million small triangles every lane has work; a wave per such primitive
//                        would idle most lanes on boxes of a dozen pixels.  It also classifies every primitive for the other two kernels.
//   raster_cover_wave    a wave per primitive whose box has up to kRasterWaveBox pixels: 64 pixels at a time, lane l takes pixel l + 64 k of the box.
//   raster_cover_grid    primitives with larger boxes (foliage cards, a triangle over the whole image), from the list that raster_cover_small appends
//                        to.  A box is cut into one share per kRasterGridShare of its pixels, at most kRasterGridBlocks of them; raster_grid_prefix
//                        sums the shares over the list, and the workgroups take the shares of all boxes in turn, finding a share's box by a binary
//                        search in the sums; 64 pixels per wave and step.  One triangle over the whole image is spread over every CU, and forty
//                        thousand cards keep every CU busy too, each workgroup touching only the boxes it has a share of.
// Ownership is atomicMin on the owner word, issued by covering lanes only: an integer minimum does not depend on arrival order.
//
// Shading.  A lane per pixel.  The owner's cross products are evaluated again with the same expressions (no float travels between the passes), the
// state comes from ommx_opacity_state.  The contour needs the alpha test of the right and the upper neighbour: those two points are sampled again
// here rather than read from a pass that wrote them.  That costs two more samples per pixel (texels a neighbouring lane fetches anyway), and buys one
// pass instead of two, no alpha-test scratch of a byte per pixel, and a picture that does not depend on which outputs were asked for.  Counts are
// per-wave ballot sums over a grid-stride loop, added across the workgroup's four waves in LDS, then one integer atomic per workgroup and counter.
#include <hip/hip_runtime.h>
#include <string.h>
#include "raster_kernels.h"
#include "tex_fetch.h"
#include "../../include/omm_mi355x_lookup.h"

namespace ommx {

constexpr uint32_t kRasterBlock = 256;
constexpr uint32_t kRasterLaneBox = 64;        // boxes of at most a wave's worth of pixels: walked by the lane that owns the primitive
constexpr uint32_t kRasterWaveBox = 4096;      // boxes up to here: a wave per primitive (at most 64 steps); above: the whole grid
constexpr uint32_t kRasterGridBlocks = 2048;   // 256 CUs x 8 blocks of 4 waves
constexpr uint32_t kRasterGridShare = 4096;    // pixels of a large box per workgroup, at least: 16 steps per lane (reasoned, not measured: the least that
                                               // spreads a box of kRasterWaveBox pixels and more at all)
constexpr uint32_t kRasterGridTurns = 64;      // ... and larger shares where the boxes of a call would otherwise make more than this many per workgroup.
                                               // 40 000 foliage cards at 4096^2, whole call: 23.3 ms with shares of 4096 pixels throughout, 14.0 / 12.0 /
                                               // 11.2 ms with 4 / 16 / 64 turns
constexpr uint32_t kRasterPeek = 4;            // owner words that a lane of raster_cover_grid reads ahead: same case, 14.2 / 12.0 / 19.6 ms with 1 / 4 / 8
constexpr uint32_t kRasterPrefixBlock = 1024;  // raster_grid_prefix is one workgroup
constexpr uint32_t kRasterShadeBlocks = 2048;  // the shading pass strides over the pixels: 2048 workgroups x 8 counters bound its atomics on 8 addresses
constexpr uint32_t kRasterCountBlocks = 1024;  // likewise for the two sums over the primitives

enum : uint8_t { kClassDegenerate = 1, kClassOutside = 2, kClassLane = 3, kClassWave = 4, kClassGrid = 5 };
enum { kCountCovered = 0, kCountState0 = 1, kCountInvalid = 5, kCountAlphaAbove = 6, kCountContradictions = 7, kCountDrawn = 8, kCountDegenerate = 9, kCounters = 10 };

// the scratch block: offsets of its parts, each a multiple of 256 bytes
struct RasterScratch {
    size_t counters, gridCount, owner, cls, drawn, gridList, gridPrefix, lowest, bytes;
};
static size_t pad256(size_t n) { return (n + 255u) & ~(size_t)255u; }
static RasterScratch raster_layout(const RasterArgs& a)
{
    RasterScratch s; size_t at = 0;
    s.counters = at; at += pad256(sizeof(uint64_t) * kCounters);
    s.gridCount = at; at += 256;
    s.owner = at; at += a.primitiveIds ? 0 : pad256(sizeof(uint32_t) * (size_t)a.view.width * a.view.height);
    s.cls = at; at += pad256(a.count);
    s.drawn = at; at += pad256(a.count);
    s.gridList = at; at += pad256(sizeof(uint2) * (size_t)a.count);
    s.gridPrefix = at; at += pad256(sizeof(unsigned long long) * ((size_t)a.count + 1u));
    s.lowest = at; at += (a.flags & ommxRasterFlags_HighlightReuse) ? pad256(sizeof(uint32_t) * (size_t)a.result.descArrayCount) : 0;
    s.bytes = at;
    return s;
}
size_t raster_scratch_bytes(const RasterArgs& a) { return raster_layout(a).bytes; }

struct RasterDevice {              // the kernels' pointers into the scratch block (and the caller's primitiveIds)
    unsigned long long* counters; uint32_t* gridCount; uint32_t* owner; uint8_t *cls, *drawn; uint2* gridList /* (primitive of the range, pixels of its box) */;
    unsigned long long* gridPrefix /* shares of the boxes before list item e; [listed]: of all */; uint32_t* lowest;
};

__device__ __forceinline__ RasterTri fetch_triangle(const ResolveParams& M, uint32_t prim)
{
    const V2 a = fetch_tex_coord(M, fetch_vertex_index(M, prim, 0)), b = fetch_tex_coord(M, fetch_vertex_index(M, prim, 1)),
             c = fetch_tex_coord(M, fetch_vertex_index(M, prim, 2));
    RasterTri t;
    t.ax = (double)a.x; t.ay = (double)a.y; t.bx = (double)b.x; t.by = (double)b.y; t.cx = (double)c.x; t.cy = (double)c.y;
    return t;
}

// pixel (x, y) of the box: the test and the ownership claim.  x < width and y < height by raster_box.
__device__ __forceinline__ void claim_pixel(const RasterTri& t, double area2, const RasterView& v, uint32_t x, uint32_t y, uint32_t prim, uint32_t* owner)
{
    uint32_t* word = owner + ((size_t)y * v.width + x);
    double w[3];
    raster_edges(t, raster_sample(v.loU, v.stepU, x), raster_sample(v.loV, v.stepV, y), w);
    if (raster_covers(w, area2)) atomicMin(word, prim);
}

// the index entry of a primitive, where the result has one
__device__ __forceinline__ bool result_entry(const ommCpuBakeResultDesc& r, uint32_t prim, int32_t* e)
{
    if (prim >= r.indexCount) return false;
    switch (r.indexFormat) {
    case ommIndexFormat_UINT_8:  *e = ((const int8_t*)r.indexBuffer)[prim]; return true;
    case ommIndexFormat_UINT_16: *e = ((const int16_t*)r.indexBuffer)[prim]; return true;
    case ommIndexFormat_UINT_32: *e = ((const int32_t*)r.indexBuffer)[prim]; return true;
    default: return false;
    }
}

// HighlightReuse: the lowest primitive of the range under every descriptor
__global__ __launch_bounds__(kRasterBlock) void raster_lowest(ommCpuBakeResultDesc r, uint32_t first, uint32_t count, uint32_t* __restrict__ lowest)
{
    const uint32_t i = blockIdx.x * kRasterBlock + threadIdx.x;
    if (i >= count) return;
    int32_t e;
    if (result_entry(r, first + i, &e) && e >= 0 && (uint32_t)e < r.descArrayCount) atomicMin(lowest + e, first + i);
}

__global__ __launch_bounds__(kRasterBlock) void raster_cover_small(ResolveParams M, RasterView v, uint32_t first, uint32_t count, RasterDevice D)
{
    const uint32_t i = blockIdx.x * kRasterBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t prim = first + i;
    const RasterTri t = fetch_triangle(M, prim);
    const double area2 = raster_area2(t);
    uint32_t box[4];
    uint8_t c;
    if (raster_degenerate(area2)) c = kClassDegenerate;
    else if (!raster_box(t, v, box)) c = kClassOutside;
    else {
        const uint32_t n = (box[1] - box[0]) * (box[3] - box[2]);   // at most 2^28
        if (n <= kRasterLaneBox) {
            c = kClassLane;
            uint32_t x = box[0], y = box[2];   // row by row
            for (uint32_t k = 0; k < n; ++k) {
                claim_pixel(t, area2, v, x, y, prim, D.owner);
                if (++x == box[1]) { x = box[0]; ++y; }
            }
        } else if (n <= kRasterWaveBox) c = kClassWave;
        else { c = kClassGrid; D.gridList[atomicAdd(D.gridCount, 1u)] = make_uint2(i, n); }   // (at most `count` entries: one per primitive)
    }
    D.cls[i] = c;
}

// the box of primitive first + i, row by row, from pixel `start` on, `stride` pixels apart: pixel k is (k % bw, k / bw) of the box, kept up by
// additions.
// PEEK: read the owner word first and leave a pixel that a lower primitive owns already alone -- the minimum is the same, and under heavy overdraw
// (40 000 foliage cards at 4096^2: 1.4e10 box pixels, 561 primitives own all 1.7e7 image pixels) nearly every step ends at this read.  The reads are
// coalesced, one per wave and step, and a lane has kRasterPeek of them in flight before it looks at the first.
template <bool PEEK>
__device__ __forceinline__ void walk_box(const ResolveParams& M, const RasterView& v, uint32_t prim, uint32_t start, uint32_t stride, uint32_t* owner)
{
    const RasterTri t = fetch_triangle(M, prim);
    const double area2 = raster_area2(t);
    uint32_t box[4];
    if (raster_degenerate(area2) || !raster_box(t, v, box)) return;   // (not so for a primitive of these classes)
    const uint32_t n = (box[1] - box[0]) * (box[3] - box[2]);
    const uint32_t bw = box[1] - box[0], dx = stride % bw, dy = stride / bw;
    uint32_t x = start % bw, y = start / bw;
    for (uint32_t k = start; k < n;) {               // (n + kRasterPeek * stride < 2^32; k < n: y is inside the box)
        uint32_t px[PEEK ? kRasterPeek : 1u], py[PEEK ? kRasterPeek : 1u], seen[PEEK ? kRasterPeek : 1u];
        #pragma unroll
        for (uint32_t j = 0; j < (PEEK ? kRasterPeek : 1u); ++j) {
            px[j] = box[0] + x; py[j] = box[2] + y;
            seen[j] = !PEEK ? kRasterNone : k < n ? __atomic_load_n(owner + ((size_t)py[j] * v.width + px[j]), __ATOMIC_RELAXED) : 0u;   // (0: nothing to do)
            k += stride; x += dx; y += dy;
            if (x >= bw) { x -= bw; ++y; }           // (x and dx are below bw)
        }
        #pragma unroll
        for (uint32_t j = 0; j < (PEEK ? kRasterPeek : 1u); ++j)
            if (seen[j] > prim) claim_pixel(t, area2, v, px[j], py[j], prim, owner);
    }
}

__global__ __launch_bounds__(kRasterBlock) void raster_cover_wave(ResolveParams M, RasterView v, uint32_t first, uint32_t count, RasterDevice D)
{
    const uint32_t i = blockIdx.x * (kRasterBlock / 64u) + threadIdx.x / 64u;
    if (i >= count || D.cls[i] != kClassWave) return;
    walk_box<false>(M, v, first + i, threadIdx.x & 63u, 64u, D.owner);
}

// the shares of a large box: the workgroups that walk it, one per `sharePixels` of its pixels and at most a grid's worth
__device__ __forceinline__ uint32_t grid_shares(uint32_t pixels, uint32_t sharePixels)
{
    const uint32_t share = (pixels + sharePixels - 1u) / sharePixels;   // (pixels <= 2^28, sharePixels >= kRasterGridShare)
    return share < kRasterGridBlocks ? share : kRasterGridBlocks;
}

// the pixels of a share for this call -- kRasterGridShare, or more where the boxes' pixels would otherwise make more than kRasterGridTurns shares per
// workgroup: each share costs a binary search and a triangle fetch, some twenty dependent loads, before its walk begins -- into
// gridCount[1]; then exclusive sums of the shares over the list of large boxes, the total behind them.  One workgroup, a contiguous piece of the list
// per thread.
__global__ __launch_bounds__(kRasterPrefixBlock) void raster_grid_prefix(uint32_t count, RasterDevice D)
{
    __shared__ unsigned long long part[kRasterPrefixBlock];
    const uint32_t listed = *D.gridCount < count ? *D.gridCount : count;
    const uint32_t per = (listed + kRasterPrefixBlock - 1u) / kRasterPrefixBlock;   // (threadIdx.x * per < 2^32: listed < 2^32 / 3)
    const uint32_t lo = threadIdx.x * per < listed ? threadIdx.x * per : listed, hi = listed - lo < per ? listed : lo + per;
    unsigned long long run = 0;
    for (uint32_t e = lo; e < hi; ++e) run += D.gridList[e].y;
    part[threadIdx.x] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long pixels = 0;
        for (uint32_t k = 0; k < kRasterPrefixBlock; ++k) pixels += part[k];
        const unsigned long long even = pixels / ((unsigned long long)kRasterGridBlocks * kRasterGridTurns);
        part[0] = even < kRasterGridShare ? kRasterGridShare : even < (1u << 28) ? even : (1u << 28);
        D.gridCount[1] = (uint32_t)part[0];
    }
    __syncthreads();
    const uint32_t sharePixels = (uint32_t)part[0];
    __syncthreads();
    run = 0;
    for (uint32_t e = lo; e < hi; ++e) run += grid_shares(D.gridList[e].y, sharePixels);
    part[threadIdx.x] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long before = 0;
        for (uint32_t k = 0; k < kRasterPrefixBlock; ++k) { const unsigned long long own = part[k]; part[k] = before; before += own; }
        D.gridPrefix[listed] = before;
    }
    __syncthreads();
    run = part[threadIdx.x];
    for (uint32_t e = lo; e < hi; ++e) { D.gridPrefix[e] = run; run += grid_shares(D.gridList[e].y, sharePixels); }
}

__global__ __launch_bounds__(kRasterBlock) void raster_cover_grid(ResolveParams M, RasterView v, uint32_t first, uint32_t count, RasterDevice D)
{
    const uint32_t listed = *D.gridCount < count ? *D.gridCount : count;
    const unsigned long long shares = D.gridPrefix[listed];
    const uint32_t sharePixels = D.gridCount[1];
    for (unsigned long long u = blockIdx.x; u < shares; u += gridDim.x) {   // (shares > 0: listed > 0)
        uint32_t lo = 0, hi = listed;                                       // the last item with gridPrefix[item] <= u
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (D.gridPrefix[mid] <= u) lo = mid; else hi = mid;
        }
        const uint2 item = D.gridList[lo];
        if (item.x >= count) continue;
        const uint32_t blocks = grid_shares(item.y, sharePixels), local = (uint32_t)(u - D.gridPrefix[lo]);   // local < blocks
        walk_box<true>(M, v, first + item.x, local * kRasterBlock + threadIdx.x, blocks * kRasterBlock, D.owner);
    }
}

// the alpha test of pixel (x, y), and its alpha
template <bool FP32>
__device__ __forceinline__ bool pixel_alpha_test(const ClassifyParams& P, const RasterView& v, uint32_t x, uint32_t y, float* alpha)
{
    const double U = raster_sample(v.loU, v.stepU, x), V = raster_sample(v.loV, v.stepV, y);
    *alpha = sample_alpha<FP32>(P, mk2((float)U, (float)V));
    return P.cutoff < *alpha;
}

__device__ __forceinline__ uint32_t wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

template <bool FP32>
__global__ __launch_bounds__(kRasterBlock) void raster_shade(RasterArgs A, RasterDevice D)
{
    const RasterView& v = A.view;
    const uint32_t total = v.width * v.height;   // at most 2^28
    const uint32_t lane = threadIdx.x & 63u, stride = gridDim.x * kRasterBlock;
    const bool contour = !(A.flags & ommxRasterFlags_NoContour) && A.rgba != nullptr;
    const bool rgbaWords = ((uintptr_t)A.rgba & 3u) == 0;
    uint32_t n[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };   // wave-uniform sums, in the counters' order
    for (uint32_t base = blockIdx.x * kRasterBlock + (threadIdx.x & ~63u); base < total; base += stride) {   // (base is the wave's: no lane leaves early)
        const uint32_t i = base + lane;
        const bool active = i < total;
        bool covered = false, above = false, contradicts = false;
        uint32_t s = kRasterStateNone;
        if (active) {
            const uint32_t x = i % v.width, y = i / v.width;
            float alpha;
            above = pixel_alpha_test<FP32>(A.mesh.tex, v, x, y, &alpha);
            const uint32_t owner = D.owner[i];
            uint32_t micro = kRasterNone;
            bool inverted = false, reused = false;
            covered = owner != kRasterNone;
            if (covered) {
                const RasterTri t = fetch_triangle(A.mesh, owner);
                double w[3];
                raster_edges(t, raster_sample(v.loU, v.stepU, x), raster_sample(v.loV, v.stepV, y), w);
                float bu, bv;
                raster_barycentrics(w, raster_area2(t), &bu, &bv);
                const ommCpuBakeResultDesc rl = A.result;
                s = ommx_opacity_state(&rl, owner, bu, bv);
                int32_t e = -1;
                if (s != OMMX_OPACITY_INVALID && result_entry(rl, owner, &e)) {
                    if (e < 0) micro = 0u;
                    else {   // (a valid state: e < descArrayCount and the level is at most 12)
                        const uint32_t level = rl.descArray[e].subdivisionLevel;
                        micro = ommx_micro_index(bu, bv, level);
                        float mv[6];
                        ommx_micro_vertices(micro, level, mv);
                        inverted = mv[2] < mv[0];
                        reused = (A.flags & ommxRasterFlags_HighlightReuse) && D.lowest[e] < owner;
                    }
                }
                const uint32_t c = above ? (uint32_t)A.mesh.tex.stateGT : (uint32_t)A.mesh.tex.stateLE;
                contradicts = s < 2u && (c & 1u) != s;
                D.drawn[owner - A.first] = 1;   // (every writer stores the same byte)
            }
            if (A.primitiveIds && A.primitiveIds != D.owner) A.primitiveIds[i] = owner;
            if (A.microTriangles) A.microTriangles[i] = micro;
            if (A.states) A.states[i] = (uint8_t)s;
            if (A.alphaTest) A.alphaTest[i] = above ? 1 : 0;
            if (A.rgba) {
                const uint32_t g = raster_grey(alpha);
                uint32_t px = covered ? raster_covered(s, g, (A.flags & ommxRasterFlags_MonochromeUnknowns) != 0, inverted, reused) : raster_background(g);
                if (contour) {
                    float other;
                    if (x + 1u < v.width && pixel_alpha_test<FP32>(A.mesh.tex, v, x + 1u, y, &other) != above) px = kRasterContour;
                    if (y + 1u < v.height && pixel_alpha_test<FP32>(A.mesh.tex, v, x, y + 1u, &other) != above) px = kRasterContour;
                }
                uint8_t* out = A.rgba + 4ull * i;
                if (rgbaWords) *(uint32_t*)out = px;
                else { out[0] = (uint8_t)px; out[1] = (uint8_t)(px >> 8); out[2] = (uint8_t)(px >> 16); out[3] = (uint8_t)(px >> 24); }
            }
        }
        n[kCountCovered] += wave_count(covered);
        #pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) n[kCountState0 + k] += wave_count(covered && s == k);
        n[kCountInvalid] += wave_count(covered && s == OMMX_OPACITY_INVALID);
        n[kCountAlphaAbove] += wave_count(above);
        n[kCountContradictions] += wave_count(contradicts);
    }
    // the four waves' sums through LDS, then one integer atomic per workgroup and counter
    __shared__ uint32_t sums[kRasterBlock / 64u][8];
    if (lane == 0) {
        #pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) sums[threadIdx.x / 64u][k] = n[k];
    }
    __syncthreads();
    if (threadIdx.x < 8u) {
        uint32_t total8 = 0;
        for (uint32_t wv = 0; wv < kRasterBlock / 64u; ++wv) total8 += sums[wv][threadIdx.x];
        if (total8) atomicAdd(D.counters + threadIdx.x, (unsigned long long)total8);
    }
}

// drawnPrimitives and degeneratePrimitives: sums over the two bytes per primitive
__global__ __launch_bounds__(kRasterBlock) void raster_count_primitives(uint32_t count, RasterDevice D)
{
    uint32_t drawn = 0, degenerate = 0;   // wave-uniform
    const uint64_t stride = (uint64_t)gridDim.x * kRasterBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kRasterBlock + (threadIdx.x & ~63u); base < count; base += stride) {
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool in = i < count;
        drawn += wave_count(in && D.drawn[i] != 0);
        degenerate += wave_count(in && D.cls[i] == kClassDegenerate);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (drawn) atomicAdd(D.counters + kCountDrawn, (unsigned long long)drawn);
        if (degenerate) atomicAdd(D.counters + kCountDegenerate, (unsigned long long)degenerate);
    }
}

static uint32_t blocks_for(uint64_t items, uint32_t perBlock) { return (uint32_t)((items + perBlock - 1u) / perBlock); }

hipError_t raster_run(const RasterArgs& a, void* scratch, RasterCounts* out, hipStream_t stream)
{
    const RasterScratch L = raster_layout(a);
    uint8_t* base = (uint8_t*)scratch;
    RasterDevice D;
    D.counters = (unsigned long long*)(base + L.counters); D.gridCount = (uint32_t*)(base + L.gridCount);
    D.owner = a.primitiveIds ? a.primitiveIds : (uint32_t*)(base + L.owner);
    D.cls = base + L.cls; D.drawn = base + L.drawn; D.gridList = (uint2*)(base + L.gridList);
    D.gridPrefix = (unsigned long long*)(base + L.gridPrefix); D.lowest = (uint32_t*)(base + L.lowest);
    const size_t pixels = (size_t)a.view.width * a.view.height;
    hipError_t e;
    if ((e = hipMemsetAsync(base, 0, L.owner, stream)) != hipSuccess) return e;                                    // counters, gridCount
    if ((e = hipMemsetAsync(D.owner, 0xFF, sizeof(uint32_t) * pixels, stream)) != hipSuccess) return e;           // nobody owns anything
    if (a.count) {
        if ((e = hipMemsetAsync(D.cls, 0, L.gridList - L.cls, stream)) != hipSuccess) return e;                    // cls, drawn
        if ((a.flags & ommxRasterFlags_HighlightReuse) && a.result.descArrayCount) {
            if ((e = hipMemsetAsync(D.lowest, 0xFF, sizeof(uint32_t) * (size_t)a.result.descArrayCount, stream)) != hipSuccess) return e;
            raster_lowest<<<blocks_for(a.count, kRasterBlock), kRasterBlock, 0, stream>>>(a.result, a.first, a.count, D.lowest);
        }
        raster_cover_small<<<blocks_for(a.count, kRasterBlock), kRasterBlock, 0, stream>>>(a.mesh, a.view, a.first, a.count, D);
        raster_cover_wave<<<blocks_for(a.count, kRasterBlock / 64u), kRasterBlock, 0, stream>>>(a.mesh, a.view, a.first, a.count, D);
        raster_grid_prefix<<<1, kRasterPrefixBlock, 0, stream>>>(a.count, D);
        raster_cover_grid<<<kRasterGridBlocks, kRasterBlock, 0, stream>>>(a.mesh, a.view, a.first, a.count, D);
    }
    const uint32_t shadeBlocks = blocks_for(pixels, kRasterBlock) < kRasterShadeBlocks ? blocks_for(pixels, kRasterBlock) : kRasterShadeBlocks;
    if (a.mesh.tex.texIsFp32) raster_shade<true><<<shadeBlocks, kRasterBlock, 0, stream>>>(a, D);
    else raster_shade<false><<<shadeBlocks, kRasterBlock, 0, stream>>>(a, D);
    if (a.count) {
        const uint32_t countBlocks = blocks_for(a.count, kRasterBlock) < kRasterCountBlocks ? blocks_for(a.count, kRasterBlock) : kRasterCountBlocks;
        raster_count_primitives<<<countBlocks, kRasterBlock, 0, stream>>>(a.count, D);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint64_t host[kCounters];
    if ((e = hipMemcpyAsync(host, D.counters, sizeof host, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    out->covered = host[kCountCovered];
    for (int k = 0; k < 4; ++k) out->perState[k] = host[kCountState0 + k];
    out->invalid = host[kCountInvalid]; out->alphaAbove = host[kCountAlphaAbove]; out->contradictions = host[kCountContradictions];
    out->drawn = host[kCountDrawn]; out->degenerate = host[kCountDegenerate];
    return hipSuccess;
}

} // namespace ommx
