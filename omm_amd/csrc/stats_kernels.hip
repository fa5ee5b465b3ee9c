// stats_kernels.hip -- ommDebugStats of a device-resident result without a download: the state histogram of every OMM block in one streaming
// pass over arrayData (stats_count_blocks), the special indices and the references of every block in one pass over the index buffer
// (stats_primitives), the known share of every primitive and the two area sums (stats_known_area), and the totals (stats_reduce).
// The host loop (collect_stats, omm_host.cpp) trusts the descriptors; nothing here reads through one that fails the bounds rule of
// include/omm_mi355x_lookup.h.  All counters are integers, so atomics do not make them depend on the order of arrival; the two fp64 sums
// have a fixed partition and a fixed tree and use no atomics.
#include <hip/hip_runtime.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include "stats_kernels.h"
#include "stats_count.h"
#include "result_read.h"
#include "bake_host.h"   // pad256
#include "wave_search.h"

namespace ommx {

constexpr uint32_t kStatsBlock = 256;
constexpr uint32_t kStatsWaves = kStatsBlock / 64;
// blocks up to this size (levels 0 - 3) are counted by the lane that checks their descriptor: a workgroup per 1 - 16 bytes would be all overhead
constexpr uint64_t kStatsInlineBytes = 16;
constexpr uint32_t kStatsMaxGrid = 65536;        // the strided kernels' grids: 32 workgroups per slot of the chip (256 CUs x 8), the rest by stride
constexpr uint32_t kStatsAreaPerLane = 8;        // stats_known_area: a workgroup owns 256 x 8 consecutive primitives, whatever the grid

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_ull(unsigned long long v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
// the same butterfly for every call: lane l adds lane l ^ 32, then l ^ 16, ...: a fixed tree, every lane ends with the same bits
__device__ __forceinline__ double wave_sum_f64(double v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// One lane per descriptor (and one for the scan's closing element): zeroes its counters, counts a small block on the spot, and says how many
// segments a larger one is cut into -- 0 for a descriptor that fails the bounds rule, which therefore is never read through.
__global__ __launch_bounds__(kStatsBlock) void stats_prepare(ommCpuBakeResultDesc r, uint32_t* __restrict__ stateCounts, uint32_t* __restrict__ refs,
                                                             unsigned long long* __restrict__ segments)
{
    const uint64_t d = (uint64_t)blockIdx.x * kStatsBlock + threadIdx.x;
    if (d > r.descArrayCount) return;
    if (d == r.descArrayCount) { segments[d] = 0ull; return; }
    const ommCpuOpacityMicromapDesc desc = r.descArray[d];
    uint32_t c[4] = { 0u, 0u, 0u, 0u };
    unsigned long long segs = 0ull;
    uint64_t bytes;
    if (desc_ok(desc, r.arrayDataSize, &bytes)) {
        if (bytes <= kStatsInlineBytes) stats_count_range((const uint8_t*)r.arrayData + desc.offset, desc.subdivisionLevel, desc.format, 0u, bytes, 0u, 1u, c);
        else segs = (bytes + kStatsSegmentBytes - 1u) / kStatsSegmentBytes;
    }
    #pragma unroll
    for (int s = 0; s < 4; ++s) stateCounts[4ull * d + s] = c[s];   // (a caller's array is only 4-byte aligned)
    refs[d] = 0u;
    segments[d] = segs;
}

// One 16 KiB segment of one block per workgroup and turn: 64 bytes per lane as four 16-byte reads, popcounts on the words, the four counts
// reduced in the wave, across the waves in LDS, and added to the block's counters by one integer atomic per state.  The grid is the host's upper
// bound on the number of segments (blocks that do not overlap); the stride covers results whose descriptors share bytes.
__global__ __launch_bounds__(kStatsBlock) void stats_count_blocks(ommCpuBakeResultDesc r, const unsigned long long* __restrict__ segStart,
                                                                  uint32_t* __restrict__ stateCounts)
{
    __shared__ uint32_t s_c[kStatsWaves][4];
    const unsigned long long total = segStart[r.descArrayCount];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned long long seg = blockIdx.x; seg < total; seg += gridDim.x) {
        const uint32_t d = owner_of_segment(segStart, r.descArrayCount, seg);
        const ommCpuOpacityMicromapDesc desc = r.descArray[d];   // (has segments, so it passed the bounds rule in stats_prepare)
        const uint64_t bytes = block_bytes(desc.subdivisionLevel, desc.format);
        const uint64_t begin = (uint64_t)(seg - segStart[d]) * kStatsSegmentBytes;
        const uint64_t end = begin + kStatsSegmentBytes < bytes ? begin + kStatsSegmentBytes : bytes;
        uint32_t c[4] = { 0u, 0u, 0u, 0u };
        stats_count_range((const uint8_t*)r.arrayData + desc.offset, desc.subdivisionLevel, desc.format, begin, end, threadIdx.x, kStatsBlock, c);
        #pragma unroll
        for (int s = 0; s < 4; ++s) { const uint32_t v = wave_sum_u32(c[s]); if (lane == 0) s_c[wave][s] = v; }
        __syncthreads();
        if (threadIdx.x < 4) {
            uint32_t v = 0;
            #pragma unroll
            for (uint32_t w = 0; w < kStatsWaves; ++w) v += s_c[w][threadIdx.x];
            if (v) atomicAdd(&stateCounts[4ull * d + threadIdx.x], v);
        }
        __syncthreads();
    }
}

// The index buffer, one lane per primitive and turn: special indices into four counters, entries that no block answers (below -4, at or beyond
// descArrayCount, or a descriptor that fails the bounds rule) into a fifth, every other entry into its block's reference count.
__global__ __launch_bounds__(kStatsBlock) void stats_primitives(ommCpuBakeResultDesc r, uint32_t* __restrict__ refs, StatsTotals* __restrict__ tot)
{
    __shared__ uint32_t s_n[kStatsWaves][5];
    uint32_t n[5] = { 0u, 0u, 0u, 0u, 0u };
    const uint64_t stride = (uint64_t)gridDim.x * kStatsBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kStatsBlock + threadIdx.x; i < r.indexCount; i += stride) {
        const int32_t e = index_entry(r.indexBuffer, (int)r.indexFormat, i);
        uint64_t bytes;
        if (e < 0) {
            #pragma unroll
            for (int k = 0; k < 4; ++k) n[k] += e == -1 - k ? 1u : 0u;   // (no runtime index into the registers)
            n[4] += e < -4 ? 1u : 0u;
        }
        else if ((uint32_t)e < r.descArrayCount && desc_ok(r.descArray[e], r.arrayDataSize, &bytes)) atomicAdd(&refs[e], 1u);
        else n[4]++;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    #pragma unroll
    for (int k = 0; k < 5; ++k) { const uint32_t v = wave_sum_u32(n[k]); if (lane == 0) s_n[wave][k] = v; }
    __syncthreads();
    if (threadIdx.x < 5) {
        uint32_t v = 0;
        #pragma unroll
        for (uint32_t w = 0; w < kStatsWaves; ++w) v += s_n[w][threadIdx.x];
        if (v) atomicAdd(threadIdx.x < 4 ? &tot->special[threadIdx.x] : &tot->skipped, v);
    }
}

// After the counts are final: knownFraction of every primitive and, with areas, sum(area * knownFraction) and sum(area) of the workgroup's
// 2048 consecutive primitives in fp64 -- each lane its eight in ascending order, the wave's butterfly, the four waves in ascending order.
__global__ __launch_bounds__(kStatsBlock) void stats_known_area(ommCpuBakeResultDesc r, const uint32_t* __restrict__ stateCounts, const float* __restrict__ areas,
                                                                float* __restrict__ knownFraction, double* __restrict__ partials)
{
    __shared__ double s_p[kStatsWaves][2];
    double known = 0.0, total = 0.0;
    const uint64_t base = (uint64_t)blockIdx.x * (kStatsBlock * kStatsAreaPerLane) + threadIdx.x;
    #pragma unroll
    for (uint32_t k = 0; k < kStatsAreaPerLane; ++k) {
        const uint64_t i = base + (uint64_t)k * kStatsBlock;
        if (i >= r.indexCount) break;
        const int32_t e = index_entry(r.indexBuffer, (int)r.indexFormat, i);
        float f = 0.f;
        uint64_t bytes;
        if (e < 0) f = e >= -2 ? 1.f : 0.f;
        else if ((uint32_t)e < r.descArrayCount && desc_ok(r.descArray[e], r.arrayDataSize, &bytes)) {
            const uint32_t* c = stateCounts + 4ull * (uint32_t)e;
            const uint32_t kn = c[0] + c[1], un = c[2] + c[3];
            f = (float)kn / (float)(kn + un);   // one IEEE division (hipcc's default; the library is built without fast-math)
        }
        if (knownFraction) knownFraction[i] = f;
        if (areas) { const float a = areas[i]; known += (double)a * (double)f; total += (double)a; }
    }
    if (!areas) return;
    known = wave_sum_f64(known); total = wave_sum_f64(total);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) { s_p[wave][0] = known; s_p[wave][1] = total; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double k2 = s_p[0][0], t2 = s_p[0][1];
        #pragma unroll
        for (uint32_t w = 1; w < kStatsWaves; ++w) { k2 += s_p[w][0]; t2 += s_p[w][1]; }
        partials[2ull * blockIdx.x] = k2; partials[2ull * blockIdx.x + 1] = t2;
    }
}

// The totals.  Every workgroup: the 32-bit products references * count of its share of the referenced blocks, as the host forms them, into the
// four 64-bit sums.  Workgroup 0 also reduces the fp64 partials: lane t adds partials t, t + 256, ... in ascending order, then the same tree as above.
__global__ __launch_bounds__(kStatsBlock) void stats_reduce(uint32_t descCount, const uint32_t* __restrict__ stateCounts, const uint32_t* __restrict__ refs,
                                                            const double* __restrict__ partials, uint32_t numPartials, StatsTotals* __restrict__ tot)
{
    __shared__ unsigned long long s_t[kStatsWaves][4];
    __shared__ double s_p[kStatsWaves][2];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long t[4] = { 0ull, 0ull, 0ull, 0ull };
    const uint64_t stride = (uint64_t)gridDim.x * kStatsBlock;
    for (uint64_t d = (uint64_t)blockIdx.x * kStatsBlock + threadIdx.x; d < descCount; d += stride) {
        const uint32_t n = refs[d];
        if (!n) continue;
        #pragma unroll
        for (int s = 0; s < 4; ++s) t[s] += (uint32_t)(n * stateCounts[4ull * d + s]);
    }
    #pragma unroll
    for (int s = 0; s < 4; ++s) { const unsigned long long v = wave_sum_ull(t[s]); if (lane == 0) s_t[wave][s] = v; }
    double known = 0.0, total = 0.0;
    if (blockIdx.x == 0 && partials) {
        for (uint32_t j = threadIdx.x; j < numPartials; j += kStatsBlock) { known += partials[2ull * j]; total += partials[2ull * j + 1]; }
        known = wave_sum_f64(known); total = wave_sum_f64(total);
        if (lane == 0) { s_p[wave][0] = known; s_p[wave][1] = total; }
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long v = 0;
        #pragma unroll
        for (uint32_t w = 0; w < kStatsWaves; ++w) v += s_t[w][threadIdx.x];
        if (v) atomicAdd(&tot->state[threadIdx.x], v);
    }
    if (blockIdx.x == 0 && partials && threadIdx.x == 0) {
        double k2 = s_p[0][0], t2 = s_p[0][1];
        #pragma unroll
        for (uint32_t w = 1; w < kStatsWaves; ++w) { k2 += s_p[w][0]; t2 += s_p[w][1]; }
        tot->knownArea = k2; tot->totalArea = t2;
    }
}

namespace {
struct StatsLayout { size_t totals, segments, counts, refs, partials, scanTemp, scanTempBytes, bytes; uint32_t numPartials; };
StatsLayout stats_layout(const StatsArgs& a)
{
    StatsLayout L; size_t o = 0;
    const size_t D = a.result.descArrayCount;
    L.totals = o; o += pad256(sizeof(StatsTotals));
    L.segments = o; o += pad256(sizeof(unsigned long long) * (D + 1));
    L.counts = o; if (!a.stateCounts) o += pad256(sizeof(uint32_t) * 4 * D);
    L.refs = o; if (!a.referenceCounts) o += pad256(sizeof(uint32_t) * D);
    L.numPartials = a.areas ? (uint32_t)(((uint64_t)a.result.indexCount + kStatsBlock * kStatsAreaPerLane - 1u) / (kStatsBlock * kStatsAreaPerLane)) : 0u;
    L.partials = o; o += pad256(sizeof(double) * 2 * (size_t)L.numPartials);
    L.scanTempBytes = 0;
    if (D) (void)rocprim::exclusive_scan(nullptr, L.scanTempBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, D + 1, rocprim::plus<unsigned long long>());
    L.scanTemp = o; o += pad256(L.scanTempBytes);
    L.bytes = o;
    return L;
}
uint32_t strided_grid(uint64_t items)
{
    const uint64_t blocks = (items + kStatsBlock - 1u) / kStatsBlock;
    return (uint32_t)(blocks < kStatsMaxGrid ? (blocks ? blocks : 1u) : kStatsMaxGrid);
}
} // namespace

size_t stats_scratch_bytes(const StatsArgs& a) { return stats_layout(a).bytes; }

#define STATS_CHECK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

hipError_t launch_stats(const StatsArgs& a, void* scratch, StatsTotals* out, hipStream_t stream)
{
    const StatsLayout L = stats_layout(a);
    uint8_t* base = (uint8_t*)scratch;
    const ommCpuBakeResultDesc& r = a.result;
    const uint32_t D = r.descArrayCount;
    StatsTotals* tot = (StatsTotals*)(base + L.totals);
    unsigned long long* segments = (unsigned long long*)(base + L.segments);
    uint32_t* counts = a.stateCounts ? a.stateCounts : (uint32_t*)(base + L.counts);
    uint32_t* refs = a.referenceCounts ? a.referenceCounts : (uint32_t*)(base + L.refs);
    double* partials = a.areas ? (double*)(base + L.partials) : nullptr;
    STATS_CHECK(hipMemsetAsync(tot, 0, sizeof(StatsTotals), stream));
    if (D) {
        stats_prepare<<<(uint32_t)(((uint64_t)D + 1u + kStatsBlock - 1u) / kStatsBlock), kStatsBlock, 0, stream>>>(r, counts, refs, segments);
        STATS_CHECK(hipGetLastError());
        size_t tb = L.scanTempBytes;   // (in place: every element is read before it is written)
        STATS_CHECK(rocprim::exclusive_scan(base + L.scanTemp, tb, segments, segments, 0ull, (size_t)D + 1, rocprim::plus<unsigned long long>(), stream));
        // no read-back to size the grid: blocks that do not overlap have at most this many segments, and the kernel strides over any more
        const uint64_t bound = (uint64_t)r.arrayDataSize / kStatsSegmentBytes + D;
        stats_count_blocks<<<(uint32_t)(bound < kStatsMaxGrid ? bound : kStatsMaxGrid), kStatsBlock, 0, stream>>>(r, segments, counts);
        STATS_CHECK(hipGetLastError());
    }
    stats_primitives<<<strided_grid(r.indexCount), kStatsBlock, 0, stream>>>(r, refs, tot);
    STATS_CHECK(hipGetLastError());
    if (a.areas || a.knownFraction) {
        const uint32_t grid = (uint32_t)(((uint64_t)r.indexCount + kStatsBlock * kStatsAreaPerLane - 1u) / (kStatsBlock * kStatsAreaPerLane));
        stats_known_area<<<grid, kStatsBlock, 0, stream>>>(r, counts, a.areas, a.knownFraction, partials);
        STATS_CHECK(hipGetLastError());
    }
    stats_reduce<<<strided_grid(D), kStatsBlock, 0, stream>>>(D, counts, refs, partials, L.numPartials, tot);
    STATS_CHECK(hipGetLastError());
    STATS_CHECK(hipMemcpyAsync(out, tot, sizeof(StatsTotals), hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

} // namespace ommx
