// fit_kernels.hip -- ommxProfileMicromapLevels (include/omm_mi355x_ext.h has the definition): for every block of a device-resident result and every
// level at or below its own, how many micro-triangles of that level would be known and how many of those opaque; how many primitives select the block
// and what they weigh.  ommxFitMicromap plans its per-block levels from these rows (fit_plan.h).
//
//   profile_mark      the index buffer once: references per descriptor (a descriptor with references is selected and passed the bounds rule), skipped
//                     primitives, the largest weight as a bit pattern
//   profile_weights   the index buffer again, only with weights: every weight as an integer of 32 bits under the largest one's exponent, summed per block
//   profile_prepare   per selected descriptor: its number of work units, its place in the deep list, its word for the planner; zeroes the rows
//   profile_units     THE pass over arrayData, in coarsen_units' shape: one workgroup per unit of 4^8 micro-triangles; 256 of them per lane as bit planes
//                     (result_words.h), four levels in the lane, three on the wave's ballot, one across the waves in LDS; the counts of every level
//                     summed per wave and per workgroup.  A block of one unit gets plain stores; a block above level 8 one integer atomic per
//                     workgroup and level, and every unit leaves the state of its root
//   profile_deep      blocks above level 8: the remaining levels on those at most 256 roots, one wave per block
//
// Nothing is written but counts, and every counter is an integer: the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include "fit_kernels.h"
#include "profile_count.h"
#include "rebuild_kernels.h"
#include "result_read.h"
#include "result_words.h"
#include "wave_search.h"

namespace ommx {
namespace {

constexpr uint32_t kFitBlock = kRebuildBlock;
constexpr uint32_t kFitWaves = kFitBlock / 64;
constexpr uint32_t kFitUnitLevel = 8;              // a workgroup's unit: 4^8 micro-triangles, 256 per lane
constexpr uint32_t kFitUnitFields = 1u << (2 * kFitUnitLevel);
static_assert(kFitLevels == kProfileLevels && kFitLevels == OMMX_PROFILE_LEVELS, "one row length");

struct ProfileHeader { uint32_t skipped, maxWeight, referenced, deepBlocks; };

// a weight that counts: finite and above zero (as a bit pattern: 1 .. 0x7F7FFFFF, ordered like the values)
__device__ __forceinline__ uint32_t weight_bits(float w) { const uint32_t b = __float_as_uint(w); return b - 1u < 0x7F7FFFFFu ? b : 0u; }
// e of M = m * 2^e, 1 <= m < 2, from M's bit pattern (not zero)
__host__ __device__ inline int32_t weight_exponent(uint32_t bits)
{
    if (bits >> 23) return (int32_t)(bits >> 23) - 127;
    int32_t top = 22; while (!((bits >> top) & 1u)) --top;   // a subnormal: its highest set bit
    return top - 149;
}
// floor(w * 2^(31 - e)) in fp64: the product of a float and a power of two in the normal range is exact
__device__ __forceinline__ unsigned long long weight_units(float w, int32_t e)
{
    if (!weight_bits(w)) return 0ull;
    return (unsigned long long)((double)w * __longlong_as_double((long long)(1023 + 31 - e) << 52));
}

// A. one lane per primitive and turn
__global__ __launch_bounds__(kFitBlock) void profile_mark(ommCpuBakeResultDesc r, const float* __restrict__ weights, uint32_t* __restrict__ refs, ProfileHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[2];
    counters_begin<2>(s_n);
    const ResultView s = view_of(r);
    uint32_t skipped = 0, top = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kFitBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kFitBlock + threadIdx.x; i < s.indexCount; i += stride) {
        const int32_t e = select_entry(s, i);
        if (e >= 0) atomicAdd(&refs[e], 1u);
        skipped += e == kSkipped ? 1u : 0u;
        if (weights) { const uint32_t b = weight_bits(weights[i]); top = b > top ? b : top; }
    }
    if (skipped) atomicAdd(&s_n[0], skipped);
    // the largest weight: in the wave, then one LDS atomic per wave, and a global one only from a workgroup that holds more than the header shows
    // (thousands of atomics on one address take turns; the header only grows, so a value at or below what is read there can be left out)
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int)top, d); top = other > top ? other : top; }
    if ((threadIdx.x & 63u) == 0u && top) atomicMax(&s_n[1], top);
    __syncthreads();
    if (threadIdx.x == 0u && s_n[0]) atomicAdd(&hdr->skipped, s_n[0]);
    if (threadIdx.x == 1u && s_n[1] > __atomic_load_n(&hdr->maxWeight, __ATOMIC_RELAXED)) atomicMax(&hdr->maxWeight, s_n[1]);
}

// A'. one lane per primitive and turn; refs stands for the bounds rule
__global__ __launch_bounds__(kFitBlock) void profile_weights(ommCpuBakeResultDesc r, const float* __restrict__ weights, const uint32_t* __restrict__ refs,
                                                             const ProfileHeader* __restrict__ hdr, unsigned long long* __restrict__ blockWeights)
{
    const uint32_t top = hdr->maxWeight;
    if (!top) return;
    const int32_t exponent = weight_exponent(top);
    const ResultView s = view_of(r);
    const uint64_t stride = (uint64_t)gridDim.x * kFitBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kFitBlock + threadIdx.x; i < s.indexCount; i += stride) {
        const int32_t e = named_entry(s, i);
        if (e < 0 || !refs[e]) continue;
        const unsigned long long q = weight_units(weights[i], exponent);
        if (q) atomicAdd(&blockWeights[e], q);
    }
}

// B. one lane per descriptor and one for the scan's closing element; then the rows, one lane per counter and turn
__global__ __launch_bounds__(kFitBlock) void profile_prepare(ommCpuBakeResultDesc r, bool haveWeights, const uint32_t* __restrict__ refs, uint32_t* __restrict__ known,
                                                             uint32_t* __restrict__ opaque, unsigned long long* __restrict__ blockWeights, uint32_t* __restrict__ shape,
                                                             unsigned long long* __restrict__ units, uint32_t* __restrict__ deepList, ProfileHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const uint64_t stride = (uint64_t)gridDim.x * kFitBlock, first = (uint64_t)blockIdx.x * kFitBlock + threadIdx.x;
    for (uint64_t d = first; d <= r.descArrayCount; d += stride) {
        unsigned long long n = 0ull;
        if (d < r.descArrayCount) {
            uint32_t w = 0u;
            const uint32_t uses = refs[d];
            if (uses) {
                const ommCpuOpacityMicromapDesc desc = load_desc(r.descArray + d);
                const uint32_t level = desc.subdivisionLevel;
                n = level > kFitUnitLevel ? 1ull << (2u * (level - kFitUnitLevel)) : 1ull;
                if (level > kFitUnitLevel) deepList[atomicAdd(&hdr->deepBlocks, 1u)] = (uint32_t)d;
                w = fit_shape(level, desc.format);
                atomicAdd(&s_n[0], 1u);
            }
            if (!haveWeights) blockWeights[d] = uses;
            if (shape) shape[d] = w;
        }
        units[d] = n;
    }
    const uint64_t counters = (uint64_t)r.descArrayCount * kFitLevels;
    for (uint64_t i = first; i < counters; i += stride) { known[i] = 0u; opaque[i] = 0u; }
    __syncthreads();
    if (threadIdx.x == 0u && s_n[0]) atomicAdd(&hdr->referenced, s_n[0]);
}

__device__ __forceinline__ uint64_t packed(ProfileCount c) { return (uint64_t)c.known | ((uint64_t)c.opaque << 16); }
__device__ __forceinline__ ProfileCount operator+(ProfileCount a, ProfileCount b) { a.known += b.known; a.opaque += b.opaque; return a; }

// C. one unit per workgroup and turn.  With k the levels taken off the unit's own: k = 0..3 are counted in the lane (a wave's sums fit 16 bits each:
// two 64-bit words carry the eight), k = 4..7 on the wave's 64 fields, k = 8 on the four waves' last fields.
__global__ __launch_bounds__(kFitBlock) void profile_units(ommCpuBakeResultDesc r, const unsigned long long* __restrict__ unitStart, uint32_t* __restrict__ known,
                                                           uint32_t* __restrict__ opaque, uint8_t* __restrict__ roots)
{
    __shared__ uint32_t s_c[kFitWaves][16];   // [2k], [2k + 1]: known, opaque of the wave at k = 0..7
    __shared__ uint32_t s_root[kFitWaves];    // the wave's last field: lo | hi << 1 | 4 where it has one
    const unsigned long long total = unitStart[r.descArrayCount];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t d = owner_of_segment(unitStart, r.descArrayCount, u);
        const ommCpuOpacityMicromapDesc desc = load_desc(r.descArray + d);   // (has units, so a primitive selects it and it passed the bounds rule)
        const uint32_t level = desc.subdivisionLevel, bits = desc.format;
        const uint64_t unit = u - unitStart[d];
        const uint32_t unitLevel = level < kFitUnitLevel ? level : kFitUnitLevel;
        const uint8_t* src = (const uint8_t*)r.arrayData + desc.offset + unit * (uint64_t)(kFitUnitFields / 8u * bits);
        const uint32_t fields = 1u << (2u * unitLevel);
        const uint32_t mine = (t << 8) >= fields ? 0u : fields < 256u ? fields : 256u;   // the lane's fields: 0, 1, 4, 16, 64 or 256
        CoarsenPlanes P[4];
        if (mine) load_fields(src, bits, t << 8, mine, P);
        else {
            #pragma unroll
            for (int i = 0; i < 4; ++i) { P[i].lo = 0ull; P[i].hi = 0ull; }
        }
        // in the lane: the valid fields of pair 0 and of pairs 1..3 (which hold fields only when the lane has all 256)
        uint32_t v0 = mine < 64u ? mine : 64u, vr = mine == 256u ? 64u : 0u;
        uint64_t sums[2] = { 0ull, 0ull };
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            const ProfileCount c = profile_count(P[0], v0) + profile_count(P[1], vr) + profile_count(P[2], vr) + profile_count(P[3], vr);
            sums[k >> 1] += packed(c) << (32 * (k & 1));
            if (k < 3) {
                #pragma unroll
                for (int i = 0; i < 4; ++i) P[i] = profile_step(P[i]);
                v0 >>= 2; vr >>= 2;
            }
        }
        // the four fields left of a lane with 256, side by side, one level up: the lane's field at k = 4
        CoarsenPlanes cat; cat.lo = 0ull; cat.hi = 0ull;
        #pragma unroll
        for (int i = 0; i < 4; ++i) { cat.lo |= (P[i].lo & 1ull) << i; cat.hi |= (P[i].hi & 1ull) << i; }
        cat = profile_step(cat);
        const bool whole = mine == 256u;
        // on the wave: its lanes with a field are a prefix, so the fields are the low bits of the ballots
        CoarsenPlanes wv; wv.lo = __ballot((int)(whole && (cat.lo & 1ull))); wv.hi = __ballot((int)(whole && (cat.hi & 1ull)));
        uint32_t vw = (uint32_t)__popcll(__ballot((int)whole));
        #pragma unroll
        for (int d2 = 32; d2 >= 1; d2 >>= 1) { sums[0] += shfl_xor_u64(sums[0], d2); sums[1] += shfl_xor_u64(sums[1], d2); }
        if (lane == 0u) {
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t both = (uint32_t)(sums[k >> 1] >> (32 * (k & 1)));
                s_c[wave][2 * k] = both & 0xFFFFu; s_c[wave][2 * k + 1] = both >> 16;
            }
        }
        #pragma unroll
        for (int k = 4; k < 8; ++k) {
            const ProfileCount c = profile_count(wv, vw);
            if (lane == 0u) { s_c[wave][2 * k] = c.known; s_c[wave][2 * k + 1] = c.opaque; }
            if (k < 7) { wv = profile_step(wv); vw >>= 2; }
        }
        if (lane == 0u) s_root[wave] = (uint32_t)(wv.lo & 1ull) | ((uint32_t)(wv.hi & 1ull) << 1) | (vw ? 4u : 0u);
        __syncthreads();
        if (t < 18u) {
            const uint32_t k = t >> 1;
            uint32_t v = 0u;
            if (k < 8u) {
                #pragma unroll
                for (uint32_t w2 = 0; w2 < kFitWaves; ++w2) v += s_c[w2][t];
            } else {
                CoarsenPlanes all; all.lo = 0ull; all.hi = 0ull;
                uint32_t have = 4u;
                #pragma unroll
                for (uint32_t w2 = 0; w2 < kFitWaves; ++w2) {
                    const uint32_t f = s_root[w2];
                    all.lo |= (uint64_t)(f & 1u) << w2; all.hi |= (uint64_t)((f >> 1) & 1u) << w2; have &= f;
                }
                all = profile_step(all);
                const ProfileCount c = profile_count(all, have ? 1u : 0u);
                v = (t & 1u) ? c.opaque : c.known;
                if (t == 16u && level > kFitUnitLevel) roots[u] = (uint8_t)((all.lo & 1ull) | ((all.hi & 1ull) << 1));
            }
            if (k <= unitLevel) {
                uint32_t* at = ((t & 1u) ? opaque : known) + (uint64_t)d * kFitLevels + (level - k);
                if (level > kFitUnitLevel) { if (v) atomicAdd(at, v); }
                else *at = v;
            }
        }
        __syncthreads();   // (the LDS words are the next unit's too)
    }
}

// C'. one wave per block above level 8: four roots per lane one level up, then the wave's fields level by level down to the block's one state
__global__ __launch_bounds__(64) void profile_deep(ommCpuBakeResultDesc r, const uint32_t* __restrict__ deepList, const unsigned long long* __restrict__ unitStart,
                                                   const uint8_t* __restrict__ roots, uint32_t* __restrict__ known, uint32_t* __restrict__ opaque)
{
    const uint32_t d = deepList[blockIdx.x], lane = threadIdx.x;
    const uint32_t level = load_desc(r.descArray + d).subdivisionLevel;   // 9..12
    const uint32_t n = 1u << (2u * (level - kFitUnitLevel));              // roots: 4..256
    const uint8_t* mine = roots + unitStart[d] + 4u * lane;
    const bool have = 4u * lane < n;
    CoarsenPlanes cat; cat.lo = 0ull; cat.hi = 0ull;
    if (have) {
        #pragma unroll
        for (int j = 0; j < 4; ++j) { const uint32_t f = mine[j]; cat.lo |= (uint64_t)(f & 1u) << j; cat.hi |= (uint64_t)((f >> 1) & 1u) << j; }
    }
    cat = profile_step(cat);
    CoarsenPlanes wv; wv.lo = __ballot((int)(have && (cat.lo & 1ull))); wv.hi = __ballot((int)(have && (cat.hi & 1ull)));
    uint32_t vw = n >> 2;
    for (uint32_t t = level - kFitUnitLevel - 1u; ; --t) {
        const ProfileCount c = profile_count(wv, vw);
        if (lane == 0u) { known[(uint64_t)d * kFitLevels + t] = c.known; opaque[(uint64_t)d * kFitLevels + t] = c.opaque; }
        if (t == 0u) break;
        wv = profile_step(wv); vw >>= 2;
    }
}

// the call's scratch: the header, the units' scan, the deep list; then whatever of the outputs the caller does not take
struct ProfileScratch { ProfileHeader* hdr; unsigned long long* units; uint32_t* deepList; uint8_t* temp; size_t tempBytes; ProfileArgs a; size_t bytes; };
ProfileScratch profile_scratch(const ProfileArgs& a, void* base)
{
    ProfileScratch s; CarveCursor c{ (uintptr_t)base };
    const size_t D = a.result.descArrayCount;
    s.hdr = c.take<ProfileHeader>(1); s.units = c.take<unsigned long long>(D + 1); s.deepList = c.take<uint32_t>(D);
    s.tempBytes = 0;
    if (D) (void)rocprim::exclusive_scan(nullptr, s.tempBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, D + 1, rocprim::plus<unsigned long long>());
    s.temp = c.take<uint8_t>(s.tempBytes);
    s.a = a;
    if (!a.known) s.a.known = c.take<uint32_t>(D * kFitLevels);
    if (!a.opaque) s.a.opaque = c.take<uint32_t>(D * kFitLevels);
    if (!a.refs) s.a.refs = c.take<uint32_t>(D);
    if (!a.blockWeights) s.a.blockWeights = c.take<unsigned long long>(D);
    s.a.shape = a.wantShape ? c.take<uint32_t>(D) : nullptr;
    s.bytes = (size_t)(c.at - (uintptr_t)base);
    return s;
}

} // namespace

size_t profile_head_bytes(const ProfileArgs& a) { return profile_scratch(a, nullptr).bytes; }
ProfileArgs profile_arrays(const ProfileArgs& a, void* head) { return profile_scratch(a, head).a; }

hipError_t profile_plan(const ProfileArgs& args, void* head, ProfilePlan* out, hipStream_t stream)
{
    const ProfileScratch s = profile_scratch(args, head);
    const ProfileArgs& a = s.a;
    const ommCpuBakeResultDesc& r = a.result;
    const uint32_t D = r.descArrayCount;
    REBUILD_CHECK(hipMemsetAsync(s.hdr, 0, sizeof(ProfileHeader), stream));
    unsigned long long units = 0;
    if (D) {
        REBUILD_CHECK(hipMemsetAsync(a.refs, 0, 4 * (size_t)D, stream));
        if (a.weights) REBUILD_CHECK(hipMemsetAsync(a.blockWeights, 0, 8 * (size_t)D, stream));
    }
    profile_mark<<<strided_grid(r.indexCount), kFitBlock, 0, stream>>>(r, a.weights, a.refs, s.hdr);
    REBUILD_CHECK(hipGetLastError());
    if (D) {
        if (a.weights) {
            profile_weights<<<strided_grid(r.indexCount), kFitBlock, 0, stream>>>(r, a.weights, a.refs, s.hdr, a.blockWeights);
            REBUILD_CHECK(hipGetLastError());
        }
        profile_prepare<<<strided_grid((uint64_t)D * kFitLevels), kFitBlock, 0, stream>>>(r, a.weights != nullptr, a.refs, a.known, a.opaque, a.blockWeights, a.shape, s.units,
                                                                                           s.deepList, s.hdr);
        REBUILD_CHECK(hipGetLastError());
        size_t tb = s.tempBytes;   // (in place: every element is read before it is written)
        REBUILD_CHECK(rocprim::exclusive_scan(s.temp, tb, s.units, s.units, 0ull, (size_t)D + 1, rocprim::plus<unsigned long long>(), stream));
        REBUILD_CHECK(hipMemcpyAsync(&units, s.units + D, sizeof units, hipMemcpyDeviceToHost, stream));
    }
    ProfileHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&h, s.hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    out->units = units; out->deepBlocks = h.deepBlocks; out->skipped = h.skipped; out->referenced = h.referenced;
    out->weightExponent = h.maxWeight ? weight_exponent(h.maxWeight) : 0;
    return hipSuccess;
}

hipError_t profile_count_blocks(const ProfileArgs& args, void* head, void* roots, const ProfilePlan& plan, hipStream_t stream)
{
    const ProfileScratch s = profile_scratch(args, head);
    const ProfileArgs& a = s.a;
    const ommCpuBakeResultDesc& r = a.result;
    const uint32_t D = r.descArrayCount;
    if (D && plan.units) {
        // (the grid as in coarsen_reduce: a bound for blocks that do not overlap, the kernel strides over any more)
        const uint64_t bound = (uint64_t)r.arrayDataSize / (kFitUnitFields / 8u) + D;
        profile_units<<<(uint32_t)(bound < kRebuildMaxGrid ? bound : kRebuildMaxGrid), kFitBlock, 0, stream>>>(r, s.units, a.known, a.opaque, (uint8_t*)roots);
        REBUILD_CHECK(hipGetLastError());
        if (plan.deepBlocks) {
            profile_deep<<<plan.deepBlocks, 64, 0, stream>>>(r, s.deepList, s.units, (const uint8_t*)roots, a.known, a.opaque);
            REBUILD_CHECK(hipGetLastError());
        }
    }
    return hipStreamSynchronize(stream);
}

} // namespace ommx
