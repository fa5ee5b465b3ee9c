// merge_kernels.hip -- ommxMergeSimilarMicromaps (include/omm_mi355x_ext.h has the definition): 4-state blocks of a device-resident result that are
// near-copies of each other are merged into the one of lowest source index, round by round, conservatively; then the tail of a bake runs on what is
// left (rebuild_kernels.hip) and the index buffer is written.  The word arithmetic is merge_words.h's.
//
//   merge_mark        the index buffer once: which descriptors are selected (and pass the bounds rule), how many primitives are skipped
//   merge_prepare     per selected descriptor: its word for the tail, the size of its staging slot, its number of copy units; candidates are counted,
//                     those of level 6 and above listed (a wave takes each of them, a lane each of the others)
//   merge_copy        THE copy (copy_unit in gather_unit.h): every selected block, bits unchanged, into its 16-byte aligned slot.  A block that is
//                     no candidate is final: its writers sum its digest and uniformity mask here.
//   per round, in place in the staging:
//   merge_signature   one lane per descriptor: the key of a live candidate from `samples` 2-bit reads, into the hash table (hash_build.h) under
//                     "lowest index wins"; the round's member counts are zeroed
//   merge_distance_*  every live candidate that is not the lowest under its key streams its own block and that leader's: XOR, fold, popcount,
//                     leaving early once the limit is passed.  An absorbed block notes its leader and is counted there.
//   (scan)            the counts become the leaders' places in the member list
//   merge_fill        absorbed blocks enter their leader's part of the list (in any order: the join does not depend on it)
//   merge_join_*      one owner per word of a leader joins the same word of every member into it.  No leader is a member and no member is written
//                     in a round, so there is neither a snapshot nor an atomic.  Sixteen waves share the vectors of a leader of level 6 and above.
//   after the rounds:
//   merge_roots       absorbed -> leader is followed to the end (a leader has the lower index; a chain is at most `rounds` long); an absorbed
//                     descriptor leaves the tail's items
//   merge_digest      digest and uniformity mask of the surviving candidates, from the staging
//   (the tail)        items are source descriptors, so representatives within a size class are ordered by source index ascending
//   merge_index       the index buffer, in the source's index format: a primitive of d gets the block of root(d)
//
// All counters are integers and every output byte has one writer, so the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include "merge_kernels.h"
#include "gather_unit.h"
#include "hash_build.h"
#include "result_read.h"
#include "result_words.h"
#include "wave_search.h"

namespace ommx {
namespace {

constexpr uint32_t kMeBlock = kRebuildBlock;
constexpr uint32_t kMeWaves = kMeBlock / 64;
constexpr uint32_t kMeLaneLevel = 5;              // a lane takes a candidate up to this level (256 bytes); a wave one above it (1 KiB and more)
constexpr uint32_t kMeNone = 0xFFFFFFFFu;
constexpr uint32_t kMeJoinRuns = 16;              // waves that share a listed leader's vectors in the join (a level-8 block has 16 runs of 64 vectors)
constexpr uint32_t kMeStep = 4;                 // 16-byte vectors per lane between two looks at a wave's partial distance

struct MergeHeader { uint32_t skipped, referenced, candidates, wide, absorbed[kMergeMaxRounds]; };

__device__ __forceinline__ bool is_candidate(uint32_t w) { return w != 0u && item_bits(w) == 2u && item_level(w) >= 1u; }

// A. one lane per primitive and turn
__global__ __launch_bounds__(kMeBlock) void merge_mark(ommCpuBakeResultDesc r, uint32_t* __restrict__ ref, MergeHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const ResultView s = view_of(r);
    uint32_t skipped = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kMeBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kMeBlock + threadIdx.x; i < s.indexCount; i += stride) skipped += mark_selected(s, i, ref);
    if (skipped) atomicAdd(&s_n[0], skipped);
    counters_end<1>(s_n, &hdr->skipped);
}

// B. one lane per descriptor and one for the scans' closing element
__global__ __launch_bounds__(kMeBlock) void merge_prepare(ommCpuBakeResultDesc r, const uint32_t* __restrict__ ref, uint32_t* __restrict__ item,
                                                          unsigned long long* __restrict__ slot, unsigned long long* __restrict__ units,
                                                          unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask, uint32_t* __restrict__ lead,
                                                          uint32_t* __restrict__ when, uint32_t* __restrict__ wideList, MergeHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[2];
    counters_begin<2>(s_n);
    const uint64_t d = (uint64_t)blockIdx.x * kMeBlock + threadIdx.x;
    if (d <= r.descArrayCount) {
        unsigned long long bytes = 0ull, n = 0ull;
        if (d < r.descArrayCount) {
            uint32_t w = 0u;
            if (ref[d]) {
                const ommCpuOpacityMicromapDesc desc = load_desc(r.descArray + d);   // (marked: it passed the bounds rule)
                bytes = block_bytes(desc.subdivisionLevel, desc.format);
                n = unit_count(bytes);
                bytes = (bytes + kRebuildSlotAlign - 1u) & ~(unsigned long long)(kRebuildSlotAlign - 1u);
                digest[d] = 0ull; umask[d] = 0xFu;
                w = item_word(desc.subdivisionLevel, desc.format);
                atomicAdd(&s_n[0], 1u);
                if (is_candidate(w)) {
                    atomicAdd(&s_n[1], 1u);
                    if (item_level(w) > kMeLaneLevel) wideList[atomicAdd(&hdr->wide, 1u)] = (uint32_t)d;
                }
            }
            item[d] = w; lead[d] = kMeNone; when[d] = 0u;
        }
        slot[d] = bytes; units[d] = n;
    }
    counters_end<2>(s_n, &hdr->referenced);
}

// C. one unit per workgroup and turn
__global__ __launch_bounds__(kMeBlock) void merge_copy(ommCpuBakeResultDesc r, const uint32_t* __restrict__ item, const unsigned long long* __restrict__ unitStart,
                                                       const unsigned long long* __restrict__ slotStart, uint8_t* __restrict__ staging,
                                                       unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask)
{
    __shared__ uint64_t s_digest[kMeWaves];
    __shared__ uint32_t s_umask[kMeWaves];
    const unsigned long long total = unitStart[r.descArrayCount];
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t d = owner_of_segment(unitStart, r.descArrayCount, u);
        const uint32_t w = item[d], level = item_level(w), bits = item_bits(w);
        const uint8_t* block = (const uint8_t*)r.arrayData + load_desc(r.descArray + d).offset;   // (has units, so it is selected and passed the bounds rule)
        UnitOut o; o.dst = staging + slotStart[d]; o.fieldBase = 0ull; o.outFields = 0u; o.bits = bits; o.digest = 0ull; o.umask = 0xFu;
        copy_unit<kMeBlock>(block, level, bits, u - unitStart[d], o);
        if (!is_candidate(w)) unit_close<kMeWaves>(o, s_digest, s_umask, digest + d, umask + d);   // (w is the workgroup's: no divergence around the barrier)
        __syncthreads();   // (the LDS words are the next unit's too)
    }
}

// R1. one lane per descriptor and one for the scan's closing element
__global__ __launch_bounds__(kMeBlock) void merge_signature(uint32_t descCount, uint32_t round, uint32_t samples, uint32_t seed, const uint32_t* __restrict__ item,
                                                            const uint32_t* __restrict__ lead, const unsigned long long* __restrict__ slotStart,
                                                            const uint8_t* __restrict__ staging, unsigned long long* __restrict__ keys,
                                                            unsigned long long* __restrict__ count, uint32_t* __restrict__ cursor, HashTable table)
{
    __shared__ uint32_t s_buckets[kMeBlock];
    const uint64_t d = (uint64_t)blockIdx.x * kMeBlock + threadIdx.x;
    bool live = false;
    uint64_t key = 0ull;
    if (d <= descCount) count[d] = 0ull;
    if (d < descCount) {
        cursor[d] = 0u;
        const uint32_t w = item[d];
        live = is_candidate(w) && lead[d] == kMeNone;
        if (live) {
            key = merge_key(staging + slotStart[d], item_level(w), round, samples, seed);
            keys[d] = key;
        }
    }
    hash_put_min_block(table, live, key, (uint32_t)d, s_buckets);
}

// the distance of two blocks of `bytes` bytes in 16-byte aligned slots, as far as one lane looks: it stops once the limit is passed
__device__ __forceinline__ uint32_t lane_distance(const uint8_t* a, const uint8_t* b, uint32_t bytes, uint32_t limit)
{
    if (bytes == 1u) return merge_distance(a[0], b[0]);
    if (bytes == 4u) return merge_distance(*(const uint32_t*)a, *(const uint32_t*)b);
    uint32_t n = 0u;
    for (uint32_t v = 0; v < bytes / 16u && n <= limit; ++v) {
        const WordsVec x = ((const WordsVec*)a)[v], y = ((const WordsVec*)b)[v];
        n += merge_distance(x[0], y[0]) + merge_distance(x[1], y[1]);
    }
    return n;
}
// candidate d joins leader l in this round
__device__ __forceinline__ void absorb(uint32_t d, uint32_t l, uint32_t round, uint32_t* __restrict__ lead, uint32_t* __restrict__ when, unsigned long long* __restrict__ count)
{
    lead[d] = l; when[d] = round + 1u;
    atomicAdd(&count[l], 1ull);
}

// R2a. one lane per descriptor: the candidates up to level 5
__global__ __launch_bounds__(kMeBlock) void merge_distance_lane(uint32_t descCount, uint32_t round, uint32_t maxDistance, const uint32_t* __restrict__ item,
                                                                uint32_t* __restrict__ lead, uint32_t* __restrict__ when, const unsigned long long* __restrict__ keys,
                                                                HashTable table, const unsigned long long* __restrict__ slotStart, const uint8_t* __restrict__ staging,
                                                                unsigned long long* __restrict__ count, MergeHeader* __restrict__ hdr)
{
    __shared__ uint32_t s_n[1];
    counters_begin<1>(s_n);
    const uint64_t d = (uint64_t)blockIdx.x * kMeBlock + threadIdx.x;
    if (d < descCount) {
        const uint32_t w = item[d], level = item_level(w);
        if (is_candidate(w) && level <= kMeLaneLevel && lead[d] == kMeNone) {
            const uint32_t l = hash_get(table, keys[d], (uint32_t)d);
            if (l < d) {
                const uint32_t limit = merge_limit(maxDistance, level);
                if (lane_distance(staging + slotStart[d], staging + slotStart[l], (uint32_t)block_bytes(level, 2u), limit) <= limit) {
                    absorb((uint32_t)d, l, round, lead, when, count);
                    atomicAdd(&s_n[0], 1u);
                }
            }
        }
    }
    counters_end<1>(s_n, &hdr->absorbed[round]);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// R2b. one wave per listed candidate (level 6 and above) and turn
__global__ __launch_bounds__(kMeBlock) void merge_distance_wave(uint32_t wide, const uint32_t* __restrict__ wideList, uint32_t round, uint32_t maxDistance,
                                                                const uint32_t* __restrict__ item, uint32_t* __restrict__ lead, uint32_t* __restrict__ when,
                                                                const unsigned long long* __restrict__ keys, HashTable table,
                                                                const unsigned long long* __restrict__ slotStart, const uint8_t* __restrict__ staging,
                                                                unsigned long long* __restrict__ count, MergeHeader* __restrict__ hdr)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t absorbed = 0u;
    for (uint64_t k = (uint64_t)blockIdx.x * kMeWaves + (threadIdx.x >> 6); k < wide; k += (uint64_t)gridDim.x * kMeWaves) {
        const uint32_t d = wideList[k];
        if (lead[d] != kMeNone) continue;                 // (the wave's: every lane reads the same word, and lane 0 writes it behind the last read)
        const uint32_t l = hash_get(table, keys[d], d);
        if (l >= d) continue;
        const uint32_t level = item_level(item[d]), limit = merge_limit(maxDistance, level);
        const uint32_t vectors = (uint32_t)(block_bytes(level, 2u) / 16u);   // 64 and more
        const WordsVec* a = (const WordsVec*)(staging + slotStart[d]);
        const WordsVec* b = (const WordsVec*)(staging + slotStart[l]);
        uint32_t n = 0u, total = 0u;
        for (uint32_t base = 0; base < vectors && total <= limit; base += 64u * kMeStep) {
            #pragma unroll
            for (uint32_t s = 0; s < kMeStep; ++s) {
                const uint32_t v = base + 64u * s + lane;
                if (v < vectors) { const WordsVec x = a[v], y = b[v]; n += merge_distance(x[0], y[0]) + merge_distance(x[1], y[1]); }
            }
            total = wave_sum_u32(n);
        }
        if (total <= limit && lane == 0u) { absorb(d, l, round, lead, when, count); ++absorbed; }
    }
    if (absorbed) atomicAdd(&hdr->absorbed[round], absorbed);
}

// R3. one lane per descriptor: a block absorbed in this round enters its leader's part of the list
__global__ __launch_bounds__(kMeBlock) void merge_fill(uint32_t descCount, uint32_t round, const uint32_t* __restrict__ lead, const uint32_t* __restrict__ when,
                                                       const unsigned long long* __restrict__ memberStart, uint32_t* __restrict__ cursor, uint32_t* __restrict__ members)
{
    const uint64_t d = (uint64_t)blockIdx.x * kMeBlock + threadIdx.x;
    if (d < descCount && when[d] == round + 1u) {
        const uint32_t l = lead[d];
        members[memberStart[l] + atomicAdd(&cursor[l], 1u)] = (uint32_t)d;
    }
}

// R4a. one lane per descriptor: a leader up to level 5 takes its members in
__global__ __launch_bounds__(kMeBlock) void merge_join_lane(uint32_t descCount, uint32_t mixedState, const uint32_t* __restrict__ item,
                                                            const unsigned long long* __restrict__ memberStart, const uint32_t* __restrict__ members,
                                                            const unsigned long long* __restrict__ slotStart, uint8_t* __restrict__ staging)
{
    const uint64_t d = (uint64_t)blockIdx.x * kMeBlock + threadIdx.x;
    if (d >= descCount) return;
    const unsigned long long first = memberStart[d], last = memberStart[d + 1u];
    if (first == last) return;
    const uint32_t level = item_level(item[d]);
    if (level > kMeLaneLevel) return;
    const uint32_t bytes = (uint32_t)block_bytes(level, 2u);
    uint8_t* mine = staging + slotStart[d];
    if (bytes < 16u) {
        uint64_t x = bytes == 1u ? mine[0] : *(const uint32_t*)mine;
        for (unsigned long long m = first; m < last; ++m) {
            const uint8_t* other = staging + slotStart[members[m]];
            x = merge_join(x, bytes == 1u ? other[0] : *(const uint32_t*)other, mixedState);
        }
        if (bytes == 1u) mine[0] = (uint8_t)x; else *(uint32_t*)mine = (uint32_t)x;
        return;
    }
    for (uint32_t v = 0; v < bytes / 16u; ++v) {
        WordsVec x = ((const WordsVec*)mine)[v];
        for (unsigned long long m = first; m < last; ++m) {
            const WordsVec y = ((const WordsVec*)(staging + slotStart[members[m]]))[v];
            x[0] = merge_join(x[0], y[0], mixedState); x[1] = merge_join(x[1], y[1], mixedState);
        }
        ((WordsVec*)mine)[v] = x;
    }
}

// R4b. one wave per listed candidate (level 6 and above) and turn: a lane owns every 64th vector of the leader
__global__ __launch_bounds__(kMeBlock) void merge_join_wave(uint32_t wide, const uint32_t* __restrict__ wideList, uint32_t mixedState, const uint32_t* __restrict__ item,
                                                            const unsigned long long* __restrict__ memberStart, const uint32_t* __restrict__ members,
                                                            const unsigned long long* __restrict__ slotStart, uint8_t* __restrict__ staging)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t k = (uint64_t)blockIdx.x * kMeWaves + (threadIdx.x >> 6); k < wide; k += (uint64_t)gridDim.x * kMeWaves) {
        const uint32_t d = wideList[k];
        const unsigned long long first = memberStart[d], last = memberStart[d + 1u];
        if (first == last) continue;
        const uint32_t vectors = (uint32_t)(block_bytes(item_level(item[d]), 2u) / 16u);
        WordsVec* mine = (WordsVec*)(staging + slotStart[d]);
        // blockIdx.y shares a leader's vectors out in runs of 64: a leader of thousands of members is a chain of joins per vector, and a level-8
        // leader has sixteen such runs.  Four members per turn: their loads do not depend on each other.
        for (uint32_t v = 64u * blockIdx.y + lane; v < vectors; v += 64u * gridDim.y) {
            WordsVec x = mine[v];
            unsigned long long m = first;
            for (; m + 4u <= last; m += 4u) {
                const WordsVec y0 = ((const WordsVec*)(staging + slotStart[members[m]]))[v], y1 = ((const WordsVec*)(staging + slotStart[members[m + 1u]]))[v];
                const WordsVec y2 = ((const WordsVec*)(staging + slotStart[members[m + 2u]]))[v], y3 = ((const WordsVec*)(staging + slotStart[members[m + 3u]]))[v];
                const uint64_t a0 = merge_join(merge_join(y0[0], y1[0], mixedState), merge_join(y2[0], y3[0], mixedState), mixedState);
                const uint64_t a1 = merge_join(merge_join(y0[1], y1[1], mixedState), merge_join(y2[1], y3[1], mixedState), mixedState);
                x[0] = merge_join(x[0], a0, mixedState); x[1] = merge_join(x[1], a1, mixedState);
            }
            for (; m < last; ++m) {
                const WordsVec y = ((const WordsVec*)(staging + slotStart[members[m]]))[v];
                x[0] = merge_join(x[0], y[0], mixedState); x[1] = merge_join(x[1], y[1], mixedState);
            }
            mine[v] = x;
        }
    }
}

// G. one lane per descriptor: its root; an absorbed descriptor is no item of the tail
__global__ __launch_bounds__(kMeBlock) void merge_roots(uint32_t descCount, uint32_t* __restrict__ item, const uint32_t* __restrict__ lead,
                                                        uint32_t* __restrict__ root, uint32_t* __restrict__ outRoots)
{
    const uint64_t d = (uint64_t)blockIdx.x * kMeBlock + threadIdx.x;
    if (d >= descCount) return;
    const uint32_t w = item[d];
    uint32_t at = kMeNone;
    if (w) {
        at = (uint32_t)d;
        for (uint32_t hop = 0; hop < kMergeMaxRounds && lead[at] != kMeNone; ++hop) at = lead[at];   // (a block is absorbed once per round at most)
    }
    root[d] = at;
    if (outRoots) outRoots[d] = at;
    item[d] = at == d ? w : 0u;
}

// one unit of a block in its staging slot: what copy_unit learns while it writes, without the writing
template <uint32_t Threads>
__device__ __forceinline__ void digest_unit(const uint8_t* slot, uint32_t level, uint32_t bits, uint64_t unit, UnitOut& o)
{
    const uint32_t t = threadIdx.x;
    const uint64_t bytes = block_bytes(level, bits);
    if (bytes < 16u) {
        if (t == 0u) {
            uint64_t word = 0ull;
            for (uint32_t b = 0; b < (uint32_t)bytes; ++b) word |= (uint64_t)slot[b] << (8u * b);
            const uint32_t used = bits << (2u * level);
            o.digest = word_digest(word, 0u); o.umask = coarsen_word_uniform(word, used < 64u ? used : 64u, bits);
        }
        return;
    }
    const uint64_t first = unit * kUnitVectors;
    const uint32_t count = bytes < kUnitBytes ? (uint32_t)(bytes / 16u) : kUnitVectors;
    const WordsVec* in = (const WordsVec*)slot + first;
    #pragma unroll 4
    for (uint32_t v = t; v < count; v += Threads) {
        const WordsVec x = in[v];
        const uint64_t word = 2u * (first + v);
        o.digest += word_digest(x[0], word) + word_digest(x[1], word + 1u);
        o.umask &= coarsen_word_uniform(x[0], 64u, bits) & coarsen_word_uniform(x[1], 64u, bits);
    }
}

// H. one unit per workgroup and turn: the candidates that are left
__global__ __launch_bounds__(kMeBlock) void merge_digest(uint32_t descCount, const uint32_t* __restrict__ item, const unsigned long long* __restrict__ unitStart,
                                                         const unsigned long long* __restrict__ slotStart, const uint8_t* __restrict__ staging,
                                                         unsigned long long* __restrict__ digest, uint32_t* __restrict__ umask)
{
    __shared__ uint64_t s_digest[kMeWaves];
    __shared__ uint32_t s_umask[kMeWaves];
    const unsigned long long total = unitStart[descCount];
    for (unsigned long long u = blockIdx.x; u < total; u += gridDim.x) {
        const uint32_t d = owner_of_segment(unitStart, descCount, u);
        const uint32_t w = item[d];
        if (!is_candidate(w)) continue;                   // (final since the copy, or absorbed; w is the workgroup's)
        UnitOut o; o.dst = nullptr; o.fieldBase = 0ull; o.outFields = 0u; o.bits = 2u; o.digest = 0ull; o.umask = 0xFu;
        digest_unit<kMeBlock>(staging + slotStart[d], item_level(w), 2u, u - unitStart[d], o);
        unit_close<kMeWaves>(o, s_digest, s_umask, digest + d, umask + d);
        __syncthreads();   // (the LDS words are the next unit's too)
    }
}

// F3. one lane per primitive and turn
__global__ __launch_bounds__(kMeBlock) void merge_index(ommCpuBakeResultDesc r, const uint32_t* __restrict__ item, const uint32_t* __restrict__ root, RebuildTables tail,
                                                        void* __restrict__ outIndex)
{
    __shared__ uint32_t s_n[kRebuildHist];
    counters_begin<kRebuildHist>(s_n);
    const ResultView s = view_of(r);
    const uint64_t stride = (uint64_t)gridDim.x * kMeBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kMeBlock + threadIdx.x; i < s.indexCount; i += stride) {
        int32_t v = named_entry(s, i);
        if (v == kSkipped) v = -4;
        else if (v >= 0) {
            const uint32_t at = root[v];                  // (none: no primitive's descriptor passed the bounds rule here)
            v = at == kMeNone ? -4 : index_back(tail, at, item[at], s_n);
        }
        index_store(outIndex, s.indexFormat, i, v);
    }
    counters_end<kRebuildHist>(s_n, tail.indexHist);
}

// the call's scratch: the header and the marks behind it (ONE memset clears both), the arrays of the rounds, the hash table, the arrays of the tail
struct MergeScratch {
    MergeHeader* hdr; uint32_t *ref, *lead, *when, *root, *cursor, *members, *wideList;
    unsigned long long *keys, *count;
    uint8_t* table; uint32_t slots;
    TailArrays t; size_t bytes;
};
MergeScratch merge_scratch(const MergeArgs& a, void* base)
{
    MergeScratch s; CarveCursor c{ (uintptr_t)base };
    const size_t D = a.result.descArrayCount;
    s.hdr = c.take<MergeHeader>(1); s.ref = c.take<uint32_t>(D);
    s.lead = c.take<uint32_t>(D); s.when = c.take<uint32_t>(D); s.root = c.take<uint32_t>(D); s.cursor = c.take<uint32_t>(D);
    s.members = c.take<uint32_t>(D); s.wideList = c.take<uint32_t>(D);
    s.keys = c.take<unsigned long long>(D); s.count = c.take<unsigned long long>(D + 1);
    s.slots = D ? hash_table_slots(D) : 0u;
    s.table = c.take<uint8_t>(s.slots ? hash_table_bytes(s.slots) : 0);
    s.t = rebuild_arrays(c, a.result.descArrayCount, a.flags);
    s.bytes = (size_t)(c.at - (uintptr_t)base);
    return s;
}

} // namespace

size_t merge_head_bytes(const MergeArgs& a) { return merge_scratch(a, nullptr).bytes; }

hipError_t merge_plan(const MergeArgs& a, void* head, MergePlan* out, hipStream_t stream)
{
    const MergeScratch s = merge_scratch(a, head);
    const ommCpuBakeResultDesc& r = a.result;
    const uint32_t D = r.descArrayCount;
    REBUILD_CHECK(hipMemsetAsync(s.hdr, 0, (size_t)((uint8_t*)s.ref - (uint8_t*)s.hdr) + 4 * (size_t)D, stream));   // (the header and the marks behind it)
    merge_mark<<<strided_grid(r.indexCount), kMeBlock, 0, stream>>>(r, s.ref, s.hdr);
    REBUILD_CHECK(hipGetLastError());
    unsigned long long stagingBytes = 0, totalUnits = 0;
    if (D) {
        merge_prepare<<<per_item_grid((uint64_t)D + 1u), kMeBlock, 0, stream>>>(r, s.ref, s.t.item, s.t.slotStart, s.t.units, s.t.digest, s.t.umask, s.lead, s.when, s.wideList, s.hdr);
        REBUILD_CHECK(hipGetLastError());
        REBUILD_CHECK(rebuild_scan(s.t, D, &stagingBytes, &totalUnits, stream));
    }
    MergeHeader h;
    REBUILD_CHECK(hipMemcpyAsync(&h, s.hdr, sizeof h, hipMemcpyDeviceToHost, stream));
    REBUILD_CHECK(hipStreamSynchronize(stream));
    out->stagingBytes = stagingBytes; out->units = totalUnits; out->skipped = h.skipped; out->referenced = h.referenced; out->candidates = h.candidates; out->wide = h.wide;
    return hipSuccess;
}

hipError_t merge_stage(const MergeArgs& a, void* head, void* staging, const MergePlan& plan, MergeRounds* rounds, RebuildCounts* out, hipStream_t stream)
{
    const MergeScratch s = merge_scratch(a, head);
    const uint32_t D = a.result.descArrayCount;
    uint8_t* st = (uint8_t*)staging;
    MergeHeader h; memset(&h, 0, sizeof h);
    if (D) {
        const uint32_t unitGrid = (uint32_t)(plan.units < kRebuildMaxGrid ? plan.units : kRebuildMaxGrid);
        const uint32_t waveGrid = strided_grid((uint64_t)plan.wide * 64u);
        if (plan.units) {
            merge_copy<<<unitGrid, kMeBlock, 0, stream>>>(a.result, s.t.item, s.t.units, s.t.slotStart, st, s.t.digest, s.t.umask);
            REBUILD_CHECK(hipGetLastError());
        }
        const HashTable table = hash_table_at(s.table, s.slots);
        for (uint32_t round = 0; round < a.rounds && plan.candidates; ++round) {
            REBUILD_CHECK(hipMemsetAsync(s.table, 0xFF, hash_table_bytes(s.slots), stream));
            merge_signature<<<per_item_grid((uint64_t)D + 1u), kMeBlock, 0, stream>>>(D, round, a.samples, a.seed, s.t.item, s.lead, s.t.slotStart, st, s.keys, s.count, s.cursor, table);
            REBUILD_CHECK(hipGetLastError());
            merge_distance_lane<<<per_item_grid(D), kMeBlock, 0, stream>>>(D, round, a.maxDistance, s.t.item, s.lead, s.when, s.keys, table, s.t.slotStart, st, s.count, s.hdr);
            REBUILD_CHECK(hipGetLastError());
            if (plan.wide) {
                merge_distance_wave<<<waveGrid, kMeBlock, 0, stream>>>(plan.wide, s.wideList, round, a.maxDistance, s.t.item, s.lead, s.when, s.keys, table, s.t.slotStart, st, s.count, s.hdr);
                REBUILD_CHECK(hipGetLastError());
            }
            size_t tb = s.t.tempBytes;   // (in place: every element is read before it is written)
            REBUILD_CHECK(rocprim::exclusive_scan(s.t.temp, tb, s.count, s.count, 0ull, (size_t)D + 1, rocprim::plus<unsigned long long>(), stream));
            merge_fill<<<per_item_grid(D), kMeBlock, 0, stream>>>(D, round, s.lead, s.when, s.count, s.cursor, s.members);
            REBUILD_CHECK(hipGetLastError());
            merge_join_lane<<<per_item_grid(D), kMeBlock, 0, stream>>>(D, a.mixedState, s.t.item, s.count, s.members, s.t.slotStart, st);
            REBUILD_CHECK(hipGetLastError());
            if (plan.wide) {
                merge_join_wave<<<dim3(waveGrid, kMeJoinRuns), kMeBlock, 0, stream>>>(plan.wide, s.wideList, a.mixedState, s.t.item, s.count, s.members, s.t.slotStart, st);
                REBUILD_CHECK(hipGetLastError());
            }
        }
        merge_roots<<<per_item_grid(D), kMeBlock, 0, stream>>>(D, s.t.item, s.lead, s.root, a.roots);
        REBUILD_CHECK(hipGetLastError());
        if (plan.units && plan.candidates) {
            merge_digest<<<unitGrid, kMeBlock, 0, stream>>>(D, s.t.item, s.t.units, s.t.slotStart, st, s.t.digest, s.t.umask);
            REBUILD_CHECK(hipGetLastError());
        }
        REBUILD_CHECK(hipMemcpyAsync(&h, s.hdr, sizeof h, hipMemcpyDeviceToHost, stream));   // (rebuild_count waits for the stream)
    }
    REBUILD_CHECK(rebuild_count(tail_inputs(s.t, D, a.flags, staging), out, stream));
    rounds->absorbed = 0u;
    for (uint32_t k = 0; k < kMergeMaxRounds; ++k) { rounds->perRound[k] = h.absorbed[k]; rounds->absorbed += h.absorbed[k]; }
    return hipSuccess;
}

hipError_t merge_emit(const MergeArgs& a, void* head, const void* staging, const RebuildCounts& counts, const RebuildOutputs& o, hipStream_t stream)
{
    const MergeScratch s = merge_scratch(a, head);
    const RebuildInputs in = tail_inputs(s.t, a.result.descArrayCount, a.flags, staging);
    REBUILD_CHECK(rebuild_emit(in, counts, o.arrayData, o.descs, stream));
    merge_index<<<strided_grid(a.result.indexCount), kMeBlock, 0, stream>>>(a.result, in.item, s.root, rebuild_tables(in), o.index);
    REBUILD_CHECK(hipGetLastError());
    return rebuild_histograms(in, o.hist, stream);
}

} // namespace ommx
