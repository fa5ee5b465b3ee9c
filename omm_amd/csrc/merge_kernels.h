// merge_kernels.h -- ommxMergeSimilarMicromaps: near-duplicate 4-state blocks of a device-resident result merged into leaders (merge_kernels.hip; the
// definition is in include/omm_mi355x_ext.h).  omm_host.cpp owns the baker, its device pool, the argument checks and the result handle; the three
// calls below are the phases between which the host has to size a block of memory.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"
#include "merge_words.h"
#include "rebuild_kernels.h"

namespace ommx {

struct MergeArgs {
    ommCpuBakeResultDesc result;   // host struct, arrays in device memory; indexFormat already checked
    uint32_t maxDistance;          // <= 4^12
    uint32_t rounds, samples;      // 1..32, 1..28 (the defaults already applied)
    uint32_t seed;
    uint32_t mixedState;           // 2 or 3
    uint32_t flags;                // ommxCoarsenFlags_DisableSpecialIndices or 0
    uint32_t* roots;               // [descArrayCount] device memory, or null
};
struct MergePlan {                 // after the index buffer has been read
    uint64_t stagingBytes, units;  // the arena the blocks are copied to; its work units
    uint32_t skipped, referenced, candidates;
    uint32_t wide;                 // candidates that a wave takes (level 6 and above)
};
struct MergeRounds { uint32_t absorbed, perRound[kMergeMaxRounds]; };

size_t merge_head_bytes(const MergeArgs& a);
// each: every launch on `stream`, the answer copied to the host, the stream synchronised.  indexCount must be > 0.
hipError_t merge_plan(const MergeArgs& a, void* head, MergePlan* out, hipStream_t stream);
hipError_t merge_stage(const MergeArgs& a, void* head, void* staging, const MergePlan& plan, MergeRounds* rounds, RebuildCounts* out, hipStream_t stream);
hipError_t merge_emit(const MergeArgs& a, void* head, const void* staging, const RebuildCounts& counts, const RebuildOutputs& o, hipStream_t stream);   // o.index: the source's format

} // namespace ommx
