// compare_kernels.h -- ommxCompareMicromaps: the state-by-state difference of two device-resident results over the same primitives
// (compare_kernels.hip; the definition is in include/omm_mi355x_ext.h).  omm_host.cpp owns the baker, its device pool and the argument checks; the
// two calls below are the phases between which the host has to size a block of memory.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"
#include "combine_kernels.h"

namespace ommx {

struct CompareArgs {
    ResultView a, b;               // (result_read.h)
    uint32_t indexCount;           // of both, > 0
    uint32_t force2;               // ommxCompareFlags_Force2State
    uint8_t *relations, *levels;   // device memory of the caller, [indexCount] each, or null
    uint32_t* confusion;           // [indexCount][16], 16-byte aligned, or null
};
struct CompareTotals {             // what the device counted; the host adds the primitives with two special entries from specialCells
    uint64_t totals[16];           // over the pairs: matrix * references * 4^(12 - T)
    uint32_t specialCells[16];     // primitives with two special entries, by [stateA][stateB]
    uint32_t identical, conflict, aWeaker, bWeaker, hint;   // primitives with a pair, by the pair's relation
    uint32_t refined;              // pairs whose sides differ in level or one of which is a special entry
    uint32_t firstConflict;        // lowest primitive with CONFLICT; 0xFFFFFFFF: none
};

size_t compare_head_bytes(const CompareArgs& a);           // scratch per primitive
size_t compare_pair_bytes(uint32_t pairs);                 // scratch per pair
// the front: every launch on `stream`, the answer copied to the host, the stream synchronised
hipError_t compare_pairs(const CompareArgs& a, void* head, CombineTuples* out, hipStream_t stream);
// the streaming pass and the small kernels; perPair may be null when t.tuples == 0.  The caller's outputs are written, *out is copied to the host,
// the stream synchronised
hipError_t compare_count(const CompareArgs& a, void* head, void* perPair, const CombineTuples& t, CompareTotals* out, hipStream_t stream);

} // namespace ommx
