// result_read.h -- reading a caller's result on the device: an index entry of any index format, a descriptor, and the bounds rule that decides
// whether a descriptor may be read through -- used by the statistics, the micro-geometry, ommxCoarsenMicromap, ommxCombineMicromaps and
// ommxGatherMicromaps -- and, for the operations that derive a new result, ResultView (a source as a kernel sees it) and the selection rule: what
// a primitive of a source selects.  The bounds rule is that of ommx_opacity_state in include/omm_mi355x_lookup.h (a public header that stands alone);
// the bounds tables of the coarsen, combine, gather and statistics GPU tests hold the two statements together.  The selection rule stands once, here,
// for the mark and index kernels of the coarsening and the gather; combine_entries states it again, around the descriptor it has to keep.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/omm_mi355x.h"
#include "result_block.h"

namespace ommx {

__device__ __forceinline__ int32_t index_entry(const void* index, int format, uint64_t i)
{
    if (format == ommIndexFormat_UINT_8) return ((const int8_t*)index)[i];
    if (format == ommIndexFormat_UINT_16) return ((const int16_t*)index)[i];
    return ((const int32_t*)index)[i];
}
__device__ __forceinline__ void index_store(void* index, int format, uint64_t i, int32_t v)
{
    if (format == ommIndexFormat_UINT_8) ((int8_t*)index)[i] = (int8_t)v;
    else if (format == ommIndexFormat_UINT_16) ((int16_t*)index)[i] = (int16_t)v;
    else ((int32_t*)index)[i] = v;
}

// A descriptor is read ONCE, as one 8-byte load, and judged from registers (a caller's array is only 4-byte aligned: the hardware takes that).
typedef uint32_t DescWords __attribute__((vector_size(8), aligned(4), may_alias));
__device__ __forceinline__ ommCpuOpacityMicromapDesc load_desc(const ommCpuOpacityMicromapDesc* p)
{
    const DescWords w = *(const DescWords*)p;
    ommCpuOpacityMicromapDesc d; d.offset = w[0]; d.subdivisionLevel = (uint16_t)(w[1] & 0xFFFFu); d.format = (uint16_t)(w[1] >> 16);
    return d;
}

// The bounds rule: level <= 12, format 1 or 2, block inside arrayDataSize.  *bytes <- the block's size (when level and format pass).
__device__ __forceinline__ bool desc_ok(const ommCpuOpacityMicromapDesc d, uint32_t arrayDataSize, uint64_t* bytes)
{
    const uint32_t level = d.subdivisionLevel, bits = d.format;
    if (level > kResultMaxLevel || (bits != 1u && bits != 2u)) return false;
    *bytes = block_bytes(level, bits);
    return (uint64_t)d.offset + *bytes <= (uint64_t)arrayDataSize;
}
__device__ __forceinline__ bool desc_ok(const ommCpuOpacityMicromapDesc d, uint32_t arrayDataSize) { uint64_t bytes; return desc_ok(d, arrayDataSize, &bytes); }

// A source result as the kernels of a derived result read it: arrays in device memory, indexFormat already checked.
struct ResultView {
    const uint8_t* arrayData; const ommCpuOpacityMicromapDesc* descs; const void* index;
    uint32_t arrayDataSize, descCount, indexCount; int32_t indexFormat;
};
__host__ __device__ inline ResultView view_of(const ommCpuBakeResultDesc& r)
{
    ResultView v;
    v.arrayData = (const uint8_t*)r.arrayData; v.descs = r.descArray; v.index = r.indexBuffer;
    v.arrayDataSize = r.arrayDataSize; v.descCount = r.descArrayCount; v.indexCount = r.indexCount; v.indexFormat = (int32_t)r.indexFormat;
    return v;
}

// The selection rule: what primitive p of a source selects.
//   -1 .. -4   a special entry, which passes through
//   e >= 0     descriptor e: it is in range and passes the bounds rule
//   kSkipped   nothing: the primitive is skipped
// named_entry is the part that needs no descriptor (e >= 0: descriptor e is in range).  Behind the mark pass an operation has one word per descriptor,
// non-zero for a descriptor that a primitive selected; it stands for the bounds rule there, so that no descriptor is read a second time
// (index_back in rebuild_kernels.h).
constexpr int32_t kSkipped = -5;
__device__ __forceinline__ int32_t named_entry(const ResultView& s, uint64_t p)
{
    const int32_t e = index_entry(s.index, s.indexFormat, p);
    if (e < 0) return e >= -4 ? e : kSkipped;
    return (uint32_t)e < s.descCount ? e : kSkipped;
}
__device__ __forceinline__ int32_t select_entry(const ResultView& s, uint64_t p)
{
    const int32_t e = named_entry(s, p);
    return e >= 0 && !desc_ok(load_desc(s.descs + e), s.arrayDataSize) ? kSkipped : e;
}
// the mark pass: the descriptor that p selects is marked in marks[descCount]; -> 1 where p is skipped
__device__ __forceinline__ uint32_t mark_selected(const ResultView& s, uint64_t p, uint32_t* __restrict__ marks)
{
    const int32_t e = select_entry(s, p);
    if (e >= 0) atomicOr(&marks[e], 1u);
    return e == kSkipped ? 1u : 0u;
}

} // namespace ommx
