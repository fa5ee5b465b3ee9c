// result_read.h -- reading a caller's result on the device: an index entry of any index format, a descriptor, and the bounds rule that decides
// whether a descriptor may be read through.  Used by the statistics, the micro-geometry, ommxCoarsenMicromap and ommxCombineMicromaps.  The rule is
// that of ommx_opacity_state in include/omm_mi355x_lookup.h (a public header that stands alone); the bounds tables of the coarsen, combine and
// statistics GPU tests hold the two statements together.
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

} // namespace ommx
