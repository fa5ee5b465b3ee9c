// result_block.h -- the two facts about an OMM block that every reader of a result shares: the highest subdivision level the bounds rule admits
// and the bytes a block occupies.  Plain C++ and HIP device code alike: stats_count.h and coarsen_reduce.h (which compile on the host for their
// native checks) and result_read.h (device only) take them from here.  include/omm_mi355x_lookup.h is a public header that stands alone and
// states the same rule with a macro of its own.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define OMMX_BLOCK_FN __host__ __device__ __forceinline__
#else
#define OMMX_BLOCK_FN static inline
#endif

namespace ommx {

constexpr uint32_t kResultMaxLevel = 12u;   // what the bounds rule admits

// bytes a block of `level` <= 12 and fieldBits 1 or 2 occupies
OMMX_BLOCK_FN uint64_t block_bytes(uint32_t level, uint32_t fieldBits) { return (((uint64_t)fieldBits << (2u * level)) + 7u) >> 3; }

} // namespace ommx
