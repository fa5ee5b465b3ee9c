/* Just enough of the HIP language to compile omm_amd/csrc/texture_kernels.hip as host C++ (tests/native/texture_gather_host.cpp): qualifiers vanish, a launch is
 * a loop over the grid's workgroups and lanes, one at a time.  The gather has no barriers, LDS or cross-lane operations, so this runs what the device runs. */
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return uint2{ a, b }; }
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{ a, b, c, d }; }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
typedef void* hipStream_t;
extern dim3 blockIdx, threadIdx, gridDim, blockDim;
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) do { const dim3 G_ = (grid), B_ = (block); gridDim = G_; blockDim = B_; \
    for (unsigned by_ = 0; by_ < G_.y; ++by_) for (unsigned bx_ = 0; bx_ < G_.x; ++bx_) for (unsigned ty_ = 0; ty_ < B_.y; ++ty_) for (unsigned tx_ = 0; tx_ < B_.x; ++tx_) { \
        blockIdx = dim3(bx_, by_); threadIdx = dim3(tx_, ty_); kernel(__VA_ARGS__); } } while (0)
