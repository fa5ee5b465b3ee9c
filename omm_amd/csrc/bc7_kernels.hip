// bc7_kernels.hip -- ommxCreateTextureBC7 / ommxCreateTextureBC7Device: the alpha of BC7 blocks in device memory -> the packed row-major UNORM8
// texel array of a texture mip (TexMip::texels, omm_host.cpp).  A streaming job like block_kernels.hip, whose launch shape this follows: 16 bytes in
// and 16 bytes out per block.  DESIGN.md section 5.16.
//
// A lane owns one block.  It reads the block with one aligned 16-byte load, decodes its alpha with bc7_decode.h, and writes its 4 rows.  Row y of the
// packed array starts at texel y * w, so a block's row of 4 texels is an aligned 4-byte run exactly when w % 4 == 0: then it is one store.  Otherwise,
// and in the partial last block column / row, texels are stored one by one, and none at x >= w or y >= h.  The 64 lanes of a wave take 64
// neighbouring blocks of one block row: one load instruction of a wave covers 1024 contiguous bytes, one store instruction 256.  No LDS, barriers or
// cross-lane operations (the file compiles as host C++ against tests/native/hip_host_shim), no run-time indexed register array, indexing is 64-bit.
#include <hip/hip_runtime.h>
#include "bc7_kernels.h"
#include "bc7_decode.h"

namespace ommx {

struct alignas(16) Bc7Block { uint64_t lo, hi; };

// WHOLE: w % 4 == 0, every block's row of 4 texels is an aligned run of the packed array (and no block column is partial)
template <bool WHOLE>
__global__ __launch_bounds__(256) void bc7_decode(const uint8_t* __restrict__ src, uint64_t pitch, uint8_t* __restrict__ dst, int w, int h)
{
    const uint32_t W = (uint32_t)w, H = (uint32_t)h, bw = (W + 3u) / 4u, bh = (H + 3u) / 4u;
    const uint32_t bx = blockIdx.x * 64u + threadIdx.x;
    for (uint32_t by = blockIdx.y * 4u + threadIdx.y; by < bh; by += gridDim.y * 4u) {
        if (bx >= bw) continue;
        const Bc7Block q = *(const Bc7Block*)(src + (uint64_t)by * pitch + (uint64_t)bx * 16u);
        const uint32_t x0 = 4u * bx, y0 = 4u * by;
        const uint32_t nx = W - x0 < 4u ? W - x0 : 4u, ny = H - y0 < 4u ? H - y0 : 4u;
        uint32_t rows[4];
        bc7_alpha_rows(q.lo, q.hi, rows);
        #pragma unroll
        for (uint32_t y = 0; y < 4u; ++y) {
            if (y >= ny) break;
            uint8_t* o = dst + ((uint64_t)(y0 + y) * (uint64_t)W + (uint64_t)x0);
            if (WHOLE) *(uint32_t*)o = rows[y];
            else {
                #pragma unroll
                for (uint32_t x = 0; x < 4u; ++x) if (x < nx) o[x] = (uint8_t)(rows[y] >> (8u * x));
            }
        }
    }
}

void launch_bc7_decode(const void* src, size_t pitch, void* dst, int w, int h, hipStream_t stream)
{
    const uint32_t bw = ((uint32_t)w + 3u) / 4u, rows4 = (((uint32_t)h + 3u) / 4u + 3u) / 4u;   // 4 block rows per workgroup
    const dim3 grid((bw + 63u) / 64u, rows4 < 65535u ? rows4 : 65535u);
    if ((w & 3) == 0) hipLaunchKernelGGL((bc7_decode<true>), grid, dim3(64, 4), 0, stream, (const uint8_t*)src, (uint64_t)pitch, (uint8_t*)dst, w, h);
    else hipLaunchKernelGGL((bc7_decode<false>), grid, dim3(64, 4), 0, stream, (const uint8_t*)src, (uint64_t)pitch, (uint8_t*)dst, w, h);
}

} // namespace ommx
