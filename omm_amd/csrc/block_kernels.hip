// block_kernels.hip -- ommxCreateTextureBC / ommxCreateTextureBCDevice: the alpha of BC1..BC5 blocks in device memory -> the packed row-major
// texel array of a texture mip (TexMip::texels, omm_host.cpp).  A pure streaming job like texture_kernels.hip: 8 bytes in per block, 16 bytes
// (UNORM8) or 64 bytes (fp32) out.  DESIGN.md section 5.15.
//
// A lane owns one block.  It reads the block's 8 relevant bytes with one aligned 8-byte load (the colour half of a BC2 / BC3 block and the other
// channel of a BC5 block are never touched), decodes them with block_decode.h, and writes its 4 rows.  Row y of the packed array starts at texel
// y * w, so a block's row of 4 texels is an aligned 4-byte (UNORM8) or 16-byte (fp32) run exactly when w % 4 == 0: then it is one store.
// Otherwise, and in the partial last block column / row, texels are stored one by one, and none at x >= w or y >= h: the codes of such texels
// are decoded to nothing.  The 64 lanes of a wave take 64 neighbouring blocks of one block row, so each store instruction of a wave covers one
// contiguous run of 256 or 1024 bytes.  No LDS, barriers or cross-lane operations (the file compiles as host C++ against
// tests/native/hip_host_shim), no run-time indexed register array (block_bc4_select), indexing is 64-bit.
//
// The fp32 values depend on -ffp-contract=off and on IEEE-correct division: see block_decode.h.
#include <hip/hip_runtime.h>
#include "block_kernels.h"
#include "block_decode.h"

namespace ommx {

// WHOLE: w % 4 == 0, every block's row of 4 texels is an aligned run of the packed array (and no block column is partial)
template <int KIND, bool WHOLE>
__global__ __launch_bounds__(256) void block_decode(const uint8_t* __restrict__ src, uint64_t pitch, uint32_t blockBytes, uint32_t byteOffset,
                                                    void* __restrict__ dst, int w, int h)
{
    const uint32_t W = (uint32_t)w, H = (uint32_t)h, bw = (W + 3u) / 4u, bh = (H + 3u) / 4u;
    const uint32_t bx = blockIdx.x * 64u + threadIdx.x;
    for (uint32_t by = blockIdx.y * 4u + threadIdx.y; by < bh; by += gridDim.y * 4u) {
        if (bx >= bw) continue;
        const uint64_t q = *(const uint64_t*)(src + (uint64_t)by * pitch + (uint64_t)bx * blockBytes + byteOffset);
        const uint32_t x0 = 4u * bx, y0 = 4u * by;
        const uint32_t nx = W - x0 < 4u ? W - x0 : 4u, ny = H - y0 < 4u ? H - y0 : 4u;
        uint32_t pal[8];
        if (KIND == kBlockBC4) block_bc4_palette(q, pal);
        #pragma unroll
        for (uint32_t y = 0; y < 4u; ++y) {
            if (y >= ny) break;
            const uint64_t i = (uint64_t)(y0 + y) * (uint64_t)W + (uint64_t)x0;
            if (KIND == kBlockBC4) {
                uint32_t v[4];
                #pragma unroll
                for (uint32_t x = 0; x < 4u; ++x) v[x] = block_bc4_select(pal, block_bc4_code(q, 4u * y + x));
                uint32_t* o = (uint32_t*)dst + i;
                if (WHOLE) *(uint4*)o = make_uint4(v[0], v[1], v[2], v[3]);
                else {
                    #pragma unroll
                    for (uint32_t x = 0; x < 4u; ++x) if (x < nx) o[x] = v[x];
                }
            } else {
                const uint32_t r = KIND == kBlockBC1 ? block_bc1_row(q, y) : block_bc2_row(q, y);
                uint8_t* o = (uint8_t*)dst + i;
                if (WHOLE) *(uint32_t*)o = r;
                else {
                    #pragma unroll
                    for (uint32_t x = 0; x < 4u; ++x) if (x < nx) o[x] = (uint8_t)(r >> (8u * x));
                }
            }
        }
    }
}

template <int KIND>
static void launch_kind(const void* src, size_t pitch, uint32_t blockBytes, uint32_t byteOffset, void* dst, int w, int h, hipStream_t stream)
{
    const uint32_t bw = ((uint32_t)w + 3u) / 4u, rows4 = (((uint32_t)h + 3u) / 4u + 3u) / 4u;   // 4 block rows per workgroup
    const dim3 grid((bw + 63u) / 64u, rows4 < 65535u ? rows4 : 65535u);
    if ((w & 3) == 0) hipLaunchKernelGGL((block_decode<KIND, true>), grid, dim3(64, 4), 0, stream, (const uint8_t*)src, (uint64_t)pitch, blockBytes, byteOffset, dst, w, h);
    else hipLaunchKernelGGL((block_decode<KIND, false>), grid, dim3(64, 4), 0, stream, (const uint8_t*)src, (uint64_t)pitch, blockBytes, byteOffset, dst, w, h);
}

void launch_block_decode(const void* src, size_t pitch, uint32_t blockBytes, uint32_t byteOffset, int kind, void* dst, int w, int h, hipStream_t stream)
{
    if (kind == kBlockBC1) launch_kind<kBlockBC1>(src, pitch, blockBytes, byteOffset, dst, w, h, stream);
    else if (kind == kBlockBC2) launch_kind<kBlockBC2>(src, pitch, blockBytes, byteOffset, dst, w, h, stream);
    else launch_kind<kBlockBC4>(src, pitch, blockBytes, byteOffset, dst, w, h, stream);
}

} // namespace ommx
