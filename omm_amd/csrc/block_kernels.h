// Decode of the alpha of BC1..BC5 blocks in device memory into the packed row-major texel array of a texture mip
// (ommxCreateTextureBC / ommxCreateTextureBCDevice, include/omm_mi355x_ext.h; kernels in block_kernels.hip; the per-block decode in block_decode.h;
// DESIGN.md section 5.15).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace ommx {

// what the 8 relevant bytes of a block hold: BC1 -> UNORM8 texels, BC2's explicit alpha -> UNORM8 texels, the BC4 block (BC3 alpha, BC4, a BC5 channel) -> fp32 texels
enum BlockKind { kBlockBC1 = 0, kBlockBC2 = 1, kBlockBC4 = 2 };

// src            first block of the mip (device-accessible); src + byteOffset, pitch and blockBytes are multiples of 8
// pitch          bytes from one row of blocks to the next, >= ceil(w / 4) * blockBytes
// blockBytes     8 or 16; byteOffset 0 or 8: where the 8 relevant bytes lie in a block
// dst            w * h packed texels from hipMalloc: bytes (kBlockBC1, kBlockBC2) or fp32 (kBlockBC4)
// Reads exactly the 8 bytes at byteOffset of each of the ceil(w / 4) * ceil(h / 4) blocks; stores nothing at or beyond texel w * h.
void launch_block_decode(const void* src, size_t pitch, uint32_t blockBytes, uint32_t byteOffset, int kind, void* dst, int w, int h, hipStream_t stream);

} // namespace ommx
