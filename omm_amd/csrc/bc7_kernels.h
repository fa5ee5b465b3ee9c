// Decode of the alpha of BC7 blocks in device memory into the packed row-major UNORM8 texel array of a texture mip
// (ommxCreateTextureBC7 / ommxCreateTextureBC7Device, include/omm_mi355x_ext.h; kernels in bc7_kernels.hip; the per-block decode in bc7_decode.h;
// DESIGN.md section 5.16).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace ommx {

// src            first block of the mip (device-accessible); src and pitch are multiples of 16
// pitch          bytes from one row of blocks to the next, >= ceil(w / 4) * 16
// dst            w * h packed bytes from hipMalloc
// Reads exactly the 16 bytes of each of the ceil(w / 4) * ceil(h / 4) blocks; stores nothing at or beyond texel w * h.
void launch_bc7_decode(const void* src, size_t pitch, void* dst, int w, int h, hipStream_t stream);

} // namespace ommx
