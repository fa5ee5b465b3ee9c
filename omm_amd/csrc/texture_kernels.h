// Gather of ONE channel of an interleaved image in device memory into the packed row-major texel array of a texture mip
// (ommxCreateTextureDevice, include/omm_mi355x_ext.h; kernels in texture_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace ommx {

enum TexGatherFormat { kTexGatherUnorm8 = 0, kTexGatherFp32 = 1, kTexGatherFp16 = 2 };

// bytes of one channel of the format (1, 4, 2)
size_t tex_gather_channel_bytes(int format);

// src            first pixel of the mip (device-accessible), aligned to the channel size only
// pitch, stride  bytes from row to row / pixel to pixel, channelOffset the byte offset of the channel inside a pixel; all multiples of the channel size,
//                channelOffset + channel size <= stride, pitch >= w * stride
// dst            w * h packed texels from hipMalloc: the source bytes (UNORM8), the source bit patterns (FP32) or the exact fp32 widening of each half (FP16)
// Reads only bytes of [row start, row start + w * stride) of each row and uses only those of the channel.  Returns the path taken (for tests and the
// design notes): 1 = the group's bytes in aligned vector loads, 0 = one channel-sized load per texel.
int launch_texture_gather(const void* src, size_t pitch, uint32_t stride, uint32_t channelOffset, int format, void* dst, int w, int h, hipStream_t stream);

} // namespace ommx
