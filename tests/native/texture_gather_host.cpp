// The gather kernels of omm_amd/csrc/texture_kernels.hip compiled as host C++ (hip_host_shim) and run lane by lane over exact-size heap blocks, built with
// -fsanitize=address,undefined by tests/test_texture_gather_host.py: a load that leaves [first pixel of the mip, last pixel's end) or is not aligned to its
// size stops the program; the texels are compared with a plain per-pixel extraction, every half bit pattern with the F16C conversion.
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "texture_kernels.hip"
#include <immintrin.h>
#include <stdio.h>
#include <stdlib.h>
using namespace ommx;

static bool same_float(uint16_t h, uint32_t got)
{
    const float f = _cvtsh_ss(h); uint32_t want; memcpy(&want, &f, 4);
    if (f != f) return (got & 0x7F800000u) == 0x7F800000u && (got & 0x7FFFFFu) != 0;   // NaN stays NaN
    return got == want;
}

int main()
{
    const int widths[] = { 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257 }, heights[] = { 1, 4, 5 };
    const struct { int format, stride; } layouts[] = { { 0, 1 }, { 0, 2 }, { 0, 3 }, { 0, 4 }, { 0, 5 }, { 2, 2 }, { 2, 4 }, { 2, 6 }, { 2, 8 }, { 1, 4 }, { 1, 8 }, { 1, 12 }, { 1, 16 } };
    long cases = 0;
    for (const auto& l : layouts) {
        const int cb = (int)tex_gather_channel_bytes(l.format), ob = l.format == kTexGatherUnorm8 ? 1 : 4;
        for (int off = 0; off + cb <= l.stride; off += cb)
        for (int w : widths) for (int h : heights) for (int pad = 0; pad < 2; ++pad) for (int disp = 0; disp < 3; ++disp) {
            const size_t pitch = (size_t)w * l.stride + (pad ? (size_t)cb * 3 : 0), need = pitch * (h - 1) + (size_t)w * l.stride;
            const size_t d = disp == 0 ? 0 : disp == 1 ? (size_t)l.stride : (size_t)cb;   // base: 16-byte aligned, displaced by a pixel, by a channel
            void* blk = nullptr;
            if (posix_memalign(&blk, 16, d + need) != 0) return 2;
            uint8_t* src = (uint8_t*)blk + d;
            for (size_t i = 0; i < d + need; ++i) ((uint8_t*)blk)[i] = (uint8_t)rand();
            void* out = nullptr;
            if (posix_memalign(&out, 256, (size_t)w * h * ob) != 0) return 2;
            memset(out, 0xCD, (size_t)w * h * ob);
            launch_texture_gather(src, pitch, (uint32_t)l.stride, (uint32_t)off, l.format, out, w, h, nullptr);
            for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
                const uint8_t* p = src + pitch * y + (size_t)x * l.stride + off; const size_t i = (size_t)y * w + x;
                bool ok;
                if (l.format == kTexGatherUnorm8) ok = ((uint8_t*)out)[i] == *p;
                else if (l.format == kTexGatherFp32) ok = memcmp((uint8_t*)out + 4 * i, p, 4) == 0;
                else { uint16_t hb; memcpy(&hb, p, 2); ok = same_float(hb, ((uint32_t*)out)[i]); }
                if (!ok) { printf("FAIL format %d stride %d offset %d %dx%d pad %d base %d at (%d, %d)\n", l.format, l.stride, off, w, h, pad, disp, x, y); return 1; }
            }
            free(out); free(blk); ++cases;
        }
    }
    for (uint32_t hb = 0; hb < 65536; ++hb) if (!same_float((uint16_t)hb, half_to_float_bits(hb))) { printf("FAIL half %04x\n", hb); return 1; }
    printf("ok %ld cases\n", cases);
    return 0;
}
