// The decode kernels of omm_amd/csrc/block_kernels.hip compiled as host C++ (hip_host_shim) and run lane by lane over exact-size heap blocks, built with
// -fsanitize=address,undefined by tests/test_block_decode_host.py: a load outside a row of blocks, one that is not aligned to its size, or a store at or
// beyond texel w * h stops the program.  Every texel is compared with a decoder written here from the definition in include/omm_mi355x_ext.h -- straight
// loops over bytes, nothing shared with omm_amd/csrc/block_decode.h.
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "block_kernels.hip"
#include <stdio.h>
#include <stdlib.h>
using namespace ommx;

// the 8 bytes at p, by the definition
static uint8_t ref_bc1(const uint8_t* p, int i)
{
    const unsigned c0 = p[0] | (p[1] << 8), c1 = p[2] | (p[3] << 8);
    const unsigned code = (p[4 + i / 4] >> (2 * (i % 4))) & 3u;
    return (c0 <= c1 && code == 3u) ? 0 : 255;
}
static uint8_t ref_bc2(const uint8_t* p, int i)
{
    const unsigned a = (i & 1) ? p[i / 2] >> 4 : p[i / 2] & 15u;
    return (uint8_t)(17u * a);
}
static float ref_bc4(const uint8_t* p, int i)
{
    const int a0 = p[0], a1 = p[1];
    unsigned long long bits = 0;
    for (int b = 0; b < 6; ++b) bits |= (unsigned long long)p[2 + b] << (8 * b);
    const int k = (int)((bits >> (3 * i)) & 7u);
    int n, D;
    if (a0 > a1) { D = 7; n = k == 0 ? 7 * a0 : k == 1 ? 7 * a1 : (8 - k) * a0 + (k - 1) * a1; }
    else { D = 5; n = k == 0 ? 5 * a0 : k == 1 ? 5 * a1 : k == 6 ? 0 : k == 7 ? 5 * 255 : (6 - k) * a0 + (k - 1) * a1; }
    volatile float quotient = (float)n / (float)D;   // (one division, then one multiplication)
    return quotient * (1.f / 255.f);
}

int main()
{
    const int widths[] = { 1, 3, 4, 5, 8, 13, 16, 17, 63, 64, 65, 252, 255, 256, 257, 260 }, heights[] = { 1, 3, 4, 5, 7, 8, 64, 65 };
    // BC1, BC2, BC3, BC4, BC5 channel 0, BC5 channel 1
    const struct { const char* name; int kind, blockBytes, off; } formats[] = { { "BC1", kBlockBC1, 8, 0 }, { "BC2", kBlockBC2, 16, 0 }, { "BC3", kBlockBC4, 16, 0 },
                                                                                { "BC4", kBlockBC4, 8, 0 }, { "BC5.0", kBlockBC4, 16, 0 }, { "BC5.1", kBlockBC4, 16, 8 } };
    long cases = 0;
    for (const auto& f : formats) for (int w : widths) for (int h : heights) for (int pad = 0; pad < 2; ++pad) {
        const int bw = (w + 3) / 4, bh = (h + 3) / 4, ob = f.kind == kBlockBC4 ? 4 : 1;
        const size_t pitch = (size_t)bw * f.blockBytes + (pad ? 8 : 0), need = pitch * (bh - 1) + (size_t)bw * f.blockBytes;
        void* blk = nullptr;
        if (posix_memalign(&blk, 16, need) != 0) return 2;
        uint8_t* src = (uint8_t*)blk;
        for (size_t i = 0; i < need; ++i) src[i] = (uint8_t)(rand() >> 7);
        // (random endpoints are rarely equal or in punch-through order with code 3: force some)
        for (int by = 0; by < bh; ++by) for (int bx = 0; bx < bw; ++bx) {
            uint8_t* p = src + pitch * by + (size_t)bx * f.blockBytes + f.off;
            const int r = rand() % 8;
            if (f.kind == kBlockBC4 && r == 0) p[1] = p[0];
            if (f.kind == kBlockBC1 && r == 0) { p[2] = p[0]; p[3] = p[1]; }
            if (f.kind == kBlockBC1 && r == 1) { p[4] = 0xFF; p[6] |= 0xC3; }
        }
        void* out = nullptr;
        if (posix_memalign(&out, 256, (size_t)w * h * ob) != 0) return 2;
        memset(out, 0xCD, (size_t)w * h * ob);
        launch_block_decode(src, pitch, (uint32_t)f.blockBytes, (uint32_t)f.off, f.kind, out, w, h, nullptr);
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
            const uint8_t* p = src + pitch * (y / 4) + (size_t)(x / 4) * f.blockBytes + f.off;
            const int i = 4 * (y % 4) + x % 4; const size_t t = (size_t)y * w + x;
            bool ok;
            if (f.kind == kBlockBC1) ok = ((uint8_t*)out)[t] == ref_bc1(p, i);
            else if (f.kind == kBlockBC2) ok = ((uint8_t*)out)[t] == ref_bc2(p, i);
            else { const float want = ref_bc4(p, i); ok = memcmp((uint8_t*)out + 4 * t, &want, 4) == 0; }
            if (!ok) { printf("FAIL %s %dx%d pad %d at (%d, %d)\n", f.name, w, h, pad, x, y); return 1; }
        }
        free(out); free(blk); ++cases;
    }
    printf("ok %ld cases\n", cases);
    return 0;
}
