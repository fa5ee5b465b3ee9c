// The decode kernels of omm_amd/csrc/bc7_kernels.hip compiled as host C++ (hip_host_shim) and run lane by lane over exact-size heap blocks, built with
// -fsanitize=address,undefined by tests/test_bc7_decode_host.py: a load outside a row of blocks, one that is not aligned to its 16 bytes, or a store at or
// beyond texel w * h stops the program.  Every texel is compared with a decoder written here from the definition in include/omm_mi355x_ext.h -- one bit at a
// time out of the 16 bytes, tables of its own, nothing shared with omm_amd/csrc/bc7_decode.h.
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "bc7_kernels.hip"
#include <stdio.h>
#include <stdlib.h>
using namespace ommx;

static const unsigned short ref_mask[64] = {
    0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
    0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
    0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A, 0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
    0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C, 0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22 };
static const unsigned char ref_anchor[64] = {
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
    15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15 };
static const int ref_w2[4] = { 0, 21, 43, 64 }, ref_w3[8] = { 0, 9, 18, 27, 37, 46, 55, 64 }, ref_w4[16] = { 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 };

// n bits from bit pos of the 16 bytes at p, one by one
static unsigned ref_bits(const uint8_t* p, int pos, int n)
{
    unsigned v = 0;
    for (int k = 0; k < n; ++k) v |= (unsigned)((p[(pos + k) / 8] >> ((pos + k) % 8)) & 1) << k;
    return v;
}
// index of texel i: n bits each from bit pos, one bit less for texel 0 and texel anchor2
static unsigned ref_index(const uint8_t* p, int pos, int n, int anchor2, int i)
{
    for (int t = 0; t < i; ++t) pos += (t == 0 || t == anchor2) ? n - 1 : n;
    return ref_bits(p, pos, (i == 0 || i == anchor2) ? n - 1 : n);
}
static int ref_lerp(int e0, int e1, int w) { return ((64 - w) * e0 + w * e1 + 32) >> 6; }
static const int* ref_weights(int n) { return n == 2 ? ref_w2 : n == 3 ? ref_w3 : ref_w4; }

static uint8_t ref_bc7(const uint8_t* p, int i)
{
    if (p[0] == 0) return 0;
    int m = 0;
    while (!((p[0] >> m) & 1)) ++m;
    if (m < 4) return 255;
    if (m == 4) {
        const int rot = (int)ref_bits(p, 5, 2), idxMode = (int)ref_bits(p, 7, 1);
        const int colourBits = idxMode ? 3 : 2, alphaBits = idxMode ? 2 : 3;
        int e0, e1, n;
        if (rot == 0) { const int a0 = (int)ref_bits(p, 38, 6), a1 = (int)ref_bits(p, 44, 6); e0 = (a0 << 2) | (a0 >> 4); e1 = (a1 << 2) | (a1 >> 4); n = alphaBits; }
        else { const int c0 = (int)ref_bits(p, 8 + 10 * (rot - 1), 5), c1 = (int)ref_bits(p, 13 + 10 * (rot - 1), 5); e0 = (c0 << 3) | (c0 >> 2); e1 = (c1 << 3) | (c1 >> 2); n = colourBits; }
        return (uint8_t)ref_lerp(e0, e1, ref_weights(n)[ref_index(p, n == 2 ? 50 : 81, n, -1, i)]);
    }
    if (m == 5) {
        const int rot = (int)ref_bits(p, 6, 2);
        int e0, e1, pos;
        if (rot == 0) { e0 = (int)ref_bits(p, 50, 8); e1 = (int)ref_bits(p, 58, 8); pos = 97; }
        else { const int c0 = (int)ref_bits(p, 8 + 14 * (rot - 1), 7), c1 = (int)ref_bits(p, 15 + 14 * (rot - 1), 7); e0 = (c0 << 1) | (c0 >> 6); e1 = (c1 << 1) | (c1 >> 6); pos = 66; }
        return (uint8_t)ref_lerp(e0, e1, ref_w2[ref_index(p, pos, 2, -1, i)]);
    }
    if (m == 6) {
        const int e0 = (int)((ref_bits(p, 49, 7) << 1) | ref_bits(p, 63, 1)), e1 = (int)((ref_bits(p, 56, 7) << 1) | ref_bits(p, 64, 1));
        return (uint8_t)ref_lerp(e0, e1, ref_w4[ref_index(p, 65, 4, -1, i)]);
    }
    const int part = (int)ref_bits(p, 8, 6), s = (ref_mask[part] >> i) & 1;
    int e[2];
    for (int k = 0; k < 2; ++k) { const int v = (int)((ref_bits(p, 74 + 5 * (2 * s + k), 5) << 1) | ref_bits(p, 94 + 2 * s + k, 1)); e[k] = (v << 2) | (v >> 4); }
    return (uint8_t)ref_lerp(e[0], e[1], ref_w2[ref_index(p, 98, 2, ref_anchor[part], i)]);
}

int main()
{
    const int widths[] = { 1, 3, 4, 5, 8, 13, 16, 17, 63, 64, 65, 252, 255, 256, 257, 260 }, heights[] = { 1, 3, 4, 5, 7, 8, 64, 65 };
    long cases = 0, alphaBlocks[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int w : widths) for (int h : heights) for (int pad = 0; pad < 2; ++pad) {
        const int bw = (w + 3) / 4, bh = (h + 3) / 4;
        const size_t pitch = (size_t)bw * 16 + (pad ? 16 : 0), need = pitch * (bh - 1) + (size_t)bw * 16;
        void* blk = nullptr;
        if (posix_memalign(&blk, 16, need) != 0) return 2;
        uint8_t* src = (uint8_t*)blk;
        for (size_t i = 0; i < need; ++i) src[i] = (uint8_t)(rand() >> 7);
        // (a block of random bytes has an alpha 6 % of the time: 5 of 8 blocks get one of the modes 4..7, one in 32 the reserved byte)
        for (int by = 0; by < bh; ++by) for (int bx = 0; bx < bw; ++bx) {
            uint8_t* p = src + pitch * by + (size_t)bx * 16;
            const int r = rand() % 32;
            if (r < 20) { const int m = 4 + r % 4; p[0] = (uint8_t)((p[0] & (0xFF ^ ((1 << (m + 1)) - 1))) | (1 << m)); }
            else if (r == 20) p[0] = 0;
            int m = 8;
            if (p[0]) { m = 0; while (!((p[0] >> m) & 1)) ++m; }
            ++alphaBlocks[m];
        }
        void* out = nullptr;
        if (posix_memalign(&out, 256, (size_t)w * h) != 0) return 2;
        memset(out, 0xCD, (size_t)w * h);
        launch_bc7_decode(src, pitch, out, w, h, nullptr);
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
            const uint8_t* p = src + pitch * (y / 4) + (size_t)(x / 4) * 16;
            const uint8_t want = ref_bc7(p, 4 * (y % 4) + x % 4), got = ((uint8_t*)out)[(size_t)y * w + x];
            if (got != want) { printf("FAIL %dx%d pad %d at (%d, %d): mode byte %02x, got %d, want %d\n", w, h, pad, x, y, p[0], got, want); return 1; }
        }
        free(out); free(blk); ++cases;
    }
    for (int m = 0; m < 9; ++m) if (alphaBlocks[m] < 100) { printf("FAIL only %ld blocks of mode %d\n", alphaBlocks[m], m); return 1; }
    printf("ok %ld cases\n", cases);
    return 0;
}
