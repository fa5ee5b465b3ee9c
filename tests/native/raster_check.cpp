// raster_check.cpp -- omm_amd/csrc/raster_cover.h and png_store.h as host code, a stand-alone program for the sanitizers (tests/test_rasterize.py):
//   1. coverage, barycentrics and the box on dyadic inputs (vertices on a 1/64 grid, power-of-two viewports and sizes: every sample point and every cross
//      product is then exact) against an evaluation in 128-bit integers and long double;
//   2. the colour arithmetic for all 5 states x 256 greys x 8 flag combinations against a per-channel table;
//   3. the PNG writer into a temporary file, read back chunk by chunk with a bitwise CRC-32, a byte-wise Adler-32 and a stored-block reader of its own.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "raster_cover.h"
#include "png_store.h"

using namespace ommx;

static long long checks = 0, failures = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { if (++failures <= 20) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

typedef __int128 wide;
static int sign_of(wide x) { return x > 0 ? 1 : (x < 0 ? -1 : 0); }

// vertices k / 64 with |k| <= 256; the viewport [lo, lo + 2^e] with lo = j / 64 and a power-of-two size n: the sample point of pixel i is
// lo + (2 i + 1) * 2^(e - 1) / n, a multiple of 2^-S for S = 20.  Everything is scaled by 2^S into integers.
static void check_cover()
{
    const int S = 20;
    for (int trial = 0; trial < 4000; ++trial) {
        int k[6];
        for (int q = 0; q < 6; ++q) k[q] = (int)(rnd() % 257u) - 128;
        if (trial % 7 == 0) { k[4] = k[0] + 2 * (k[2] - k[0]); k[5] = k[1] + 2 * (k[3] - k[1]); }   // collinear
        if (trial % 11 == 0) { k[2] = k[0]; k[3] = k[1]; }                                           // a repeated vertex
        RasterTri t;
        t.ax = k[0] / 64.0; t.ay = k[1] / 64.0; t.bx = k[2] / 64.0; t.by = k[3] / 64.0; t.cx = k[4] / 64.0; t.cy = k[5] / 64.0;
        const int e = (int)(rnd() % 4u) - 1;                  // extent 2^e: 0.5 .. 4
        const uint32_t n = 1u << (1 + rnd() % 5u);            // 2 .. 32 pixels
        const int j = (int)(rnd() % 257u) - 192;
        const float lo[2] = { j / 64.f, (j + 16) / 64.f };
        const float ext = e >= 0 ? (float)(1 << e) : 0.5f;
        const float hi[2] = { lo[0] + ext, lo[1] + ext };
        const RasterView v = raster_view(lo, hi, n, n);
        const double area2 = raster_area2(t);
        const wide unit = (wide)1 << (S - 6);   // 1 / 64
        const wide X[3] = { k[0] * unit, k[2] * unit, k[4] * unit }, Y[3] = { k[1] * unit, k[3] * unit, k[5] * unit };
        const wide area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
        CHECK(raster_degenerate(area2) == (area == 0), "trial %d", trial);
        CHECK((long double)area2 * (long double)(1ull << S) * (long double)(1ull << S) == (long double)area, "trial %d: area2", trial);
        if (area == 0) continue;
        uint32_t box[4] = { 0, 0, 0, 0 };
        const bool any = raster_box(t, v, box);
        CHECK(box[1] <= n && box[3] <= n, "trial %d: box beyond the view", trial);
        for (uint32_t y = 0; y < n; ++y)
            for (uint32_t x = 0; x < n; ++x) {
                const double U = raster_sample(v.loU, v.stepU, x), V = raster_sample(v.loV, v.stepV, y);
                // lo * 2^S + (2 i + 1) * 2^(S + e - 1) / n
                const wide PU = j * unit + (wide)(2 * x + 1) * (((wide)1 << (S + e + 4)) / n) / 32;
                const wide PV = (j + 16) * unit + (wide)(2 * y + 1) * (((wide)1 << (S + e + 4)) / n) / 32;
                CHECK((long double)U * (long double)(1ull << S) == (long double)PU && (long double)V * (long double)(1ull << S) == (long double)PV, "trial %d: sample point", trial);
                double w[3];
                raster_edges(t, U, V, w);
                const wide W[3] = { (X[1] - PU) * (Y[2] - PV) - (Y[1] - PV) * (X[2] - PU), (X[2] - PU) * (Y[0] - PV) - (Y[2] - PV) * (X[0] - PU),
                                    (X[0] - PU) * (Y[1] - PV) - (Y[0] - PV) * (X[1] - PU) };
                bool inside = true;
                for (int q = 0; q < 3; ++q) {
                    CHECK((long double)w[q] * (long double)(1ull << S) * (long double)(1ull << S) == (long double)W[q], "trial %d: w[%d]", trial, q);
                    inside = inside && (sign_of(W[q]) == 0 || sign_of(W[q]) == sign_of(area));
                }
                CHECK(W[0] + W[1] + W[2] == area, "trial %d: the three areas add up", trial);
                CHECK(raster_covers(w, area2) == inside, "trial %d pixel %u %u", trial, x, y);
                if (!inside) continue;
                CHECK(any && x >= box[0] && x < box[1] && y >= box[2] && y < box[3], "trial %d: covered pixel %u %u outside the box %u %u %u %u", trial, x, y, box[0], box[1], box[2], box[3]);
                float bu, bv;
                raster_barycentrics(w, area2, &bu, &bv);
                const long double eu = (long double)W[1] / (long double)area, ev = (long double)W[2] / (long double)area;
                CHECK(bu == (float)(double)eu && bv == (float)(double)ev, "trial %d: barycentrics", trial);
                CHECK(bu >= 0.f && bv >= 0.f && bu <= 1.f && bv <= 1.f, "trial %d: barycentrics out of range", trial);
                // the hit convention: (1-u-v) A + u B + v C is the sample point
                const long double rx = (1 - eu - ev) * t.ax + eu * t.bx + ev * t.cx, ry = (1 - eu - ev) * t.ay + eu * t.by + ev * t.cy;
                CHECK(rx - U < 1e-15L && U - rx < 1e-15L && ry - V < 1e-15L && V - ry < 1e-15L, "trial %d: the barycentrics do not give the point back", trial);
            }
    }
    // not finite: NaN and the infinities are degenerate; the box of a triangle far outside is empty, of one all around is the view
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    CHECK(raster_degenerate(nan) && raster_degenerate(inf) && raster_degenerate(-inf) && raster_degenerate(0.0) && raster_degenerate(-0.0) && !raster_degenerate(1e-300), "degenerate");
    const float lo[2] = { 0.f, 0.f }, hi[2] = { 1.f, 1.f };
    const RasterView v = raster_view(lo, hi, 257, 65);
    uint32_t box[4];
    RasterTri far = { 5, 5, 6, 5, 5, 6 };
    CHECK(!raster_box(far, v, box), "a triangle beyond the view");
    RasterTri around = { -3e38, -3e38, 3e38, -3e38, 0, 3e38 };
    CHECK(raster_box(around, v, box) && box[0] == 0 && box[1] == 257 && box[2] == 0 && box[3] == 65, "a triangle around the view");
    RasterTri left = { -1, 0.5, -0.5, 0.5, -1, 0.6 };
    CHECK(!raster_box(left, v, box), "a triangle left of the view");
}

static void check_colours()
{
    static const int lut[5][3] = { { 0, 0, 255 }, { 0, 255, 0 }, { 255, 0, 255 }, { 255, 255, 0 }, { 255, 128, 0 } };
    for (uint32_t s = 0; s < 5; ++s)
        for (uint32_t g = 0; g < 256; ++g)
            for (uint32_t f = 0; f < 8; ++f) {
                const bool mono = f & 1, inverted = f & 2, reused = f & 4;
                const uint32_t px = raster_covered(s == 4 ? 0xFFu : s, g, mono, inverted, reused);
                const int* row = lut[(mono && s == 2) ? 3 : s];
                for (int ch = 0; ch < 3; ++ch) {
                    int c = (row[ch] + (int)g + 1) / 2;
                    if (inverted) c = c - c / 8;
                    if (reused) c = c / 2;
                    CHECK((int)((px >> (8 * ch)) & 0xFF) == c, "state %u grey %u flags %u channel %d", s, g, f, ch);
                }
                CHECK((px >> 24) == 255, "alpha");
            }
    for (uint32_t g = 0; g < 256; ++g) {
        CHECK(raster_background(g) == (0xFF000000u | g * 0x010101u), "background %u", g);
        CHECK(raster_grey((float)g / 255.f) == g, "grey of %u / 255", g);
    }
    CHECK(raster_grey(-1.f) == 0 && raster_grey(2.f) == 255 && raster_grey(__builtin_nanf("")) == 0 && raster_grey(__builtin_inff()) == 255 && raster_grey(0.5f) == 128, "grey at the ends");
    CHECK(raster_covered(7u, 0, false, false, false) == raster_covered(0xFFu, 0, false, false, false), "any other state is the invalid colour");
}

static uint32_t crc_bitwise(const uint8_t* p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) { c ^= p[i]; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); }
    return ~c;
}
static uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

static void check_png(const char* path, uint32_t w, uint32_t h, size_t pitch)
{
    std::vector<uint8_t> img(pitch * h);
    for (auto& b : img) b = (uint8_t)rnd();
    FILE* f = fopen(path, "wb");
    CHECK(f != nullptr, "cannot create %s", path);
    if (!f) return;
    const bool ok = png_store_rgba8(f, img.data(), w, h, pitch);
    fclose(f);
    CHECK(ok, "png_store_rgba8 %u x %u", w, h);
    f = fopen(path, "rb");
    std::vector<uint8_t> file;
    for (int c; (c = fgetc(f)) != EOF; ) file.push_back((uint8_t)c);
    fclose(f);
    remove(path);
    static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n' };
    CHECK(file.size() > 8 && memcmp(file.data(), sig, 8) == 0, "signature");
    size_t at = 8; int chunk = 0; std::vector<uint8_t> z;
    static const char* names[3] = { "IHDR", "IDAT", "IEND" };
    while (at + 12 <= file.size() && chunk < 3) {
        const uint32_t len = be32(&file[at]);
        CHECK(at + 12 + (size_t)len <= file.size() && memcmp(&file[at + 4], names[chunk], 4) == 0, "chunk %d", chunk);
        if (at + 12 + (size_t)len > file.size()) return;
        CHECK(crc_bitwise(&file[at + 4], 4 + (size_t)len) == be32(&file[at + 8 + len]), "CRC of %s", names[chunk]);
        if (chunk == 0) {
            CHECK(len == 13 && be32(&file[at + 8]) == w && be32(&file[at + 12]) == h && file[at + 16] == 8 && file[at + 17] == 6 && file[at + 18] == 0 && file[at + 19] == 0 && file[at + 20] == 0, "IHDR");
        }
        if (chunk == 1) z.assign(file.begin() + at + 8, file.begin() + at + 8 + len);
        if (chunk == 2) CHECK(len == 0, "IEND");
        at += 12 + (size_t)len; ++chunk;
    }
    CHECK(chunk == 3 && at == file.size(), "three chunks and nothing behind them");
    // the zlib stream: header, stored blocks, Adler-32
    CHECK(z.size() >= 6 && z[0] == 0x78 && ((z[0] << 8) | z[1]) % 31 == 0 && !(z[1] & 0x20), "zlib header");
    std::vector<uint8_t> raw; size_t p = 2; bool last = false;
    while (!last && p + 5 <= z.size()) {
        last = z[p] == 1;
        CHECK(z[p] <= 1, "a stored block");
        const uint32_t n = z[p + 1] | (z[p + 2] << 8), nn = z[p + 3] | (z[p + 4] << 8);
        CHECK((n ^ nn) == 0xFFFFu && p + 5 + n <= z.size(), "block length");
        if (p + 5 + n > z.size()) return;
        CHECK(last || n == 65535u, "only the last block may be short");
        raw.insert(raw.end(), z.begin() + p + 5, z.begin() + p + 5 + n);
        p += 5 + n;
    }
    CHECK(last && p + 4 == z.size(), "the stream ends with the Adler-32");
    uint32_t a = 1, b = 0;
    for (uint8_t v : raw) { a = (a + v) % 65521u; b = (b + a) % 65521u; }
    CHECK(p + 4 <= z.size() && be32(&z[p]) == ((b << 16) | a), "Adler-32");
    CHECK(raw.size() == (size_t)h * (1 + 4 * (size_t)w), "raw size");
    if (raw.size() != (size_t)h * (1 + 4 * (size_t)w)) return;
    bool rows = true;
    for (uint32_t y = 0; y < h; ++y) rows = rows && raw[y * (1 + 4 * (size_t)w)] == 0 && memcmp(&raw[y * (1 + 4 * (size_t)w) + 1], &img[y * pitch], 4 * (size_t)w) == 0;
    CHECK(rows, "filter byte 0 and the pixels of every row");
}

int main(int argc, char** argv)
{
    const char* path = argc > 1 ? argv[1] : "raster_check.png";
    check_cover();
    check_colours();
    check_png(path, 1, 1, 4);
    check_png(path, 3, 2, 12);
    check_png(path, 3, 2, 19);          // a pitch that is not a multiple of 4
    check_png(path, 16384, 1, 65536);   // one row longer than a stored block
    check_png(path, 16383, 5, 65532);   // a row of exactly 65 533 bytes: blocks end inside rows
    check_png(path, 257, 65, 1028);
    CHECK(png_crc32(0, (const uint8_t*)"123456789", 9) == 0xCBF43926u, "CRC-32 check value");
    CHECK(png_adler32(1, (const uint8_t*)"Wikipedia", 9) == 0x11E60398u, "Adler-32 check value");
    printf("raster_check: %lld checks, %lld failures\n", checks, failures);
    return failures ? 1 : 0;
}
