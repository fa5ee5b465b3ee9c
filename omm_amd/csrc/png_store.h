// png_store.h -- ommxDebugSaveImagePNG's writer as plain C++ (omm_host.cpp; tests/native/raster_check.cpp): an 8-bit RGBA image as a PNG whose one
// IDAT chunk holds one zlib stream of stored (uncompressed) deflate blocks.  CRC-32 (chunks) and Adler-32 (zlib) are computed here.
#pragma once
#include <stdint.h>
#include <stdio.h>

namespace ommx {

constexpr uint32_t kPngStoredBlock = 65535;   // the most a stored deflate block holds

inline uint32_t png_crc32(uint32_t crc, const uint8_t* p, size_t n)   // running value: start with 0, feed the bytes in order
{
    struct Table {
        uint32_t v[256];
        Table() { for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1; v[i] = c; } }
    };
    static const Table built;   // (initialised once, by whichever thread comes first)
    const uint32_t* table = built.v;
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 0xFFu] ^ (crc >> 8);
    return ~crc;
}

inline uint32_t png_adler32(uint32_t adler, const uint8_t* p, size_t n)   // running value: start with 1
{
    uint32_t a = adler & 0xFFFFu, b = adler >> 16;
    while (n) {
        const size_t run = n < 5552 ? n : 5552;   // the most bytes before b can pass 2^32
        for (size_t i = 0; i < run; ++i) { a += p[i]; b += a; }
        a %= 65521u; b %= 65521u;
        p += run; n -= run;
    }
    return (b << 16) | a;
}

// the bytes of one chunk in flight: everything written through it is part of the chunk's CRC
struct PngSink {
    FILE* f; uint32_t crc; bool ok;
    void put(const uint8_t* p, size_t n) { if (ok && fwrite(p, 1, n, f) != n) ok = false; crc = png_crc32(crc, p, n); }
    void put32(uint32_t v) { const uint8_t b[4] = { (uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v }; put(b, 4); }
    void begin(uint32_t length, const char type[4]) { put32(length); crc = 0; put((const uint8_t*)type, 4); }
    void end() { put32(crc); }
};

// false: the file could not be written (what was written is removed by the caller).  width, height >= 1, pitch >= 4 * width
inline bool png_store_rgba8(FILE* f, const uint8_t* rgba, uint32_t width, uint32_t height, size_t pitch)
{
    static const uint8_t signature[8] = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n' };
    PngSink s; s.f = f; s.crc = 0; s.ok = true;
    s.put(signature, 8);
    s.begin(13, "IHDR");
    s.put32(width); s.put32(height);
    const uint8_t head[5] = { 8, 6, 0, 0, 0 };   // bit depth, colour type RGBA, deflate, adaptive filtering (each row says None), no interlace
    s.put(head, 5);
    s.end();
    const uint64_t row = 1ull + 4ull * width, raw = row * height;
    const uint64_t blocks = (raw + kPngStoredBlock - 1) / kPngStoredBlock;
    const uint64_t idat = 2 + raw + 5 * blocks + 4;
    if (idat > 0x7FFFFFFFull) return false;   // (a chunk's length field; 16384 x 16384 is half of it)
    s.begin((uint32_t)idat, "IDAT");
    const uint8_t zhead[2] = { 0x78, 0x01 };   // deflate with a 32 KiB window, no preset dictionary, check bits
    s.put(zhead, 2);
    uint32_t adler = 1;
    uint64_t left = raw, room = 0;   // bytes of the stream still to come; room left in the open stored block
    for (uint32_t y = 0; y < height; ++y) {
        const uint8_t filter = 0;
        const uint8_t* parts[2] = { &filter, rgba + (size_t)y * pitch };
        const size_t sizes[2] = { 1, (size_t)4 * width };
        for (int k = 0; k < 2; ++k) {
            const uint8_t* p = parts[k]; size_t n = sizes[k];
            adler = png_adler32(adler, p, n);
            while (n) {
                if (room == 0) {
                    room = left < kPngStoredBlock ? left : kPngStoredBlock;
                    const uint8_t bh[5] = { (uint8_t)(left <= kPngStoredBlock ? 1 : 0), (uint8_t)room, (uint8_t)(room >> 8), (uint8_t)~room, (uint8_t)(~room >> 8) };
                    s.put(bh, 5);
                }
                const size_t take = n < room ? n : (size_t)room;
                s.put(p, take);
                p += take; n -= take; room -= take; left -= take;
            }
        }
    }
    s.put32(adler);
    s.end();
    s.begin(0, "IEND");
    s.end();
    return s.ok;
}

} // namespace ommx
