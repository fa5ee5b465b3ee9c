// stats_count_check.cpp -- the plain C++ build of omm_amd/csrc/stats_count.h (the word counting of the device statistics) against a decode per
// field: every level 0..12 in both formats, the block at byte offsets 0..17 of a 16-byte aligned buffer, cut into segments of 1, 15, 16, 17 and
// 16384 bytes whose lanes' shares are added up the way the kernel's reduction does.  Prints "ok <cases>" or the first mismatch (tests/test_stats_reference.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "stats_count.h"

using namespace ommx;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main()
{
    const uint32_t cuts[5] = { 1u, 15u, 16u, 17u, kStatsSegmentBytes };
    const size_t maxBytes = (size_t)block_bytes(kResultMaxLevel, 2u);
    uint8_t* buf = (uint8_t*)aligned_alloc(64, maxBytes + 64);
    std::vector<uint8_t> block(maxBytes);
    if (!buf) return 2;
    unsigned cases = 0;
    for (uint32_t level = 0; level <= kResultMaxLevel; ++level)
        for (uint32_t bits = 1; bits <= 2; ++bits) {
            const uint64_t bytes = block_bytes(level, bits), fields = 1ull << (2u * level);
            if (bytes != (fields * bits + 7u) / 8u) { printf("block bytes of level %u, %u bits: %llu\n", level, bits, (unsigned long long)bytes); return 1; }
            for (uint64_t i = 0; i < bytes; ++i) block[i] = (uint8_t)(rng() >> 32);
            uint32_t want[4] = { 0, 0, 0, 0 };
            for (uint64_t f = 0; f < fields; ++f) want[(block[(f * bits) >> 3] >> ((f * bits) & 7u)) & ((1u << bits) - 1u)]++;
            for (uint32_t ofs = 0; ofs <= 17; ++ofs) {
                memset(buf, 0xFF, maxBytes + 64);   // the bytes (and the unused bits of a single-byte block) around the block must not count
                memcpy(buf + ofs, block.data(), bytes);
                if (bytes == 1 && fields * bits < 8) buf[ofs] |= (uint8_t)(0xFFu << (fields * bits));
                for (uint32_t cut : cuts) {
                    const uint32_t lanes = cut == kStatsSegmentBytes ? 256u : (cut == 1u ? 1u : 2u);
                    uint32_t got[4] = { 0, 0, 0, 0 };
                    for (uint64_t begin = 0; begin < bytes; begin += cut) {
                        const uint64_t end = begin + cut < bytes ? begin + cut : bytes;
                        for (uint32_t lane = 0; lane < lanes; ++lane) stats_count_range(buf + ofs, level, bits, begin, end, lane, lanes, got);
                    }
                    if (memcmp(got, want, sizeof got) != 0) {
                        printf("level %u, %u bits, offset %u, cut %u: got %u %u %u %u, want %u %u %u %u\n", level, bits, ofs, cut,
                               got[0], got[1], got[2], got[3], want[0], want[1], want[2], want[3]);
                        return 1;
                    }
                    cases++;
                }
            }
        }
    // the word function by itself: valid bits below a full word, bits above them set
    for (int k = 0; k < 100000; ++k) {
        const uint32_t w = (uint32_t)rng(), bits = 1u + (uint32_t)(rng() & 1u), nf = 1u + (uint32_t)(rng() % (32u / bits));
        uint32_t got[4] = { 0, 0, 0, 0 }, want[4] = { 0, 0, 0, 0 };
        stats_count_word(w, nf * bits, bits, got);
        for (uint32_t f = 0; f < nf; ++f) want[(w >> (f * bits)) & ((1u << bits) - 1u)]++;
        if (memcmp(got, want, sizeof got) != 0) { printf("word %08x, %u fields of %u bits\n", w, nf, bits); return 1; }
    }
    free(buf);
    printf("ok %u\n", cases);
    return 0;
}
