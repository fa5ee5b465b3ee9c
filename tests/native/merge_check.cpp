// Host check of the word arithmetic of ommxMergeSimilarMicromaps (omm_amd/csrc/merge_words.h compiled as plain C++) against loops over single fields
// that apply the definition of include/omm_mi355x_ext.h:
//   1. the distance of two random words and of words that differ in chosen fields, against a loop over the 32 fields;
//   2. the join for mixedState 2 and 3, against the sentence of the header field by field; symmetric, associative, idempotent, conservative;
//   3. pos() against a table written out here (computed from the formula with Python integers), its range at every level;
//   4. the key at samples 1, 27 and 28: each sample in its own two bits, the level above them, nothing else set;
//   5. the limit of a level: d * 4^(12 - L) <= maxDistance exactly when d <= merge_limit.
// Built and run by tests/test_merge.py:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I omm_amd/csrc tests/native/merge_check.cpp -o merge_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "merge_words.h"

using namespace ommx;

static unsigned long long g_checked = 0, g_bad = 0;
#define EXPECT(cond, ...) do { g_checked++; if (!(cond)) { if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t g_seed = 0x13198A2E03707344ull;
static uint64_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

static uint32_t field(uint64_t w, uint32_t f) { return (uint32_t)(w >> (2u * f)) & 3u; }
static uint32_t join_field(uint32_t x, uint32_t y, uint32_t mixed)   // the sentence of the header
{
    if ((x & 1u) != (y & 1u)) return mixed;
    return (x & 1u) | (((x >> 1) | (y >> 1)) ? 2u : 0u);
}

static void check_distance_and_join()
{
    for (int trial = 0; trial < 60000; ++trial) {
        const uint64_t a = rnd();
        uint64_t b = rnd();
        if (trial % 3 == 1) b = a ^ (rnd() & rnd() & rnd());            // few fields differ
        if (trial % 3 == 2) b = a ^ ((uint64_t)(1u + (rnd() & 2u)) << (2u * (rnd() & 31u)));   // one field differs, in one bit or in both
        uint32_t want = 0;
        for (uint32_t f = 0; f < 32; ++f) want += field(a, f) != field(b, f);
        EXPECT(merge_distance(a, b) == want, "distance of %016llx and %016llx", (unsigned long long)a, (unsigned long long)b);
        EXPECT(merge_distance(a, a) == 0u && merge_distance(b, a) == want, "distance: zero on equal words, symmetric");
        for (uint32_t mixed = 2; mixed <= 3; ++mixed) {
            const uint64_t j = merge_join(a, b, mixed);
            bool same = true, safe = true;
            for (uint32_t f = 0; f < 32; ++f) {
                const uint32_t got = field(j, f);
                same = same && got == join_field(field(a, f), field(b, f), mixed);
                safe = safe && (got >= 2u || (got == field(a, f) && got == field(b, f)));
            }
            EXPECT(same, "join %u of %016llx and %016llx", mixed, (unsigned long long)a, (unsigned long long)b);
            EXPECT(safe, "join %u claims a state that a side does not", mixed);
            EXPECT(merge_join(b, a, mixed) == j && merge_join(a, a, mixed) == a, "join %u: symmetric, idempotent", mixed);
            const uint64_t c = rnd() & rnd();
            EXPECT(merge_join(merge_join(a, b, mixed), c, mixed) == merge_join(a, merge_join(b, c, mixed), mixed), "join %u: associative", mixed);
        }
    }
    // a byte and a 32-bit block go through the same functions with zeros above them
    EXPECT(merge_distance(0xE4u, 0x1Bu) == 4u && merge_join(0xE4u, 0xE4u, 2u) == 0xE4u && merge_join(0x00u, 0x55u, 2u) == 0xAAu && merge_join(0x00u, 0x55u, 3u) == 0xFFu, "bytes");
}

static void check_pos()
{
    static const struct { uint32_t L, r, j, seed, want; } kTable[] = {
        { 1u, 0u, 0u, 0x00000000u, 1u },
        { 1u, 31u, 27u, 0xFFFFFFFFu, 1u },
        { 2u, 0u, 1u, 0x00000001u, 14u },
        { 5u, 3u, 7u, 0x00003039u, 350u },
        { 8u, 7u, 15u, 0xDEADBEEFu, 35004u },
        { 12u, 31u, 27u, 0x80000000u, 11538736u },
        { 12u, 0u, 0u, 0x00000000u, 3390933u },
        { 6u, 1u, 0u, 0x0000002Au, 3973u },
        { 3u, 2u, 9u, 0x00000007u, 27u },
    };
    for (const auto& t : kTable) EXPECT(merge_pos(t.seed, t.L, t.r, t.j) == t.want, "pos(L %u, r %u, j %u, seed %08x) = %u, not %u", t.L, t.r, t.j, t.seed, merge_pos(t.seed, t.L, t.r, t.j), t.want);
    EXPECT(merge_lowbias32(1u) == 0x688990c0u && merge_lowbias32(0xFFFFFFFFu) == 0x6768824au, "lowbias32");
    for (uint32_t L = 1; L <= 12; ++L)
        for (uint32_t r = 0; r < kMergeMaxRounds; ++r)
            for (uint32_t j = 0; j < kMergeMaxSamples; ++j) EXPECT(merge_pos((uint32_t)rnd(), L, r, j) < (1u << (2u * L)), "pos outside a block of level %u", L);
}

static void check_key()
{
    static const uint32_t kSamples[3] = { 1u, 27u, 28u };
    for (int trial = 0; trial < 3000; ++trial) {
        const uint32_t L = 1u + (uint32_t)(rnd() % 6u), r = (uint32_t)(rnd() & 31u), seed = (uint32_t)rnd();
        std::vector<uint8_t> block((size_t)1 << (2u * L - 2u));          // an exact-size allocation: a read past it is AddressSanitizer's
        for (auto& b : block) b = (uint8_t)rnd();
        for (uint32_t samples : kSamples) {
            const uint64_t key = merge_key(block.data(), L, r, samples, seed);
            bool ok = (key >> 56) == L;
            for (uint32_t j = 0; j < 28u; ++j) {
                const uint32_t p = merge_pos(seed, L, r, j);
                const uint32_t want = j < samples ? (uint32_t)(block[p / 4u] >> (2u * (p % 4u))) & 3u : 0u;
                ok = ok && ((key >> (2u * j)) & 3u) == want;
            }
            EXPECT(ok, "key of a level-%u block with %u samples", L, samples);
            EXPECT(key != ~0ull, "a key that is all ones");
        }
    }
    uint8_t ones[1] = { 0xFF };
    EXPECT(merge_key(ones, 1u, 0u, 28u, 0u) == ((1ull << 56) | ((1ull << 56) - 1ull)), "28 samples of state 3 fill the 56 bits below the level");
}

static void check_limit()
{
    for (uint32_t L = 0; L <= 12; ++L)
        for (int trial = 0; trial < 400; ++trial) {
            const uint32_t maxDistance = trial < 4 ? (trial & 1 ? kMergeUnit : 0u) : (uint32_t)(rnd() % (kMergeUnit + 1u));
            const uint32_t limit = merge_limit(maxDistance, L);
            const uint64_t weight = 1ull << (2u * (12u - L));
            EXPECT((uint64_t)limit * weight <= maxDistance && ((uint64_t)limit + 1u) * weight > maxDistance, "limit of level %u under %u", L, maxDistance);
            EXPECT(limit <= (1u << (2u * L)), "a limit above the number of fields");
        }
}

int main()
{
    check_distance_and_join();
    check_pos();
    check_key();
    check_limit();
    printf("merge_check: %llu checks, %llu failures\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
