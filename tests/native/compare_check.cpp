// Host check of the word arithmetic of ommxCompareMicromaps (omm_amd/csrc/compare_count.h compiled as plain C++) against loops over single fields
// that apply the definition of include/omm_mi355x_ext.h:
//   1. the sixteen counts of two words of fields: random words, every valid-field count 1, 4, 16 and 64, each side from a 2-state word (a low plane
//      alone) or from two 4-state words (coarsen_split), with and without Force2State, garbage above the valid fields;
//   2. the four state masks of a side partition the valid fields;
//   3. counts add up over several words, as a lane's four plane pairs do;
//   4. the relation of every matrix with cells in {0, 1} (all 65536) and of random matrices, against the four sentences of the definition.
// Built and run by tests/test_compare.py:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I omm_amd/csrc tests/native/compare_check.cpp -o compare_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "compare_count.h"

using namespace ommx;

static unsigned long long g_checked = 0, g_bad = 0;
#define EXPECT(cond, ...) do { g_checked++; if (!(cond)) { if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t g_seed = 0x243F6A8885A308D3ull;
static uint64_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

// 64 fields of a side: bits 1: one word of 1-bit fields; bits 2: two words of 2-bit fields
struct Side { uint32_t bits; uint64_t w0, w1; };
static Side random_side(uint32_t bits) { Side s; s.bits = bits; s.w0 = rnd(); s.w1 = rnd(); return s; }
static uint32_t state_of(const Side& s, uint32_t i)   // the definition: field i of the packed words
{
    if (s.bits == 1u) return (uint32_t)(s.w0 >> i) & 1u;
    const uint64_t w = i < 32u ? s.w0 : s.w1;
    return (uint32_t)(w >> (2u * (i & 31u))) & 3u;
}
static CoarsenPlanes planes_of(const Side& s)
{
    if (s.bits == 2u) return coarsen_split(s.w0, s.w1);
    CoarsenPlanes p; p.lo = s.w0; p.hi = 0ull;
    return p;
}

static void loops(const Side& a, const Side& b, uint32_t fields, uint32_t force2, uint32_t want[16])
{
    for (uint32_t i = 0; i < fields; ++i) {
        uint32_t sa = state_of(a, i), sb = state_of(b, i);
        if (force2) { sa &= 1u; sb &= 1u; }
        want[4 * sa + sb]++;
    }
}

static void check_counts()
{
    static const uint32_t kFields[4] = { 1u, 4u, 16u, 64u };
    for (int trial = 0; trial < 12000; ++trial)
        for (uint32_t f = 0; f < 4; ++f)
            for (uint32_t ba = 1; ba <= 2; ++ba)
                for (uint32_t bb = 1; bb <= 2; ++bb)
                    for (uint32_t force2 = 0; force2 < 2; ++force2) {
                        const Side a = random_side(ba), b = random_side(bb);
                        uint32_t want[16], got[16];
                        memset(want, 0, sizeof want); memset(got, 0, sizeof got);
                        loops(a, b, kFields[f], force2, want);
                        const uint64_t valid = compare_valid_mask(kFields[f]);
                        compare_count_add(planes_of(a), planes_of(b), valid, force2, got);
                        uint32_t sum = 0;
                        for (int c = 0; c < 16; ++c) sum += got[c];
                        EXPECT(memcmp(want, got, sizeof want) == 0, "counts: %u fields, widths %u and %u, force2 %u", kFields[f], ba, bb, force2);
                        EXPECT(sum == kFields[f], "counts: %u fields add up to %u", kFields[f], sum);
                        if (force2) EXPECT(got[2] + got[3] + got[6] + got[7] + got[8] + got[9] + got[10] + got[11] + got[12] + got[13] + got[14] + got[15] == 0, "force2: an unknown state was counted");
                        // the planes of a short block are zero above its last field: without the mask they would count as (0, 0)
                        CoarsenPlanes za = planes_of(a), zb = planes_of(b);
                        za.lo &= valid; za.hi &= valid; zb.lo &= valid; zb.hi &= valid;
                        uint32_t again[16]; memset(again, 0, sizeof again);
                        compare_count_add(za, zb, valid, force2, again);
                        EXPECT(memcmp(want, again, sizeof want) == 0, "counts: %u fields with zeros above them", kFields[f]);
                        const CompareMasks k = compare_state_masks(planes_of(a), valid, force2);
                        EXPECT((k.m[0] | k.m[1] | k.m[2] | k.m[3]) == valid && (k.m[0] & k.m[1]) == 0 && (k.m[2] & k.m[3]) == 0 && ((k.m[0] | k.m[1]) & (k.m[2] | k.m[3])) == 0,
                               "masks: no partition of %u fields", kFields[f]);
                    }
    EXPECT(compare_valid_mask(1) == 1ull && compare_valid_mask(4) == 0xFull && compare_valid_mask(16) == 0xFFFFull && compare_valid_mask(64) == ~0ull, "valid masks");
}

static void check_accumulation()
{
    for (int trial = 0; trial < 4000; ++trial) {
        uint32_t want[16], got[16];
        memset(want, 0, sizeof want); memset(got, 0, sizeof got);
        const uint32_t ba = 1u + (uint32_t)(rnd() & 1u), bb = 1u + (uint32_t)(rnd() & 1u), force2 = (uint32_t)(rnd() & 1u);
        for (int j = 0; j < 4; ++j) {
            const Side a = random_side(ba), b = random_side(bb);
            loops(a, b, 64u, force2, want);
            compare_count_add(planes_of(a), planes_of(b), ~0ull, force2, got);
        }
        EXPECT(memcmp(want, got, sizeof want) == 0, "four plane pairs do not add up");
    }
}

static uint32_t relation_by_sentences(const uint32_t m[16])
{
    uint32_t r = 0;
    for (uint32_t sa = 0; sa < 4; ++sa)
        for (uint32_t sb = 0; sb < 4; ++sb) {
            if (sa == sb || m[4 * sa + sb] == 0) continue;
            if (sa < 2 && sb < 2) r |= 0x01u;
            if (sa >= 2 && sb < 2) r |= 0x02u;
            if (sa < 2 && sb >= 2) r |= 0x04u;
            if (sa >= 2 && sb >= 2) r |= 0x08u;
        }
    return r;
}

static void check_relation()
{
    for (uint32_t c = 0; c < 65536u; ++c) {
        uint32_t m[16];
        for (uint32_t k = 0; k < 16; ++k) m[k] = (c >> k) & 1u;
        EXPECT(compare_relation(m) == relation_by_sentences(m), "relation of the matrix with cells %04x", c);
    }
    for (int trial = 0; trial < 20000; ++trial) {
        uint32_t m[16];
        for (uint32_t k = 0; k < 16; ++k) m[k] = (rnd() & 3u) ? 0u : (uint32_t)rnd();
        EXPECT(compare_relation(m) == relation_by_sentences(m), "relation of a random matrix");
    }
    uint32_t diag[16]; memset(diag, 0, sizeof diag);
    diag[0] = diag[5] = diag[10] = diag[15] = 7u;
    EXPECT(compare_relation(diag) == 0u, "a diagonal matrix has a relation");
    EXPECT(kRelationConflict == 0x01u && kRelationAWeaker == 0x02u && kRelationBWeaker == 0x04u && kRelationHint == 0x08u && kRelationSkipped == 0x80u, "the bits of the header");
}

int main()
{
    check_counts();
    check_accumulation();
    check_relation();
    printf("compare_check: %llu checks, %llu failures\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
