// Host check of the word arithmetic of ommxCoarsenMicromap (omm_amd/csrc/coarsen_reduce.h compiled as plain C++) against a loop over single states
// that applies the definition of include/omm_mi355x_ext.h:
//   1. one-level reductions of 8-field groups, exhaustively (4^8 groups of 4-state fields, 2^8 of 2-state fields), both values of mixedState, at every
//      position of the group in the 64 fields, through coarsen_reduce_word and through split / coarsen_reduce_planes / join;
//   2. two- and three-level reductions of seeded random 64-field words with planted uniform and one-sided groups, both formats;
//   3. the group AND / OR and the compaction on their own, split / join as inverses;
//   4. coarsen_word_uniform for every valid length, with garbage above the valid bits.
// Built and run by tests/test_coarsen.py:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I omm_amd/csrc tests/native/coarsen_check.cpp -o coarsen_check
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "coarsen_reduce.h"

using namespace ommx;

static unsigned long long g_checked = 0, g_bad = 0;
#define EXPECT(cond, ...) do { g_checked++; if (!(cond)) { if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t g_seed = 0x243F6A8885A308D3ull;
static uint64_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

// ---- the definition, one state at a time ----
static uint32_t state_of(const std::vector<uint8_t>& covered, uint32_t fieldBits, uint32_t mixedState)
{
    bool side0 = false, side1 = false, unknown = false;
    for (uint8_t s : covered) { if (s & 1) side1 = true; else side0 = true; if (s >> 1) unknown = true; }
    if (side0 && side1) return fieldBits == 2 ? mixedState : (mixedState & 1u);
    return (side1 ? 1u : 0u) | (unknown ? 2u : 0u);
}
static std::vector<uint8_t> reduce_states(const std::vector<uint8_t>& in, uint32_t levels, uint32_t fieldBits, uint32_t mixedState)
{
    const size_t span = (size_t)1 << (2 * levels);
    std::vector<uint8_t> out;
    for (size_t j = 0; j * span < in.size(); ++j) out.push_back((uint8_t)state_of(std::vector<uint8_t>(in.begin() + (long)(j * span), in.begin() + (long)((j + 1) * span)), fieldBits, mixedState));
    return out;
}
static CoarsenPlanes planes_of(const std::vector<uint8_t>& s)   // up to 64 states
{
    CoarsenPlanes p; p.lo = 0; p.hi = 0;
    for (size_t i = 0; i < s.size(); ++i) { p.lo |= (uint64_t)(s[i] & 1) << i; p.hi |= (uint64_t)(s[i] >> 1) << i; }
    return p;
}
static uint64_t word_of(const std::vector<uint8_t>& s, uint32_t fieldBits)   // up to 64 / fieldBits states, packed as a block packs them
{
    uint64_t w = 0;
    for (size_t i = 0; i < s.size(); ++i) w |= (uint64_t)s[i] << (fieldBits * i);
    return w;
}

static void check_against(const std::vector<uint8_t>& s64, uint32_t levels, uint32_t fieldBits, uint32_t mixedState, const char* what)
{
    const std::vector<uint8_t> want = reduce_states(s64, levels, fieldBits, mixedState);
    const CoarsenPlanes got = coarsen_reduce_planes(planes_of(s64), levels, fieldBits, mixedState), ref = planes_of(want);
    EXPECT(got.lo == ref.lo && got.hi == ref.hi, "%s: planes, %u levels, %u bits, mixed %u: %016llx %016llx, want %016llx %016llx", what, levels, fieldBits, mixedState,
           (unsigned long long)got.lo, (unsigned long long)got.hi, (unsigned long long)ref.lo, (unsigned long long)ref.hi);
    if (fieldBits == 1) {
        EXPECT(coarsen_reduce_word(word_of(s64, 1), levels, 1, mixedState) == word_of(want, 1), "%s: 2-state word, %u levels", what, levels);
    } else {
        // the packed form: two words in, through split / join; and each word alone where a word holds whole groups (one or two levels)
        const std::vector<uint8_t> a(s64.begin(), s64.begin() + 32), b(s64.begin() + 32, s64.end());
        uint64_t w0, w1;
        coarsen_join(coarsen_reduce_planes(coarsen_split(word_of(a, 2), word_of(b, 2)), levels, 2, mixedState), &w0, &w1);
        if (levels == 0) EXPECT(w0 == word_of(a, 2) && w1 == word_of(b, 2), "%s: 4-state split / join without a reduction", what);
        else EXPECT(w0 == word_of(want, 2) && w1 == 0, "%s: 4-state split / reduce / join, %u levels", what, levels);
        if (levels <= 2) {
            EXPECT(coarsen_reduce_word(word_of(a, 2), levels, 2, mixedState) == word_of(reduce_states(a, levels, 2, mixedState), 2), "%s: 4-state word, %u levels", what, levels);
            EXPECT(coarsen_reduce_word(word_of(b, 2), levels, 2, mixedState) == word_of(reduce_states(b, levels, 2, mixedState), 2), "%s: 4-state word, %u levels", what, levels);
        }
    }
}

// 1. every group of 8 fields (two output fields), at every position, the other 56 fields random
static void check_one_level()
{
    for (uint32_t fieldBits = 1; fieldBits <= 2; ++fieldBits)
        for (uint32_t mixedState = 2; mixedState <= 3; ++mixedState) {
            const uint32_t top = fieldBits == 1 ? 2u : 4u, combos = fieldBits == 1 ? 256u : 65536u;
            for (uint32_t c = 0; c < combos; ++c) {
                std::vector<uint8_t> s(64);
                for (auto& x : s) x = (uint8_t)(rnd() % top);
                const uint32_t at = 8u * (c % 8u);
                for (uint32_t i = 0; i < 8; ++i) s[at + i] = (uint8_t)(fieldBits == 1 ? (c >> i) & 1u : (c >> (2 * i)) & 3u);
                check_against(s, 1, fieldBits, mixedState, "one level");
            }
        }
}

// random words in which aligned groups of 4, 16 and 64 are planted uniform or one-sided, so that every outcome occurs at every level
static std::vector<uint8_t> planted(uint32_t fieldBits)
{
    const uint32_t top = fieldBits == 1 ? 2u : 4u;
    std::vector<uint8_t> s(64);
    for (auto& x : s) x = (uint8_t)(rnd() % top);
    for (uint32_t span = 4; span <= 64; span *= 4)
        for (uint32_t g = 0; g < 64 / span; ++g) {
            const uint64_t r = rnd();
            const uint8_t st = (uint8_t)((r >> 8) % top);
            if (r % 10 < 3) for (uint32_t i = 0; i < span; ++i) s[g * span + i] = st;
            else if (r % 10 < 6 && fieldBits == 2) for (uint32_t i = 0; i < span; ++i) s[g * span + i] = (uint8_t)((st & 1) | ((rnd() & 3) == 0 ? 2 : 0));
        }
    return s;
}
static void check_deeper()
{
    for (uint32_t fieldBits = 1; fieldBits <= 2; ++fieldBits)
        for (uint32_t mixedState = 2; mixedState <= 3; ++mixedState)
            for (uint32_t levels = 0; levels <= 3; ++levels)
                for (int trial = 0; trial < 8000; ++trial) {
                    const std::vector<uint8_t> s = planted(fieldBits);
                    check_against(s, levels, fieldBits, mixedState, "random");
                    if (levels >= 2) {   // the rule is associative: one level at a time gives the same bits
                        CoarsenPlanes p = planes_of(s);
                        for (uint32_t l = 0; l < levels; ++l) p = coarsen_reduce_planes(p, 1, fieldBits, mixedState);
                        const CoarsenPlanes q = coarsen_reduce_planes(planes_of(s), levels, fieldBits, mixedState);
                        EXPECT(p.lo == q.lo && p.hi == q.hi, "level by level differs from %u levels at once", levels);
                    }
                }
}

// 3. the pieces
static void check_pieces()
{
    for (int trial = 0; trial < 50000; ++trial) {
        const uint64_t x = rnd() & rnd() & (trial % 3 ? ~0ull : rnd()), y = x | rnd();
        for (uint32_t n = 0; n <= 3; ++n) {
            const uint32_t span = 1u << (2 * n);
            uint64_t wantAnd = 0, wantOr = 0, compactY = 0;
            for (uint32_t g = 0; g < 64 / span; ++g) {
                bool all = true, any = false;
                for (uint32_t i = 0; i < span; ++i) { const bool bit = (y >> (g * span + i)) & 1; all = all && bit; any = any || bit; }
                wantAnd |= (uint64_t)all << g; wantOr |= (uint64_t)any << g;
                compactY |= ((y >> (g * span)) & 1ull) << g;
            }
            EXPECT(coarsen_compact(coarsen_group_and(y, n), n) == wantAnd, "group AND, n = %u", n);
            EXPECT(coarsen_compact(coarsen_group_or(y, n), n) == wantOr, "group OR, n = %u", n);
            EXPECT(coarsen_compact(y, n) == compactY, "compaction, n = %u", n);
        }
        const uint64_t w0 = rnd(), w1 = rnd();
        uint64_t r0, r1;
        coarsen_join(coarsen_split(w0, w1), &r0, &r1);
        EXPECT(r0 == w0 && r1 == w1, "join(split(w)) != w");
        EXPECT(coarsen_spread_bits(coarsen_even_bits(w0)) == (w0 & 0x5555555555555555ull), "spread(even(w))");
    }
    for (uint32_t level = 0; level <= 12; ++level)
        for (uint32_t fieldBits = 1; fieldBits <= 2; ++fieldBits) {
            const uint64_t bits = (uint64_t)fieldBits << (2 * level);
            EXPECT(block_bytes(level, fieldBits) == (bits < 8 ? 1 : bits / 8), "block bytes of level %u", level);
        }
}

// 4. the uniformity test
static void check_uniform()
{
    for (uint32_t fieldBits = 1; fieldBits <= 2; ++fieldBits) {
        const uint32_t top = fieldBits == 1 ? 2u : 4u;
        for (uint32_t fields = 1; fields * fieldBits <= 64; ++fields)
            for (int trial = 0; trial < 400; ++trial) {
                std::vector<uint8_t> s(fields);
                const uint8_t st = (uint8_t)(rnd() % top);
                for (auto& x : s) x = st;
                if (trial % 4 == 1) s[rnd() % fields] = (uint8_t)(rnd() % top);          // one field may differ
                if (trial % 4 == 2) for (auto& x : s) x = (uint8_t)(rnd() % top);
                uint32_t want = 0;
                for (uint32_t c = 0; c < top; ++c) { bool all = true; for (uint8_t x : s) all = all && x == c; if (all) want |= 1u << c; }
                uint64_t w = word_of(s, fieldBits);
                if (fields * fieldBits < 64) w |= rnd() << (fields * fieldBits);          // garbage above the valid bits
                EXPECT(coarsen_word_uniform(w, fields * fieldBits, fieldBits) == want, "uniform: %u fields of %u bits: %x, want %x", fields, fieldBits,
                       coarsen_word_uniform(w, fields * fieldBits, fieldBits), want);
            }
    }
}

int main()
{
    check_one_level();
    check_deeper();
    check_pieces();
    check_uniform();
    printf("coarsen_check: %llu checks, %llu failures\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
