// Host check of the word arithmetic of ommxCombineMicromaps (omm_amd/csrc/combine_expand.h compiled as plain C++) against loops over single fields
// that apply the definition of include/omm_mi355x_ext.h:
//   1. the repetition n = 1, 2, 3 levels down: every 8-field group (4^8 of 4-state fields; the group spans 32, 128 or 512 output fields, so for
//      n >= 2 it is checked through the shifts the kernel uses to pick a word's share), then seeded random words;
//   2. the broadcast of one state, and repetition by three levels as the broadcast of one field;
//   3. the K-way join for K = 1..16 on planted random planes, both output formats and both mixedState values, in a shuffled order too;
//   4. repetition undone by coarsen_reduce_planes, and a join of a block with itself.
// Built and run by tests/test_combine.py:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I omm_amd/csrc tests/native/combine_check.cpp -o combine_check
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "combine_expand.h"

using namespace ommx;

static unsigned long long g_checked = 0, g_bad = 0;
#define EXPECT(cond, ...) do { g_checked++; if (!(cond)) { if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t g_seed = 0x13198A2E03707344ull;
static uint64_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

static CoarsenPlanes planes_of(const std::vector<uint8_t>& s)   // up to 64 states
{
    CoarsenPlanes p; p.lo = 0; p.hi = 0;
    for (size_t i = 0; i < s.size(); ++i) { p.lo |= (uint64_t)(s[i] & 1) << i; p.hi |= (uint64_t)(s[i] >> 1) << i; }
    return p;
}
static uint8_t field_of(CoarsenPlanes p, uint32_t i) { return (uint8_t)(((p.lo >> i) & 1u) | (((p.hi >> i) & 1u) << 1)); }

// the definition: output field j of the word that starts at output field `first` reads source field (first + j) >> 2n
static void check_repeat_of(const std::vector<uint8_t>& src /* 64 fields */, const char* what)
{
    const CoarsenPlanes p = planes_of(src);
    for (uint32_t n = 1; n <= 3; ++n) {
        const uint32_t per = 64u >> (2 * n);                      // source fields per output word
        for (uint32_t word = 0; word < 64u / per; ++word) {       // the kernel's shift: the word's share of the source planes
            CoarsenPlanes q; q.lo = p.lo >> (per * word); q.hi = p.hi >> (per * word);
            const CoarsenPlanes got = combine_repeat_planes(q, n);
            bool same = true;
            for (uint32_t j = 0; j < 64; ++j) same = same && field_of(got, j) == src[(64u * word + j) >> (2 * n)];
            EXPECT(same, "%s: repetition by %u levels, word %u: %016llx %016llx", what, n, word, (unsigned long long)got.lo, (unsigned long long)got.hi);
        }
    }
    const CoarsenPlanes same = combine_repeat_planes(p, 0);
    EXPECT(same.lo == p.lo && same.hi == p.hi, "%s: repetition by 0 levels changes the planes", what);
}

static void check_repeat()
{
    for (uint32_t c = 0; c < 65536u; ++c) {        // every group of 8 four-state fields (the 2-state groups are those without high bits), at every position
        std::vector<uint8_t> s(64);
        for (auto& x : s) x = (uint8_t)(rnd() & 3u);
        const uint32_t at = 8u * (c % 8u);
        for (uint32_t i = 0; i < 8; ++i) s[at + i] = (uint8_t)((c >> (2 * i)) & 3u);
        check_repeat_of(s, "8-field group");
    }
    for (int trial = 0; trial < 20000; ++trial) {
        std::vector<uint8_t> s(64);
        const uint32_t top = trial % 3 == 0 ? 2u : 4u;
        for (auto& x : s) x = (uint8_t)(rnd() % top);
        check_repeat_of(s, "random word");
    }
    // the pieces on raw bits, garbage above the bits that count
    for (int trial = 0; trial < 50000; ++trial) {
        const uint64_t x = rnd();
        for (uint32_t n = 1; n <= 3; ++n) {
            uint64_t want = 0;
            for (uint32_t j = 0; j < 64; ++j) want |= ((x >> (j >> (2 * n))) & 1ull) << j;
            EXPECT(combine_repeat_bits(x, n) == want, "repeat_bits, n = %u", n);
            EXPECT(coarsen_compact(combine_repeat_bits(x, n), n) == (x & (n == 3 ? 1ull : (1ull << (64u >> (2 * n))) - 1ull)), "compact(repeat), n = %u", n);
        }
    }
}

static void check_broadcast()
{
    for (uint32_t s = 0; s < 4; ++s) {
        const CoarsenPlanes b = combine_broadcast(s);
        bool same = true;
        for (uint32_t j = 0; j < 64; ++j) same = same && field_of(b, j) == s;
        EXPECT(same, "broadcast of state %u", s);
        for (int trial = 0; trial < 1000; ++trial) {       // one field read four and more levels down: the field, whatever lies above it
            CoarsenPlanes q; q.lo = (rnd() << 1) | (s & 1u); q.hi = (rnd() << 1) | (s >> 1);
            const CoarsenPlanes r = combine_repeat_planes(q, 3);
            EXPECT(r.lo == b.lo && r.hi == b.hi, "repetition by 3 levels is not the broadcast of field 0");
        }
    }
}

// ---- the join ----
static uint32_t state_of(const std::vector<uint8_t>& states, uint32_t fieldBits, uint32_t mixedState)
{
    bool side0 = false, side1 = false, unknown = false;
    for (uint8_t s : states) { if (s & 1) side1 = true; else side0 = true; if (s >> 1) unknown = true; }
    const uint32_t r = side0 && side1 ? mixedState : ((side1 ? 1u : 0u) | (unknown ? 2u : 0u));
    return fieldBits == 2 ? r : (r & 1u);
}
// K rows of 64 states in which a field is, with some probability, the same in every row, one-sided, or left random
static std::vector<std::vector<uint8_t>> planted_rows(uint32_t K)
{
    std::vector<std::vector<uint8_t>> rows(K, std::vector<uint8_t>(64));
    for (uint32_t j = 0; j < 64; ++j) {
        const uint64_t r = rnd();
        const uint8_t st = (uint8_t)((r >> 8) & 3u);
        for (uint32_t k = 0; k < K; ++k) {
            if (r % 10 < 3) rows[k][j] = st;
            else if (r % 10 < 6) rows[k][j] = (uint8_t)((st & 1) | ((rnd() & 3) == 0 ? 2 : 0));
            else if (r % 10 < 7) rows[k][j] = (uint8_t)(rnd() & 1u);          // a 2-state source
            else rows[k][j] = (uint8_t)(rnd() & 3u);
        }
    }
    return rows;
}
static CoarsenPlanes join_rows(const std::vector<std::vector<uint8_t>>& rows, const std::vector<uint32_t>& order, uint32_t fieldBits, uint32_t mixedState)
{
    CombineJoin j = combine_join_begin();
    for (uint32_t k : order) combine_join_add(j, planes_of(rows[k]));
    return combine_join_end(j, fieldBits, mixedState);
}
static void check_join()
{
    for (uint32_t K = 1; K <= 16; ++K)
        for (uint32_t fieldBits = 1; fieldBits <= 2; ++fieldBits)
            for (uint32_t mixedState = 2; mixedState <= 3; ++mixedState)
                for (int trial = 0; trial < 1500; ++trial) {
                    const std::vector<std::vector<uint8_t>> rows = planted_rows(K);
                    std::vector<uint32_t> order(K);
                    for (uint32_t k = 0; k < K; ++k) order[k] = k;
                    const CoarsenPlanes got = join_rows(rows, order, fieldBits, mixedState);
                    std::vector<uint8_t> want(64);
                    for (uint32_t j = 0; j < 64; ++j) {
                        std::vector<uint8_t> col(K);
                        for (uint32_t k = 0; k < K; ++k) col[k] = rows[k][j];
                        want[j] = (uint8_t)state_of(col, fieldBits, mixedState);
                    }
                    const CoarsenPlanes ref = planes_of(want);
                    EXPECT(got.lo == ref.lo && got.hi == ref.hi, "join of %u, %u bits, mixed %u: %016llx %016llx, want %016llx %016llx", K, fieldBits, mixedState,
                           (unsigned long long)got.lo, (unsigned long long)got.hi, (unsigned long long)ref.lo, (unsigned long long)ref.hi);
                    for (uint32_t k = K; k > 1; --k) std::swap(order[k - 1], order[rnd() % k]);      // symmetric
                    const CoarsenPlanes again = join_rows(rows, order, fieldBits, mixedState);
                    EXPECT(again.lo == got.lo && again.hi == got.hi, "join of %u in another order differs", K);
                    if (K >= 3 && fieldBits == 2) {                                                  // associative: a joined prefix joined with the rest
                        const std::vector<uint32_t> head(order.begin(), order.begin() + K / 2), tail(order.begin() + K / 2, order.end());
                        CombineJoin j = combine_join_begin();
                        combine_join_add(j, join_rows(rows, head, 2, mixedState));
                        combine_join_add(j, join_rows(rows, tail, 2, mixedState));
                        const CoarsenPlanes two = combine_join_end(j, 2, mixedState);
                        EXPECT(two.lo == got.lo && two.hi == got.hi, "join of joins differs, K = %u", K);
                    }
                    if (K == 1 && fieldBits == 2) EXPECT(got.lo == planes_of(rows[0]).lo && got.hi == planes_of(rows[0]).hi, "join of one source changes it");
                    if (K == 2) {                                                                    // idempotent
                        const CoarsenPlanes twice = join_rows(rows, {0, 0}, 2, mixedState), once = planes_of(rows[0]);
                        EXPECT(twice.lo == once.lo && twice.hi == once.hi, "join of a source with itself changes it");
                    }
                }
}

// repetition is undone by the coarsening's reduction, whatever mixedState is (the groups are uniform)
static void check_round_trip()
{
    for (int trial = 0; trial < 20000; ++trial)
        for (uint32_t n = 1; n <= 3; ++n) {
            std::vector<uint8_t> s(64u >> (2 * n));
            for (auto& x : s) x = (uint8_t)(rnd() & 3u);
            const CoarsenPlanes p = planes_of(s), back = coarsen_reduce_planes(combine_repeat_planes(p, n), n, 2, 2u + (uint32_t)(trial & 1));
            EXPECT(back.lo == p.lo && back.hi == p.hi, "reduce(repeat) by %u levels", n);
        }
}

int main()
{
    check_repeat();
    check_broadcast();
    check_join();
    check_round_trip();
    printf("combine_check: %llu checks, %llu failures\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
