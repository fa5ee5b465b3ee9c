// Host check of ommxProfileMicromapLevels' counting (omm_amd/csrc/profile_count.h compiled as plain C++) and of ommxFitMicromap's planner
// (omm_amd/csrc/fit_plan.h) against loops that apply the definitions of include/omm_mi355x_ext.h:
//   1. profile_step + profile_count on 8-field groups exhaustively (4^8 groups of 4-state fields, 2^8 of 2-state fields) at every position of the group
//      in the 64 fields, against a loop over single states;
//   2. every level of seeded random 64-, 16-, 4- and 1-field words with planted uniform and one-sided groups, both formats, with zeros and with garbage
//      above the last field: the validity mask must keep the padding out of every count;
//   3. fit_plan against a second planner that rescans every candidate at every step, on seeded tables of up to 40 blocks: equal ratios (ties go to the
//      lower index), zero weights, chain ends where a step saves no byte, blocks that are free at their start level, the infeasible case.
// With the argument "tables" the program prints the tables of 3 and its plans instead, for tests/test_fit.py to hold the Python statement against.
// Built and run by tests/test_fit.py:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I omm_amd/csrc tests/native/fit_check.cpp -o fit_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "profile_count.h"
#include "fit_plan.h"

using namespace ommx;

static unsigned long long g_checked = 0, g_bad = 0;
#define EXPECT(cond, ...) do { g_checked++; if (!(cond)) { if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t g_seed = 0x13198A2E03707344ull;
static uint64_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

// ---- the definition, one state at a time ----
static void count_states(const std::vector<uint8_t>& s, size_t span, uint32_t* known, uint32_t* opaque)
{
    *known = 0; *opaque = 0;
    for (size_t j = 0; j * span < s.size(); ++j) {
        bool ok = true;
        for (size_t i = 0; i < span; ++i) ok = ok && s[j * span + i] < 2 && s[j * span + i] == s[j * span];
        if (ok) { ++*known; *opaque += s[j * span]; }
    }
}
static CoarsenPlanes planes_of(const std::vector<uint8_t>& s)
{
    CoarsenPlanes p; p.lo = 0; p.hi = 0;
    for (size_t i = 0; i < s.size(); ++i) { p.lo |= (uint64_t)(s[i] & 1) << i; p.hi |= (uint64_t)(s[i] >> 1) << i; }
    return p;
}
// every level of the first s.size() fields of p (a power of four)
static void check_levels(CoarsenPlanes p, const std::vector<uint8_t>& s, const char* what)
{
    uint32_t fields = (uint32_t)s.size();
    for (size_t span = 1; span <= s.size(); span *= 4, fields /= 4) {
        uint32_t known, opaque;
        count_states(s, span, &known, &opaque);
        const ProfileCount c = profile_count(p, fields);
        EXPECT(c.known == known && c.opaque == opaque, "%s: %zu fields, span %zu: %u known %u opaque, want %u %u", what, s.size(), span, c.known, c.opaque, known, opaque);
        p = profile_step(p);
    }
}

static void check_one_level()
{
    for (uint32_t fieldBits = 1; fieldBits <= 2; ++fieldBits) {
        const uint32_t top = fieldBits == 1 ? 2u : 4u, combos = fieldBits == 1 ? 256u : 65536u;
        for (uint32_t c = 0; c < combos; ++c) {
            std::vector<uint8_t> s(64);
            for (auto& x : s) x = (uint8_t)(rnd() % top);
            const uint32_t at = 8u * (c % 8u);
            for (uint32_t i = 0; i < 8; ++i) s[at + i] = (uint8_t)(fieldBits == 1 ? (c >> i) & 1u : (c >> (2 * i)) & 3u);
            check_levels(planes_of(s), s, "one level");
        }
    }
}

static std::vector<uint8_t> planted(uint32_t fields, uint32_t fieldBits)
{
    const uint32_t top = fieldBits == 1 ? 2u : 4u;
    std::vector<uint8_t> s(fields);
    for (auto& x : s) x = (uint8_t)(rnd() % top);
    for (uint32_t span = 4; span <= fields; span *= 4)
        for (uint32_t g = 0; g < fields / span; ++g) {
            const uint64_t r = rnd();
            const uint8_t st = (uint8_t)((r >> 8) % top);
            if (r % 10 < 4) for (uint32_t i = 0; i < span; ++i) s[g * span + i] = st;
            else if (r % 10 < 6 && fieldBits == 2) for (uint32_t i = 0; i < span; ++i) s[g * span + i] = (uint8_t)((st & 1) | ((rnd() & 3) == 0 ? 2 : 0));
        }
    return s;
}
static void check_masks()
{
    for (uint32_t fieldBits = 1; fieldBits <= 2; ++fieldBits)
        for (uint32_t fields = 1; fields <= 64; fields *= 4)
            for (int trial = 0; trial < 6000; ++trial) {
                const std::vector<uint8_t> s = planted(fields, fieldBits);
                CoarsenPlanes p = planes_of(s);
                check_levels(p, s, "zeros above");   // (zeros above the last field read as known transparent: only the mask keeps them out)
                if (fields < 64) {
                    // garbage above, in whole groups of the block's own size so that no group mixes fields and garbage
                    const uint64_t above = ~profile_valid(fields);
                    p.lo |= rnd() & above; if (fieldBits == 2 || (trial & 1)) p.hi |= rnd() & above;
                    check_levels(p, s, "garbage above");
                }
            }
    EXPECT(profile_valid(0) == 0 && profile_valid(1) == 1 && profile_valid(4) == 0xF && profile_valid(16) == 0xFFFF && profile_valid(64) == ~0ull, "profile_valid");
    CoarsenPlanes z; z.lo = 0; z.hi = 0;
    EXPECT(profile_count(z, 0).known == 0 && profile_count(z, 16).known == 16 && profile_count(z, 16).opaque == 0, "the padding is masked, not the fields");
}

// ---- the planner ----
struct Table {
    std::vector<uint32_t> shape, known, opaque; std::vector<uint64_t> weight;
    uint32_t maxLevel; bool special; uint64_t budget;
    FitTable view() const { FitTable T; T.count = (uint32_t)shape.size(); T.shape = shape.data(); T.known = known.data(); T.opaque = opaque.data(); T.weight = weight.data(); return T; }
};
// a row that a block could have: known[t-1] * 4 <= known[t] <= 4^t, and the opaque groups among them likewise
static void random_row(uint32_t level, uint32_t kind, uint32_t* known, uint32_t* opaque)
{
    for (uint32_t t = 0; t < kFitLevels; ++t) { known[t] = 0; opaque[t] = 0; }
    for (uint32_t t = 0; t <= level; ++t) {
        const uint32_t fields = 1u << (2 * t);
        if (kind == 0) { known[t] = fields; opaque[t] = 0; }                                  // uniform transparent: free at every level
        else if (kind == 1) { known[t] = fields; opaque[t] = fields; }                        // uniform opaque
        else if (kind == 2) { known[t] = t ? fields : 0; opaque[t] = t ? fields / 2 : 0; }    // quadrants: whole down to level 1
        else if (kind == 3) { known[t] = t == level ? fields : 0; opaque[t] = t == level ? fields / 2 : 0; }   // alternating: all lost at the first step
        else {
            const uint32_t k0 = t ? 4 * known[t - 1] : 0, o0 = t ? 4 * opaque[t - 1] : 0;
            const uint32_t room = fields - k0;
            const uint32_t more = (uint32_t)(rnd() % 4 == 0 ? room : rnd() % 3 == 0 ? 0 : rnd() % (room + 1));
            known[t] = k0 + more;
            opaque[t] = o0 + (uint32_t)(rnd() % (more + 1));
        }
    }
}
static Table random_table(uint32_t trial)
{
    Table T;
    const uint32_t D = 1 + (uint32_t)(rnd() % 40);
    T.maxLevel = trial % 5 == 0 ? (uint32_t)(rnd() % 8) : 12u;
    T.special = trial % 4 != 3;
    for (uint32_t d = 0; d < D; ++d) {
        uint32_t known[kFitLevels], opaque[kFitLevels];
        if (d && rnd() % 4 == 0) {            // a copy of an earlier row: equal ratios at every step
            const uint32_t from = (uint32_t)(rnd() % d);
            T.shape.push_back(T.shape[from]); T.weight.push_back(T.weight[from]);
            for (uint32_t t = 0; t < kFitLevels; ++t) { T.known.push_back(T.known[from * kFitLevels + t]); T.opaque.push_back(T.opaque[from * kFitLevels + t]); }
            continue;
        }
        if (rnd() % 8 == 0) {                 // unselected or invalid
            T.shape.push_back(0); T.weight.push_back(0);
            for (uint32_t t = 0; t < kFitLevels; ++t) { T.known.push_back(0); T.opaque.push_back(0); }
            continue;
        }
        const uint32_t level = (uint32_t)(trial % 7 == 0 ? rnd() % 13 : rnd() % 6), bits = 1 + (uint32_t)(rnd() & 1);
        random_row(level, (uint32_t)(rnd() % 8), known, opaque);
        T.shape.push_back(fit_shape(level, bits));
        const uint64_t r = rnd();
        T.weight.push_back(r % 5 == 0 ? 0ull : r % 5 == 1 ? 1ull + (r >> 8) % 4 : r % 5 == 2 ? r : (r >> 40));
        for (uint32_t t = 0; t < kFitLevels; ++t) { T.known.push_back(known[t]); T.opaque.push_back(opaque[t]); }
    }
    std::vector<uint8_t> levels(D);
    const FitPlan whole = fit_plan(T.view(), T.maxLevel, T.special, ~0ull, levels.data());
    const FitPlan none = fit_plan(T.view(), T.maxLevel, T.special, 0ull, levels.data());
    // budgets: anywhere between what is left when no candidate remains and the unfitted size; now and then below that (infeasible without special indices)
    T.budget = none.planned + (whole.unfitted > none.planned ? rnd() % (whole.unfitted - none.planned + 1) : 0);
    if (trial % 6 == 5) T.budget = none.planned ? rnd() % none.planned : 0;
    return T;
}
// the rule with a rescan of every candidate at every step
static FitPlan rescan_plan(const FitTable& T, uint32_t maxLevel, bool special, uint64_t budget, std::vector<uint8_t>& levels, uint64_t* ties)
{
    FitPlan p; p.steps = 0; uint64_t total = 0;
    for (uint32_t d = 0; d < T.count; ++d) {
        levels[d] = kFitNoLevel;
        if (!(T.shape[d] & kFitLive)) continue;
        const uint32_t level = fit_shape_level(T.shape[d]);
        levels[d] = (uint8_t)(level < maxLevel ? level : maxLevel);
        total += fit_size(T, d, levels[d], special);
    }
    p.unfitted = total;
    while (total > budget) {
        bool have = false; FitWide bv = 0; uint64_t bs = 1; uint32_t bd = 0; bool tie = false;
        for (uint32_t d = 0; d < T.count; ++d) {
            if (levels[d] == kFitNoLevel || levels[d] == 0) continue;
            const uint32_t t = levels[d];
            const uint64_t s1 = fit_size(T, d, t, special), s0 = fit_size(T, d, t - 1, special);
            if (s1 <= s0) continue;
            const FitWide dv = fit_value(T, d, t) - fit_value(T, d, t - 1);
            const uint64_t ds = s1 - s0;
            if (!have || dv * bs < bv * ds) { have = true; bv = dv; bs = ds; bd = d; tie = false; }
            else if (dv * bs == bv * ds) tie = true;
        }
        if (!have) break;
        --levels[bd]; total -= bs; ++p.steps; *ties += tie;
    }
    p.planned = total; p.feasible = total <= budget;
    return p;
}

static void check_plans(bool print)
{
    uint64_t ties = 0, infeasible = 0, free_start = 0, zero_weight = 0, chain_ends = 0;
    for (uint32_t trial = 0; trial < (print ? 120u : 3000u); ++trial) {
        const Table T = random_table(trial);
        const FitTable V = T.view();
        std::vector<uint8_t> a(V.count), b(V.count);
        const FitPlan p = fit_plan(V, T.maxLevel, T.special, T.budget, a.data());
        const FitPlan q = rescan_plan(V, T.maxLevel, T.special, T.budget, b, &ties);
        EXPECT(p.feasible == q.feasible && p.unfitted == q.unfitted && p.planned == q.planned && p.steps == q.steps && a == b,
               "trial %u: plan differs: %d %llu %llu %llu, rescan %d %llu %llu %llu", trial, (int)p.feasible, (unsigned long long)p.unfitted, (unsigned long long)p.planned,
               (unsigned long long)p.steps, (int)q.feasible, (unsigned long long)q.unfitted, (unsigned long long)q.planned, (unsigned long long)q.steps);
        EXPECT(p.planned <= p.unfitted && (!p.feasible || p.planned <= T.budget), "trial %u: sizes out of order", trial);
        infeasible += !p.feasible;
        for (uint32_t d = 0; d < V.count; ++d) {
            if (!(V.shape[d] & kFitLive)) { EXPECT(a[d] == kFitNoLevel, "trial %u: a level for a descriptor without a word", trial); continue; }
            const uint32_t level = fit_shape_level(V.shape[d]), start = level < T.maxLevel ? level : T.maxLevel;
            EXPECT(a[d] <= start, "trial %u: a level above the start", trial);
            free_start += fit_size(V, d, start, T.special) == 0; zero_weight += V.weight[d] == 0;
            FitStep s;
            chain_ends += a[d] > 0 && !fit_next_step(V, d, a[d], T.special, &s);
        }
        if (print) {
            printf("table %u %u %d %llu\n", V.count, T.maxLevel, (int)T.special, (unsigned long long)T.budget);
            for (uint32_t d = 0; d < V.count; ++d) {
                printf("row %u %llu", V.shape[d], (unsigned long long)V.weight[d]);
                for (uint32_t t = 0; t < kFitLevels; ++t) printf(" %u %u", V.known[d * kFitLevels + t], V.opaque[d * kFitLevels + t]);
                printf("\n");
            }
            printf("plan %d %llu %llu %llu", (int)p.feasible, (unsigned long long)p.unfitted, (unsigned long long)p.planned, (unsigned long long)p.steps);
            for (uint32_t d = 0; d < V.count; ++d) printf(" %u", a[d]);
            printf("\n");
        }
    }
    EXPECT(print || (ties > 20 &&infeasible > 20 && free_start > 100 && zero_weight > 100 && chain_ends > 100), "the cases were not met: %llu ties, %llu infeasible, %llu free, %llu weightless, %llu chain ends",
           (unsigned long long)ties, (unsigned long long)infeasible, (unsigned long long)free_start, (unsigned long long)zero_weight, (unsigned long long)chain_ends);
    // the largest products stay inside 128 bits: a level-12 block of full weight that is known only at its own level
    FitStep big; big.dv = ((FitWide)~0ull) << 24; big.ds = 1u << 21; big.d = 0;
    FitStep small; small.dv = 1; small.ds = 1u << 21; small.d = 1;
    EXPECT(fit_step_before(small, big) && !fit_step_before(big, small) && fit_step_before(big, FitStep{ big.dv, big.ds, 5 }), "128-bit comparison");
}

int main(int argc, char** argv)
{
    const bool print = argc > 1 && !strcmp(argv[1], "tables");
    if (!print) { check_one_level(); check_masks(); }
    check_plans(print);
    printf("fit_check: %llu checks, %llu failures\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
