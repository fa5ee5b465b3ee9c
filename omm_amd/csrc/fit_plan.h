// fit_plan.h -- the planner of ommxFitMicromap (include/omm_mi355x_ext.h has the rule): from the profile of every block (ommxProfileMicromapLevels)
// to one level per block whose blocks together fit a byte budget.  Plain C++ (no HIP), in bake_host.h's style: omm_host.cpp calls it on the table it
// read back, tests/native/fit_check.cpp runs it under sanitizers beside a planner that rescans every candidate at every step.
//
// The plan is the greedy of a multiple-choice knapsack: the block whose next level costs the least value per byte saved goes down one level, until the
// budget holds.  Each step changes the next ratio of ONE block, so the steps are sequential by nature; a heap keyed by (ratio, index) makes a step
// O(log blocks).  All arithmetic is in integers -- ratios are compared by cross-multiplication in 128 bits -- so the plan is a pure function of the table.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ommx {

typedef unsigned __int128 FitWide;

constexpr uint32_t kFitLevels = 13u;              // a profile row: one count per level 0..12
constexpr uint8_t kFitNoLevel = 0xFFu;            // the level of a descriptor that is unselected or invalid
// The word of a descriptor in the table: 0 for one that no primitive selects or that fails the bounds rule, otherwise its level and format.
constexpr uint32_t kFitLive = 0x80000000u;
constexpr uint32_t fit_shape(uint32_t level, uint32_t bits) { return kFitLive | (level << 2) | bits; }
constexpr uint32_t fit_shape_level(uint32_t w) { return (w >> 2) & 0xFFu; }
constexpr uint32_t fit_shape_bits(uint32_t w) { return w & 3u; }

struct FitTable {                  // 116 bytes per source descriptor, as four arrays
    uint32_t count;
    const uint32_t* shape;         // [count] the words above
    const uint32_t* known;         // [count][kFitLevels]  knownCounts
    const uint32_t* opaque;        // [count][kFitLevels]  knownOpaqueCounts
    const uint64_t* weight;        // [count] blockWeights
};
struct FitPlan {
    bool feasible;                 // false: no candidate was left above the budget; the other members then describe where the plan stopped
    uint64_t unfitted, planned, steps;
};

// the bytes block d occupies in a result at level t (0 when it is promoted to a special index)
inline uint64_t fit_size(const FitTable& T, uint32_t d, uint32_t t, bool specialIndices)
{
    const uint64_t fields = 1ull << (2u * t);
    if (specialIndices) {
        const uint64_t k = T.known[(size_t)d * kFitLevels + t], o = T.opaque[(size_t)d * kFitLevels + t];
        if (t == 0u || (k == fields && (o == 0ull || o == fields))) return 0ull;
    }
    const uint64_t bytes = (fields * fit_shape_bits(T.shape[d])) >> 3;
    return bytes ? bytes : 1ull;
}
// weight times known share, in units of 4^-12 of the block
inline FitWide fit_value(const FitTable& T, uint32_t d, uint32_t t)
{
    return (FitWide)T.weight[d] * (FitWide)((uint64_t)T.known[(size_t)d * kFitLevels + t] << (2u * (12u - t)));
}

struct FitStep { FitWide dv; uint64_t ds; uint32_t d; };   // block d one level down: value lost, bytes saved (> 0)
// a goes before b: the smaller dv / ds, then the lower descriptor
inline bool fit_step_before(const FitStep& a, const FitStep& b)
{
    const FitWide l = a.dv * (FitWide)b.ds, r = b.dv * (FitWide)a.ds;   // (dv < 2^88, ds < 2^22)
    return l != r ? l < r : a.d < b.d;
}
// the next step of block d at level t, if it is a candidate
inline bool fit_next_step(const FitTable& T, uint32_t d, uint32_t t, bool specialIndices, FitStep* out)
{
    if (t == 0u) return false;
    const uint64_t s1 = fit_size(T, d, t, specialIndices), s0 = fit_size(T, d, t - 1u, specialIndices);
    if (s1 <= s0) return false;
    out->dv = fit_value(T, d, t) - fit_value(T, d, t - 1u); out->ds = s1 - s0; out->d = d;
    return true;
}

// levels: [T.count], kFitNoLevel for descriptors without a word.  maxLevel: the global cap (>= 12: none).
inline FitPlan fit_plan(const FitTable& T, uint32_t maxLevel, bool specialIndices, uint64_t budget, uint8_t* levels)
{
    FitPlan p; p.feasible = true; p.unfitted = 0; p.steps = 0;
    const auto later = [](const FitStep& a, const FitStep& b) { return fit_step_before(b, a); };   // (std's heaps keep the LAST element on top)
    std::vector<FitStep> heap;
    uint64_t total = 0;
    for (uint32_t d = 0; d < T.count; ++d) {
        levels[d] = kFitNoLevel;
        if (!(T.shape[d] & kFitLive)) continue;
        const uint32_t level = fit_shape_level(T.shape[d]), t = level < maxLevel ? level : maxLevel;
        levels[d] = (uint8_t)t;
        total += fit_size(T, d, t, specialIndices);
        FitStep s;
        if (fit_next_step(T, d, t, specialIndices, &s)) heap.push_back(s);
    }
    std::make_heap(heap.begin(), heap.end(), later);
    p.unfitted = total;
    while (total > budget && !heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), later);
        const FitStep s = heap.back(); heap.pop_back();
        total -= s.ds; ++p.steps;
        const uint32_t t = --levels[s.d];
        FitStep n;
        if (fit_next_step(T, s.d, t, specialIndices, &n)) { heap.push_back(n); std::push_heap(heap.begin(), heap.end(), later); }
    }
    p.planned = total; p.feasible = total <= budget;
    return p;
}

} // namespace ommx
