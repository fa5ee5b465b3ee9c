// Host check of the two pieces of ommxExtractMicroGeometry / ommxExpandMicroNodes that compile as plain C++:
//   1. ommx_micro_vertices (include/omm_mi355x_lookup.h) for every index of levels 0..12: equal to the oracle's forward decode orc_index2bary bit for
//      bit, ommx_micro_index of its centroid is the index, orientation is positive, and the children of node j are the nodes 4j..4j+3 (their
//      vertices lie in the parent's closure and their areas add up to the parent's);
//   2. geo_cut64 (omm_amd/csrc/geometry_cut.h) against a scalar loop over the definition: every word with at most two entries that differ from the
//      rest, and 10^5 seeded random words per number of classes in use, for every word size k and every position t of the emit level.
// Built and run by tests/test_geometry.py:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I include -I omm_amd/csrc tests/native/geometry_check.cpp oracle/libomm_oracle.so -o geometry_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "omm_mi355x_lookup.h"
#include "geometry_cut.h"

extern "C" void orc_index2bary(uint32_t index, uint32_t level, float uv[6]);

using namespace ommx;

static unsigned long long g_checked = 0, g_bad = 0;
#define EXPECT(cond, ...) do { g_checked++; if (!(cond)) { if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- 1. the vertices ----
static int64_t cross2(const int64_t a[2], const int64_t b[2], const int64_t c[2]) { return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]); }

static void grid(const float uv[6], uint32_t level, int64_t g[3][2])   // vertices on the integer grid of spacing 2^-level
{
    for (int k = 0; k < 3; ++k) { g[k][0] = (int64_t)(uv[2 * k] * (float)(1u << level)); g[k][1] = (int64_t)(uv[2 * k + 1] * (float)(1u << level)); }
}

static void check_vertices()
{
    for (uint32_t level = 0; level <= 12; ++level) {
        for (uint32_t index = 0; index < (1u << (2 * level)); ++index) {
            float mine[6], ref[6];
            ommx_micro_vertices(index, level, mine);
            orc_index2bary(index, level, ref);
            EXPECT(memcmp(mine, ref, sizeof mine) == 0, "level %u index %u: vertices differ from the forward decode", level, index);
            const float cu = (mine[0] + mine[2] + mine[4]) / 3.f, cv = (mine[1] + mine[3] + mine[5]) / 3.f;
            EXPECT(ommx_micro_index(cu, cv, level) == index, "level %u index %u: its centroid maps to %u", level, index, ommx_micro_index(cu, cv, level));
            int64_t g[3][2];
            grid(mine, level, g);
            EXPECT(cross2(g[0], g[1], g[2]) == 1, "level %u index %u: orientation %lld", level, index, (long long)cross2(g[0], g[1], g[2]));
            if (level < 12) {   // the four children, on the child level's grid (the parent's vertices doubled)
                int64_t p[3][2], area = 0;
                for (int k = 0; k < 3; ++k) { p[k][0] = 2 * g[k][0]; p[k][1] = 2 * g[k][1]; }
                for (uint32_t q = 0; q < 4; ++q) {
                    float child[6]; int64_t c[3][2];
                    ommx_micro_vertices(4 * index + q, level + 1, child);
                    grid(child, level + 1, c);
                    area += cross2(c[0], c[1], c[2]);
                    for (int k = 0; k < 3; ++k)
                        EXPECT(cross2(p[0], p[1], c[k]) >= 0 && cross2(p[1], p[2], c[k]) >= 0 && cross2(p[2], p[0], c[k]) >= 0,
                               "level %u node %u: vertex %d of child %u lies outside it", level, index, k, q);
                }
                EXPECT(area == cross2(p[0], p[1], p[2]), "level %u node %u: its children do not add up to it", level, index);
            }
        }
    }
    float a[6], b[6];   // levels above 12 are 12, an index is reduced modulo 4^level
    ommx_micro_vertices(123456u, 13u, a); ommx_micro_vertices(123456u, 12u, b);
    EXPECT(memcmp(a, b, sizeof a) == 0, "level 13 is not level 12");
    ommx_micro_vertices(64u + 37u, 3u, a); ommx_micro_vertices(37u, 3u, b);
    EXPECT(memcmp(a, b, sizeof a) == 0, "the index is not reduced modulo 4^level");
}

// ---- 2. the cut of 64 ----
// entries: class 0..4 or kGeoNoClass per entry.  The definition, one node at a time: class of the node j levels above the entries ...
static uint32_t scalar_class(const uint8_t* entry, uint32_t j, uint32_t at, int32_t t, uint32_t mixed)
{
    if (j == 0) return entry[at];
    const uint32_t span = 1u << (2 * (j - 1));
    uint32_t kid[4];
    for (uint32_t q = 0; q < 4; ++q) kid[q] = scalar_class(entry, j - 1, at + q * span, t, mixed);
    if (kid[0] != kGeoNoClass && kid[0] == kid[1] && kid[0] == kid[2] && kid[0] == kid[3]) return kid[0];
    return (int32_t)j == t ? mixed : kGeoNoClass;
}
// ... and its emission: below a parent without a class, at or above the emit level
static void scalar_emit(const uint8_t* entry, uint32_t j, uint32_t at, int32_t t, uint32_t mixed, GeoCut* g)
{
    const uint32_t c = scalar_class(entry, j, at, t, mixed);
    if (c != kGeoNoClass) {
        if (c < 4 && (int32_t)j >= t) {
            g->start[c] |= 1ull << at;
            if (j == 1) g->up1 |= 1ull << at;
            if (j == 2) g->up2 |= 1ull << at;
        }
        return;
    }
    if (j == 0) return;
    for (uint32_t q = 0; q < 4; ++q) scalar_emit(entry, j - 1, at + q * (1u << (2 * (j - 1))), t, mixed, g);
}

static void check_word(const uint8_t* entry, uint32_t k, int32_t t, uint32_t mixed)
{
    uint64_t m[5] = { 0, 0, 0, 0, 0 };
    for (uint32_t i = 0; i < 64; ++i) if (entry[i] < 5) m[entry[i]] |= 1ull << i;   // (entries at or above 4^k are set as well: they must be ignored)
    const GeoCut got = geo_cut64(m, k, t, mixed);
    GeoCut want; memset(&want, 0, sizeof want);
    want.whole = scalar_class(entry, k, 0, t, mixed);
    if (want.whole == kGeoNoClass) for (uint32_t q = 0; q < 4 && k; ++q) scalar_emit(entry, k - 1, q * (1u << (2 * (k - 1))), t, mixed, &want);
    const bool same = got.whole == want.whole && memcmp(got.start, want.start, sizeof got.start) == 0 && got.up1 == want.up1 && got.up2 == want.up2;
    EXPECT(same, "cut differs: k %u t %d mixed %u whole %u (want %u) start0 %016llx (want %016llx)", k, t, mixed, got.whole, want.whole,
           (unsigned long long)got.start[0], (unsigned long long)want.start[0]);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

static void check_cut()
{
    uint8_t entry[64];
    for (uint32_t k = 0; k <= 3; ++k) for (int32_t t = -1; t <= 4; ++t) for (uint32_t mixed = 0; mixed < 5; ++mixed) {
        // every word with at most two entries that differ from the rest (the rest: class 1; the two: class 0, 4 or none)
        const uint8_t other[3] = { 0, (uint8_t)kGeoDrop, (uint8_t)kGeoNoClass };
        if (mixed == 0 || mixed == 2 || mixed == 4) for (uint32_t a = 0; a < 64; ++a) for (uint32_t b = a; b < 64; ++b) for (uint32_t oa = 0; oa < 3; ++oa) for (uint32_t ob = 0; ob < 3; ++ob) {
            memset(entry, 1, sizeof entry);
            entry[a] = other[oa]; entry[b] = other[ob];
            check_word(entry, k, t, mixed);
        }
        memset(entry, 2, sizeof entry); check_word(entry, k, t, mixed);
        memset(entry, (int)kGeoDrop, sizeof entry); check_word(entry, k, t, mixed);
        memset(entry, (int)kGeoNoClass, sizeof entry); check_word(entry, k, t, mixed);
    }
    // seeded random words: `classes` classes in use (1..6: the sixth is "no class"), runs of equal entries of random length so that quads do merge
    for (uint32_t classes = 1; classes <= 6; ++classes) for (uint32_t n = 0; n < 100000; ++n) {
        for (uint32_t i = 0; i < 64;) {
            const uint32_t c = rnd() % classes, run = 1u << (2 * (rnd() % 4)), len = (rnd() & 1) ? run : 1 + rnd() % 8;
            for (uint32_t e = 0; e < len && i < 64; ++e) entry[i++] = c == 5 ? (uint8_t)kGeoNoClass : (uint8_t)c;
        }
        check_word(entry, rnd() % 4, (int32_t)(rnd() % 6) - 1, rnd() % 5);
    }
}

// the class masks of a word of micro-triangles: every state at every position, both formats
static void check_masks()
{
    const uint8_t cls[4] = { 4, 0, 3, 0 };
    for (uint32_t n = 0; n < 20000; ++n) {
        uint8_t state[64]; uint64_t w4[2] = { 0, 0 }, w2 = 0, m[5];
        for (uint32_t i = 0; i < 64; ++i) { state[i] = (uint8_t)(rnd() & 3); w4[i >> 5] |= (uint64_t)state[i] << (2 * (i & 31)); w2 |= (uint64_t)(state[i] & 1) << i; }
        geo_class_masks(w4[0], w4[1], 2, cls, m);
        for (uint32_t i = 0; i < 64; ++i) for (uint32_t c = 0; c < 5; ++c) EXPECT(((m[c] >> i) & 1) == (cls[state[i]] == c), "4-state masks: entry %u class %u", i, c);
        geo_class_masks(w2, 0, 1, cls, m);
        for (uint32_t i = 0; i < 64; ++i) for (uint32_t c = 0; c < 5; ++c) EXPECT(((m[c] >> i) & 1) == (cls[state[i] & 1] == c), "2-state masks: entry %u class %u", i, c);
    }
}

int main()
{
    check_vertices();
    const unsigned long long v = g_checked;
    check_cut();
    check_masks();
    printf("geometry_check: %llu vertex checks, %llu cut checks, %llu failures\n", v, g_checked - v, g_bad);
    return g_bad ? 1 : 0;
}
