// Exhaustive host check of ommx_micro_index (include/omm_mi355x_lookup.h, plain C++ build) against the oracle's forward decode orc_index2bary,
// for every micro-triangle of every level 0..12 (22 M micro-triangles):
//   - the centroid of micro-triangle i maps to i;
//   - each of its three vertices and three edge midpoints maps to a micro-triangle whose closure contains the point (exact integer test).
// Built and run by tests/test_lookup.py:
//   g++ -O2 -std=c++17 -I include tests/native/lookup_check.cpp oracle/libomm_oracle.so -o lookup_check && ./lookup_check
#include <stdint.h>
#include <stdio.h>
#include "omm_mi355x_lookup.h"

extern "C" void orc_index2bary(uint32_t index, uint32_t level, float uv[6]);

// vertices of micro-triangle `index` on the integer grid of spacing 2^-(level+1) (every vertex and edge midpoint is a grid point)
static void grid_tri(uint32_t index, uint32_t level, int64_t g[6])
{
    float uv[6];
    orc_index2bary(index, level, uv);
    const float s = (float)(2u << level);
    for (int k = 0; k < 6; ++k) g[k] = (int64_t)(uv[k] * s);
}

static bool closure_contains(const int64_t t[6], int64_t px, int64_t py)
{
    int64_t d[3];
    for (int e = 0; e < 3; ++e) {
        const int64_t ax = t[2 * e], ay = t[2 * e + 1], bx = t[(2 * e + 2) % 6], by = t[(2 * e + 3) % 6];
        d[e] = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
    }
    return (d[0] >= 0 && d[1] >= 0 && d[2] >= 0) || (d[0] <= 0 && d[1] <= 0 && d[2] <= 0);
}

int main()
{
    unsigned long long checked = 0, bad = 0;
    for (uint32_t level = 0; level <= 12; ++level) {
        const float inv = 1.f / (float)(2u << level);
        for (uint32_t index = 0; index < (1u << (2 * level)); ++index) {
            float uv[6];
            orc_index2bary(index, level, uv);
            const float cu = (uv[0] + uv[2] + uv[4]) / 3.f, cv = (uv[1] + uv[3] + uv[5]) / 3.f;
            const uint32_t c = ommx_micro_index(cu, cv, level);
            checked++;
            if (c != index) { if (bad++ < 10) printf("centroid of level %u index %u -> %u\n", level, index, c); }
            int64_t g[6];
            grid_tri(index, level, g);
            const int64_t pts[12] = { g[0], g[1], g[2], g[3], g[4], g[5],
                                      (g[0] + g[2]) / 2, (g[1] + g[3]) / 2, (g[2] + g[4]) / 2, (g[3] + g[5]) / 2, (g[4] + g[0]) / 2, (g[5] + g[1]) / 2 };
            for (int p = 0; p < 6; ++p) {
                const uint32_t j = ommx_micro_index((float)pts[2 * p] * inv, (float)pts[2 * p + 1] * inv, level);
                checked++;
                int64_t h[6];
                if (j >= (1u << (2 * level))) { if (bad++ < 10) printf("level %u: index %u out of range\n", level, j); continue; }
                grid_tri(j, level, h);
                if (!closure_contains(h, pts[2 * p], pts[2 * p + 1])) {
                    if (bad++ < 10) printf("level %u index %u point %d (%lld, %lld)/%u -> %u, which does not contain it\n", level, index, p,
                                           (long long)pts[2 * p], (long long)pts[2 * p + 1], 2u << level, j);
                }
            }
        }
    }
    printf("lookup_check: %llu points, %llu failures\n", checked, bad);
    return bad ? 1 : 0;
}
