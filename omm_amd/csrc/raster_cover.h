// raster_cover.h -- the arithmetic of ommxRasterizeMicromap's rule (include/omm_mi355x_ext.h) as plain C++: the sample point of a pixel, the four
// cross products and the coverage decision, the barycentrics, a conservative pixel range of a triangle's bounding box, and the colours.  Device code
// in raster_kernels.hip, host code in tests/native/raster_check.cpp.  Everything is fp64 or integer, one rounding per written operation: the
// including translation unit must not contract a * b + c (-ffp-contract=off) and must keep IEEE semantics (no -ffast-math).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define OMMX_RASTER_FN __host__ __device__ __forceinline__
#else
#define OMMX_RASTER_FN static inline
#endif

namespace ommx {

constexpr uint32_t kRasterNone = 0xFFFFFFFFu;        // owner word / primitiveIds / microTriangles: nothing here
constexpr uint32_t kRasterStateInvalid = 0xFFu;      // states: the owner's state is OMMX_OPACITY_INVALID
constexpr uint32_t kRasterStateNone = 0xFEu;         // states: no primitive
constexpr uint32_t kRasterContour = 0xFF0000FFu;     // (255, 0, 0, 255) as the four bytes r, g, b, a of a little-endian word

struct RasterTri { double ax, ay, bx, by, cx, cy; };                                      // A, B, C in index-buffer order, widened from fp32
struct RasterView { double loU, loV, stepU, stepV; uint32_t width, height; };             // the viewport and its pixel grid

OMMX_RASTER_FN RasterView raster_view(const float uvMin[2], const float uvMax[2], uint32_t width, uint32_t height)
{
    RasterView v;
    v.loU = (double)uvMin[0]; v.loV = (double)uvMin[1];
    v.stepU = ((double)uvMax[0] - (double)uvMin[0]) / (double)width;
    v.stepV = ((double)uvMax[1] - (double)uvMin[1]) / (double)height;
    v.width = width; v.height = height;
    return v;
}

// the sample point of pixel i on one axis: the pixel's centre
OMMX_RASTER_FN double raster_sample(double lo, double step, uint32_t i) { return lo + ((double)i + 0.5) * step; }

OMMX_RASTER_FN double raster_area2(const RasterTri& t) { return (t.bx - t.ax) * (t.cy - t.ay) - (t.by - t.ay) * (t.cx - t.ax); }

// zero or not finite (x - x is 0 for every finite x and NaN otherwise).  A triangle with a coordinate that is not finite has such an area2: each of the
// two products then has an infinite or NaN factor
OMMX_RASTER_FN bool raster_degenerate(double area2) { return area2 == 0.0 || !(area2 - area2 == 0.0); }

// w[0..2] = wA, wB, wC at the point (U, V): twice the signed areas of (P, B, C), (P, C, A), (P, A, B).  A shared edge gives exactly negated values on
// its two sides: the differences are the same numbers and IEEE products and differences commute with negation
OMMX_RASTER_FN void raster_edges(const RasterTri& t, double U, double V, double w[3])
{
    w[0] = (t.bx - U) * (t.cy - V) - (t.by - V) * (t.cx - U);
    w[1] = (t.cx - U) * (t.ay - V) - (t.cy - V) * (t.ax - U);
    w[2] = (t.ax - U) * (t.by - V) - (t.ay - V) * (t.bx - U);
}

// the closed triangle, either winding: each of wA, wB, wC is zero or has area2's sign (area2 is not degenerate)
OMMX_RASTER_FN bool raster_covers(const double w[3], double area2)
{
    return area2 > 0.0 ? (w[0] >= 0.0 && w[1] >= 0.0 && w[2] >= 0.0) : (w[0] <= 0.0 && w[1] <= 0.0 && w[2] <= 0.0);
}

// the hit convention (1-u-v) V0 + u V1 + v V2
OMMX_RASTER_FN void raster_barycentrics(const double w[3], double area2, float* u, float* v)
{
    *u = (float)(w[1] / area2);
    *v = (float)(w[2] / area2);
}

// One axis of the box: the pixels [first, end) whose sample point can lie in [cmin, cmax].  Pixel i samples lo + (i + 0.5) * step, so it needs
// q(cmin) - 0.5 <= i <= q(cmax) - 0.5 with q(c) = (c - lo) / step; floor(q(cmin)) - 1 and ceil(q(cmax)) + 1 leave at least half a pixel on either
// side for the roundings of q, of the sample point and of the cross products.  Cut to [0, n]; the comparisons are written so that a NaN gives 0.
OMMX_RASTER_FN uint32_t raster_first_pixel(double cmin, double lo, double step, uint32_t n)
{
    const double f = __builtin_floor((cmin - lo) / step) - 1.0;
    return !(f > 0.0) ? 0u : (f >= (double)n ? n : (uint32_t)f);
}
OMMX_RASTER_FN uint32_t raster_end_pixel(double cmax, double lo, double step, uint32_t n)
{
    const double f = __builtin_ceil((cmax - lo) / step) + 1.0;
    return !(f > 0.0) ? 0u : (f >= (double)n ? n : (uint32_t)f);
}
OMMX_RASTER_FN double raster_min3(double a, double b, double c) { const double m = a < b ? a : b; return m < c ? m : c; }
OMMX_RASTER_FN double raster_max3(double a, double b, double c) { const double m = a > b ? a : b; return m > c ? m : c; }

// box = x0, x1, y0, y1: the pixels [x0, x1) x [y0, y1) of the view outside of which the triangle covers nothing; false: there are none.  Conservative;
// the exact predicate (raster_covers) decides inside.
OMMX_RASTER_FN bool raster_box(const RasterTri& t, const RasterView& v, uint32_t box[4])
{
    box[0] = raster_first_pixel(raster_min3(t.ax, t.bx, t.cx), v.loU, v.stepU, v.width);
    box[1] = raster_end_pixel(raster_max3(t.ax, t.bx, t.cx), v.loU, v.stepU, v.width);
    box[2] = raster_first_pixel(raster_min3(t.ay, t.by, t.cy), v.loV, v.stepV, v.height);
    box[3] = raster_end_pixel(raster_max3(t.ay, t.by, t.cy), v.loV, v.stepV, v.height);
    return box[0] < box[1] && box[2] < box[3];
}

// ---- the picture: integers only ----
// the background grey of an alpha value: clamped to [0, 1], NaN reads 0
OMMX_RASTER_FN uint32_t raster_grey(float alpha)
{
    const float a = alpha > 0.f ? (alpha < 1.f ? alpha : 1.f) : 0.f;
    return (uint32_t)(a * 255.f + 0.5f);
}
OMMX_RASTER_FN uint32_t raster_background(uint32_t g) { return g | (g << 8) | (g << 16) | 0xFF000000u; }

// the SDK's state colours as r | g << 8 | b << 16: Transparent, Opaque, UnknownTransparent, UnknownOpaque; anything else: invalid
OMMX_RASTER_FN uint32_t raster_state_colour(uint32_t state, bool monochromeUnknowns)
{
    switch (state) {
    case 0u: return 0xFF0000u;                                   // (0, 0, 255)
    case 1u: return 0x00FF00u;                                   // (0, 255, 0)
    case 2u: return monochromeUnknowns ? 0x00FFFFu : 0xFF00FFu;  // (255, 0, 255), drawn like UnknownOpaque under MonochromeUnknowns
    case 3u: return 0x00FFFFu;                                   // (255, 255, 0)
    default: return 0x0080FFu;                                   // (255, 128, 0)
    }
}

// a covered pixel: the state's colour averaged with the grey, rounding up; then darker by an eighth for an inverted micro-triangle, then halved for a
// reused block
OMMX_RASTER_FN uint32_t raster_covered(uint32_t state, uint32_t g, bool monochromeUnknowns, bool inverted, bool reused)
{
    const uint32_t lut = raster_state_colour(state, monochromeUnknowns);
    uint32_t out = 0xFF000000u;
    for (uint32_t k = 0; k < 3u; ++k) {
        uint32_t c = (((lut >> (8u * k)) & 0xFFu) + g + 1u) >> 1;
        if (inverted) c -= c >> 3;
        if (reused) c >>= 1;
        out |= c << (8u * k);
    }
    return out;
}

} // namespace ommx
