"""SetupWorkItems at its rounding, format and tile boundaries: a numpy restatement of the reference's per-triangle arithmetic and the case builders of
tests/test_setup_reference.py (oracle + numpy, no GPU) and tests/test_setup_gpu.py (HIP library vs oracle, and the library's result against the restatement).

The restatement follows bake_cpu_impl.cpp:470-560 (levels), :662-680 (workload), :1904-1915 with util/geometry.h:141-149 (areas) and util/geometry.h:37-47,
191-239 (fetch, validity, degenerate test) in fp32, one rounding per operation (numpy float32 arrays round every operation), conversions as x86 cvttss2si
does them (out of range or NaN: the integer indefinite, 0x80...0).  Two deliberately wrong variants exist to show that the case families can notice a
subtly wrong kernel: `fused` (a * b + c rounded once wherever area0, nz and eMax have that shape) and `approx_div` (the quotient as area * (1 / target)).

A case ("bake") is a dict: name, w, h, fp32 (texture format), buf (uint8 bytes of the coordinate buffer), offset (first coordinate's byte), stride (0 = default),
uv_format, ix (indices, dtype = index format), gmax (maxSubdivisionLevel), scale (dynamicSubdivisionScale), flags, levels (per triangle or None),
max_workload."""
import ctypes as C
import functools
import numpy as np
import ommtest as ot

F = np.float32
FLAG_DEGENERATE_INVALID = 1 << 8      # DisableLevelLineIntersection: degenerate triangles are not baked (bake_cpu_impl.cpp:563-575)
FLAG_AABB = 1 << 7                    # EnableAABBTesting: refused without bit 8, right behind the workload validation (:718-719)
FLAG_EDGE = 1 << 11                   # EnableEdgeHeuristic (:48, :547)
UNORM_SCALE = F(1.5259021896696421759314870504694e-5)
BASE_FLAGS = ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------
def half_to_float(h):
    """binary16 bit patterns -> float32 without a loop and without numpy's float16: normal numbers by re-biasing, denormals as m * 2^-24 (exact)"""
    h = np.asarray(h, np.uint32)
    sign, e, m = (h & 0x8000) << 16, (h >> 10) & 0x1F, h & 0x3FF
    normal = (sign | ((e + 112) << 23) | (m << 13)).astype(np.uint32).view(F)
    special = (sign | 0x7F800000 | (m << 13)).astype(np.uint32).view(F)
    den = (m.astype(F) * F(2.0 ** -24)).view(np.uint32) | sign.astype(np.uint32)
    return np.where(e == 0, den.view(F), np.where(e == 31, special, normal)).astype(F)


def default_stride(uv_format):
    return 8 if uv_format == ot.UV32_FLOAT else 4


def fetch(buf, uv_format, stride, ix, offset=0):
    """(T, 6) float32: FetchUVTriangle.  buf: uint8 array, ix: any integer array of 3 T indices"""
    buf = np.asarray(buf, np.uint8)
    stride = stride or default_stride(uv_format)
    base = offset + stride * np.asarray(ix, np.int64).reshape(-1)
    nbytes = 8 if uv_format == ot.UV32_FLOAT else 4
    raw = buf[base[:, None] + np.arange(nbytes)[None, :]]
    if uv_format == ot.UV32_FLOAT:
        p = np.ascontiguousarray(raw).view("<f4")
    else:
        v = np.ascontiguousarray(raw).view("<u2").astype(np.uint32)
        p = v.astype(F) * UNORM_SCALE if uv_format == ot.UV16_UNORM else half_to_float(v)
    return np.ascontiguousarray(p.reshape(-1, 6).astype(F))


def invalid(p):
    return ~np.all(np.isfinite(p), axis=1)


def _fma(a, b, c):
    """a * b + c rounded once (float64 holds the product of two float32 exactly)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def area0(p, fused=False):
    """util/geometry.h:44-47"""
    with np.errstate(all="ignore"):
        d0, d1, d2 = p[:, 3] - p[:, 5], p[:, 5] - p[:, 1], p[:, 1] - p[:, 3]
        if fused:
            s = _fma(p[:, 4], d2, _fma(p[:, 2], d1, p[:, 0] * d0))
        else:
            s = (p[:, 0] * d0 + p[:, 2] * d1) + p[:, 4] * d2
        return F(0.5) * np.abs(s)


def degenerate(p, fused=False):
    return area0(p, fused).astype(np.float64) < 1e-9


def area2d(ax, ay, bx, by, cx, cy, fused=False):
    """util/geometry.h:141-149: half the length of cross((c - a, 0), (b - a, 0)); the x and y components are +-0 for finite input"""
    with np.errstate(all="ignore"):
        v0x, v0y, v1x, v1y = cx - ax, cy - ay, bx - ax, by - ay
        nz = _fma(v0x, v1y, -(v1x * v0y)) if fused else v0x * v1y - v1x * v0y
        return F(0.5) * np.sqrt(nz * nz)       # (nz * nz is rounded to fp32: it underflows and overflows as the reference's does)


def uv_area(p):
    return area2d(p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4], p[:, 5])


def pixel_area(p, w, h, fused=False):
    fw, fh = F(w), F(h)
    with np.errstate(all="ignore"):
        return area2d(p[:, 0] * fw, p[:, 1] * fh, p[:, 2] * fw, p[:, 3] * fh, p[:, 4] * fw, p[:, 5] * fh, fused)


def cvt_u32(q):
    """uint32_t(float) on x86-64: cvttss2si r64, low 32 bits; NaN and |q| >= 2^63 give 0x8000000000000000, low bits 0"""
    q = np.asarray(q, F)
    ok = (q >= F(-2.0 ** 63)) & (q < F(2.0 ** 63))
    t = np.trunc(np.where(ok, q, F(0))).astype(np.float64)
    i = np.array([int(x) & 0xFFFFFFFF for x in t], np.uint64) if t.size else np.zeros(0, np.uint64)
    return np.where(ok, i, 0).astype(np.uint64)


def cvt_i32(x):
    """int(float) on x86: cvttss2si r32; NaN and out of range give INT_MIN"""
    x = np.asarray(x, F)
    ok = (x > F(-2147483904.0)) & (x < F(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, x, F(0))), -2147483648.0).astype(np.int64)


def level_of_count(v):
    """:502-508: next power of two in 32 bits, its log2, >> 1"""
    v = np.asarray(v, np.uint64)
    out = np.zeros(v.shape, np.int64)
    for i, x in enumerate(v.reshape(-1).tolist()):
        x = (x - 1) & 0xFFFFFFFF
        for s in (1, 2, 4, 8, 16):
            x |= x >> s
        x = (x + 1) & 0xFFFFFFFF
        out.reshape(-1)[i] = (x.bit_length() - 1 if x else 0) >> 1
    return out


def quotient(area, scale, approx_div=False):
    with np.errstate(all="ignore"):
        target = F(scale) * F(scale)
        return area * (F(1.0) / target) if approx_div else area / target


def area_level(p, w, h, scale, gmax, fused=False, approx_div=False):
    lv = level_of_count(cvt_u32(quotient(pixel_area(p, w, h, fused), scale, approx_div)))
    return np.minimum(lv, gmax)


def edge_emax(p, w, h, fused=False):
    fw, fh = F(w), F(h)
    with np.errstate(all="ignore"):
        out = None
        for a, b in ((0, 2), (0, 4), (2, 4)):
            ex, ey = fw * (p[:, b] - p[:, a]), fh * (p[:, b + 1] - p[:, a + 1])
            l = _fma(ex, ex, ey * ey) if fused else ex * ex + ey * ey
            out = l if out is None else np.where(out < l, l, out)
        return out


_LIBM = None


def glibc_log2f(x):
    global _LIBM
    if _LIBM is None:
        _LIBM = C.CDLL("libm.so.6")
        _LIBM.log2f.restype, _LIBM.log2f.argtypes = C.c_float, [C.c_float]
    return np.array([_LIBM.log2f(float(v)) for v in np.asarray(x, F).reshape(-1)], F).reshape(np.shape(x))


def log2f(x):
    """log2 of float32 values, rounded once: numpy's float64 log2 rounded to float32.  (numpy's float32 log2 differs from glibc's log2f, the oracle's, on
    2.2 % of 20 000 random inputs over 2^-20 ... 2^20, this one on 0.09 %; inputs on which it differs leave the edge-heuristic family, log2_agrees)"""
    with np.errstate(all="ignore"):
        return np.log2(np.asarray(x, F).astype(np.float64)).astype(F)


def edge_level(p, w, h, scale, gmax, fused=False):
    """:511-528"""
    e = edge_emax(p, w, h, fused)
    with np.errstate(all="ignore"):
        n = np.where(e.astype(np.float64) < 1e-6, F(0), log2f(np.maximum(e, F(1e-45))) / F(2) - log2f(F(scale)))
    return np.clip(cvt_i32(np.ceil(n.astype(F))), 0, gmax)


def log2_agrees(p, w, h, scale):
    """False where numpy's log2 and glibc's log2f differ on the edge heuristic's two arguments (such inputs leave the family)"""
    e = edge_emax(p, w, h)
    big = e.astype(np.float64) >= 1e-6
    ok = np.ones(len(p), bool)
    with np.errstate(all="ignore"):
        ok[big] = log2f(e[big]).view(np.uint32) == glibc_log2f(e[big]).view(np.uint32)
        return ok & bool(log2f(F(scale)).view(np.uint32) == glibc_log2f(F(scale)).view(np.uint32))


def setup(case, fused=False, approx_div=False):
    """per triangle: p, invalid, degenerate, level, area -- GetSubdivisionLevelForPrimitive and GetIsInvalid (:542-575)"""
    p = fetch(case["buf"], case["uv_format"], case["stride"], case["ix"], case["offset"])
    T = len(p)
    w, h, scale, gmax, flags = case["w"], case["h"], F(case["scale"]), case["gmax"], case["flags"]
    deg = degenerate(p, fused)
    inv = invalid(p) | (deg if flags & FLAG_DEGENERATE_INVALID else False)
    level = np.full(T, gmax, np.int64)
    if scale > 0:       # (NaN and negative scales compare false: the global level)
        use_edge = deg | bool(flags & FLAG_EDGE)
        level = np.where(use_edge, edge_level(p, w, h, scale, gmax, fused), area_level(p, w, h, scale, gmax, fused, approx_div))
    if case["levels"] is not None:
        lv = np.asarray(case["levels"], np.int64)
        level = np.where(lv <= 12, lv, level)
    area = np.where(inv, F(0), uv_area(p)).astype(F)
    return dict(p=p, invalid=inv, degenerate=deg, level=level, area=area)


def first_occurrence(p, level, inv, dedup=True):
    """first[t]: the triangle that owns t's work item (t itself for invalid triangles): equal coordinates (+-0 are one value to std::hash<float>) at equal level"""
    T = len(p)
    first = np.arange(T, dtype=np.int64)
    if not dedup:
        return first
    bits = np.where(p == 0, F(0), p).view(np.uint32).astype(np.uint64)
    key = np.concatenate([bits, np.asarray(level, np.uint64)[:, None]], axis=1)
    live = np.nonzero(~inv)[0]
    if len(live):
        _, idx, inverse = np.unique(key[live], axis=0, return_index=True, return_inverse=True)
        first[live] = live[idx[inverse.reshape(-1)]]
    return first


def workload(p, first, inv, w, h):
    """ComputeWorkloadSize (:662-680) over the work items: int2((aabb_e - aabb_s) * size), int product, sign-extended, summed in 64 bits"""
    items = np.nonzero((first == np.arange(len(p))) & ~inv)[0]
    q = p[items]
    with np.errstate(all="ignore"):
        dx = (np.max(q[:, 0::2], axis=1) - np.min(q[:, 0::2], axis=1)) * F(w)
        dy = (np.max(q[:, 1::2], axis=1) - np.min(q[:, 1::2], axis=1)) * F(h)
    total = 0
    for ax, ay in zip(cvt_i32(dx).tolist(), cvt_i32(dy).tolist()):
        prod = ((ax & 0xFFFFFFFF) * (ay & 0xFFFFFFFF)) & 0xFFFFFFFF
        total += prod - (1 << 32) if prod & 0x80000000 else prod
    return total & 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------------------------
# running a case
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def texture(w, h, fp32):
    """one to three texel noise around the cut-off 0.5"""
    n = ot.value_noise(1000 + 7 * w + h, max(w, 2), max(h, 2), octaves=2, base_cell=2)[:h, :w]
    n = np.ascontiguousarray(n)
    return n if fp32 else np.ascontiguousarray((n * 255).astype(np.uint8))


def make_case(name, w, h, uv, ix, gmax, *, fp32=True, scale=0.0, flags=BASE_FLAGS, levels=None, uv_format=ot.UV32_FLOAT, stride=0, offset=0,
              max_workload=0xFFFFFFFFFFFFFFFF, buf=None):
    if buf is None:
        buf = np.ascontiguousarray(uv).view(np.uint8).reshape(-1)
    return dict(name=name, w=w, h=h, fp32=fp32, buf=np.ascontiguousarray(buf), offset=offset, stride=stride, uv_format=uv_format, ix=np.ascontiguousarray(ix),
                gmax=gmax, scale=float(F(scale)), flags=flags,
                levels=None if levels is None else np.ascontiguousarray(levels, np.uint8), max_workload=max_workload)


def desc_of(case, tex):
    """the bake desc of a case over a texture handle; the desc keeps its buffers alive"""
    d = ot.make_desc(tex, case["buf"], case["ix"], case["gmax"], addr=ot.WRAP, promo=ot.PROMO_NEAREST, flags=case["flags"], dyn_scale=case["scale"],
                     uv_format=case["uv_format"], levels=case["levels"], max_workload=case["max_workload"])
    d.texCoords = case["buf"].ctypes.data + case["offset"]
    d.texCoordStrideInBytes = case["stride"]
    return d


def run(lib, case, expect=ot.SUCCESS, want_areas=False, validation=False):
    """one bake of `case` on a fresh baker: dict(result=BakeResult or None, code, messages, areas (oracle only))"""
    msgs = []
    b = lib.create_baker(callback=lambda s, m, u: msgs.append(m.decode()))
    t = lib.create_texture(b, [texture(case["w"], case["h"], case["fp32"])], alpha_cutoff=0.5)
    d = desc_of(case, t)
    if validation:
        d.bakeFlags |= ot.FLAG_VALIDATION
    out = dict(result=None, areas=None)
    code, handle = lib.bake_raw(b, d)
    assert code == expect, (case["name"], lib.which, code, expect, msgs)
    if code == ot.SUCCESS:
        pd = C.POINTER(ot.BakeResultDesc)()
        assert lib.fn("ommCpuGetBakeResultDesc")(handle, C.byref(pd)) == ot.SUCCESS
        out["result"] = ot.BakeResult(pd.contents)
        st2 = ot.DebugStats()
        assert lib.fn("ommDebugGetStats2")(b, handle, C.byref(st2)) == ot.SUCCESS
        out["result"].stats2 = st2
        if want_areas and lib.which == "oracle":
            lib.dll.oracle_bake_result_areas.restype, lib.dll.oracle_bake_result_areas.argtypes = C.POINTER(C.c_float), [C.c_void_p]
            T = len(case["ix"]) // 3
            out["areas"] = np.ctypeslib.as_array(lib.dll.oracle_bake_result_areas(handle), (T,)).copy() if T else np.zeros(0, F)
        assert lib.fn("ommCpuDestroyBakeResult")(handle) == ot.SUCCESS
    else:
        assert not handle.value
    lib.destroy_texture(b, t)
    lib.destroy_baker(b)
    out["code"], out["messages"] = code, msgs
    return out


def check_result_against_restatement(case, res, s=None, first=None):
    """descriptor levels of valid triangles, the unresolved index of invalid ones, one descriptor per work item shared with its first occurrence
    (cases carry DisableSpecialIndices, so every valid triangle has a descriptor)"""
    s = s or setup(case)
    idx = res.index.astype(np.int64)
    assert len(idx) == len(s["p"])
    assert np.array_equal(idx < 0, s["invalid"]), (case["name"], np.nonzero((idx < 0) != s["invalid"])[0][:8])
    assert np.all(idx[s["invalid"]] == ot.SPECIAL_FUO)
    valid = ~s["invalid"]
    got = res.descs[idx[valid], 1] if valid.any() else np.zeros(0, np.int64)
    bad = np.nonzero(got != s["level"][valid])[0]
    assert bad.size == 0, (case["name"], "levels differ for %d triangles, first %r: got %r want %r" % (bad.size, np.nonzero(valid)[0][bad[:5]], got[bad[:5]], s["level"][valid][bad[:5]]))
    if first is not None:
        assert np.array_equal(idx, idx[first]), case["name"]
    return s


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family 1: level boundaries of the area heuristic
# ---------------------------------------------------------------------------------------------------------------------------------------------
def nextf(x, n=1):
    x = F(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F(np.inf) if n > 0 else F(-np.inf))
    return x


LISTED_K = sorted({1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65} | {4 ** L + d for L in range(13) for d in (-1, 0, 1) if 4 ** L + d >= 1})
# where the level really steps: count 2 * 4^L -> 2 * 4^L + 1 (next power of two 2^(2L+1) -> 2^(2L+2)); the listed k mostly sit inside a level
STEP_K = [2 * 4 ** L + 1 for L in range(12)]
BIG_K = [2.0 ** 24, 2.0 ** 31, 2.0 ** 32, 2.0 ** 63]
POW2_SCALES = [2.0, 0.5, 2.0 ** -10, 2.0 ** -16]
ROUNDED_SCALES = [0.7, 1.5, 3.0, 1.0 / 3.0, 1e-3, 255.99, 1e-5, 1e-9]
ODD_SCALES = [1e-23, 1e20, float("inf"), float("nan"), -1.0, -0.0, 1e-40]
SHAPES = [(64, 64), (300, 200), (1, 64), (64, 1), (8, 8)]
MAX_PIXEL_AREA, MIN_PIXEL_AREA = 300.0, 1e-4


def reachable(k, scale):
    """a triangle of a few texels reaches count k at this scale (counts to 5 are level 0 or 1: there a large triangle stays cheap)"""
    a_px = k * float(F(scale) * F(scale))
    return MIN_PIXEL_AREA <= a_px and (a_px <= MAX_PIXEL_AREA or (k <= 5 and a_px <= 4e5))


def _areas_around(k, scale):
    """{side: area}: float32 areas whose fp32 quotient by scale^2 is the largest reachable float below k (-1), k itself (0, if some area gives it) and
    the smallest reachable float above k (+1).  With an exact division these are k's neighbours; a rounded division skips quotients (the area's spacing
    divided by scale^2 can exceed the quotient's), then the nearest reachable ones stand in"""
    target = F(scale) * F(scale)
    with np.errstate(all="ignore"):
        a0 = F(k) * target
    if not np.isfinite(a0) or a0 <= 0:
        return {}
    cand = np.array([nextf(a0, d) for d in range(-4, 5)], F)
    q = cand / target
    wrong = (cand * (F(1) / target) != q)          # where several areas serve, one on which a multiplication by the reciprocal shows is preferred
    out = {}
    below = q[q < F(k)]
    for side, m in ((-1, q == below[-1] if len(below) else q != q), (0, q == F(k))):
        if m.any():
            out[side] = cand[m & wrong][0] if (m & wrong).any() else cand[m][0]
    if (q > F(k)).any():
        out[1] = cand[q > F(k)][0]
    return out


def _triangle_with_pixel_area(A, w, h, skew, origin):
    """a triangle whose restated pixel area is exactly A, or None: legs x (free) and y (a power of two times h), checked through the restatement"""
    two_a = F(2) * F(A)
    for ylog in (0, -1, 1, -2, 2, -3):
        cv = F(2.0 ** (ylog - int(np.ceil(np.log2(h)))))          # y = cv * h px, about 2^ylog
        y = F(cv * F(h))
        for dx in (0, -1, 1, -2, 2):
            x = nextf(two_a / y, dx)
            for du in (0, -1, 1):
                bu = nextf(x / F(w), du)
                p = np.array([[origin[0], origin[1], origin[0] + bu, origin[1], origin[0] + (bu * F(0.375) if skew else F(0)), origin[1] + cv]], F)
                if pixel_area(p, w, h)[0].view(np.uint32) == F(A).view(np.uint32) and not degenerate(p)[0]:
                    return p[0]
    return None


@functools.lru_cache(maxsize=None)
def family1_triangles(scale):
    """(T, 6) triangles, their (w, h), and for each the boundary it serves: (k, side) with side -1 / 0 / +1 = the quotient is the (nearest reachable) float below k / k / above k"""
    scale = float(scale)
    out = []
    ks = [(float(k), k in STEP_K or k == 3) for k in sorted(set(LISTED_K) | set(STEP_K))] + [(k, True) for k in BIG_K] + [(2.0 ** 32 + 512, True)]
    for k, real in ks:
        if not reachable(k, scale):
            continue
        shapes = (SHAPES[:2] if scale in POW2_SCALES else SHAPES) if real else SHAPES[:1]
        for side, A in sorted(_areas_around(k, scale).items()):
            for si, (w, h) in enumerate(shapes):
                for skew in ((False, True) if real else (bool(si & 1),)):
                    for origin in (((F(0), F(0)), (F(0.25), F(0.5))) if real and side <= 0 else ((F(0), F(0)),)):
                        p = _triangle_with_pixel_area(A, w, h, skew, origin)
                        if p is not None:
                            out.append((p, (w, h), float(k), side))
    return out


FAMILY1_VARIANTS = ["max6", "max2", "max6-overrides"]
ALL_K = sorted(set(float(k) for k in LISTED_K) | set(float(k) for k in STEP_K) | set(BIG_K) | {2.0 ** 32 + 512})


def family1_cases(scale, variant=None):
    """the triangles of one scale grouped by texture shape; each shape with and without per-triangle overrides, a global maximum that never clamps
    a level below 7 (6) and one that does (2).  `variant`: one of FAMILY1_VARIANTS, or None for all"""
    tris = family1_triangles(scale)
    cases = []
    for si, (w, h) in enumerate(SHAPES):
        sel = [t for t in tris if t[1] == (w, h)]
        if not sel:
            continue
        uv = np.array([t[0] for t in sel], F).reshape(-1, 2)
        ix = np.arange(len(uv), dtype=np.uint32)
        T = len(sel)
        over = np.where(np.arange(T) % 3 == 1, np.array([0, 5, 1, 3] if scale < 16 else [0, 2, 1, 2])[np.arange(T) % 4], 0xF).astype(np.uint8)      # (large scales: large triangles, low levels)
        for gmax, levels, tag in ((6, None, "max6"), (2, None, "max2"), (6, over, "max6-overrides")):
            if variant not in (None, tag):
                continue
            c = make_case("f1-s%g-%dx%d-%s" % (scale, w, h, tag), w, h, uv, ix, gmax, fp32=bool(si & 1) ^ (gmax == 2), scale=scale, levels=levels)
            c["boundary"] = [(t[2], t[3]) for t in sel]
            cases.append(c)
    return cases


def family1_odd_scale_cases():
    """scales whose square underflows, overflows or is not a positive number: a handful of ordinary triangles each"""
    uv, ix = ot.random_triangles(77, 24, 0.1)
    return [make_case("f1-odd-%r" % s, 64, 64, uv, ix, 3, scale=F(s), fp32=bool(i & 1)) for i, s in enumerate(ODD_SCALES)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family 2: the degenerate threshold and the host's edge heuristic
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family2_threshold_triangles():
    """area0 = the floats around float32(1e-9) (which is below the double 1e-9: degenerate; its successor is not), then triangles on which the fused
    variant disagrees about `degenerate`: at the origin (sum of two products) and at offsets of 100 - 4000 UV units where three products cancel"""
    T9 = F(1e-9)
    tris = []
    for d in range(-3, 4):
        target = nextf(T9, d)
        a = F(2.0 ** -14)
        b = F(F(2) * target / a)
        tris.append([0, 0, a, 0, 0, b])                  # right triangle: area0 = 0.5 * fl(a * b), a a power of two
        tris.append([0, 0, a, 0, a * F(0.25), b])        # skew
    exact = np.array(tris, F)
    assert all(area0(exact).view(np.uint32)[2 * i] == nextf(T9, d).view(np.uint32) for i, d in enumerate(range(-3, 4)))
    rng = np.random.default_rng(2024)
    found = []
    for mag in (1.0, 100.0, 1000.0, 4000.0):
        n = 400000
        o = (rng.random((n, 2)) * mag).astype(F)
        size = F(4e-4) if mag == 1.0 else F(2e-3)
        e = ((rng.random((n, 4)) - 0.5) * size).astype(F)
        if mag == 1.0:
            e[:, 2:] = e[:, :2] * F(0.5) + e[:, 2:] * F(0.05)     # slivers inside [0, 1): an area0 around 1e-9 left over by products of 1e-4
        p = np.stack([o[:, 0], o[:, 1], o[:, 0] + e[:, 0], o[:, 1] + e[:, 1], o[:, 0] + e[:, 2], o[:, 1] + e[:, 3]], axis=1).astype(F)
        flips = np.nonzero(degenerate(p) != degenerate(p, fused=True))[0][:40]
        found.append(p[flips])
    return exact, np.concatenate(found)


def family2_threshold_cases():
    exact, flips = family2_threshold_triangles()
    uv = np.concatenate([exact, flips]).reshape(-1, 2)
    ix = np.arange(len(uv), dtype=np.uint32)
    cases = []
    for tag, scale, flags in (("dyn-off", 0.0, BASE_FLAGS), ("dyn-on", 2.0 ** -6, BASE_FLAGS), ("dyn-on-invalid", 2.0 ** -6, BASE_FLAGS | FLAG_DEGENERATE_INVALID),
                              ("dyn-off-invalid", 0.0, BASE_FLAGS | FLAG_DEGENERATE_INVALID)):
        cases.append(make_case("f2-threshold-" + tag, 64, 64, uv, ix, 3, scale=scale, flags=flags, fp32=scale == 0.0))
    return cases


def _edge_with_emax(E, w, h):
    """(ex, ey) in pixels with fl(fl(ex * ex) + fl(ey * ey)) == E, both realisable as w * du and h * dv for power-of-two w, h; or None"""
    E = F(E)
    root = np.sqrt(E)
    for j in range(0, 6):
        ex = nextf(root, -j)
        r = np.float64(E) - np.float64(ex) * np.float64(ex)
        if r < 0:
            continue
        for d in range(-3, 4):
            ey = nextf(F(np.sqrt(r)), d) if r > 0 else F(0)
            if ey >= 0 and (ex * ex + ey * ey).view(np.uint32) == E.view(np.uint32):
                return ex, ey
    return None


def _log2_of_scale_agrees(s):
    return bool(log2f(F(s)).view(np.uint32) == glibc_log2f(F(s)).view(np.uint32))


# powers of two and not; of the latter only scales whose own log2f numpy and glibc agree on (it enters every triangle's level)
EDGE_SCALES = [2.0 ** -12, 0.25, 1.0] + [s for s in (0.7, 1e-3, 1.0 / 3.0, 1.5, 3.0, 0.3) if _log2_of_scale_agrees(s)][:3]


@functools.lru_cache(maxsize=None)
def family2_edge_triangles(scale, w=64, h=32):
    """collinear triangles (p1 = p2 / 2: degenerate, so they reach the host with and without bit 11) whose eMax sits at the ceilf boundary of level k -> k + 1
    for k = 0 ... 6 (found by scanning the floats around 4^k * scale^2), and around 1e-6.  Returns (triangles, dropped-for-log2f count)"""
    gmax = 7
    want = [nextf(F(1e-6), d) for d in (-1, 0, 1, 2)]
    for k in range(7):
        c = F(4.0 ** k) * (F(scale) * F(scale))
        if not (1e-6 < float(c) < 1e7):
            continue
        cand = np.array([nextf(c, d) for d in range(-24, 25)], F)
        q = np.zeros((len(cand), 6), F)
        q[:, 4] = np.sqrt(cand) / F(w)        # a stand-in triangle whose only job is to carry eMax through the restatement below
        with np.errstate(all="ignore"):
            n = log2f(cand) / F(2) - log2f(F(scale))
        lv = cvt_i32(np.ceil(n))
        step = np.nonzero(lv[1:] != lv[:-1])[0]
        for s in step:
            want += [cand[s - 1], cand[s], cand[s + 1], cand[s + 2]]
        want.append(c)
    tris = []
    for E in want:
        e = _edge_with_emax(E, w, h)
        if e is None:
            continue
        px, py = F(e[0] / F(w)), F(e[1] / F(h))
        p = np.array([[0, 0, px * F(0.5), py * F(0.5), px, py]], F)
        if edge_emax(p, w, h)[0].view(np.uint32) == F(E).view(np.uint32) and degenerate(p)[0]:
            tris.append(p[0])
    tris = np.array(tris, F).reshape(-1, 6)
    ok = log2_agrees(tris, w, h, scale)
    return tris[ok], int((~ok).sum())


def family2_edge_cases():
    cases = []
    for i, scale in enumerate(EDGE_SCALES):
        tris, _ = family2_edge_triangles(scale)
        if not len(tris):
            continue
        uv = tris.reshape(-1, 2)
        for tag, flags in (("degenerate", BASE_FLAGS), ("bit11", BASE_FLAGS | FLAG_EDGE)):
            cases.append(make_case("f2-edge-s%g-%s" % (scale, tag), 64, 32, uv, np.arange(len(uv), dtype=np.uint32), 7, scale=scale, flags=flags, fp32=bool(i & 1)))
    return cases


PENDING_COUNTS = [1, 255, 256, 257, 8191, 8192, 8193]


def family2_pending_case(count, threads=True, w=64, h=64, scale=2.0 ** -4):
    """`count` pending (degenerate, no override) triangles whose level depends on their position, between ordinary triangles; every 16th pending
    triangle repeats the one 5 before it; behind them, non-pending copies (override = the heuristic's level: merged by the rehash; override one level
    up: a separate item) of some pending triangles"""
    k = np.arange(count)
    lvl = (k * 7 + k // 5) % 4                                   # edge of 2^lvl * scale px -> n = lvl exactly
    length = (F(2.0) ** lvl.astype(F)) * F(scale) / F(w)
    ox = ((k % 61) / F(64)).astype(F)
    oy = ((k // 61 % 64) / F(64)).astype(F) + ((k // 3904) * F(2.0 ** -9)).astype(F)
    deg = np.stack([ox, oy, ox + length * F(0.5), oy, ox + length, oy], axis=1).astype(F)
    rep = np.nonzero((k % 16 == 15) & (k >= 5))[0]
    deg[rep] = deg[rep - 5]
    lvl = lvl.copy()
    lvl[rep] = lvl[rep - 5]
    plain, _ = ot.random_triangles(5, (count + 2) // 3, 0.01)
    plain = plain.reshape(-1, 6)
    tris, over = [], []
    for i in range(count):
        tris.append(deg[i]); over.append(0xF)
        if i % 3 == 2:
            tris.append(plain[i // 3]); over.append(1)
    picks = list(range(0, count, max(1, count // 40)))[:40]
    for j in picks:
        tris.append(deg[j]); over.append(int(lvl[j]))            # merges with the pending triangle once the host's level is hashed in
        tris.append(deg[j]); over.append(int(lvl[j]) + 1)        # same coordinates, another level: its own item
    uv = np.array(tris, F).reshape(-1, 2)
    flags = BASE_FLAGS if threads else (BASE_FLAGS & ~ot.FLAG_THREADS)
    c = make_case("f2-pending-%d-%s" % (count, "threads" if threads else "nothreads"), w, h, uv, np.arange(len(uv), dtype=np.uint32), 3, scale=scale, flags=flags,
                  levels=np.array(over, np.uint8), fp32=bool(count & 1))
    c["pending"] = count
    return c


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family 3: every 16-bit coordinate, strides, index formats
# ---------------------------------------------------------------------------------------------------------------------------------------------
SLICE = 8192
HALF_FIXED = 0x3800          # 0.5
HALF_PARTNER = 0x3802        # 0.5 + two half spacings
UNORM_FIXED, UNORM_PARTNER = 32768, 32770


def family3_sweep_case(uv_format, axis, lo, hi=None, stride=0, gmax=1):
    """patterns lo ... hi - 1 of a 16-bit format along `axis` (0 = u, 1 = v), the other coordinate fixed near 0.5.  Vertex j carries pattern lo + j (one more
    than the slice, the last wraps to pattern 0), vertex n + 1 + j its partner (same pattern, the other coordinate two spacings further): triangle i =
    (vertex i, vertex i + 1, partner i), thin, levels cycling 0 ... gmax per triangle"""
    hi = lo + SLICE if hi is None else hi
    n = hi - lo
    pat = (np.arange(lo, hi + 1) & 0xFFFF).astype(np.uint16)
    fixed, partner = (HALF_FIXED, HALF_PARTNER) if uv_format == ot.UV16_FLOAT else (UNORM_FIXED, UNORM_PARTNER)
    verts = np.zeros((2 * (n + 1), 2), np.uint16)
    verts[:n + 1, axis], verts[:n + 1, 1 - axis] = pat, fixed
    verts[n + 1:, axis], verts[n + 1:, 1 - axis] = pat, partner
    i = np.arange(n, dtype=np.uint32)
    ix = np.stack([i, i + 1, i + n + 1], axis=1).reshape(-1)
    st = stride or 4
    buf = np.full(len(verts) * st + 8, 0xA5, np.uint8)      # padding bytes that are no valid coordinate of the sweep
    raw = verts.view(np.uint8).reshape(-1, 4)
    for b in range(4):
        buf[b:b + len(verts) * st:st][:len(verts)] = raw[:, b]
    levels = (i % (gmax + 1)).astype(np.uint8)
    name = "f3-%s-%s-%d-%d-stride%d" % ("half" if uv_format == ot.UV16_FLOAT else "unorm", "uv"[axis], lo, hi, stride)
    return make_case(name, 8, 8, None, ix, gmax, fp32=bool(lo // SLICE & 1), uv_format=uv_format, stride=stride, levels=levels, buf=buf)


def family3_sweeps():
    return [(f, axis, lo) for f in (ot.UV16_FLOAT, ot.UV16_UNORM) for axis in (0, 1) for lo in range(0, 65536, SLICE)]


def family3_stride_cases():
    """strides and base offsets for the three formats, on a short sweep / 75 ordinary triangles"""
    cases = []
    for f in (ot.UV16_FLOAT, ot.UV16_UNORM):
        for stride in (0, 4, 8, 12, 16, 5, 6, 7):
            cases.append(family3_sweep_case(f, stride & 1, 0x3000, 0x3000 + 301, stride=stride))
    uv, ix = ot.random_triangles(31, 75, 0.08)
    for stride, offset in ((0, 0), (8, 0), (12, 0), (16, 0), (8, 1), (9, 0), (11, 3), (12, 2), (16, 4)):
        buf = np.full(len(uv) * (stride or 8) + offset + 8, 0x5A, np.uint8)
        raw = uv.view(np.uint8).reshape(-1, 8)
        for b in range(8):
            buf[offset + b::(stride or 8)][:len(uv)] = raw[:, b]
        cases.append(make_case("f3-f32-stride%d-offset%d" % (stride, offset), 32, 32, None, ix, 2, uv_format=ot.UV32_FLOAT, stride=stride, offset=offset, buf=buf,
                               fp32=bool(stride & 1)))
    return cases


def family3_index_cases():
    """8 / 16 / 32-bit mesh indices whose largest representable (or last) vertex is referenced; triangle counts that are no multiple of 4"""
    cases = []
    for dtype, nverts, T in ((np.uint8, 256, 85), (np.uint16, 65536, 1023), (np.uint32, 70001, 1021)):
        rng = np.random.default_rng(nverts)
        uv = np.zeros((nverts, 2), F)
        ix = np.zeros((T, 3), np.int64)
        corners = rng.permutation(nverts - 1)[:3 * T - 1]
        corners = np.concatenate([corners, [nverts - 1]])               # the last vertex = the largest index, referenced once
        rng.shuffle(corners)
        ix[:] = corners.reshape(T, 3)
        tri, _ = ot.random_triangles(nverts, T, 0.05)
        uv[ix.reshape(-1)] = tri
        assert ix.max() == nverts - 1 and T % 4
        for f in (ot.UV32_FLOAT, ot.UV16_UNORM, ot.UV16_FLOAT):
            if f == ot.UV32_FLOAT:
                buf = uv.view(np.uint8).reshape(-1)
            elif f == ot.UV16_UNORM:
                buf = np.clip(np.rint(uv * 65535), 0, 65535).astype(np.uint16).view(np.uint8).reshape(-1)
            else:
                buf = uv.astype(np.float16).view(np.uint8).reshape(-1)
            cases.append(make_case("f3-index%d-format%d" % (np.dtype(dtype).itemsize * 8, f), 32, 32, None, ix.astype(dtype).reshape(-1), 2, uv_format=f, buf=buf.copy()))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family 4: dedup, numbering and the level split at their tile edges
# ---------------------------------------------------------------------------------------------------------------------------------------------
COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 65 * 1024 + 1, 64 * 4096 + 1]
SMALL_COUNTS = [c for c in COUNTS if c <= 4097]
BIG_COUNTS = [c for c in COUNTS if c > 4097]
RUN_LENGTHS = [1, 2, 3, 63, 64, 65]
PATTERNS = ["unique", "equal", "every1024", "every4096", "last-lane", "runs0", "runs1", "runs31", "abab", "abcabc", "nan-edges", "levels", "runs31-nodedup"]


def family4_keys(pattern, n):
    """(key, nan, level) per triangle: triangles with equal key carry equal coordinates; level follows the key except for `levels`"""
    t = np.arange(n, dtype=np.int64)
    nan = np.zeros(n, bool)
    key = t.copy()
    if pattern == "equal":
        key[:] = 0
    elif pattern == "every1024":
        key = t % 1024
    elif pattern == "every4096":
        key = t % 4096
    elif pattern == "last-lane":
        m = (t % 64 == 0) & (t > 0)                      # the copy sits in the first lane of a wave / tile, its first occurrence in the last lane before
        key[m] = t[m] - 1
    elif pattern.startswith("runs"):
        shift = int(pattern[4:].split("-")[0])
        u = t - shift
        slot, o = u // 128, u % 128
        length = np.array(RUN_LENGTHS)[slot % 6]
        m = (u >= 0) & (o < length)
        key[m] = (slot[m] * 128 + shift)
    elif pattern == "abab":
        key = t // 256 * 256 + t % 2
    elif pattern == "abcabc":
        key = t // 192 * 192 + t % 3
    elif pattern == "nan-edges":
        for edge in (64, 256, 1024, 4096):
            nan |= (t % edge == 0) | (t % edge == edge - 1)
        nan[0] = nan[n - 1] = True
        if n > 4:
            nan[1::2] &= (t[1::2] % 1024 >= 1022) | (t[1::2] % 1024 == 0) | (t[1::2] == n - 1)      # keep most 64-edges one-sided
    level = key % 4
    if pattern in ("abab", "abcabc"):
        level = (key + t // (256 if pattern == "abab" else 192)) % 4     # (two or three keys per segment: the segment number brings in the other levels)
    if pattern == "levels":
        key, level = t // 8, (t % 8) // 2                # equal coordinates at four levels, each twice
    return key, nan, level


def family4_case(pattern, n):
    key, nan, level = family4_keys(pattern, n)
    # the triangle of key k: a 1 / 2048 UV (0.03 px) triangle at grid position k of a 512-wide grid over [0, 1)
    ox, oy = ((key % 512) / F(512)).astype(F), ((key // 512) / F(1024)).astype(F)
    e = F(1.0 / 2048)
    p = np.stack([ox, oy, ox + e, oy, ox, oy + e * F(0.5)], axis=1).astype(F)
    p[nan, (np.arange(n) % 6)[nan]] = np.nan
    flags = BASE_FLAGS | (ot.FLAG_NO_DEDUP if pattern.endswith("nodedup") else 0)
    c = make_case("f4-%s-%d" % (pattern, n), 64, 64, p.reshape(-1, 2), np.arange(3 * n, dtype=np.uint32), 3, levels=level.astype(np.uint8), flags=flags, fp32=bool(n & 1))
    c["key"], c["nan"] = key, nan
    return c


def hot_key_cases(n=20000):
    """the worst cases of the two hash builds (tests/scripts/hot_keys.py times them at 500 000 triangles): texture and (name, uv, expectation on the
    block count) -- n copies of one triangle, one hot key in the UV-dedup table; n shifted copies with identical content, one hot key in the digest table"""
    period = 64
    tile = np.zeros((period, period), np.uint8)
    tile[:, period // 2:] = 255
    tile[:, period // 2 - 2:period // 2 + 2] = np.array([40, 100, 160, 220], np.uint8)[None, :]
    tex = np.tile(tile, (2048 // period, 2048 // period))
    base = np.array([[0.0146, 0.0113], [0.0166, 0.0109], [0.0154, 0.0138]], F)
    uv_a = np.tile(base, (n, 1)).astype(F)
    k = np.arange(n)
    shift = np.stack([(k % 32) * (period / 2048.0), ((k // 32) % 32) * (period / 2048.0)], 1).astype(F)
    shift += np.stack([(k // 1024) * 1.0, np.zeros(n)], 1).astype(F)
    uv_b = (base[None, :, :] + shift[:, None, :]).reshape(-1, 2).astype(F)
    return tex, [("one-triangle", uv_a, lambda blocks: blocks == 1), ("shifted-copies", uv_b, lambda blocks: blocks <= 64)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family 5: the workload figure
# ---------------------------------------------------------------------------------------------------------------------------------------------
def family5_mesh():
    """64x64 texture: boxes of x.999 px, duplicates (count once), NaN triangles (count not at all)"""
    rng = np.random.default_rng(5)
    n = 90
    o = (rng.random((n, 2)) * 0.7).astype(F)
    ext = ((rng.integers(1, 9, (n, 2)) + 0.999) / 64.0).astype(F)        # 1.999 ... 8.999 px: the conversion truncates
    p = np.stack([o[:, 0], o[:, 1], o[:, 0] + ext[:, 0], o[:, 1], o[:, 0], o[:, 1] + ext[:, 1]], axis=1).astype(F)
    p[10:20] = p[0:10]                                                   # duplicates
    p[25::9, 3] = np.nan                                                 # invalid
    return make_case("f5-mesh", 64, 64, p.reshape(-1, 2), np.arange(3 * n, dtype=np.uint32), 2)


def family5_wrap_cases():
    """one triangle whose box makes the 32-bit product wrap (46341^2 = 2^31 + 4633: negative; 65536 * 65537 = 2^32 + 65536: small and positive) among a few
    ordinary ones.  Only for bakes that both libraries refuse."""
    out = []
    for tag, ax, ay in (("negative", 46341.0, 46341.0), ("small-positive", 65536.0, 65537.0)):
        base = family5_mesh()
        p = fetch(base["buf"], ot.UV32_FLOAT, 0, base["ix"])[:12].copy()
        p[5] = np.array([0, 0, (ax + 0.5) / 64, 0, 0, (ay + 0.5) / 64], F)
        out.append(make_case("f5-wrap-" + tag, 64, 64, p.reshape(-1, 2), np.arange(36, dtype=np.uint32), 2))
    return out


def with_limit(case, limit, extra_flags=0):
    c = dict(case)
    c["max_workload"], c["flags"] = limit, case["flags"] | extra_flags
    return c
