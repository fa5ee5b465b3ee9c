"""Shared by tests/test_rasterize.py, tests/test_rasterize_gpu.py and tests/scripts/rasterize_throughput.py: the ctypes view of ommxRasterizeMicromap
(include/omm_mi355x_ext.h), a float64 numpy model of its rule, a second model with loops over pixels and primitives in Python floats, and the device
side of a scene (texture, mesh, result) with a call that guards every output.  See tests/README_rasterize.md."""
import ctypes as C
import numpy as np
import ommtest as ot
import lookup_util as lu

NONE = 0xFFFFFFFF
STATE_INVALID, STATE_NONE = 0xFF, 0xFE
ALL = 0xFFFFFFFF
NO_CONTOUR, MONOCHROME_UNKNOWNS, HIGHLIGHT_REUSE = 1, 2, 4
MAX_SIZE = 16384
LUT = {0: (0, 0, 255), 1: (0, 255, 0), 2: (255, 0, 255), 3: (255, 255, 0), STATE_INVALID: (255, 128, 0)}   # the SDK's colours: data
CONTOUR = (255, 0, 0, 255)
FILL = 0xAB
OUTPUTS = ("primitiveIds", "microTriangles", "states", "alphaTest", "rgba")
OUT_DTYPE = dict(primitiveIds=np.uint32, microTriangles=np.uint32, states=np.uint8, alphaTest=np.uint8, rgba=np.uint8)
OUT_BYTES = dict(primitiveIds=4, microTriangles=4, states=1, alphaTest=1, rgba=4)
INFO_FIELDS = ("coveredPixels", "pixelsPerState", "invalidPixels", "alphaAbovePixels", "contradictions", "drawnPrimitives", "degeneratePrimitives")


class RasterDesc(C.Structure):
    _fields_ = [("uvMin", C.c_float * 2), ("uvMax", C.c_float * 2), ("width", C.c_uint32), ("height", C.c_uint32), ("firstPrimitive", C.c_uint32),
                ("primitiveCount", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint8 * 4)]


class RasterOutputs(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in OUTPUTS]


class RasterInfo(C.Structure):
    _fields_ = [("coveredPixels", C.c_uint64), ("pixelsPerState", C.c_uint64 * 4), ("invalidPixels", C.c_uint64), ("alphaAbovePixels", C.c_uint64),
                ("contradictions", C.c_uint64), ("drawnPrimitives", C.c_uint32), ("degeneratePrimitives", C.c_uint32)]


def bind(dll):
    dll.ommxRasterizeMicromap.argtypes = [C.c_void_p, C.POINTER(ot.BakeInputDesc), C.POINTER(ot.BakeResultDesc), C.POINTER(RasterDesc),
                                          C.POINTER(RasterOutputs), C.POINTER(RasterInfo), C.c_void_p]
    dll.ommxDebugSaveImagePNG.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    return dll


def c_desc(view=(0.0, 0.0, 1.0, 1.0), width=4, height=4, first=0, count=ALL, flags=0, reserved=(0, 0, 0, 0)):
    d = RasterDesc()
    d.uvMin[0], d.uvMin[1], d.uvMax[0], d.uvMax[1] = view
    d.width, d.height, d.firstPrimitive, d.primitiveCount, d.flags = width, height, first, count, flags
    for k in range(4):
        d.reserved[k] = reserved[k]
    return d


def info_dict(info):
    d = {f: getattr(info, f) for f in INFO_FIELDS}
    d["pixelsPerState"] = list(info.pixelsPerState)
    return d


# ---- a scene: everything a call reads, on the host ----
class Scene:
    """tex: mip 0 (2-D uint8 or float32); uv: float (n, 2) coordinates, encoded in `uv_format` (12-byte stride) unless raw / stride / offset / uv_read are
    given; ix: indices of any of the three widths; host: a HostResult"""

    def __init__(self, tex, uv, ix, host, uv_format=ot.UV32_FLOAT, addr=ot.CLAMP, filt=ot.NEAREST, border=0.0, cutoff=0.5, le=ot.T, gt=ot.O, raw=None,
                 stride=12, offset=0, uv_read=None):
        self.tex, self.ix, self.host = np.ascontiguousarray(tex), np.ascontiguousarray(ix), host
        self.uv_format, self.addr, self.filt, self.border, self.cutoff, self.le, self.gt = uv_format, addr, filt, border, cutoff, le, gt
        if raw is None:
            raw, uv_read = lu.uv_encoded(np.asarray(uv), uv_format)
        self.raw, self.stride, self.offset, self.uv_read = np.ascontiguousarray(raw).reshape(-1), stride, offset, np.asarray(uv_read, np.float32)

    @property
    def triangles(self):
        return self.ix.size // 3


class HostResult:
    """what the model reads of a result: an ommCpuBakeResultDesc over HOST arrays, the index entries and the descriptors' levels"""

    def __init__(self, desc, index, levels, keep=None):
        self.desc, self.index, self.levels, self._keep = desc, np.asarray(index, np.int64), np.asarray(levels, np.int64), keep

    @classmethod
    def of(cls, res):
        """of a lookup_util.Result"""
        return cls(res.desc, res.index, res.descs["l"], keep=res)

    @classmethod
    def of_arrays(cls, arrays, index_format):
        """of (arrayData, descArray bytes, index bytes) as lookup_util.DeviceBake.host_arrays holds them"""
        a, d, i = arrays
        idt = {ot.IDX_U8: np.int8, ot.IDX_U16: np.int16, ot.IDX_U32: np.int32}[index_format]
        index = np.ascontiguousarray(i).view(idt)
        desc = lu.result_desc_over((a, d, index), index_format)
        return cls(desc, index, np.ascontiguousarray(d).view(np.dtype([("o", "<u4"), ("l", "<u2"), ("f", "<u2")]))["l"], keep=(a, d, index))


def strided_fp32(uv, stride, offset):
    """FP32 coordinates at a byte offset and a stride that need not be multiples of 4 -> (raw bytes, the values read back)"""
    uv = np.ascontiguousarray(uv, np.float32)
    raw = np.zeros(offset + stride * len(uv) + 16, np.uint8)
    rows = np.lib.stride_tricks.as_strided(raw[offset:], (len(uv), 8), (stride, 1))
    rows[:] = uv.view(np.uint8).reshape(len(uv), 8)
    return raw, uv


# ---- the sampler: lookup_util's addressing; the Linear blend restated in fp32, which is what the kernel computes ----
def sample_alpha32(sc, tu, tv):
    """float32 alpha at float32 texture coordinates.  Nearest is lookup_util.sample_alpha (a texel: exact).  Linear takes lookup_util's texel addressing
    and fp32 weights and blends in fp32 in the sampler's written order -- lookup_util.sample_alpha blends in float64, which agrees with the kernel to
    1e-6 but not to the byte; tests/test_rasterize.py holds the two to each other."""
    tu, tv = np.asarray(tu, np.float32), np.asarray(tv, np.float32)
    if sc.filt == ot.NEAREST:
        return lu.sample_alpha(sc.tex, tu, tv, sc.addr, sc.filt, sc.border).astype(np.float32)
    h, w = sc.tex.shape
    p2 = lu.is_pow2(w, h)
    a = sc.tex if sc.tex.dtype == np.float32 else sc.tex.astype(np.float32) * np.float32(1.0 / 255.0)
    px, py = tu * np.float32(w) - np.float32(0.5), tv * np.float32(h) - np.float32(0.5)
    fx, fy = np.floor(px), np.floor(py)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0, y1 = lu._addr(sc.addr, ix, w, p2), lu._addr(sc.addr, ix + 1, w, p2), lu._addr(sc.addr, iy, h, p2), lu._addr(sc.addr, iy + 1, h, p2)
    t00, t01, t10, t11 = (lu._texel(a, x, y, sc.border) for x, y in ((x0, y0), (x0, y1), (x1, y0), (x1, y1)))
    wx, wy, one = (px - fx).astype(np.float32), (py - fy).astype(np.float32), np.float32(1.0)
    ac = t00 * (one - wx) + t10 * wx
    bd = t01 * (one - wx) + t11 * wx
    return (ac * (one - wy) + bd * wy).astype(np.float32)


# ---- the rule ----
def sample_points(view, width, height):
    lo, hi = np.asarray(view[:2], np.float32), np.asarray(view[2:], np.float32)
    step_u = (np.float64(hi[0]) - np.float64(lo[0])) / np.float64(width)
    step_v = (np.float64(hi[1]) - np.float64(lo[1])) / np.float64(height)
    U = np.float64(lo[0]) + (np.arange(width, dtype=np.float64) + 0.5) * step_u
    V = np.float64(lo[1]) + (np.arange(height, dtype=np.float64) + 0.5) * step_v
    return U, V


def primitive_range(sc, first, count):
    end = sc.triangles if count == ALL else min(first + count, sc.triangles)
    return range(first, max(end, first))


def triangles_of(sc):
    return sc.uv_read[sc.ix.astype(np.int64).reshape(-1, 3)].astype(np.float64)   # (n, 3, 2)


def edges(t, U, V):
    """wA, wB, wC, area2 in the written order; t: (..., 3, 2)"""
    ax, ay, bx, by, cx, cy = t[..., 0, 0], t[..., 0, 1], t[..., 1, 0], t[..., 1, 1], t[..., 2, 0], t[..., 2, 1]
    wa = (bx - U) * (cy - V) - (by - V) * (cx - U)
    wb = (cx - U) * (ay - V) - (cy - V) * (ax - U)
    wc = (ax - U) * (by - V) - (ay - V) * (bx - U)
    area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    return wa, wb, wc, area2


def _span(points, lo, hi):
    """the (ascending) sample points that can lie in [lo, hi], generously: three steps either side -> slice bounds"""
    step = points[1] - points[0] if len(points) > 1 else 0.0
    first, last = np.searchsorted(points, lo - 3 * step, "left"), np.searchsorted(points, hi + 3 * step, "right")
    return max(int(first) - 1, 0), min(int(last) + 1, len(points))


def owners(sc, view, width, height, first, count):
    """(owner map int64 (h, w), NONE where nobody covers; degenerate primitives of the range)"""
    U, V = sample_points(view, width, height)
    tris = triangles_of(sc)
    owner = np.full((height, width), NONE, np.int64)
    degenerate = 0
    with np.errstate(all="ignore"):
        for p in primitive_range(sc, first, count):
            t = tris[p]
            area2 = edges(t, 0.0, 0.0)[3]
            if area2 == 0 or not np.isfinite(area2):
                degenerate += 1
                continue
            x0, x1 = _span(U, t[:, 0].min(), t[:, 0].max())
            y0, y1 = _span(V, t[:, 1].min(), t[:, 1].max())
            if x0 >= x1 or y0 >= y1:
                continue
            wa, wb, wc, _ = edges(t, U[None, x0:x1], V[y0:y1, None])
            cov = (wa >= 0) & (wb >= 0) & (wc >= 0) if area2 > 0 else (wa <= 0) & (wb <= 0) & (wc <= 0)
            sub = owner[y0:y1, x0:x1]
            sub[cov & (sub == NONE)] = p
    return owner, degenerate


BIRD_DIGITS = np.array([(0x5020f008800f0205 >> (2 * k)) & 3 for k in range(32)], np.int64)   # OMMX_BIRD_DIGIT_TABLE, two bits per key


def micro_index(u, v, level):
    """ommx_micro_index restated: float32 (u, v) and a level per point -> index (int64)"""
    f32 = np.float32
    u, v, level = np.asarray(u, f32), np.asarray(v, f32), np.minimum(np.asarray(level, np.int64), 12)
    with np.errstate(invalid="ignore"):
        u = np.where(u > 0, np.where(u < 1, u, f32(1)), f32(0)).astype(f32)
        v = np.where(v > 0, np.where(v < 1, v, f32(1)), f32(0)).astype(f32)
    n = np.int64(1) << level
    fu, fv = u * n.astype(f32), v * n.astype(f32)
    iu, iv = np.minimum(fu.astype(np.int64), n - 1), np.minimum(fv.astype(np.int64), n - 1)
    edge = iu + iv >= n - 1
    over = iu + iv - (n - 1)
    du = np.minimum(over, iu)
    ru, rv = (fu - iu.astype(f32)).astype(f32), (fv - iv.astype(f32)).astype(f32)
    s = (ru + rv).astype(f32)
    bv = (s - ru).astype(f32)
    err = ((ru - (s - bv).astype(f32)).astype(f32) + (rv - bv).astype(f32)).astype(f32)
    upright = np.where(edge, True, (s < 1) | ((s == 1) & (err < 0)))
    iu, iv = np.where(edge, iu - du, iu), np.where(edge, iv - (over - du), iv)
    iw = np.where(upright, n - 1, n - 2) - iu - iv
    index, x, y = np.zeros(len(u), np.int64), np.zeros(len(u), np.int64), np.zeros(len(u), np.int64)
    for i in range(11, -1, -1):
        on = i < level
        key = x | (y << 1) | (((iu >> i) & 1) << 2) | (((iv >> i) & 1) << 3) | (((iw >> i) & 1) << 4)
        digit = BIRD_DIGITS[key]
        index = np.where(on, (index << 2) | digit, index)
        x, y = np.where(on, x ^ (digit & 1), x), np.where(on, y ^ (digit == 1), y)
    return index


def reuse_table(sc, first, count):
    """the lowest primitive of the range under every descriptor (NONE: nobody)"""
    host = sc.host
    lowest = np.full(max(int(host.desc.descArrayCount), 1), NONE, np.int64)
    for p in primitive_range(sc, first, count):
        if p < host.desc.indexCount:
            e = int(host.index[p])
            if 0 <= e < host.desc.descArrayCount:
                lowest[e] = min(lowest[e], p)
    return lowest


def shade(dll, sc, view, width, height, first, count, flags, owner, degenerate, u32, v32):
    """everything behind the owners and their barycentrics (float32, one per covered pixel in np.nonzero order): states through ommxLookupOpacityHost,
    micro-triangles, the alpha test, the picture and the info, in integers"""
    host = sc.host
    U, V = sample_points(view, width, height)
    ys, xs = np.nonzero(owner != NONE)
    o = owner[ys, xs]
    hits = np.empty(len(o), lu.HIT)
    hits["prim"], hits["u"], hits["v"] = o, u32, v32
    st = lu.lookup_host(dll, host.desc, hits).astype(np.int64) if len(o) else np.zeros(0, np.int64)
    valid = st != STATE_INVALID
    entry = np.full(len(o), -1, np.int64)
    entry[valid] = host.index[o[valid]]                                               # (a valid state: the primitive is below indexCount)
    block = valid & (entry >= 0)
    level = np.where(block, host.levels[np.where(block, entry, 0)] if len(host.levels) else 0, 0)
    micro = np.where(valid, 0, NONE).astype(np.int64)
    if block.any():
        micro[block] = micro_index(u32[block], v32[block], level[block])
    inverted = np.zeros(len(o), bool)
    if block.any():
        inverted[block] = ~lu.micro_cells(micro[block].astype(np.uint32), level[block].astype(np.uint32))[2]
        vt = lu.micro_vertices(micro[block].astype(np.uint32), level[block].astype(np.uint32))
        assert np.array_equal(inverted[block], vt[:, 1, 0] < vt[:, 0, 0])          # d < 0 in ommx_micro_vertices
    reused = np.zeros(len(o), bool)
    if flags & HIGHLIGHT_REUSE and block.any():
        lowest = reuse_table(sc, first, count)
        reused[block] = lowest[entry[block]] < o[block]
    # the alpha test of every pixel
    uu, vv = np.meshgrid(U.astype(np.float32), V.astype(np.float32))
    alpha = sample_alpha32(sc, uu.reshape(-1), vv.reshape(-1)).reshape(height, width)
    with np.errstate(invalid="ignore"):
        above = np.float32(sc.cutoff) < alpha
        a = np.where(alpha > 0, np.where(alpha < 1, alpha, np.float32(1)), np.float32(0)).astype(np.float32)
    g = (a * np.float32(255.0) + np.float32(0.5)).astype(np.float32).astype(np.int64)
    c = np.where(above[ys, xs], sc.gt, sc.le)
    contradiction = (st < 2) & ((c & 1) != st)
    out = dict(primitiveIds=np.where(owner == NONE, NONE, owner).astype(np.uint32), microTriangles=np.full((height, width), NONE, np.uint32),
               states=np.full((height, width), STATE_NONE, np.uint8), alphaTest=above.astype(np.uint8))
    out["microTriangles"][ys, xs] = micro
    out["states"][ys, xs] = st
    rgba = np.stack([g, g, g, np.full_like(g, 255)], -1)
    lut = np.array([LUT[0], LUT[1], LUT[3] if flags & MONOCHROME_UNKNOWNS else LUT[2], LUT[3], LUT[STATE_INVALID]], np.int64)
    px = (lut[np.where(valid, st, 4)] + g[ys, xs][:, None] + 1) >> 1
    px = np.where(inverted[:, None], px - (px >> 3), px)
    px = np.where(reused[:, None], px >> 1, px)
    rgba[ys, xs, :3] = px
    if not flags & NO_CONTOUR:
        edge = np.zeros((height, width), bool)
        edge[:, :-1] |= above[:, :-1] != above[:, 1:]
        edge[:-1, :] |= above[:-1, :] != above[1:, :]
        rgba[edge] = CONTOUR
    out["rgba"] = rgba.astype(np.uint8)
    out["info"] = dict(coveredPixels=len(o), pixelsPerState=[int((st == s).sum()) for s in range(4)], invalidPixels=int((~valid).sum()),
                       alphaAbovePixels=int(above.sum()), contradictions=int(contradiction.sum()), drawnPrimitives=len(set(o.tolist())),
                       degeneratePrimitives=degenerate)
    return out


def model(dll, sc, view, width, height, first=0, count=ALL, flags=0):
    """the vectorised model: every output as the call writes it, and the info"""
    owner, degenerate = owners(sc, view, width, height, first, count)
    U, V = sample_points(view, width, height)
    ys, xs = np.nonzero(owner != NONE)
    with np.errstate(all="ignore"):
        wa, wb, wc, area2 = edges(triangles_of(sc)[owner[ys, xs]], U[xs], V[ys])
        u32, v32 = (wb / area2).astype(np.float32), (wc / area2).astype(np.float32)
    return shade(dll, sc, view, width, height, first, count, flags, owner, degenerate, u32, v32)


def brute(dll, sc, view, width, height, first=0, count=ALL, flags=0):
    """the same rule as loops over pixels and primitives in Python floats, without any box: owners and barycentrics; the rest is shade()"""
    lo, hi = [float(np.float32(x)) for x in view[:2]], [float(np.float32(x)) for x in view[2:]]
    step_u, step_v = (hi[0] - lo[0]) / float(width), (hi[1] - lo[1]) / float(height)
    tris = [[float(x) for x in t.reshape(-1)] for t in triangles_of(sc)]
    inf = float("inf")
    owner = np.full((height, width), NONE, np.int64)
    u32, v32, degenerate = [], [], 0
    for p in primitive_range(sc, first, count):
        ax, ay, bx, by, cx, cy = tris[p]
        area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        degenerate += area2 == 0 or area2 != area2 or abs(area2) == inf
    for y in range(height):
        V = lo[1] + (float(y) + 0.5) * step_v
        for x in range(width):
            U = lo[0] + (float(x) + 0.5) * step_u
            for p in primitive_range(sc, first, count):
                ax, ay, bx, by, cx, cy = tris[p]
                area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
                if area2 == 0 or area2 != area2 or abs(area2) == inf:
                    continue
                wa = (bx - U) * (cy - V) - (by - V) * (cx - U)
                wb = (cx - U) * (ay - V) - (cy - V) * (ax - U)
                wc = (ax - U) * (by - V) - (ay - V) * (bx - U)
                if (wa >= 0 and wb >= 0 and wc >= 0) if area2 > 0 else (wa <= 0 and wb <= 0 and wc <= 0):
                    owner[y, x] = p
                    u32.append(np.float32(wb / area2))
                    v32.append(np.float32(wc / area2))
                    break
    return shade(dll, sc, view, width, height, first, count, flags, owner, int(degenerate), np.array(u32, np.float32), np.array(v32, np.float32))


# ---- the device side ----
class DeviceScene:
    """a Scene on the device: the texture, the mesh and the result's arrays, and the two descs a call takes"""

    def __init__(self, lib, hip, baker, sc, result_arrays=None):
        self.lib, self.hip, self.baker, self.sc = lib, hip, baker, sc
        self.tex = lib.create_texture(baker, [sc.tex])
        self.bufs = [hip.upload(sc.raw), hip.upload(sc.ix)]
        d = ot.make_desc(self.tex, sc.uv_read, sc.ix, 4, alpha_cutoff=sc.cutoff, addr=sc.addr, filt=sc.filt, le=sc.le, gt=sc.gt, uv_format=sc.uv_format,
                         border_alpha=sc.border)
        d.texCoords, d.indexBuffer, d.texCoordStrideInBytes = self.bufs[0].value + sc.offset, self.bufs[1], sc.stride
        self.ddesc = d
        h = sc.host.desc
        isz = {ot.IDX_U8: 1, ot.IDX_U16: 2, ot.IDX_U32: 4}.get(h.indexFormat, 4)
        self.sources = [np.ctypeslib.as_array(C.cast(h.arrayData, C.POINTER(C.c_uint8)), (h.arrayDataSize,)).copy() if h.arrayDataSize else np.zeros(0, np.uint8),
                        np.ctypeslib.as_array(C.cast(h.descArray, C.POINTER(C.c_uint8)), (8 * h.descArrayCount,)).copy() if h.descArrayCount else np.zeros(0, np.uint8),
                        np.ctypeslib.as_array(C.cast(h.indexBuffer, C.POINTER(C.c_uint8)), (isz * len(sc.host.index),)).copy() if len(sc.host.index) else np.zeros(0, np.uint8)]
        self.rbufs = [hip.upload(s) for s in self.sources]
        r = ot.BakeResultDesc.from_buffer_copy(h)
        r.arrayData, r.descArray, r.indexBuffer = self.rbufs[0], C.cast(self.rbufs[1], C.POINTER(ot.MicromapDesc)), self.rbufs[2]
        self.rdesc = r

    def sources_unchanged(self):
        got = [self.hip.download(p, s.nbytes) for p, s in zip(self.rbufs, self.sources)] + [self.hip.download(self.bufs[0], self.sc.raw.nbytes)]
        return all(np.array_equal(g, s) for g, s in zip(got, self.sources + [self.sc.raw.view(np.uint8)]))

    def close(self):
        for p in self.bufs + self.rbufs:
            self.hip.free(p)
        self.bufs = self.rbufs = []
        if self.tex:
            self.lib.destroy_texture(self.baker, self.tex)
            self.tex = None


GUARD = 64


def rasterize(dll, hip, dev, view, width, height, first=0, count=ALL, flags=0, want=OUTPUTS, want_info=True, stream=None, ddesc=None, rdesc=None):
    """one call: the outputs in `want` are handed in, each pre-filled with FILL and followed by GUARD bytes that must come back untouched; the buffers
    of the other outputs exist too and must keep their fill -> dict of the outputs that were asked for (shaped) and the info"""
    pixels = width * height
    bufs = {name: hip.upload(np.full(pixels * OUT_BYTES[name] + GUARD, FILL, np.uint8)) for name in OUTPUTS}
    try:
        o = RasterOutputs(*[bufs[name] if name in want else None for name in OUTPUTS])
        info = RasterInfo()
        d = c_desc(view, width, height, first, count, flags)
        r = dll.ommxRasterizeMicromap(dev.baker, C.byref(ddesc if ddesc is not None else dev.ddesc), C.byref(rdesc if rdesc is not None else dev.rdesc),
                                      C.byref(d), C.byref(o) if want else None, C.byref(info) if want_info else None, stream)
        assert r == ot.SUCCESS, r
        out = {}
        for name in OUTPUTS:
            raw = hip.download(bufs[name], pixels * OUT_BYTES[name] + GUARD)
            if name not in want:
                assert (raw == FILL).all(), "%s was written although it was not handed in" % name
                continue
            assert (raw[pixels * OUT_BYTES[name]:] == FILL).all(), "bytes behind %s were written" % name
            a = raw[:pixels * OUT_BYTES[name]].view(OUT_DTYPE[name])
            out[name] = a.reshape(height, width, 4) if name == "rgba" else a.reshape(height, width)
        if want_info:
            out["info"] = info_dict(info)
        return out
    finally:
        for p in bufs.values():
            hip.free(p)


def same(got, ref, names=OUTPUTS + ("info",)):
    """byte for byte; the first difference in words"""
    for name in names:
        if name == "info":
            assert got["info"] == ref["info"], (got["info"], ref["info"])
            continue
        if not np.array_equal(got[name], ref[name]):
            where = np.argwhere(got[name] != ref[name])
            at = tuple(where[0])
            raise AssertionError("%s differs at %d places, first at %r: got %r, model %r" % (name, len(where), at, got[name][at], ref[name][at]))
    return True


def check(dll, hip, dev, view, width, height, first=0, count=ALL, flags=0):
    """the call with every output against the model -> the model's answer"""
    ref = model(dll, dev.sc, view, width, height, first, count, flags)
    same(rasterize(dll, hip, dev, view, width, height, first, count, flags), ref)
    return ref
