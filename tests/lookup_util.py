"""Shared by tests/test_lookup.py, tests/test_lookup_gpu.py and tests/scripts/lookup_throughput.py: device-resident bakes that stay alive for the
lookup entry points (ommxLookupOpacity, ommxResolveHits), hand-built results (the bounds-rule table, the digit result), a numpy restatement of
the bird-curve decode, the micro-triangles whose closure holds a point, and a numpy sampler of mip 0 (the resolve kernel's sampler)."""
import ctypes as C
import functools
import numpy as np
import ommtest as ot

HIT = np.dtype([("prim", "<u4"), ("u", "<f4"), ("v", "<f4")])
FORCE_2STATE, IGNORE_MICROMAP = 1, 2
INVALID = 0xFF


def bind(dll):
    dll.ommxLookupOpacityHost.argtypes = [C.POINTER(ot.BakeResultDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    dll.ommxLookupOpacity.argtypes = [C.POINTER(ot.BakeResultDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    dll.ommxResolveHits.argtypes = [C.c_void_p, C.POINTER(ot.BakeInputDesc), C.POINTER(ot.BakeResultDesc), C.c_void_p, C.c_uint32, C.c_void_p,
                                    C.c_uint32, C.c_void_p]
    dll.ommxBakeDevice.argtypes = [C.c_void_p, C.POINTER(ot.BakeInputDesc), C.POINTER(C.c_void_p)]
    dll.ommxGetDeviceBakeResultDesc.argtypes = [C.c_void_p, C.POINTER(C.POINTER(ot.BakeResultDesc))]
    dll.ommxDestroyDeviceBakeResult.argtypes = [C.c_void_p]
    return dll


class DeviceBake:
    """ommxBakeDevice of `desc` whose result (and uploaded inputs) stay alive: .ddesc is the device-resident input desc, .rdesc the result desc
    (device arrays), .host a host copy (ommtest.BakeResult) and .hdesc an ommCpuBakeResultDesc over that copy"""

    def __init__(self, lib, hip, baker, desc, uv, ix, levels=None, uv_offset=0):
        self.lib, self.hip = lib, hip
        self.bufs = [hip.upload(uv), hip.upload(ix)]
        self.ddesc = ot.BakeInputDesc.from_buffer_copy(desc)
        self.ddesc.texCoords, self.ddesc.indexBuffer = self.bufs[0].value + uv_offset, self.bufs[1]   # uv_offset: first coordinate's byte in `uv`
        self.ddesc.subdivisionLevels = None
        if levels is not None:
            self.bufs.append(hip.upload(np.ascontiguousarray(levels, dtype=np.uint8)))
            self.ddesc.subdivisionLevels = self.bufs[-1]
        self.out = C.c_void_p()
        r = lib.dll.ommxBakeDevice(baker, C.byref(self.ddesc), C.byref(self.out))
        assert r == ot.SUCCESS, r
        pd = C.POINTER(ot.BakeResultDesc)()
        assert lib.dll.ommxGetDeviceBakeResultDesc(self.out, C.byref(pd)) == ot.SUCCESS
        self.rdesc = pd.contents
        dev = self.rdesc
        isz = {ot.IDX_U8: 1, ot.IDX_U16: 2, ot.IDX_U32: 4}[dev.indexFormat]
        self.host_arrays = [hip.download(dev.arrayData, dev.arrayDataSize), hip.download(dev.descArray, 8 * dev.descArrayCount),
                            hip.download(dev.indexBuffer, isz * dev.indexCount)]
        self.hdesc = ot.BakeResultDesc.from_buffer_copy(dev)
        self.hdesc.arrayData = self.host_arrays[0].ctypes.data
        self.hdesc.descArray = C.cast(self.host_arrays[1].ctypes.data, C.POINTER(ot.MicromapDesc))
        self.hdesc.indexBuffer = self.host_arrays[2].ctypes.data
        self.host = ot.BakeResult(self.hdesc)

    def close(self):
        if self.out:
            assert self.lib.dll.ommxDestroyDeviceBakeResult(self.out) == ot.SUCCESS
            self.out = None
        for p in self.bufs:
            self.hip.free(p)
        self.bufs = []


def result_desc_over(arrays, index_format):
    """ommCpuBakeResultDesc over host numpy arrays (array data, descs as uint8 bytes, index) -- e.g. an ommCpuBake result's host copy"""
    a, d, i = arrays
    r = ot.BakeResultDesc()
    r.arrayData, r.arrayDataSize = a.ctypes.data, a.size
    r.descArray, r.descArrayCount = C.cast(d.ctypes.data, C.POINTER(ot.MicromapDesc)), d.size // 8
    r.indexBuffer, r.indexCount, r.indexFormat = i.ctypes.data, i.size, index_format
    r._keep = arrays   # the desc points into these arrays: they live as long as it does
    return r


def host_arrays_of(res):
    """(arrayData, descArray bytes, index) of an ommtest.BakeResult as contiguous numpy arrays"""
    return (np.ascontiguousarray(res.array_data), np.frombuffer(res.desc_bytes, np.uint8).copy() if res.desc_bytes else np.zeros(8, np.uint8),
            np.ascontiguousarray(res.index))


def lookup_host(dll, rdesc, hits, flags=0):
    out = np.full(len(hits), 0xAB, np.uint8)
    assert dll.ommxLookupOpacityHost(C.byref(rdesc), hits.ctypes.data, len(hits), out.ctypes.data, flags) == ot.SUCCESS
    return out


def sync(hip):
    assert hip.rt.hipDeviceSynchronize() == 0


def lookup_device(dll, hip, rdesc, hits, flags=0):
    d_hits, d_out = hip.upload(hits), hip.alloc(len(hits))
    try:
        assert dll.ommxLookupOpacity(C.byref(rdesc), d_hits, len(hits), d_out, flags, None) == ot.SUCCESS
        sync(hip)
        return hip.download(d_out, len(hits))
    finally:
        hip.free(d_hits)
        hip.free(d_out)


def resolve_device(dll, hip, baker, ddesc, rdesc, hits, flags=0):
    d_hits, d_out = hip.upload(hits), hip.alloc(len(hits))
    try:
        r = dll.ommxResolveHits(baker, C.byref(ddesc), C.byref(rdesc), d_hits, len(hits), d_out, flags, None)
        assert r == ot.SUCCESS, r
        sync(hip)
        return hip.download(d_out, len(hits))
    finally:
        hip.free(d_hits)
        hip.free(d_out)


CANARY = 64


def guarded_call(hip, hits, call, stream=None):
    """`call(d_hits, d_out, count, stream)` with `out` in the middle of a buffer pre-filled with 0xAB: CANARY bytes before and after the `count`
    answer bytes must come back untouched.  With a stream, only that stream is synchronised.  Returns the answer bytes."""
    n = len(hits)
    d_hits, d_buf = hip.upload(hits), hip.upload(np.full(n + 2 * CANARY, 0xAB, np.uint8))
    try:
        assert call(d_hits, C.c_void_p(d_buf.value + CANARY), n, stream) == ot.SUCCESS
        if stream is None:
            sync(hip)
        else:
            hip.stream_sync(stream)
        buf = hip.download(d_buf, n + 2 * CANARY)
        assert (buf[:CANARY] == 0xAB).all() and (buf[CANARY + n:] == 0xAB).all(), "bytes outside out[0, count) were written"
        return buf[CANARY:CANARY + n].copy()
    finally:
        hip.free(d_hits)
        hip.free(d_buf)


# ---- bird curve (the forward decode of omm_amd/csrc/classify_device.h), vectorised ----
def _even_bits(x):
    x = x & np.uint32(0x55555555)
    for s, m in ((1, 0x33333333), (2, 0x0f0f0f0f), (4, 0x00ff00ff), (8, 0x0000ffff)):
        x = (x | (x >> np.uint32(s))) & np.uint32(m)
    return x


def _pxor(x):
    for s in (1, 2, 4, 8):
        x = x ^ (x >> np.uint32(s))
    return x


def micro_cells(index, level):
    """the forward decode's integers: (iu, iv, upright) of micro-triangles `index` at `level` -- the grid cell (iu, iv) and which half of it"""
    index = np.asarray(index, np.uint32)
    level = np.asarray(level, np.uint32) * np.ones_like(index)
    b0, b1 = _even_bits(index), _even_bits(index >> np.uint32(1))
    fx, fy = _pxor(b0), _pxor(b0 & ~b1)
    t = fy ^ b1
    m = (np.uint32(1) << level) - np.uint32(1)
    iu = ((fx & ~t) | (b0 & ~t) | (~b0 & ~fx & t)) & m
    iv = (fy ^ b0) & m
    iw = ((~fx & ~t) | (b0 & ~t) | (~b0 & fx & t)) & m
    up = ((iu ^ iv ^ iw) & np.uint32(1)) != 0
    up |= level == 0
    return iu, iv, up


def micro_vertices(index, level):
    """(n, 3, 2) float64 barycentric (u, v) vertices of micro-triangles `index` at `level` (arrays of equal length)"""
    index = np.asarray(index, np.uint32)
    level = np.asarray(level, np.uint32) * np.ones_like(index)
    iu, iv, up = micro_cells(index, level)
    iu = iu.astype(np.float64) + np.where(up, 0, 1)
    iv = iv.astype(np.float64) + np.where(up, 0, 1)
    d = np.where(up, 1.0, -1.0)
    s = 1.0 / (2.0 ** level.astype(np.float64))
    v = np.empty((len(index), 3, 2))
    v[:, 0] = np.stack([iu * s, iv * s], 1)
    v[:, 1] = np.stack([(iu + d) * s, iv * s], 1)
    v[:, 2] = np.stack([iu * s, (iv + d) * s], 1)
    return v


def interior_points(rng, verts, lo=0.05):
    """a random point strictly inside each micro-triangle (every barycentric weight >= lo / (1 + 3 lo))"""
    w = rng.random((len(verts), 3)) + lo
    w /= w.sum(axis=1, keepdims=True)
    p = (w[:, :, None] * verts).sum(axis=1)
    return p[:, 0].astype(np.float32), p[:, 1].astype(np.float32)


def centroid_points(verts):
    c = verts.mean(axis=1)
    return c[:, 0].astype(np.float32), c[:, 1].astype(np.float32)


def prim_levels(res):
    """per primitive: the subdivision level of its OMM (0 for special indices) and whether it has one"""
    e = res.index.astype(np.int64)
    has = e >= 0
    lv = np.zeros(len(e), np.int64)
    if res.descs.size:
        lv[has] = res.descs[e[has], 1]
    return lv, has


def numpy_states(res, prims, micro):
    """the state a host result stores for micro-triangle `micro` of primitive `prims` (special indices: -(e+1))"""
    e = res.index.astype(np.int64)[prims]
    out = np.where(e < 0, -(e + 1), 0).astype(np.int64)
    k = e >= 0
    if k.any():
        d = res.descs[e[k]]
        bits = d[:, 2]
        bit = micro[k].astype(np.int64) * bits
        byte = res.array_data[d[:, 0] + (bit >> 3)].astype(np.int64)
        out[k] = (byte >> (bit & 7)) & ((1 << bits) - 1)
    return out


# ---- numpy restatement of the resolve kernel's sampler (mip 0; classify_device.h tex_coord / bilinear), any texture size ----
def is_pow2(w, h):
    """the texture-wide flag the kernels dispatch on: both sides are powers of two"""
    return (w & (w - 1)) == 0 and (h & (h - 1)) == 0


def _addr(mode, x, size, pow2):
    """texel coordinate `x` (int64 array, |x| < 2^23) addressed on an axis of `size` texels; -1 = the border sentinel.  `pow2` is the
    texture-wide flag, not the axis's own.  Equal to the oracle's orc_get_tex_coord (tests/test_lookup.py), which is pinned to the reference's tables."""
    if mode == ot.WRAP:
        return x & (size - 1) if pow2 else (x & 0xFFFFFFFF) % size   # (not a power of two: the remainder of the coordinate read as unsigned 32-bit)
    if mode == ot.MIRROR:
        xa = np.abs(x) - (x < 0)
        flipped = (xa // size) & 1
        w = xa & (size - 1) if pow2 else xa % size
        return np.where(flipped == 1, size - w - 1, w)
    if mode == ot.CLAMP:
        return np.clip(x, 0, size - 1)
    if mode == ot.BORDER:
        return np.where((x >= size) | (x < 0), -1, x)
    if mode == ot.MIRROR_ONCE:
        return np.clip(np.where(x >= 0, x, -x - 1), 0, size - 1)
    raise ValueError(mode)


def _texel(a, x, y, border):
    out = np.full(x.shape, np.float32(border), np.float32)
    ok = (x >= 0) & (y >= 0)
    out[ok] = a[y[ok], x[ok]]
    return out


def sample_alpha(tex, tu, tv, addr, filt, border=0.0):
    """alpha of `tex` (mip 0: a 2-D uint8 or float32 array of any size) at texture coordinates (tu, tv).  The texel coordinate and the filter
    weights are the kernel's fp32 values -- they define which texels are read, and coordinates reach thousands of texels -- the blend is float64."""
    h, w = tex.shape
    p2 = is_pow2(w, h)
    a = tex if tex.dtype == np.float32 else tex.astype(np.float32) * np.float32(1.0 / 255.0)
    tu, tv = tu.astype(np.float32), tv.astype(np.float32)
    if filt == ot.NEAREST:
        x = _addr(addr, np.floor(tu * np.float32(w)).astype(np.int64), w, p2)
        y = _addr(addr, np.floor(tv * np.float32(h)).astype(np.int64), h, p2)
        return _texel(a, x, y, border).astype(np.float64)
    px, py = tu * np.float32(w) - np.float32(0.5), tv * np.float32(h) - np.float32(0.5)
    fx, fy = np.floor(px), np.floor(py)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0, y1 = _addr(addr, ix, w, p2), _addr(addr, ix + 1, w, p2), _addr(addr, iy, h, p2), _addr(addr, iy + 1, h, p2)
    t00, t01, t10, t11 = (_texel(a, x, y, border).astype(np.float64) for x, y in ((x0, y0), (x0, y1), (x1, y0), (x1, y1)))
    wx, wy = (px - fx).astype(np.float32).astype(np.float64), (py - fy).astype(np.float32).astype(np.float64)
    return (t00 * (1.0 - wx) + t10 * wx) * (1.0 - wy) + (t01 * (1.0 - wx) + t11 * wx) * wy


def hit_tex_coords(uv, ix, prims, u, v):
    """texture coordinate of each hit, interpolated with weights (1-u-v, u, v) in fp32 as the kernel does (uv: float32 (n, 2))"""
    tri = ix.reshape(-1, 3)[prims]
    p0, p1, p2 = uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]]
    u, v = u.astype(np.float32), v.astype(np.float32)
    bx = (np.float32(1.0) - u - v).astype(np.float32)
    tu = p0[:, 0] * bx + p1[:, 0] * u + p2[:, 0] * v
    tv = p0[:, 1] * bx + p1[:, 1] * u + p2[:, 1] * v
    return tu.astype(np.float32), tv.astype(np.float32)


# ---- the micro-triangles whose closure holds a point: from the forward decode alone (micro_cells / micro_vertices), in float64 ----
@functools.lru_cache(maxsize=1)
def cell_table(level):
    """tab[upright, iv, iu] = the index whose forward decode is that half of grid cell (iu, iv) at `level`, -1 where there is none"""
    n = 1 << level
    tab = np.full((2, n, n), -1, np.int32)
    step = 1 << 22
    for lo in range(0, 4 ** level, step):
        idx = np.arange(lo, min(lo + step, 4 ** level), dtype=np.uint32)
        iu, iv, up = micro_cells(idx, level)
        tab[up.astype(np.intp), iv.astype(np.intp), iu.astype(np.intp)] = idx.astype(np.int32)
    assert (tab >= 0).sum() == 4 ** level   # the decode visits every half cell of the triangle once
    return tab


def closure_holders(level, u, v):
    """for float32 points (u, v): cand (k, 18) = the indices of the micro-triangles in the 3 x 3 grid cells around each point (-1: none) and
    holds (k, 18) = whether the closure of that micro-triangle, as micro_vertices gives it, contains the point.  The table only proposes
    candidates; containment is decided on the decoded vertices.  All quantities are dyadic, so the float64 arithmetic is exact."""
    n = 1 << level
    tab = cell_table(level)
    pu, pv = np.asarray(u, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
    cx, cy = np.floor(pu * n).astype(np.int64), np.floor(pv * n).astype(np.int64)
    cand = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            x, y = cx + dx, cy + dy
            for up in (1, 0):
                exists = (x >= 0) & (y >= 0) & (x + y <= (n - 1 if up else n - 2))
                cand.append(np.where(exists, tab[up, np.clip(y, 0, n - 1), np.clip(x, 0, n - 1)], -1))
    cand = np.stack(cand, 1).astype(np.int64)
    k = len(pu)
    verts = micro_vertices(np.maximum(cand, 0).reshape(-1), np.full(cand.size, level)).reshape(k, 18, 3, 2)
    p = np.stack([pu, pv], 1)[:, None, :]

    def cross(a, b, c):
        return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])
    a, b, c = verts[:, :, 0], verts[:, :, 1], verts[:, :, 2]
    s = np.sign(cross(a, b, c))
    holds = (s * cross(a, b, p) >= 0) & (s * cross(b, c, p) >= 0) & (s * cross(c, a, p) >= 0) & (cand >= 0)
    return cand, holds


def edge_and_vertex_points(index, level):
    """per micro-triangle: its three vertices, its three edge midpoints (all exact in fp32), and the midpoint of its edge on the cell diagonal
    moved one ulp of u to either side -> float32 (u, v), 8 points per micro-triangle"""
    vt = micro_vertices(index, np.full(len(index), level))
    mids = (vt + np.roll(vt, -1, axis=1)) * 0.5
    exact = np.concatenate([vt.reshape(-1, 2), mids.reshape(-1, 2)])
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
    du, dv = mids[:, 1, 0].astype(np.float32), mids[:, 1, 1].astype(np.float32)   # vertices 1 and 2 span the diagonal of the cell
    u = np.concatenate([exact[:, 0].astype(np.float32), np.nextafter(du, np.float32(2)), np.nextafter(du, np.float32(-1))])
    v = np.concatenate([exact[:, 1].astype(np.float32), dv, dv])
    return u, v


def edge_level_sample(rng, level, cap=1 << 14):
    """every micro-triangle of `level`, or `cap` random ones where there are more"""
    n = 4 ** level
    return np.arange(n, dtype=np.int64) if n <= cap else rng.choice(n, cap, replace=False).astype(np.int64)


def check_index_is_a_holder(level, u, v, idx):
    """`idx`: the index a lookup chose for each point.  Wherever the point lies in the closure of the triangle, idx must be one of the
    micro-triangles whose closure holds it; the points it does not (an ulp beyond the edge u + v = 1) are returned as a count."""
    cand, holds = closure_holders(level, u, v)
    pu, pv = u.astype(np.float64), v.astype(np.float64)
    inside = (pu >= 0) & (pv >= 0) & (pu + pv <= 1.0)   # (the sum of two floats of this size is exact in float64)
    assert (holds.any(axis=1) == inside).all()
    ok = (holds & (cand == idx.astype(np.int64)[:, None])).any(axis=1)
    bad = inside & ~ok
    assert not bad.any(), "level %d: %d points read a micro-triangle that does not hold them, e.g. (%r, %r) -> %d, holders %r" % (
        level, int(bad.sum()), u[bad][0], v[bad][0], idx[bad][0], cand[bad][0][holds[bad][0]])
    return int((~inside).sum())


# ---- hand-built results ----
class Result:
    """an ommCpuBakeResultDesc over numpy arrays (kept alive by the object)"""

    def __init__(self, array_data, descs, index, index_format):
        self.array = np.ascontiguousarray(array_data, np.uint8)
        self.descs = np.ascontiguousarray(np.array(descs, dtype=[("o", "<u4"), ("l", "<u2"), ("f", "<u2")]).reshape(-1))
        idt = {ot.IDX_U8: np.int8, ot.IDX_U16: np.int16, ot.IDX_U32: np.int32}.get(index_format, np.int32)
        self.index = np.ascontiguousarray(np.array(index, dtype=np.int64).astype(idt))
        d = ot.BakeResultDesc()
        d.arrayData, d.arrayDataSize = self.array.ctypes.data, self.array.size
        d.descArray, d.descArrayCount = C.cast(self.descs.ctypes.data, C.POINTER(ot.MicromapDesc)), self.descs.size
        d.indexBuffer, d.indexCount, d.indexFormat = self.index.ctypes.data, self.index.size, index_format
        self.desc = d


def pack(states, bits):
    """micro-triangle states -> block bytes: state i at bit i (2-state) / bits 2i..2i+1 (4-state), little-endian within bytes"""
    s = np.asarray(states, np.uint8)
    per = 8 // bits
    s = np.concatenate([s, np.zeros((-len(s)) % per, np.uint8)]).reshape(-1, per)
    out = np.zeros(len(s), np.uint8)
    for k in range(per):
        out |= s[:, k] << np.uint8(bits * k)
    return out


def unpack(block, i, bits):
    return (block[(i * bits) >> 3] >> ((i * bits) & 7)) & ((1 << bits) - 1)


@functools.lru_cache(maxsize=2)
def digit_result(level):
    """one 4-state block per base-4 digit of the index: in block p micro-triangle i stores (i >> 2p) & 3, so the states a point reads in
    primitives 0..level-1 spell the index the lookup chose"""
    n = 4 ** level
    i = np.arange(n, dtype=np.uint32)
    blocks = [pack(((i >> np.uint32(2 * p)) & np.uint32(3)).astype(np.uint8), 2) for p in range(max(level, 1))]
    size = len(blocks[0])
    return Result(np.concatenate(blocks), [(p * size, level, 2) for p in range(len(blocks))], list(range(len(blocks))), ot.IDX_U32)


def digit_hits(level, u, v):
    """the hits that read every digit of the index at the points (u, v): primitive p for digit p"""
    k, digits = len(u), max(level, 1)
    h = np.empty(k * digits, HIT)
    h["prim"], h["u"], h["v"] = np.repeat(np.arange(digits, dtype=np.uint32), k), np.tile(u, digits), np.tile(v, digits)
    return h


def digits_to_index(level, states, k):
    """the index the states of digit_hits spell (every state must be a state, not INVALID)"""
    assert (states < 4).all()
    s = states.reshape(max(level, 1), k).astype(np.uint32)
    idx = np.zeros(k, np.uint32)
    for p in range(len(s)):
        idx |= s[p] << np.uint32(2 * p)
    return idx


class DeviceResult:
    """device copies of a result's three arrays and a caller-filled desc over them (the documented use of a host result on the device)"""

    def __init__(self, hip, array, desc_bytes, index, index_format):
        self.hip = hip
        self.bufs = [hip.upload(np.ascontiguousarray(array)), hip.upload(np.ascontiguousarray(desc_bytes)), hip.upload(np.ascontiguousarray(index))]
        r = ot.BakeResultDesc()
        r.arrayData, r.arrayDataSize = self.bufs[0], array.size
        r.descArray, r.descArrayCount = C.cast(self.bufs[1], C.POINTER(ot.MicromapDesc)), desc_bytes.nbytes // 8
        r.indexBuffer, r.indexCount, r.indexFormat = self.bufs[2], index.size, index_format
        self.rdesc = r

    def close(self):
        for p in self.bufs:
            self.hip.free(p)
        self.bufs = []


# ---- the bounds rule: one hand-built table for the host and the device ----
BOUNDS_MICRO = 37   # every hit of the table is the centroid of this micro-triangle of level 3


def bounds_hit():
    u, v = centroid_points(micro_vertices(np.array([BOUNDS_MICRO]), np.array([3])))
    return u[0], v[0]


def bounds_table(index_format):
    """A 16-byte array (one level-3 4-state block), eight descs and index entries of `index_format` that exercise every clause of the bounds
    rule.  rows: (index entry, expected answer at bounds_hit(), near) -- `near` is False where a kernel without the check would form an
    address far outside any allocation (those rows stay on the host).  beyond: (primitive, near) past indexCount."""
    lvl3 = pack(np.arange(64) % 4, 2)
    descs = [(0, 3, 2),     # 0: the block that fills the array exactly
             (0, 13, 2),    # 1: level 13
             (0, 2, 0),     # 2: format INVALID (0)
             (0, 2, 3),     # 3: format MAX_NUM (3)
             (1, 3, 2),     # 4: 16-byte block at offset 1: ends 1 byte past arrayDataSize
             (8, 3, 1),     # 5: 8-byte 2-state block at 8: ends exactly at arrayDataSize
             (9, 3, 1),     # 6: ... at 9: ends 1 byte past it
             (16, 0, 1)]    # 7: level-0 block at offset == arrayDataSize
    s0, s5 = int(unpack(lvl3, BOUNDS_MICRO, 2)), int(unpack(lvl3[8:], BOUNDS_MICRO, 1))
    inv = INVALID
    rows = [(0, s0, True), (1, inv, True), (2, inv, True), (3, inv, True), (4, inv, True), (5, s5, True), (6, inv, True), (7, inv, True),
            (8, inv, True), (9, inv, True), (11, inv, True),                                  # entries >= descArrayCount (8)
            (-1, 0, True), (-2, 1, True), (-3, 2, True), (-4, 3, True), (0, s0, True)]        # special indices; a valid entry last
    top = {ot.IDX_U8: 127, ot.IDX_U16: 32767, ot.IDX_U32: 0x7FFFFFFF}[index_format]
    rows.append((top, inv, index_format != ot.IDX_U32))
    # entries below -4.  A kernel without the `e >= -4` check forms no address from them: it answers -(e + 1), which is not 0xFF, and fails
    # the comparison without a read.  `near` guards against one other wrong kernel only, the one that reads the entry WITHOUT its sign: 8- and
    # 16-bit entries then index descArray below 65536, inside the arena's padding, and 32-bit ones far outside it (host only).  A kernel that
    # sign-extends and still indexes with a negative entry is not covered by the arena.
    low = {ot.IDX_U8: [-5, -128], ot.IDX_U16: [-5, -128, -32768], ot.IDX_U32: [-5, -128, -(1 << 31)]}[index_format]
    rows += [(e, inv, index_format != ot.IDX_U32) for e in low]
    n = len(rows)
    beyond = [(n, True), (n + 1, True), (n + 5, True), (0xFFFFFFFF, False), (0x80000000, False)]
    return dict(array=lvl3, descs=descs, rows=rows, beyond=beyond, index_format=index_format)


def bounds_variants(table):
    """(name, desc overrides, prims, expected bytes, near mask) for the table itself and the malformed descs over the same arrays"""
    rows, beyond = table["rows"], table["beyond"]
    n = len(rows)
    prims = np.array(list(range(n)) + [p for p, _ in beyond], np.uint32)
    near = np.array([r[2] for r in rows] + [k for _, k in beyond])
    expect = np.array([r[1] for r in rows] + [INVALID] * len(beyond), np.uint8)
    out = [("table", {}, prims, expect, near)]
    for fmt in (3, 7, 0x7FFFFFFF):   # unknown index formats: nothing can be read
        out.append(("indexFormat %d" % fmt, dict(indexFormat=fmt), prims[:n], np.full(n, INVALID, np.uint8), np.ones(n, bool)))
    out.append(("empty", dict(arrayDataSize=0, descArrayCount=0, indexCount=0), prims[:4], np.full(4, INVALID, np.uint8), np.ones(4, bool)))
    special = np.array([-4 <= r[0] < 0 for r in rows])
    out.append(("arrayDataSize 0", dict(arrayDataSize=0), prims[:n], np.where(special, expect[:n], INVALID).astype(np.uint8), near[:n]))
    return out


def bounds_hits(prims):
    h = np.empty(len(prims), HIT)
    h["prim"] = prims
    h["u"], h["v"] = bounds_hit()
    return h


def with_fields(desc, **fields):
    d = ot.BakeResultDesc.from_buffer_copy(desc)
    d._keep = desc
    for k, v in fields.items():
        setattr(d, k, v)
    return d


ARENA_INDEX_BYTES = 1024          # the index entries, then entries 0 (a valid desc)
ARENA_DESCS = 65536 + 128         # the descs, then descs of a valid block: every 8- and 16-bit entry read without its sign lands here
ARENA_ARRAY_BYTES = (4 << 20) + (1 << 16)   # the array, then state bytes != 0: a level-13 desc read as level 12 spans 4 MiB


def bounds_arena(table):
    """the table's three arrays inside ONE buffer, each followed by padding that looks valid, so that a kernel which reads past a declared
    size stays inside the buffer and returns a plausible state instead of OMMX_OPACITY_INVALID -> (bytes, index offset, desc offset, array offset)"""
    res = Result(table["array"], table["descs"], [r[0] for r in table["rows"]], table["index_format"])
    buf = np.zeros(ARENA_INDEX_BYTES + 8 * ARENA_DESCS + ARENA_ARRAY_BYTES, np.uint8)
    ib = res.index.view(np.uint8)
    assert ib.size + 4 * 8 <= ARENA_INDEX_BYTES
    buf[:ib.size] = ib
    d = np.zeros(ARENA_DESCS, res.descs.dtype)
    d["o"], d["l"], d["f"] = 0, 3, 2
    d[:len(res.descs)] = res.descs
    d_off, a_off = ARENA_INDEX_BYTES, ARENA_INDEX_BYTES + 8 * ARENA_DESCS
    buf[d_off:a_off] = d.view(np.uint8)
    buf[a_off:] = 0x6D
    buf[a_off:a_off + res.array.size] = res.array
    return buf, res, 0, d_off, a_off


def mesh_arena(uv, ix, num_tris, pad_tris=64):
    """texture coordinates (float32 (n, 2), 8-byte stride) and the first `num_tris` triangles of the 32-bit index buffer in ONE buffer, the
    declared indices followed by indices 0 and the coordinates by (0.5, 0.5) -> (bytes, index offset, texcoord offset)"""
    decl = np.ascontiguousarray(ix[:3 * num_tris], np.uint32)
    idx = np.concatenate([decl, np.zeros(3 * pad_tris, np.uint32)])
    nv = int(decl.max()) + 1
    tc = np.concatenate([np.ascontiguousarray(uv[:nv], np.float32), np.full((64, 2), 0.5, np.float32)])
    return np.concatenate([idx.view(np.uint8), tc.reshape(-1).view(np.uint8)]), 0, idx.nbytes


# ---- the sampler cases of resolve_hits: everything but the bake is made here, so the numpy reference can be checked without a GPU ----
def uv_encoded(uv, fmt):
    """texture coordinates in `fmt` with a 12-byte stride, and the float32 values the bake reads back"""
    n = len(uv)
    raw = np.zeros((n, 12), np.uint8)
    if fmt == ot.UV32_FLOAT:
        raw[:, :8] = np.ascontiguousarray(uv, np.float32).view(np.uint8).reshape(n, 8)
        return raw, uv.astype(np.float32)
    if fmt == ot.UV16_UNORM:
        q = np.clip(np.round(uv * 65535.0), 0, 65535).astype(np.uint16)
        raw[:, :4] = q.view(np.uint8).reshape(n, 4)
        return raw, (q.astype(np.float32) * np.float32(1.5259021896696421759314870504694e-5)).astype(np.float32)
    q = uv.astype(np.float16)
    raw[:, :4] = q.view(np.uint8).reshape(n, 4)
    return raw, q.astype(np.float32)


def grid_mesh(seed, side, spacing, origin, index_dtype):
    """side x side shared vertices on a jittered grid and the 2 (side-1)^2 triangles between them"""
    gy, gx = np.mgrid[0:side, 0:side].astype(np.float32)
    jx = (ot.uniform01(seed, side * side, 0).reshape(side, side) - np.float32(0.5)) * np.float32(0.5)
    jy = (ot.uniform01(seed, side * side, 1).reshape(side, side) - np.float32(0.5)) * np.float32(0.5)
    uv = np.stack([(gx + jx) * np.float32(spacing) + np.float32(origin), (gy + jy) * np.float32(spacing) + np.float32(origin)], -1).reshape(-1, 2)
    v = (np.arange(side - 1)[:, None] * side + np.arange(side - 1)[None, :]).reshape(-1)
    tris = np.concatenate([np.stack([v, v + 1, v + side], 1), np.stack([v + 1, v + side + 1, v + side], 1)])
    assert tris.max() <= np.iinfo(index_dtype).max
    return uv.astype(np.float32), tris.reshape(-1).astype(index_dtype)


def without_slivers(uv, extent, w, h):
    """unshared triangles (n, 3 vertices) with every triangle whose smallest altitude, measured in texels of a w x h texture, is below a quarter
    replaced by a fixed well-shaped one about the same centre -> (triangles, how many were replaced).  Finding: the
    level-line classification, in the oracle as in the product, can call a micro-triangle of such a sliver known against the bilinear value
    inside it -- a property of the bake, not of the sampler these cases test.  The sampler cases therefore never exercise slivers."""
    t = uv.reshape(-1, 3, 2).astype(np.float64)
    tx = t * np.array([w, h], np.float64)
    e = np.stack([tx[:, 1] - tx[:, 0], tx[:, 2] - tx[:, 1], tx[:, 0] - tx[:, 2]], 1)
    area2 = np.abs(e[:, 0, 0] * e[:, 1, 1] - e[:, 0, 1] * e[:, 1, 0])
    thin = area2 / np.sqrt((e ** 2).sum(axis=2)).max(axis=1) < 0.25
    shape = np.array([[-1.0, -1.0], [1.0, -0.5], [-0.5, 1.0]]) * (extent / 3.0)
    t[thin] = t[thin].mean(axis=1, keepdims=True) + shape
    return t.reshape(-1, 2).astype(np.float32), int(thin.sum())


BAND = 1e-6        # |alpha - cutoff| <= BAND: the kernel's fp32 blend and the float64 reference may fall on different sides
BAND_CAP = 0.001   # a condition on the cases, not a measurement: at most this share of a case's sampled hits may lie in the band

SHAPES = [(1000, 600), (333, 517), (1024, 256)]   # (width, height)
MAPPINGS = {"O_T": (ot.O, ot.T), "UT_O": (ot.UT, ot.O), "T_UO": (ot.T, ot.UO), "UT_UO": (ot.UT, ot.UO)}   # (LessEqual, Greater)


def sampler_case_names():
    names = ["border_linear_%s" % b for b in ("025", "075")]
    names += ["shape_%dx%d_a%d_f%d" % (w, h, a, f) for w, h in SHAPES for a in range(5) for f in (ot.NEAREST, ot.LINEAR)]
    names += ["mips_f%d" % f for f in (ot.NEAREST, ot.LINEAR)]
    names += ["cutoff_%s_%s" % (t, c) for t in ("foliage", "noise") for c in ("03", "07")]
    names += ["mapping_%s" % m for m in MAPPINGS]
    names += ["index16", "index8", "unaligned_uv32"]
    return names


def sampler_case(name):
    """the inputs of one case: mips (mip 0 first), raw texture coordinates + their byte offset / stride / format and the float32 values read
    back, indices, per-triangle levels, sampler, cut-off, mapping, and the hits (primitive, micro-triangle at the triangle's level, u, v)"""
    names = sampler_case_names()
    seed = 7000 + 13 * names.index(name)
    c = dict(name=name, addr=ot.WRAP, filt=ot.LINEAR, border=0.0, cutoff=0.5, le=ot.T, gt=ot.O, uv_format=ot.UV32_FLOAT, uv_offset=0, stride=12,
             size=(1024, 1024), kind="foliage", lo=-0.3, hi=1.3, n=2000, m=200000, mesh=None, slivers=0)
    part = name.split("_")
    if part[0] == "border":
        c.update(addr=ot.BORDER, border={"025": 0.25, "075": 0.75}[part[2]])
    elif part[0] == "shape":
        w, h = part[1].split("x")
        c.update(size=(int(w), int(h)), addr=int(part[2][1:]), filt=int(part[3][1:]), lo=-1.3, hi=2.3, border=0.75,
                 kind="noise" if (int(part[2][1:]) + int(part[3][1:])) % 2 else "foliage")
    elif part[0] == "mips":
        c.update(size=(512, 512), filt=int(part[1][1:]), kind="mips")
    elif part[0] == "cutoff":
        c.update(kind=part[1], cutoff={"03": 0.3, "07": 0.7}[part[2]], addr=ot.MIRROR)
    elif part[0] == "mapping":
        c["le"], c["gt"] = MAPPINGS[name[len("mapping_"):]]
        c.update(kind="noise", addr=ot.CLAMP)
    elif name == "index16":
        c.update(mesh=(64, np.uint16))
    elif name == "index8":
        c.update(mesh=(16, np.uint8), m=100000)
    elif name == "unaligned_uv32":
        c.update(uv_offset=1, stride=9, n=1000)
    w, h = c["size"]
    if c["kind"] == "noise":
        mips = [ot.value_noise(seed, w, h, octaves=4, base_cell=64)]
    else:
        mips = [ot.foliage_texture(seed, w, h, feature=48)]
    if c["kind"] == "mips":   # mips 1 and 2 hold the inverted alpha: a sampler that leaves mip 0 flips its answers
        mips += [np.ascontiguousarray(255 - mips[0][::2, ::2]), np.ascontiguousarray(255 - mips[0][::4, ::4])]
    ext = 16.0 / min(w, h)   # at least 16 texels along either axis
    if c["mesh"] is not None:
        side, dt = c["mesh"]
        uvf, ix = grid_mesh(seed, side, ext, -0.1, dt)
    else:
        uvf, ix = ot.random_triangles(seed, c["n"], ext, lo=c["lo"], hi=c["hi"])
        uvf, c["slivers"] = without_slivers(uvf, ext, w, h)
    n = len(ix) // 3
    if c["stride"] == 12:
        raw, uv_read = uv_encoded(uvf, c["uv_format"])
    else:   # UV32_FLOAT at a base and a stride that are not multiples of 4
        uv_read = uvf.astype(np.float32)
        raw = np.zeros(c["uv_offset"] + c["stride"] * len(uvf) + 16, np.uint8)
        rows = np.lib.stride_tricks.as_strided(raw[c["uv_offset"]:], (len(uvf), 8), (c["stride"], 1))
        rows[:] = np.ascontiguousarray(uv_read).view(np.uint8).reshape(len(uvf), 8)
    levels = (3 + ot.hash_u32(np.arange(n) + seed) % 4).astype(np.uint8)
    rng = np.random.default_rng(seed)
    m = c["m"]
    prims = rng.integers(0, n, m)
    micro = (rng.random(m) * (4.0 ** levels[prims])).astype(np.int64)
    u, v = interior_points(rng, micro_vertices(micro, levels[prims]))
    c.update(mips=mips, raw=raw, uv_read=uv_read, ix=ix, levels=levels, prims=prims, micro=micro, u=u, v=v, ntris=n)
    return c


def reference_alpha(c):
    """the numpy sampler's alpha at every hit of the case, and which hits lie in the exclusion band"""
    tu, tv = hit_tex_coords(c["uv_read"], c["ix"], c["prims"], c["u"], c["v"])
    alpha = sample_alpha(c["mips"][0], tu, tv, c["addr"], c["filt"], c["border"])
    return alpha, np.abs(alpha - np.float64(np.float32(c["cutoff"]))) <= BAND
