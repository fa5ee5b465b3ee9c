"""Shared by tests/test_lookup_gpu.py and tests/scripts/lookup_throughput.py: device-resident bakes that stay alive for the lookup entry points
(ommxLookupOpacity, ommxResolveHits), a numpy restatement of the bird-curve decode, and a numpy sampler of mip 0 (the resolve kernel's sampler)."""
import ctypes as C
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

    def __init__(self, lib, hip, baker, desc, uv, ix, levels=None):
        self.lib, self.hip = lib, hip
        self.bufs = [hip.upload(uv), hip.upload(ix)]
        self.ddesc = ot.BakeInputDesc.from_buffer_copy(desc)
        self.ddesc.texCoords, self.ddesc.indexBuffer = self.bufs[0], self.bufs[1]
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


def micro_vertices(index, level):
    """(n, 3, 2) float64 barycentric (u, v) vertices of micro-triangles `index` at `level` (arrays of equal length)"""
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


# ---- numpy restatement of the resolve kernel's sampler (mip 0; classify_device.h tex_coord / bilinear), power-of-two textures ----
def _addr(mode, x, size):
    if mode == ot.WRAP:
        return x & (size - 1)
    if mode == ot.MIRROR:
        xa = np.abs(x) - (x < 0)
        flipped = (xa // size) & 1
        w = xa & (size - 1)
        return np.where(flipped == 1, size - w - 1, w)
    if mode == ot.CLAMP:
        return np.clip(x, 0, size - 1)
    if mode == ot.BORDER:
        return np.where((x >= size) | (x < 0), -1, x)
    if mode == ot.MIRROR_ONCE:
        return np.clip(np.where(x >= 0, x, -x - 1), 0, size - 1)
    raise ValueError(mode)


def _texel(tex, x, y, border):
    h, w = tex.shape
    a = (tex.astype(np.float32) if tex.dtype == np.float32 else tex.astype(np.float32) * np.float32(1.0 / 255.0))
    out = np.full(x.shape, np.float32(border), np.float32)
    ok = (x >= 0) & (y >= 0)
    out[ok] = a[y[ok], x[ok]]
    return out


def sample_alpha(tex, tu, tv, addr, filt, border=0.0):
    h, w = tex.shape
    tu, tv = tu.astype(np.float32), tv.astype(np.float32)
    if filt == ot.NEAREST:
        x = _addr(addr, np.floor(tu * np.float32(w)).astype(np.int64), w)
        y = _addr(addr, np.floor(tv * np.float32(h)).astype(np.int64), h)
        return _texel(tex, x, y, border)
    px, py = tu * np.float32(w) - np.float32(0.5), tv * np.float32(h) - np.float32(0.5)
    fx, fy = np.floor(px), np.floor(py)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0, y1 = _addr(addr, ix, w), _addr(addr, ix + 1, w), _addr(addr, iy, h), _addr(addr, iy + 1, h)
    a, b, c, d = _texel(tex, x0, y0, border), _texel(tex, x0, y1, border), _texel(tex, x1, y0, border), _texel(tex, x1, y1, border)
    wx, wy = (px - fx).astype(np.float32), (py - fy).astype(np.float32)
    one = np.float32(1.0)
    ac = a * (one - wx) + c * wx
    bd = b * (one - wx) + d * wx
    return (ac * (one - wy) + bd * wy).astype(np.float32)


def hit_tex_coords(uv, ix, prims, u, v):
    """texture coordinate of each hit, interpolated with weights (1-u-v, u, v) in fp32 as the kernel does (uv: float32 (n, 2))"""
    tri = ix.reshape(-1, 3)[prims]
    p0, p1, p2 = uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]]
    u, v = u.astype(np.float32), v.astype(np.float32)
    bx = (np.float32(1.0) - u - v).astype(np.float32)
    tu = p0[:, 0] * bx + p1[:, 0] * u + p2[:, 0] * v
    tv = p0[:, 1] * bx + p1[:, 1] * u + p2[:, 1] * v
    return tu.astype(np.float32), tv.astype(np.float32)
