"""Host checks of the micromap consumer (include/omm_mi355x_lookup.h): the barycentrics -> micro-triangle map, the decoding of hand-built results
through ommxLookupOpacityHost (the same header code the lookup_opacity kernel runs), and the bounds rule.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import ommtest as ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 0xFF
HIT = np.dtype([("prim", "<u4"), ("u", "<f4"), ("v", "<f4")])
FORCE_2STATE, IGNORE_MICROMAP = 1, 2


@pytest.fixture(scope="module")
def lib():
    dll = C.CDLL(ot.product_path())
    dll.ommxLookupOpacityHost.argtypes = [C.POINTER(ot.BakeResultDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    dll.ommxLookupOpacity.argtypes = [C.POINTER(ot.BakeResultDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    dll.ommxResolveHits.argtypes = [C.c_void_p, C.POINTER(ot.BakeInputDesc), C.POINTER(ot.BakeResultDesc), C.c_void_p, C.c_uint32, C.c_void_p,
                                    C.c_uint32, C.c_void_p]
    return dll


@pytest.fixture(scope="module")
def orc():
    dll = C.CDLL(ot.oracle_path())
    dll.orc_index2bary.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    dll.orc_micro_triangle.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    return dll


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


def lookup(lib, res, prims, u, v, flags=0):
    hits = np.empty(len(prims), HIT)
    hits["prim"], hits["u"], hits["v"] = prims, u, v
    out = np.full(len(prims), 0xAB, np.uint8)
    assert lib.ommxLookupOpacityHost(C.byref(res.desc), hits.ctypes.data, len(hits), out.ctypes.data, flags) == ot.SUCCESS
    return out


def pack(states, bits):
    """micro-triangle states -> block bytes: state i at bit i (2-state) / bits 2i..2i+1 (4-state), little-endian within bytes"""
    s = np.asarray(states, np.uint8)
    per = 8 // bits
    s = np.concatenate([s, np.zeros((-len(s)) % per, np.uint8)]).reshape(-1, per)
    return (s.astype(np.uint32) << (bits * np.arange(per, dtype=np.uint32))).sum(axis=1).astype(np.uint8)


def unpack(block, i, bits):
    return (block[(i * bits) >> 3] >> ((i * bits) & 7)) & ((1 << bits) - 1)


def centroids(orc, level):
    n = 4 ** level
    uv = np.empty((n, 6), np.float32)
    for i in range(n):
        orc.orc_index2bary(i, level, uv[i].ctypes.data_as(C.POINTER(C.c_float)))
    return ((uv[:, 0] + uv[:, 2] + uv[:, 4]) / np.float32(3)).astype(np.float32), ((uv[:, 1] + uv[:, 3] + uv[:, 5]) / np.float32(3)).astype(np.float32)


# ---- the index map ----
def test_index_map_every_micro_triangle_of_every_level(tmp_path):
    """centroid of every micro-triangle (levels 0..12) -> its own index; vertices and edge midpoints -> a micro-triangle whose closure holds
    them (tests/native/lookup_check.cpp, the plain C++ build of the header, against the oracle's forward decode)"""
    exe = str(tmp_path / "lookup_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "lookup_check.cpp"),
                    ot.oracle_path(), "-Wl,-rpath," + os.path.dirname(ot.oracle_path()), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "156587347 points, 0 failures" in r.stdout, r.stdout


def test_digit_table_is_the_inverse_of_the_forward_decode():
    """OMMX_BIRD_DIGIT_TABLE rebuilt from the forward decode (classify_device.h micro_triangle) of every index of levels 1..6"""
    src = open(os.path.join(ROOT, "include", "omm_mi355x_lookup.h")).read()
    table = int(re.search(r"#define OMMX_BIRD_DIGIT_TABLE (0x[0-9a-f]+)ull", src).group(1), 16)

    def even_bits(x):
        return sum(((x >> (2 * i)) & 1) << i for i in range(16))

    def pxor(x):
        for s in (1, 2, 4, 8):
            x ^= x >> s
        return x
    seen = {}
    for level in range(1, 7):
        for index in range(4 ** level):
            b0, b1 = even_bits(index), even_bits(index >> 1)
            fx, fy = pxor(b0), pxor(b0 & ~b1)
            t = fy ^ b1
            m = (1 << level) - 1
            iu, iv, iw = ((fx & ~t) | (b0 & ~t) | (~b0 & ~fx & t)) & m, (fy ^ b0) & m, ((~fx & ~t) | (b0 & ~t) | (~b0 & fx & t)) & m
            x = y = 0
            for i in range(level - 1, -1, -1):
                d = (index >> (2 * i)) & 3
                key = x | y << 1 | ((iu >> i) & 1) << 2 | ((iv >> i) & 1) << 3 | ((iw >> i) & 1) << 4
                assert seen.setdefault(key, d) == d, "digit not a function of the key"
                x ^= d & 1
                y ^= 1 if d == 1 else 0
    assert len(seen) == 16
    assert sum(d << (2 * k) for k, d in seen.items()) == table


def digit_result(level):
    """one 4-state block per base-4 digit of the index: in block p micro-triangle i stores (i >> 2p) & 3, so the states a point reads in
    primitives 0..level-1 spell the index the lookup chose"""
    n = 4 ** level
    i = np.arange(n, dtype=np.uint32)
    blocks = [pack((i >> (2 * p)) & 3, 2) for p in range(max(level, 1))]
    size = len(blocks[0])
    return Result(np.concatenate(blocks), [(p * size, level, 2) for p in range(len(blocks))], list(range(len(blocks))), ot.IDX_U32)


def lookup_index(lib, res, level, u, v):
    idx = np.zeros(len(u), np.uint32)
    for p in range(max(level, 1)):
        s = lookup(lib, res, np.full(len(u), p, np.uint32), u, v)
        assert (s < 4).all()
        idx |= s.astype(np.uint32) << np.uint32(2 * p)
    return idx


@pytest.mark.parametrize("level", [0, 1, 2, 3, 5, 7])
def test_barycentric_convention_against_uv_space(lib, orc, level):
    """independent of the index map above: the UV-space centroid of orc_micro_triangle(tri, i, level) of random triangles, solved for the DXR
    (u, v) of that point (hit = (1-u-v) V0 + u V1 + v V2), reads index i through ommxLookupOpacityHost.  A swapped or rotated convention fails."""
    res = digit_result(level)
    n = 4 ** level
    for seed in range(4):
        rng = np.random.default_rng(1000 * level + seed)
        tri = rng.uniform(-1.0, 2.0, 6).astype(np.float32)
        p0, p1, p2 = tri[0:2].astype(np.float64), tri[2:4].astype(np.float64), tri[4:6].astype(np.float64)
        e1, e2 = p1 - p0, p2 - p0
        if abs(e1[0] * e2[1] - e1[1] * e2[0]) < 0.05:
            continue
        cent = np.empty((n, 2))
        out = (C.c_float * 6)()
        tp = tri.ctypes.data_as(C.POINTER(C.c_float))
        for i in range(n):
            orc.orc_micro_triangle(tp, i, level, out)
            cent[i] = ((out[0] + out[2] + out[4]) / 3.0, (out[1] + out[3] + out[5]) / 3.0)
        m = np.stack([p1 - p0, p2 - p0], axis=1)
        uv = np.linalg.solve(m, (cent - p0).T).T
        got = lookup_index(lib, res, level, uv[:, 0].astype(np.float32), uv[:, 1].astype(np.float32))
        assert np.array_equal(got, np.arange(n, dtype=np.uint32)), np.nonzero(got != np.arange(n))[0][:10]


# ---- decoding ----
@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32])
@pytest.mark.parametrize("bits", [1, 2])
def test_decoding_of_hand_built_results(lib, orc, index_format, bits):
    """blocks of levels 0..3 (the ones below a byte included), packed back to back at odd offsets, all four special indices, every index
    format, both formats; every micro-triangle's centroid reads the state a numpy decode of the block gives; Force2State"""
    rng = np.random.default_rng(7 * bits + index_format)
    array, descs, expect_blocks = [np.zeros(3, np.uint8)], [], []
    off = 3
    for level in range(4):
        for rep in range(2):
            states = rng.integers(0, 1 << bits, 4 ** level)
            blk = pack(states, bits)
            descs.append((off, level, bits))
            expect_blocks.append((level, blk))
            array.append(blk)
            off += len(blk)
    index = [7, -1, 0, -2, 3, -3, 5, -4, 1, 2, 4, 6]
    res = Result(np.concatenate(array), descs, index, index_format)
    for prim, e in enumerate(index):
        if e < 0:
            s = lookup(lib, res, [prim] * 3, [0.1, 0.5, 0.0], [0.1, 0.2, 1.0])
            assert (s == -(e + 1)).all(), (e, s)
            f = lookup(lib, res, [prim], [0.2], [0.3], FORCE_2STATE)
            assert f[0] == {-1: 0, -2: 1, -3: 0, -4: 1}[e]
            continue
        level, blk = expect_blocks[e]
        cu, cv = centroids(orc, level)
        s = lookup(lib, res, np.full(len(cu), prim, np.uint32), cu, cv)
        expect = np.array([unpack(blk, i, bits) for i in range(4 ** level)], np.uint8)
        assert np.array_equal(s, expect), (prim, level, s, expect)
        f = lookup(lib, res, np.full(len(cu), prim, np.uint32), cu, cv, FORCE_2STATE)
        assert np.array_equal(f, np.where(expect >= 2, expect - 2, expect))


# ---- the bounds rule (host only) ----
def test_bounds_rule(lib):
    """every input the result cannot answer reads OMMX_OPACITY_INVALID, with no read outside the arrays given"""
    lvl3 = pack(np.arange(64) % 4, 2)                       # 16 bytes
    descs = [(0, 3, 2), (0, 13, 2), (0, 2, 0), (0, 2, 3), (1, 3, 2), (8, 3, 1), (9, 3, 1), (16, 0, 1)]
    res = Result(lvl3, descs, [0, 1, 2, 3, 4, 5, 6, 7, 8, -5, -128, -1, 0], ot.IDX_U8)
    hit = dict(u=[0.3], v=[0.3])
    def one(prim, r=res, **kw):
        return lookup(lib, r, [prim], kw.get("u", hit["u"]), kw.get("v", hit["v"]))[0]
    assert one(0) < 4 and one(11) == 0 and one(12) < 4       # valid: a block that fits, a special index
    assert one(1) == INVALID                                 # level 13
    assert one(2) == INVALID and one(3) == INVALID           # format INVALID (0) / MAX_NUM (3)
    assert one(4) == INVALID                                 # 16-byte block at offset 1 of a 16-byte array
    assert one(5) < 2                                        # 8-byte 2-state block at 8: the last byte of the array
    assert one(6) == INVALID                                 # ... at 9
    assert one(7) == INVALID                                 # level-0 block at offset 16 == arrayDataSize
    assert one(8) == INVALID                                 # entry 8 >= descArrayCount (8)
    assert one(9) == INVALID and one(10) == INVALID          # entries below -4
    assert one(13) == INVALID and one(0xFFFFFFFF) == INVALID  # prim >= indexCount
    for fmt in (3, 7, 0x7FFFFFFF):                      # unknown index formats
        bad = Result(lvl3, descs[:1], [0], ot.IDX_U32)
        bad.desc.indexFormat = fmt
        assert one(0, bad) == INVALID
    empty = Result(np.zeros(0, np.uint8), [], [], ot.IDX_U32)
    assert one(0, empty) == INVALID
    nodata = Result(np.zeros(0, np.uint8), [(0, 0, 1)], [0], ot.IDX_U16)
    assert one(0, nodata) == INVALID                         # arrayDataSize 0
    # NaN, infinities and points outside the triangle still read a valid micro-triangle of a valid block
    for u, v in [(np.nan, 0.2), (0.2, np.nan), (np.inf, -np.inf), (-1.0, 5.0), (0.9, 0.9), (1e30, 1e30), (-0.0, 1.0)]:
        assert one(0, u=[u], v=[v]) < 4


def test_micro_index_stays_in_range_for_any_float(lib):
    """random bit patterns for u and v (NaN, infinities, denormals, huge values) never leave the block: the digit result reads an index < 4^level"""
    rng = np.random.default_rng(5)
    for level in (1, 4, 6):
        res = digit_result(level)
        bits = rng.integers(0, 1 << 32, size=(2, 4000), dtype=np.uint64).astype(np.uint32)
        u, v = bits[0].view(np.float32), bits[1].view(np.float32)
        idx = lookup_index(lib, res, level, u, v)
        assert (idx < 4 ** level).all()


# ---- argument checks that need no device ----
def test_argument_checks(lib):
    res = Result(pack([1], 2), [(0, 0, 2)], [0], ot.IDX_U32)
    hits = np.zeros(1, HIT)
    out = np.zeros(1, np.uint8)
    host = lib.ommxLookupOpacityHost
    assert host(None, hits.ctypes.data, 1, out.ctypes.data, 0) == ot.INVALID_ARGUMENT
    assert host(C.byref(res.desc), None, 1, out.ctypes.data, 0) == ot.INVALID_ARGUMENT
    assert host(C.byref(res.desc), hits.ctypes.data, 1, None, 0) == ot.INVALID_ARGUMENT
    assert host(C.byref(res.desc), hits.ctypes.data, 1, out.ctypes.data, IGNORE_MICROMAP) == ot.INVALID_ARGUMENT   # no texture here
    assert host(C.byref(res.desc), None, 0, None, 0) == ot.SUCCESS
    assert host(C.byref(res.desc), hits.ctypes.data, 1, out.ctypes.data, 0) == ot.SUCCESS and out[0] == 1
    # the device entry points refuse before they touch a device; count == 0 launches nothing
    dev = lib.ommxLookupOpacity
    assert dev(None, None, 0, None, 0, None) == ot.INVALID_ARGUMENT
    assert dev(C.byref(res.desc), None, 4, None, 0, None) == ot.INVALID_ARGUMENT
    assert dev(C.byref(res.desc), None, 0, None, 4, None) == ot.INVALID_ARGUMENT
    assert dev(C.byref(res.desc), None, 0, None, 0, None) == ot.SUCCESS
    rh = lib.ommxResolveHits
    d = ot.default_bake_desc()
    assert rh(None, C.byref(d), C.byref(res.desc), None, 0, None, 0, None) == ot.INVALID_ARGUMENT
    logged = []
    prod = ot.Lib("product")
    b = prod.create_baker(callback=lambda sev, msg, user: logged.append(msg))
    try:
        assert rh(b, None, C.byref(res.desc), None, 0, None, 0, None) == ot.INVALID_ARGUMENT
        assert rh(b, C.byref(d), C.byref(res.desc), None, 0, None, 0, None) == ot.INVALID_ARGUMENT   # no texture: as ommxBakeDevice
        assert len(logged) == 2, logged
    finally:
        prod.destroy_baker(b)
