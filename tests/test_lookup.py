"""Host checks of the micromap consumer (include/omm_mi355x_lookup.h): the barycentrics -> micro-triangle map, the decoding of hand-built results
through ommxLookupOpacityHost (the same header code the lookup_opacity kernel runs), and the bounds rule; and checks of the reference code the
GPU tests (tests/test_lookup_gpu.py) compare the kernels with: the numpy texel addressing against the oracle's, the closure-holder sets against
the host lookup, and the share of each sampler case's hits that lies in the exclusion band.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
from lookup_util import Result, pack, unpack, digit_result

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


def lookup(lib, res, prims, u, v, flags=0):
    hits = np.empty(len(prims), HIT)
    hits["prim"], hits["u"], hits["v"] = prims, u, v
    out = np.full(len(prims), 0xAB, np.uint8)
    assert lib.ommxLookupOpacityHost(C.byref(res.desc), hits.ctypes.data, len(hits), out.ctypes.data, flags) == ot.SUCCESS
    return out


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


# ---- the bounds rule on the host (the same table goes through both kernels in tests/test_lookup_gpu.py) ----
def test_bounds_rule(lib):
    """every input the result cannot answer reads OMMX_OPACITY_INVALID, with no read outside the arrays given: the table of
    lookup_util.bounds_table -- level 13, formats 0 and 3, blocks that end at / one byte past / start at arrayDataSize, entries >= descArrayCount
    and below -4, special indices, primitives >= indexCount, unknown index formats, empty arrays -- in all three index formats"""
    for index_format in (ot.IDX_U8, ot.IDX_U16, ot.IDX_U32):
        table = lu.bounds_table(index_format)
        res = Result(table["array"], table["descs"], [r[0] for r in table["rows"]], index_format)
        assert res.array.size == 16 and res.desc.descArrayCount == 8
        for name, fields, prims, expect, near in lu.bounds_variants(table):
            for flags in (0, FORCE_2STATE):
                hits = lu.bounds_hits(prims)
                got = lu.lookup_host(lib, lu.with_fields(res.desc, **fields), hits, flags)
                want = np.where((expect == 2) | (expect == 3), expect - 2, expect).astype(np.uint8) if flags else expect
                assert np.array_equal(got, want), (index_format, name, flags, got, want)
        # what the table must contain, whatever its layout: valid blocks that end exactly at arrayDataSize, every special index, every refusal
        name, fields, prims, expect, near = lu.bounds_variants(table)[0]
        assert {0, 1, 2, 3} <= set(expect.tolist()) and (expect == INVALID).sum() >= 14 and not near.all()
    res = Result(pack(np.arange(64) % 4, 2), [(0, 3, 2)], [0], ot.IDX_U8)
    def one(prim, r=res, **kw):
        return lookup(lib, r, [prim], kw["u"], kw["v"])[0]
    nodata = Result(np.zeros(0, np.uint8), [(0, 0, 1)], [0], ot.IDX_U16)
    assert one(0, nodata, u=[0.3], v=[0.3]) == INVALID           # arrayDataSize 0 with a null array
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


# ---- the reference code of the GPU tests ----
@pytest.mark.parametrize("level", [0, 1, 2, 3, 5, 8, 10])
def test_edge_and_vertex_points_read_a_micro_triangle_that_holds_them(lib, level):
    """lookup_util.closure_holders (candidates from the forward decode, containment on the decoded vertices in float64) against the host lookup
    at every vertex, every edge midpoint and one ulp to either side of the cell diagonal -- the check the GPU test makes of the kernel"""
    rng = np.random.default_rng(40 + level)
    micro = lu.edge_level_sample(rng, level)
    u, v = lu.edge_and_vertex_points(micro, level)
    assert len(u) == 8 * len(micro)
    res = digit_result(level)
    idx = lu.digits_to_index(level, lu.lookup_host(lib, res.desc, lu.digit_hits(level, u, v)), len(u))
    assert (idx < 4 ** level).all()
    beyond = lu.check_index_is_a_holder(level, u, v, idx)
    assert beyond <= len(micro)   # only diagonal midpoints moved outwards across the edge u + v = 1 leave the triangle
    # the holders are what they claim: a centroid is held by its own micro-triangle alone, a shared vertex by up to six
    cu, cv = lu.centroid_points(lu.micro_vertices(micro, np.full(len(micro), level)))
    cand, holds = lu.closure_holders(level, cu, cv)
    assert (holds.sum(axis=1) == 1).all() and np.array_equal(cand[holds], micro)
    cand, holds = lu.closure_holders(level, u[:3 * len(micro)], v[:3 * len(micro)])
    assert holds.sum(axis=1).max() == (6 if level >= 2 else (3 if level == 1 else 1)) and holds.sum(axis=1).min() >= 1
    # and the check fails for a neighbour: the index of another micro-triangle is not accepted at a centroid
    if level >= 1:
        with pytest.raises(AssertionError):
            lu.check_index_is_a_holder(level, cu, cv, (micro + 1) % 4 ** level)


def test_numpy_addressing_equals_the_oracle():
    """lookup_util._addr == orc_get_tex_coord (pinned to the reference's tables in test_oracle_units.py) for x in -3w..3w, every address mode,
    sizes that are powers of two and sizes that are not, and the texture-wide flag both ways where the size allows it"""
    dll = C.CDLL(ot.oracle_path())
    dll.orc_get_tex_coord.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)]
    out = (C.c_int * 2)()
    for size in (1, 2, 7, 64, 256, 333, 517, 600, 1000, 1024):
        x = np.arange(-3 * size, 3 * size + 1, dtype=np.int64)
        pow2_axis = (size & (size - 1)) == 0
        for flag in ((0, 1) if pow2_axis else (0,)):   # flag 0 with a power-of-two side: the other side of the texture is not one
            for mode in (ot.WRAP, ot.MIRROR, ot.CLAMP, ot.BORDER, ot.MIRROR_ONCE):
                got = lu._addr(mode, x, size, bool(flag))
                want = np.empty(len(x), np.int64)
                for k, xi in enumerate(x):
                    dll.orc_get_tex_coord(mode, flag, int(xi), int(xi), size, size, out)
                    assert out[0] == out[1]
                    want[k] = out[0]
                border = want == 0x7FFFFFFE if mode == ot.BORDER else np.zeros(len(x), bool)
                assert border.any() == (mode == ot.BORDER)
                assert np.array_equal(got, np.where(border, -1, want)), (size, flag, mode, x[got != np.where(border, -1, want)][:5])
                assert ((got >= 0) & (got < size) | border).all()


def test_numpy_sampler_against_a_scalar_restatement():
    """sample_alpha on a non-square texture that is not a power of two, every mode and filter, against a per-point Python restatement with
    Python floats (float64) of the same definition: fp32 texel coordinate and weights, float64 blend"""
    rng = np.random.default_rng(3)
    tex = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    h, w = tex.shape
    tu, tv = rng.uniform(-2.5, 3.5, 300).astype(np.float32), rng.uniform(-2.5, 3.5, 300).astype(np.float32)
    f32 = np.float32
    for mode in (ot.WRAP, ot.MIRROR, ot.CLAMP, ot.BORDER, ot.MIRROR_ONCE):
        def texel(x, y):
            ax, ay = int(lu._addr(mode, np.array([x]), w, False)[0]), int(lu._addr(mode, np.array([y]), h, False)[0])
            return 0.625 if ax < 0 or ay < 0 else float(f32(tex[ay, ax]) * f32(1.0 / 255.0))
        near = lu.sample_alpha(tex, tu, tv, mode, ot.NEAREST, 0.625)
        lin = lu.sample_alpha(tex, tu, tv, mode, ot.LINEAR, 0.625)
        for k in range(len(tu)):
            assert near[k] == texel(int(np.floor(tu[k] * f32(w))), int(np.floor(tv[k] * f32(h))))
            px, py = tu[k] * f32(w) - f32(0.5), tv[k] * f32(h) - f32(0.5)
            x, y = int(np.floor(px)), int(np.floor(py))
            wx, wy = float(f32(px - np.floor(px))), float(f32(py - np.floor(py)))
            want = (texel(x, y) * (1 - wx) + texel(x + 1, y) * wx) * (1 - wy) + (texel(x, y + 1) * (1 - wx) + texel(x + 1, y + 1) * wx) * wy
            assert abs(lin[k] - want) < 1e-15


def test_sampler_cases_are_well_posed(oracle):
    """the conditions tests/test_lookup_gpu.py::test_resolve_sampler_paths rests on, decided here without the product's kernels: by the numpy
    reference alone, at most 0.1 % of any case's hits have an alpha within 1e-6 of the cut-off (the GPU test asserts it again) and every case
    samples both sides of its cut-off; and in the ORACLE's bake of the case every known state agrees with the numpy sampler"""
    for name in lu.sampler_case_names():
        c = lu.sampler_case(name)
        alpha, near = lu.reference_alpha(c)
        above = alpha > np.float64(np.float32(c["cutoff"]))
        assert near.sum() <= lu.BAND_CAP * len(near), (name, int(near.sum()))
        assert 0.02 < above.mean() < 0.98, (name, above.mean())
        b = oracle.create_baker()
        t = oracle.create_texture(b, c["mips"], alpha_cutoff=c["cutoff"])
        d = ot.make_desc(t, c["raw"].reshape(-1)[c["uv_offset"]:], c["ix"], 6, levels=c["levels"], addr=c["addr"], filt=c["filt"],
                         promo=ot.PROMO_NEAREST, flags=ot.FLAG_THREADS, uv_format=c["uv_format"], border_alpha=c["border"],
                         alpha_cutoff=c["cutoff"], le=c["le"], gt=c["gt"])
        d.texCoordStrideInBytes = c["stride"]
        res = oracle.bake(b, d, want_stats=False)
        oracle.destroy_texture(b, t)
        oracle.destroy_baker(b)
        lv, has = lu.prim_levels(res)
        assert np.array_equal(lv[has], c["levels"][has]), name
        state = lu.numpy_states(res, c["prims"], c["micro"])
        q = c["uv_read"][c["ix"].reshape(-1, 3)].reshape(-1, 6)
        area = np.float32(0.5) * np.abs(q[:, 0] * (q[:, 3] - q[:, 5]) + q[:, 2] * (q[:, 5] - q[:, 1]) + q[:, 4] * (q[:, 1] - q[:, 3]))
        degenerate = (area.astype(np.float64) < 1e-9)[c["prims"]] if c["filt"] == ot.NEAREST else np.zeros(c["m"], bool)
        known = (state < 2) & ~near & ~degenerate
        bad = known & ((np.where(above, c["gt"], c["le"]) & 1) != state)
        print("%s: %d of %d hits in the band, %.1f %% above the cut-off, %d known hits, %d of %d triangles re-drawn as slivers" % (
            name, int(near.sum()), len(near), 100.0 * above.mean(), int(known.sum()), c["slivers"], c["ntris"]))
        assert c["slivers"] <= c["ntris"] // 10, name
        assert not bad.any(), (name, int(bad.sum()))


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
