"""ommxReorientMicromap on the GPU.  Every case compares arrayData, descArray, the index buffer, both histograms (as mappings) and the info fields with
tests/reorient_util.py's restate_reorient byte for byte, info-only and full -- there is no tolerance anywhere.  The sources are hand-built results
with random bytes, as in tests/test_gather_gpu.py; the shapes are the edges of the stage kernel (a block below a tile, of one tile, of one, two and
many units, at every misalignment, ending with its array), of the items (mixed orientations, one descriptor under all six) and of the wiring to the
shared tail, not a workload."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import combine_util as mu
import fit_util as fu
import gather_util as gt
import geometry_util as gu
import reorient_util as rt
import workloads as wl

pytestmark = pytest.mark.gpu

FORMATS = [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32]
TILE = 3   # kReorientTileDepth of omm_amd/csrc/reorient_map.h


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    gu.bind(product.dll)
    gt.bind(product.dll)
    fu.bind(product.dll)
    return rt.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def random_states(level, bits, seed):
    """random states, not uniform (a level-0 block always is) and symmetric under no orientation but 0 (levels >= 1, with overwhelming odds)"""
    return np.random.default_rng(seed * 977 + level * 13 + bits).integers(0, 2 * bits, 4 ** level).astype(np.uint8)


def per_primitive_states(r):
    """what each primitive of a result (model or download) decodes to: its special entry, or level, format and states"""
    out = []
    for e in r["index"]:
        if e < 0:
            out.append(int(e))
        else:
            o, l, f = (int(x) for x in r["descs"][int(e)])
            out.append((l, f, cu.block_states(r["array"], o, l, f).tobytes()))
    return out


def destroy(dll, handles):
    for h in handles:
        assert dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS


# ---- levels and formats ----
@pytest.fixture(scope="module")
def blocks_to_level_8():
    return [(random_states(level, bits, 100 + level), level, bits) for level in range(8, -1, -1) for bits in (2, 1)]


@pytest.mark.parametrize("misalignment", range(16))
def test_every_level_under_every_orientation_at_every_misalignment(dll, hip, baker, blocks_to_level_8, misalignment):
    """one block per level 8..0 in both formats, packed without gaps behind `misalignment` bytes, every block under all six orientations: blocks below
    a tile (levels 0..2), of one tile (level 3), of several, of one unit (16 KiB) and of two; the last block ends with the array, which ends the
    allocation"""
    table = cu.table_of_blocks(blocks_to_level_8, first_offset=misalignment)
    n = len(blocks_to_level_8)
    assert all(o % 16 == misalignment for o, l, f in table[1].tolist() if f * 4 ** l >= 128)
    src = cu.Source(hip, *table, np.repeat(np.arange(n)[::-1], 6), ot.IDX_U8, array_align=16)
    try:
        ref = rt.reorient_and_check(dll, hip, baker, src, np.tile(np.arange(6, dtype=np.uint8), n))
        info = ref["info"]
        assert info["referencedBlocks"] == 6 * n and info["reorientedBlocks"] == 5 * n and info["uniformBlocks"] == 12 and info["skippedPrimitives"] == 0
        assert info["descArrayCount"] + info["duplicateBlocks"] == 6 * n - 12 and info["descArrayCount"] > 5 * (n - 4)
    finally:
        src.close()


@pytest.mark.parametrize("level", [TILE - 1, TILE, TILE + 1])
def test_levels_around_the_tile(dll, hip, baker, level):
    """the level below a tile (one lane, field by field), of exactly one tile and of four, in both formats, each orientation through the desc: every
    output block is the model's and differs from the source's"""
    blocks = [(random_states(level, bits, 31), level, bits) for bits in (1, 2)]
    src = cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=3), [0, 1, -2, 1], ot.IDX_U16, array_align=1)
    try:
        plain = rt.reorient_and_check(dll, hip, baker, src, 0)
        for o in range(1, 6):
            ref = rt.reorient_and_check(dll, hip, baker, src, o)
            assert ref["info"]["reorientedBlocks"] == 2 and ref["info"]["descArrayCount"] == 2 and not np.array_equal(ref["array"], plain["array"])
    finally:
        src.close()


@pytest.fixture(scope="module")
def blocks_above_level_8():
    return [(random_states(12, 2, 7), 12, 2)] + [(random_states(level, bits, 200 + level), level, bits) for level in (11, 10, 9) for bits in (2, 1)]


@pytest.mark.parametrize("misalignment", [0, 5])
def test_levels_9_to_12(dll, hip, baker, blocks_above_level_8, misalignment):
    """blocks of many units: level 12 in the 4-state format -- 256 units, nine digits above the tile -- once, at an odd address under a rotation;
    levels 9..11 in both formats at an aligned and at an odd address under a rotation and a reflection each"""
    blocks = blocks_above_level_8[0 if misalignment else 1:]
    n = len(blocks)
    src = cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=misalignment), list(range(n)) + list(range(1 if misalignment else 0, n)), ot.IDX_U16, array_align=16)
    try:
        orient = np.array([2] + [1] * (n - 1) + [4] * (n - 1) if misalignment else [1] * n + [3] * n, np.uint8)
        ref = rt.reorient_and_check(dll, hip, baker, src, orient)
        assert ref["info"]["descArrayCount"] == len(orient) and ref["descs"][0, 1] == (12 if misalignment else 11)
    finally:
        src.close()


def test_small_blocks_with_garbage(dll, hip, baker):
    """levels 0 and 1 with ones in the unused bits of their byte, under every orientation: they merge with their clean twin, they are promoted when
    their used bits are uniform, and the output byte has zeros in the unused bits"""
    shapes = [(0, 1), (0, 2), (1, 1), (1, 2)]
    clean = [(np.array(s, np.uint8), l, b) for (l, b), s in zip(shapes, ([1], [2], [1, 0, 0, 1], [1, 3, 0, 2]))]
    uniform = [(np.full(4 ** l, 1, np.uint8), l, b) for l, b in shapes]
    table, descs = cu.table_of_blocks(clean + uniform, first_offset=5, gap=2)
    dirty = table.copy()
    for o, l, f in descs.tolist():
        dirty[o] |= (0xFF << (f * 4 ** l)) & 0xFF
    assert (dirty != table).sum() == 6
    index = np.repeat(np.arange(8), 6)
    orient = np.tile(np.arange(6, dtype=np.uint8), 8)
    srcs = [cu.Source(hip, dirty, descs, index, ot.IDX_U8, array_align=1), cu.Source(hip, table, descs, index, ot.IDX_U16, array_align=16)]
    try:
        a = rt.reorient_and_check(dll, hip, baker, srcs[0], orient)
        b = rt.reorient_and_check(dll, hip, baker, srcs[1], orient)
        cu.assert_same(a, b)
        assert a["info"]["referencedBlocks"] == 48 and a["info"]["uniformBlocks"] == 36 and a["info"]["descArrayCount"] >= 4
        kept = rt.reorient_and_check(dll, hip, baker, srcs[0], orient, flags=rt.NO_SPECIAL | rt.NO_DEDUP)
        assert kept["info"]["descArrayCount"] == 48 and all(kept["array"][o] >> (f * 4 ** l) == 0 for o, l, f in kept["descs"].tolist() if f * 4 ** l < 8)
    finally:
        for s in srcs:
            s.close()


@pytest.mark.parametrize("array_align", [1, 4, 16, 256])
def test_a_block_that_ends_with_the_allocation(dll, hip, baker, array_align):
    """the array is the tail of its allocation and its last block ends with it: blocks of 1 byte, 8 and 16 bytes (one tile), 1 KiB and 16 KiB + an odd
    lead, under a rotation and a reflection"""
    for level, bits, lead in ((0, 2, 0), (3, 1, 1), (3, 2, 3), (6, 2, 7), (8, 2, 1)):
        blocks = [(random_states(2, 2, 3), 2, 2), (random_states(level, bits, 5), level, bits)]
        table = cu.table_of_blocks(blocks, first_offset=lead)
        assert table[1][-1, 0] + su.block_bytes(level, bits) == len(table[0])
        src = cu.Source(hip, *table, [1, 0, 1], ot.IDX_U32, array_align=array_align)
        try:
            ref = rt.reorient_and_check(dll, hip, baker, src, np.array([1, 5, 3], np.uint8), flags=rt.NO_SPECIAL)
            assert ref["info"]["descArrayCount"] == (3 if level else 2)
        finally:
            src.close()


# ---- orientations and items ----
def test_items_symmetry_and_a_near_twin(dll, hip, baker):
    """mixed orientations per primitive; one descriptor under all six; a block that is symmetric under reflection 3 merges with its orientation-0
    item and with nothing else; a twin that differs from the symmetric block's image in ONE field is kept"""
    level = 5
    s = random_states(level, 2, 77)
    m3 = rt.source_map(level, 3)
    sym = np.maximum(s, s[m3])
    near = sym.copy()
    near[-1] ^= 1
    blocks = [(random_states(level, 2, 78), level, 2), (sym, level, 2), (near, level, 2), (random_states(4, 1, 79), 4, 1)]
    index = [1, 1, 1, 1, 1, 1, 2, 2, 0, 3, 0, 3, -1, 0]
    orient = [0, 1, 2, 3, 4, 5, 0, 3, 1, 1, 4, 2, 5, 1]
    src = cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=9, gap=1), index, ot.IDX_U8, array_align=1)
    try:
        ref = rt.reorient_and_check(dll, hip, baker, src, np.array(orient, np.uint8))
        info = ref["info"]
        assert info["referencedBlocks"] == 12 and info["reorientedBlocks"] == 10 and info["uniformBlocks"] == 0
        # of the symmetric block's six items: 3 == 0, and the images under 1, 2 pair up with those under the other reflections (o then 3)
        assert info["duplicateBlocks"] == 3 and ref["index"][0] == ref["index"][3] and ref["index"][6] != ref["index"][7] != ref["index"][0]
        assert ref["index"][8] == ref["index"][13] and ref["index"][12] == -1
        apart = rt.reorient_and_check(dll, hip, baker, src, np.array(orient, np.uint8), flags=rt.NO_DEDUP)
        assert apart["info"]["descArrayCount"] == 12 and apart["info"]["duplicateBlocks"] == 0
    finally:
        src.close()


# ---- specials and skipping ----
def test_uniform_blocks_specials_and_orientation_bytes(dll, hip, baker):
    """uniform blocks are promoted under every orientation (and kept with DisableSpecialIndices, where all their orientations merge); special entries
    pass through under every valid orientation; orientation bytes 6 and 255 skip the primitive, whatever its entry"""
    blocks = [(np.full(4 ** 4, 2, np.uint8), 4, 2), (np.ones(4 ** 6, np.uint8), 6, 1), (random_states(4, 2, 5), 4, 2)]
    index = [0, 0, 1, 1, 2, 2, -1, -2, -3, -4, -1, 2, 0, -3]
    orient = [0, 4, 1, 5, 2, 2, 0, 1, 3, 5, 6, 255, 7, 128]
    src = cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=2), index, ot.IDX_U16)
    try:
        ref = rt.reorient_and_check(dll, hip, baker, src, np.array(orient, np.uint8))
        assert ref["index"].tolist() == [-3, -3, -2, -2, 0, 0, -1, -2, -3, -4, -4, -4, -4, -4]
        assert ref["info"]["skippedPrimitives"] == 4 and ref["info"]["uniformBlocks"] == 4 and ref["info"]["referencedBlocks"] == 5
        kept = rt.reorient_and_check(dll, hip, baker, src, np.array(orient, np.uint8), flags=rt.NO_SPECIAL)
        assert kept["info"]["descArrayCount"] == 3 and kept["info"]["duplicateBlocks"] == 2
    finally:
        src.close()


@pytest.mark.parametrize("index_format", FORMATS)
def test_bounds_table(dll, hip, baker, index_format):
    """lookup_util.bounds_table under mixed orientations: an entry below -4, an entry at or beyond descArrayCount, level 13, formats 0 and 3, a block
    one byte past arrayDataSize -- each is -4, counted once, and never read through: the arrays are followed by padding that looks valid
    (Source(declared=...)), so a kernel that reads past a declared size answers differently"""
    tb = lu.bounds_table(index_format)
    rows = [r for r in tb["rows"] if r[2]]
    index = [r[0] for r in rows] + [0] * 64
    descs = list(tb["descs"]) + [(0, 3, 2)] * 70000
    array_data = np.concatenate([tb["array"], np.full((4 << 20) + 64, 0x6D, np.uint8)])
    bad = cu.Source(hip, array_data, descs, index, index_format, array_align=16, declared=(len(tb["array"]), len(tb["descs"]), len(rows)))
    none = cu.Source(hip, array_data, descs, index, index_format, array_align=16, declared=(0, len(tb["descs"]), len(rows)))
    try:
        invalid = [i for i, r in enumerate(rows) if r[1] == lu.INVALID]
        orient = (np.arange(len(rows)) % 6).astype(np.uint8)
        ref = rt.reorient_and_check(dll, hip, baker, bad, orient, flags=rt.NO_SPECIAL)
        assert ref["info"]["skippedPrimitives"] == len(invalid) > 8 and (ref["index"][invalid] == -4).all() and ref["info"]["referencedBlocks"] >= 2
        for o in (0, 4):
            ref = rt.reorient_and_check(dll, hip, baker, bad, o)
            assert ref["info"]["skippedPrimitives"] == len(invalid)
        ref = rt.reorient_and_check(dll, hip, baker, none, orient)
        assert ref["info"]["skippedPrimitives"] == len(rows) - 4 and ref["info"]["referencedBlocks"] == 0      # arrayDataSize 0: only the specials remain
    finally:
        bad.close()
        none.close()


# ---- flags and streams ----
@pytest.fixture(scope="module")
def mixed_source(hip):
    rng = np.random.default_rng(80)
    blocks = [(random_states(level, 1 + level % 2, 500), level, 1 + level % 2) for level in range(1, 8)]
    blocks += [blocks[4], (np.full(64, 3, np.uint8), 3, 2)]
    src = cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=3, gap=1), np.concatenate([np.arange(9), rng.integers(-4, 9, 91)]), ot.IDX_U16, array_align=1)
    yield src, rng.integers(0, 6, 100).astype(np.uint8)
    src.close()


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_flags(dll, hip, baker, mixed_source, flags):
    """both flags and their combination, with mixed orientations and with one orientation through the desc"""
    src, orient = mixed_source
    ref = rt.reorient_and_check(dll, hip, baker, src, orient, flags=flags)
    assert ref["info"]["referencedBlocks"] > 30 and (flags & 2 or ref["info"]["duplicateBlocks"] >= 1)
    one = rt.reorient_and_check(dll, hip, baker, src, 2, flags=flags)
    assert one["info"]["referencedBlocks"] == one["info"]["reorientedBlocks"] == 9


def test_many_primitives_on_a_stream(dll, hip, baker):
    """4000 descriptors and 2^17 + 17 primitives with random orientation bytes 0..6 on a caller's stream: every per-primitive and per-item kernel
    over many workgroups; two calls return the same bytes"""
    rng = np.random.default_rng(8)
    protos = [(cu.planted_states(level, bits, seed), level, bits) for level in range(6) for bits in (1, 2) for seed in range(8)]
    table, pdescs = cu.table_of_blocks(protos, first_offset=2, gap=1)
    n = (1 << 17) + 17
    src = cu.Source(hip, table, pdescs[rng.integers(0, len(protos), 4000)], rng.integers(-6, 4002, n), ot.IDX_U32, array_align=1)
    orient = rng.integers(0, 7, n).astype(np.uint8)
    stream = hip.stream_create(non_blocking=True)
    try:
        ref, h1 = rt.reorient_and_check(dll, hip, baker, src, orient, stream=stream, keep=True)
        try:
            assert ref["info"]["duplicateBlocks"] > 10000 and ref["info"]["skippedPrimitives"] > n // 8 and ref["info"]["referencedBlocks"] > 20000
            d_o = hip.upload(orient)
            r, info, h2 = rt.reorient(dll, baker, src.rd, d_o)
            hip.free(d_o)
            assert (r, info) == (ot.SUCCESS, ref["info"])
            try:
                cu.assert_same(cu.download_result(dll, hip, h2), cu.download_result(dll, hip, h1))
            finally:
                destroy(dll, [h2])
        finally:
            destroy(dll, [h1])
    finally:
        hip.stream_destroy(stream)
        src.close()


# ---- cross-checks that do not use the model ----
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_orientation_0_equals_a_coarsening_that_keeps_every_level(dll, hip, baker, flags):
    """orientation 0 through the desc against ommxCoarsenMicromap at cap 12 with the same flags, both on the device: arrayData, descArray, the index
    values, the histograms and the shared info fields are equal"""
    blocks = [(random_states(level, 1 + level % 2, 70), level, 1 + level % 2) for level in range(10)]
    blocks += [blocks[5], (np.ones(4 ** 4, np.uint8), 4, 2)]
    array_data, descs = cu.table_of_blocks(blocks, first_offset=3, gap=1)
    descs = np.concatenate([descs, [(len(array_data) - 1, 3, 2)]])                        # descriptor 12: its block ends behind the array
    index = list(range(13)) + [-1, -2, -3, -4, 10, 3, 5, -7, 11, 0, 9, 12]
    src = cu.Source(hip, array_data, descs, index, ot.IDX_U8, array_align=1)
    made = []
    try:
        r, coarse_info, coarse = cu.coarsen(dll, baker, src.rd, 12, 3, flags)
        assert r == ot.SUCCESS
        made.append(coarse)
        r, info, turned = rt.reorient(dll, baker, src.rd, None, 0, flags)
        assert r == ot.SUCCESS
        made.append(turned)
        a, b = cu.download_result(dll, hip, coarse), cu.download_result(dll, hip, turned)
        assert (a["index_format"], b["index_format"]) == (ot.IDX_U8, ot.IDX_U32)
        assert np.array_equal(a["array"], b["array"]) and np.array_equal(a["descs"], b["descs"]) and len(a["descs"]) >= 9
        assert np.array_equal(a["index"].astype(np.int64), b["index"].astype(np.int64))
        assert a["array_hist"] == b["array_hist"] and a["index_hist"] == b["index_hist"]
        for field in ("descArrayCount", "arrayDataSize", "referencedBlocks", "uniformBlocks", "duplicateBlocks", "skippedPrimitives"):
            assert coarse_info[field] == info[field], field
        assert info["skippedPrimitives"] == 3 and info["reorientedBlocks"] == 0
    finally:
        destroy(dll, made)
        src.close()


def test_lookups_inverses_and_the_other_entries(dll, hip, baker, mixed_source):
    """without the model: ommxLookupOpacity on the output at centroids equals the lookup on the source at the permuted barycentrics, with Force2State
    off and on; o then its inverse decodes to the source's states per primitive; ommxDebugGetStatsDevice totals are equal before and after; two
    calls give the same bytes; geometry, coarsen, combine, gather, fit and this entry accept the output"""
    src, orient = mixed_source
    a, d, index = src.host
    rng = np.random.default_rng(90)
    made = []
    d_o = hip.upload(orient)
    d_back = hip.upload(np.array(rt.INVERSE, np.uint8)[orient])
    try:
        r, info, h = rt.reorient(dll, baker, src.rd, d_o)
        assert r == ot.SUCCESS and info["skippedPrimitives"] == 0
        made.append(h)
        out = cu.download_result(dll, hip, h)
        levels = np.array([d[e, 1] if e >= 0 else 0 for e in index.tolist()], np.int64)
        prims = np.arange(len(index), dtype=np.uint32)
        for flags in (0, 1):                                                              # ommxLookupFlags_Force2State
            for _ in range(4):
                micro = (rng.random(len(prims)) * (4.0 ** levels)).astype(np.int64)
                u, v = lu.centroid_points(lu.micro_vertices(micro, levels))
                new = np.stack([np.float32(1) - u - v, u, v], 1)
                old = np.zeros_like(new)
                for o in range(6):
                    rows = orient == o
                    for k in range(3):
                        old[rows, rt.PERMS[o][k]] = new[rows, k]
                hits, theirs = np.empty(len(prims), lu.HIT), np.empty(len(prims), lu.HIT)
                hits["prim"], hits["u"], hits["v"] = prims, u, v
                theirs["prim"], theirs["u"], theirs["v"] = prims, old[:, 1], old[:, 2]
                got = lu.lookup_device(dll, hip, out["rdesc"], hits, flags)
                assert np.array_equal(got, lu.lookup_device(dll, hip, src.rd, theirs, flags)), flags
                assert (got < 4).all() and (flags == 0 or (got < 2).all())
        # there and back
        r, info_back, hb = rt.reorient(dll, baker, out["rdesc"], d_back)
        assert r == ot.SUCCESS and info_back["skippedPrimitives"] == 0
        made.append(hb)
        r, _, h0 = rt.reorient(dll, baker, src.rd, None, 0)
        assert r == ot.SUCCESS
        made.append(h0)
        assert per_primitive_states(cu.download_result(dll, hip, hb)) == per_primitive_states(cu.download_result(dll, hip, h0))
        # a permutation keeps the totals of the statistics: those of the source when no block is promoted to a special index (the source holds a
        # uniform block as a block), and those of the orientation-0 output, which promotes the same blocks, with default flags
        r, _, hk = rt.reorient(dll, baker, src.rd, d_o, flags=rt.NO_SPECIAL)
        assert r == ot.SUCCESS
        made.append(hk)
        assert cu.device_stats(dll, baker, cu.result_desc_of(dll, hk)) == cu.device_stats(dll, baker, src.rd)
        assert cu.device_stats(dll, baker, out["rdesc"]) == cu.device_stats(dll, baker, cu.result_desc_of(dll, h0))
        # purity
        r, info2, h2 = rt.reorient(dll, baker, src.rd, d_o)
        assert r == ot.SUCCESS and info2 == info
        made.append(h2)
        cu.assert_same(cu.download_result(dll, hip, h2), out)
        # the other entries accept it
        counts, skipped = (C.c_uint64 * 4)(), C.c_uint32(7)
        assert dll.ommxExtractMicroGeometry(baker, C.byref(out["rdesc"]), C.byref(gu.c_desc(gu.IDENTITY)), None, counts, C.byref(skipped), None) == ot.SUCCESS
        assert sum(counts) > 0 and skipped.value == 0
        r, cinfo, hc = cu.coarsen(dll, baker, out["rdesc"], 2, 3)
        assert r == ot.SUCCESS and cinfo["coarsenedBlocks"] > 0 and cinfo["skippedPrimitives"] == 0
        made.append(hc)
        r, minfo, hm = mu.combine(dll, baker, [out["rdesc"], out["rdesc"]], 2, 3)
        assert r == ot.SUCCESS and minfo["skippedPrimitives"] == 0 and minfo["combinedTuples"] == info["descArrayCount"]
        made.append(hm)
        r, ginfo, hg = gt.gather(dll, baker, [out["rdesc"]])
        assert r == ot.SUCCESS and ginfo["descArrayCount"] == info["descArrayCount"] and ginfo["skippedPrimitives"] == 0
        made.append(hg)
        cu.assert_same(cu.download_result(dll, hip, hg), out)
        r, finfo, _, hf = fu.fit(dll, hip, baker, out["rdesc"], info["arrayDataSize"] // 2)
        assert r == ot.SUCCESS and finfo["result"]["arrayDataSize"] <= info["arrayDataSize"] // 2
        made.append(hf)
    finally:
        hip.free(d_o)
        hip.free(d_back)
        destroy(dll, [h for h in made if h is not None])


# ---- a real bake ----
def test_a_real_bake(product, dll, hip):
    """one small ommxBakeDevice result (tests/workloads.py: 300 triangles over value noise, baked at level 5) with random orientations equals the
    model, on a caller's stream and on the null stream"""
    b = product.create_baker()
    stream = hip.stream_create(non_blocking=True)
    tex = bake = None
    made = []
    try:
        t, uv, ix, lv, kw = wl.workload("c1", 300)
        level = min(kw.pop("level"), 5)
        tex = product.create_texture(b, [t], alpha_cutoff=0.5)
        bake = lu.DeviceBake(product, hip, b, ot.make_desc(tex, uv, ix, level, levels=lv, **kw), uv, ix, lv)
        host = (bake.host.array_data, bake.host.descs, bake.host.index, None)
        every = np.asarray(bake.host.index)
        assert len(every) == 300 and (every >= 0).any() and int(np.asarray(bake.host.descs)[:, 1].max()) <= 5
        orient = np.random.default_rng(4).integers(0, 6, len(every)).astype(np.uint8)
        ref = rt.restate_reorient(host, orient)
        d_o = hip.upload(orient)
        try:
            for s in (stream, None):
                r, info, h = rt.reorient(dll, b, bake.rdesc, d_o, want_result=False, stream=s)
                assert (r, info, h) == (ot.SUCCESS, ref["info"], None)
                r, info, h = rt.reorient(dll, b, bake.rdesc, d_o, stream=s)
                assert r == ot.SUCCESS
                made.append(h)
                rt.check_result(dll, hip, b, h, info, ref)
                assert info["skippedPrimitives"] == 0 and info["reorientedBlocks"] > 0
        finally:
            hip.free(d_o)
    finally:
        hip.stream_destroy(stream)
        destroy(dll, made)
        if bake is not None:
            bake.close()
        if tex is not None:
            product.destroy_texture(b, tex)
        product.destroy_baker(b)
