"""ommxCoarsenMicromap on the GPU.  Every case compares arrayData, descArray, the index buffer, both histograms (as mappings) and the info fields with
tests/coarsen_util.py's restate_coarsen byte for byte -- there is no tolerance anywhere.  The shapes are the tier edges of the reduction (a lane's 256
micro-triangles, part of a wave, a workgroup's unit of 4^8, several units, the second pass of a deep block), not a workload."""
import ctypes as C
import types
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import kat_cases
import kat_runner

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("bits,mixed", [(1, 2), (1, 3), (2, 2), (2, 3)], ids=["2state_ut", "2state_uo", "4state_ut", "4state_uo"])


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    return cu.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


# ---- every tier edge ----
@BOTH
def test_every_level_pair_up_to_9(dll, hip, baker, bits, mixed):
    """one block per source level 0..9, coarsened to every level 0..9 (blocks at or below the cap pass through): random states with planted uniform and
    one-sided regions at every scale, so known, leaning and mixed outcomes occur at every level of the cross-lane and cross-wave combine.  With default
    flags (blocks that turn uniform are promoted) and with both flags disabled (every block's bytes are compared)."""
    blocks = [(cu.planted_states(level, bits, seed=3), level, bits) for level in range(10)]
    array_data, descs = cu.table_of_blocks(blocks)
    src = cu.Source(hip, array_data, descs, list(range(10)), ot.IDX_U8, array_align=16)
    try:
        seen = set()
        for cap in range(10):
            ref = cu.coarsen_and_check(dll, hip, baker, src, cap, mixed, cu.NO_SPECIAL | cu.NO_DEDUP)
            assert ref["info"]["descArrayCount"] == 10 and ref["info"]["coarsenedBlocks"] == 9 - cap
            for d, (o, l, f) in enumerate(ref["descs"]):
                seen |= set(cu.block_states(ref["array"], int(o), int(l), int(f)).tolist())
            cu.coarsen_and_check(dll, hip, baker, src, cap, mixed)
        assert seen == ({0, 1} if bits == 1 else {0, 1, 2, 3})
    finally:
        src.close()


@pytest.mark.parametrize("caps", [range(0, 7), range(7, 13)], ids=["to_0_6", "to_7_12"])
@BOTH
def test_level_12(dll, hip, baker, bits, mixed, caps):
    """a level-12 block (4 MiB in the 4-state format: 256 units, and a second pass below level 7) to every level 0..12, beside a level-10 block"""
    blocks = [(cu.planted_states(12, bits, seed=5), 12, bits), (cu.planted_states(10, bits, seed=6), 10, bits)]
    array_data, descs = cu.table_of_blocks(blocks)
    src = cu.Source(hip, array_data, descs, [0, 1, 0], ot.IDX_U32, array_align=256)
    try:
        for cap in caps:
            ref = cu.coarsen_and_check(dll, hip, baker, src, cap, mixed, cu.NO_SPECIAL | cu.NO_DEDUP)
            assert ref["info"]["descArrayCount"] == 2 and ref["descs"][0, 1] == cap
    finally:
        src.close()


# ---- odd byte offsets ----
@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32])
def test_statistics_table(dll, hip, baker, index_format):
    """stats_util's table: levels 0 - 3 in both formats at odd offsets with random bytes (garbage in the unused bits of the one-byte blocks), a level-7 and a
    level-9 block at odd addresses, level 13, formats 0 and 3, a block one byte past the array, the specials, -5 and descArrayCount, a block three times"""
    array_data, descs, index, _ = su.table_arrays()
    src = cu.Source(hip, array_data, descs, index, index_format, array_align=1)
    try:
        for cap, mixed, flags in ((0, 3, cu.NONE), (1, 2, cu.NO_SPECIAL), (2, 3, cu.NONE), (3, 2, cu.NO_DEDUP), (5, 3, cu.NONE), (8, 2, cu.NONE), (12, 3, cu.NONE), (0xFFFFFFFF, 2, cu.NO_SPECIAL)):
            ref = cu.coarsen_and_check(dll, hip, baker, src, cap, mixed, flags)
            assert ref["info"]["skippedPrimitives"] == 8 and ref["info"]["referencedBlocks"] == 9
            assert [int(x) for x in ref["index"][[0, 2, 4, 6]]] == [-1, -2, -3, -4]                  # source specials pass through
            assert all(int(ref["index"][i]) == -4 for i in (8, 9, 12, 14, 16, 18, 23, 24))           # the skipped primitives
    finally:
        src.close()


@BOTH
def test_large_blocks_at_odd_addresses(dll, hip, baker, bits, mixed):
    """level-8 and level-9 blocks at offset % 16 of 3 and 8, and one-byte blocks (levels 0 and 1) whose unused bits are set: ignored on input, zero on output"""
    blocks = [(cu.planted_states(level, bits, seed=level), level, bits) for level in (8, 0, 9, 1, 1, 0)]
    for first, gap in ((3, 0), (8, 16)):
        array_data, descs = cu.table_of_blocks(blocks, first_offset=first, gap=gap, filler=0xFF)
        for d in (1, 3, 4, 5):                     # garbage above the fields of the one-byte blocks
            array_data[descs[d, 0]] |= (0xFF << (bits * 4 ** int(descs[d, 1]))) & 0xFF
        src = cu.Source(hip, array_data, descs, [0, 1, 2, 3, 4, 5], ot.IDX_U16, array_align=16)
        try:
            for cap in (0, 1, 3, 4, 7, 8, 12):
                ref = cu.coarsen_and_check(dll, hip, baker, src, cap, mixed, cu.NO_SPECIAL | cu.NO_DEDUP)
                small = ref["descs"][ref["descs"][:, 1] <= 1]
                assert len(small) >= 4 and all(ref["array"][o] >> (f * 4 ** l) == 0 for o, l, f in small.tolist())
        finally:
            src.close()


# ---- promotion ----
def test_promotion(dll, hip, baker):
    """blocks that become uniform only after coarsening, for each of the four states (0 and 1 through the 2-state format's mixed rule, 2 and 3 through one
    side with unknowns), blocks uniform at L <= T, the same with DisableSpecialIndices, and maxSubdivisionLevel 0: no descriptors at all"""
    n = 4 ** 3
    half = np.arange(n) % 2
    blocks = [(half.astype(np.uint8), 3, 1),                       # 0: 2-state, both sides -> mixedState & 1
              ((2 * half).astype(np.uint8), 3, 2),                 # 1: T and UT -> UT everywhere
              ((1 + 2 * half).astype(np.uint8), 3, 2),             # 2: O and UO -> UO everywhere
              (np.full(16, 1, np.uint8), 2, 2),                    # 3: uniform O at level 2
              (np.full(16, 0, np.uint8), 2, 1),                    # 4: uniform T at level 2, 2-state
              (np.full(1, 3, np.uint8), 0, 2),                     # 5: level 0
              ((np.arange(n) // 16).astype(np.uint8), 3, 2)]       # 6: four quarters: stays a block down to level 1
    array_data, descs = cu.table_of_blocks(blocks, first_offset=1, gap=1)
    index = [0, 1, 2, 3, 4, 5, 6, -3, 1]
    src = cu.Source(hip, array_data, descs, index, ot.IDX_U8, array_align=1)
    try:
        for mixed in (2, 3):
            ref = cu.coarsen_and_check(dll, hip, baker, src, 2, mixed)
            assert ref["index"].tolist() == [-1 - (mixed & 1), -3, -4, -2, -1, -4, 0, -3, -3] and ref["info"]["uniformBlocks"] == 6
            ref = cu.coarsen_and_check(dll, hip, baker, src, 3, mixed)           # nothing is coarsened: only the blocks uniform as they are
            assert ref["index"].tolist()[3:6] == [-2, -1, -4] and ref["info"]["uniformBlocks"] == 3 and ref["info"]["coarsenedBlocks"] == 0
            ref = cu.coarsen_and_check(dll, hip, baker, src, 2, mixed, cu.NO_SPECIAL)
            assert ref["info"]["uniformBlocks"] == 6 and (ref["index"][:7] >= 0).all() and ref["index"][7] == -3
            ref = cu.coarsen_and_check(dll, hip, baker, src, 0, mixed)
            assert ref["info"]["descArrayCount"] == 0 and ref["info"]["arrayDataSize"] == 0 and (ref["index"] < 0).all()
            r, info, handle = cu.coarsen(dll, baker, src.rd, 0, mixed)
            rd = cu.result_desc_of(dll, handle)
            assert r == ot.SUCCESS and not rd.arrayData and rd.arrayDataSize == 0 and rd.descArrayCount == 0 and rd.indexBuffer and rd.indexCount == len(index)
            assert cu.device_stats(dll, baker, rd)[1] == 0
            assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
    finally:
        src.close()


# ---- duplicates ----
def test_duplicates(dll, hip, baker):
    """two different source blocks that are equal after coarsening (the representative is the lower source index), equal bytes at another level or in
    another format are not merged, a block selected by many primitives is reduced once, an unreferenced block is dropped; the same with detection off"""
    a = cu.planted_states(4, 2, 21)
    fine1, fine2 = np.repeat(a, 4), np.repeat(a, 4)          # level 5: both equal to `a` at level 4 ...
    j = int(np.nonzero(a >= 2)[0][0])
    fine2[4 * j + 1] &= 1                                    # ... and different at level 5: one known micro-triangle in a group that stays unknown
    one_byte = np.array([1, 0, 1, 1], np.uint8)              # level 1, 2-state: byte 0x0D
    same_byte = np.array([1, 3, 0, 0], np.uint8)             # level 1, 4-state: byte 0x0D
    blocks = [(cu.planted_states(6, 2, 1), 6, 2),            # 0: unreferenced
              (fine2, 5, 2), (a, 4, 2), (fine1, 5, 2),       # 1, 2, 3: one class at level 4
              (one_byte, 1, 1), (same_byte, 1, 2),           # 4, 5: equal bytes, another format
              (np.repeat(same_byte, 4), 2, 2)]               # 6: level 2; at level 1 equal to block 5
    assert lu.pack(one_byte, 1)[0] == lu.pack(same_byte, 2)[0] == 0x0D and not np.array_equal(fine1, fine2)
    array_data, descs = cu.table_of_blocks(blocks, gap=3)
    index = [3, 2, 1] + [2] * 300 + [4, 5, 6, 3, -2]
    src = cu.Source(hip, array_data, descs, index, ot.IDX_U16, array_align=16)
    try:
        ref = cu.coarsen_and_check(dll, hip, baker, src, 4)
        assert ref["info"]["referencedBlocks"] == 6 and ref["info"]["duplicateBlocks"] == 2 and ref["info"]["descArrayCount"] == 4
        assert ref["index"][0] == ref["index"][1] == ref["index"][2] == 0 and ref["descs"][0].tolist() == [0, 4, 2]     # the class of blocks 1, 2, 3
        assert np.array_equal(ref["array"][:64], lu.pack(a, 2))
        ref = cu.coarsen_and_check(dll, hip, baker, src, 5)
        assert ref["info"]["duplicateBlocks"] == 0 and ref["info"]["descArrayCount"] == 6
        ref = cu.coarsen_and_check(dll, hip, baker, src, 1)
        assert ref["index"][303] != ref["index"][304] and ref["index"][304] == ref["index"][305]       # 4 vs 5: formats differ; 5 and 6: merged
        ref = cu.coarsen_and_check(dll, hip, baker, src, 4, flags=cu.NO_DEDUP)
        assert ref["info"]["duplicateBlocks"] == 0 and ref["info"]["descArrayCount"] == 6 and len(set(ref["index"][:3].tolist())) == 3
        assert (ref["index"][3:303] == ref["index"][1]).all()                                          # selected by many primitives: one block
    finally:
        src.close()


def test_many_blocks(dll, hip, baker):
    """20 000 descriptors of levels 0..5 in both formats with many equal blocks, 2^17 + 17 primitives, a caller's stream: every per-descriptor and
    per-primitive kernel over many workgroups, every size class in the partition, 16-bit entries above 127"""
    rng = np.random.default_rng(8)
    protos = [(cu.planted_states(level, bits, seed), level, bits) for level in range(6) for bits in (1, 2) for seed in range(12)]
    table, pdescs = cu.table_of_blocks(protos, first_offset=2, gap=1)
    descs = pdescs[rng.integers(0, len(protos), 20000)]
    index = rng.integers(-6, 20002, (1 << 17) + 17)
    src = cu.Source(hip, table, descs, index, ot.IDX_U32, array_align=1)
    stream = hip.stream_create(non_blocking=True)
    try:
        ref = cu.coarsen_and_check(dll, hip, baker, src, 3, 3, stream=stream)
        assert ref["info"]["duplicateBlocks"] > 5000 and 20 < ref["info"]["descArrayCount"] <= len(protos)
        ref = cu.coarsen_and_check(dll, hip, baker, src, 12, 2, cu.NO_DEDUP, stream=stream)
        assert ref["info"]["descArrayCount"] > 5000 and ref["info"]["skippedPrimitives"] > 0
    finally:
        hip.stream_destroy(stream)
        src.close()
    small = cu.Source(hip, table, pdescs, np.arange(len(protos))[::-1], ot.IDX_U16, array_align=16)     # 144 descriptors: entries above 127 in 16 bits
    try:
        ref = cu.coarsen_and_check(dll, hip, baker, small, 12, 3, cu.NO_SPECIAL | cu.NO_DEDUP)
        assert ref["index"].max() == len(protos) - 1 > 127
    finally:
        small.close()


# ---- the bounds rule ----
@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32])
def test_bounds_table(dll, hip, baker, index_format):
    """lookup_util.bounds_table: malformed descriptors are skipped and never read through -- the three arrays are followed by padding that looks valid
    (index entries 0, descriptors of a valid block, state bytes), so a kernel that reads past a declared size answers differently"""
    tb = lu.bounds_table(index_format)
    rows = [r for r in tb["rows"] if r[2]]
    index = [r[0] for r in rows] + [0] * 64
    descs = list(tb["descs"]) + [(0, 3, 2)] * 70000
    array_data = np.concatenate([tb["array"], np.full((4 << 20) + 64, 0x6D, np.uint8)])
    src = cu.Source(hip, array_data, descs, index, index_format, array_align=16, declared=(len(tb["array"]), len(tb["descs"]), len(rows)))
    try:
        invalid = [i for i, r in enumerate(rows) if r[1] == lu.INVALID]
        for cap in (0, 2, 3):
            ref = cu.coarsen_and_check(dll, hip, baker, src, cap, 2, cu.NO_SPECIAL)
            assert ref["info"]["skippedPrimitives"] == len(invalid) > 8 and (ref["index"][invalid] == -4).all() and ref["info"]["referencedBlocks"] == 2
    finally:
        src.close()
    none = cu.Source(hip, array_data, descs, index, index_format, array_align=16, declared=(0, len(tb["descs"]), len(rows)))
    try:
        ref = cu.coarsen_and_check(dll, hip, baker, none, 3, 3)
        assert ref["info"]["skippedPrimitives"] == len(rows) - 4 and ref["info"]["referencedBlocks"] == 0      # arrayDataSize 0: only the specials remain
    finally:
        none.close()


# ---- info-only, determinism ----
def test_info_only_and_two_calls(dll, hip, baker):
    """the info-only call returns the full call's info (and no handle); two full calls return identical bytes; with default flags
    referencedBlocks == descArrayCount + uniformBlocks + duplicateBlocks"""
    rng = np.random.default_rng(4)
    protos = [(cu.planted_states(level, 2, seed), level, 2) for level in (2, 5, 7, 8) for seed in range(5)]
    table, pdescs = cu.table_of_blocks(protos)
    descs = pdescs[rng.integers(0, len(protos), 300)]
    src = cu.Source(hip, table, descs, rng.integers(-4, 300, 5000), ot.IDX_U16)
    try:
        for cap in (1, 4, 6):
            r0, info0, none = cu.coarsen(dll, baker, src.rd, cap, want_result=False)
            r1, info1, h1 = cu.coarsen(dll, baker, src.rd, cap)
            r2, info2, h2 = cu.coarsen(dll, baker, src.rd, cap)
            assert (r0, r1, r2) == (ot.SUCCESS,) * 3 and none is None and info0 == info1 == info2 == src.model(cap)["info"]
            assert info0["referencedBlocks"] == info0["descArrayCount"] + info0["uniformBlocks"] + info0["duplicateBlocks"]
            a, b = cu.download_result(dll, hip, h1), cu.download_result(dll, hip, h2)
            cu.assert_same(a, b)
            assert dll.ommxDestroyDeviceBakeResult(h1) == ot.SUCCESS and dll.ommxDestroyDeviceBakeResult(h2) == ot.SUCCESS
    finally:
        src.close()


# ---- real bakes ----
def _host_view(ref):
    return types.SimpleNamespace(array_data=ref["array"], descs=ref["descs"], index=ref["index"])


def _hits(rng, res, count):
    """random interior hits at each primitive's own level -> (HIT array, primitives, micro-triangle indices)"""
    plevel, _ = lu.prim_levels(res)
    prims = rng.integers(0, len(res.index), count)
    micro = (rng.random(count) * (4.0 ** plevel[prims])).astype(np.int64)
    u, v = lu.interior_points(rng, lu.micro_vertices(micro, plevel[prims]))
    hits = np.empty(count, lu.HIT)
    hits["prim"], hits["u"], hits["v"] = prims, u, v
    return hits, prims, micro


@pytest.mark.parametrize("fmt", [ot.FMT_2STATE, ot.FMT_4STATE], ids=["2state", "4state"])
@pytest.mark.parametrize("name,level", [("Mandelbrot", 7), ("Mandelbrot3", 9)])
def test_real_bakes(product, dll, hip, name, level, fmt):
    """ommxBakeDevice of a known-answer case's texture and geometry (tests/kat_cases.py) at level 7 / 9.  For every maxSubdivisionLevel down to 0: the
    output equals the model from the downloaded source; ommxLookupOpacity on it answers the model's state at random hits; ommxDebugGetStatsDevice on it
    equals numpy counts of the model.  At level 12 every lookup equals the source's.  Two chained calls equal one call at the lower level."""
    c = next(k for k in kat_cases.CASES if k["name"] == name)
    b = product.create_baker()
    tex = product.create_texture(b, [kat_runner.texture_array(c["tex"], c["size"], c["param"])])
    uv, ix = np.array(c["uv"], np.float32), np.array(c["ix"], np.uint32)
    rng = np.random.default_rng(level)
    try:
        d = ot.make_desc(tex, uv, ix, level, fmt=fmt, promo=ot.PROMO_NEAREST)
        bake = lu.DeviceBake(product, hip, b, d, uv, ix)
        try:
            res = bake.host
            assert len(res.descs) >= 1 and (res.descs[:, 1] == level).all()
            src_hits, src_prims, src_micro = _hits(rng, res, 20000)
            src_states = lu.lookup_device(dll, hip, bake.rdesc, src_hits)
            assert np.array_equal(src_states, lu.numpy_states(res, src_prims, src_micro))
            for cap in list(range(level + 1)) + [12]:
                ref = cu.restate_coarsen(res.array_data, res.descs, res.index, res.index_format, cap, 3)
                r, info, handle = cu.coarsen(dll, b, bake.rdesc, cap, 3)
                assert (r, info) == (ot.SUCCESS, ref["info"]), (cap, r, info, ref["info"])
                try:
                    got = cu.download_result(dll, hip, handle)
                    cu.assert_same(got, ref)
                    view = _host_view(ref)
                    hits, prims, micro = _hits(rng, view, 20000)
                    assert np.array_equal(lu.lookup_device(dll, hip, got["rdesc"], hits), lu.numpy_states(view, prims, micro))
                    want = su.reference_stats(ref["array"], ref["descs"], ref["index"])
                    assert cu.device_stats(dll, b, got["rdesc"]) == (want["fields"], 0)
                    if cap == 12:
                        assert np.array_equal(lu.lookup_device(dll, hip, got["rdesc"], src_hits), src_states)
                finally:
                    assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
            # a then b == min(a, b), mixedState 3 throughout
            for first, second in ((level - 1, 2), (3, level - 2), (4, 4)):
                r, _, h1 = cu.coarsen(dll, b, bake.rdesc, first, 3)
                assert r == ot.SUCCESS
                r, info2, h2 = cu.coarsen(dll, b, cu.result_desc_of(dll, h1), second, 3)
                assert r == ot.SUCCESS
                r, info3, h3 = cu.coarsen(dll, b, bake.rdesc, min(first, second), 3)
                assert r == ot.SUCCESS
                try:
                    assert (info2["arrayDataSize"], info2["descArrayCount"]) == (info3["arrayDataSize"], info3["descArrayCount"])
                    once = cu.download_result(dll, hip, h3)
                    hits, _, _ = _hits(rng, _host_view(once), 20000)
                    assert np.array_equal(lu.lookup_device(dll, hip, cu.result_desc_of(dll, h2), hits), lu.lookup_device(dll, hip, once["rdesc"], hits))
                finally:
                    for h in (h1, h2, h3):
                        assert dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS
        finally:
            bake.close()
    finally:
        product.destroy_texture(b, tex)
        product.destroy_baker(b)


# ---- scale ----
def test_a_million_primitives(dll, hip, baker):
    """2^20 + 3 primitives over 60 000 descriptors (32-bit entries): what the index buffer selects does not depend on the level asked for or on the
    call -- every descriptor is selected, no primitive is skipped, and referencedBlocks is the number of distinct valid entries, call after call"""
    rng = np.random.default_rng(20)
    protos = [(cu.planted_states(level, bits, seed), level, bits) for level in range(5) for bits in (1, 2) for seed in range(20)]
    table, pdescs = cu.table_of_blocks(protos)
    D, T = 60000, (1 << 20) + 3
    descs = pdescs[rng.integers(0, len(protos), D)]
    index = np.concatenate([np.arange(D), rng.integers(-4, D, T - D)])
    rng.shuffle(index)
    src = cu.Source(hip, table, descs, index, ot.IDX_U32, array_align=16)
    try:
        ref = cu.coarsen_and_check(dll, hip, baker, src, 2, 3)
        assert ref["info"]["referencedBlocks"] == D and ref["info"]["skippedPrimitives"] == 0
        for cap in (0, 1, 3, 4, 2, 2):
            r, info, _ = cu.coarsen(dll, baker, src.rd, cap, 3, want_result=False)
            assert r == ot.SUCCESS and (info["referencedBlocks"], info["skippedPrimitives"]) == (D, 0), (cap, info)
            assert info["referencedBlocks"] == info["descArrayCount"] + info["uniformBlocks"] + info["duplicateBlocks"]
    finally:
        src.close()
