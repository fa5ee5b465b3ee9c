"""ommxGatherMicromaps on the GPU.  Every case compares arrayData, descArray, the index buffer, both histograms (as mappings) and the info fields with
tests/gather_util.py's restate_gather byte for byte, info-only and full -- there is no tolerance anywhere.  The shapes are the edges of the copy (a
block at every misalignment, below a vector, of one, two and many units, ending with its array), of the selection (the scan over up to 4096 sources
with empty ones among them, references beyond the sources, malformed entries) and of the wiring to the shared tail, not a workload."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import combine_util as mu
import gather_util as gt
import geometry_util as gu
import workloads as wl

pytestmark = pytest.mark.gpu

FORMATS = [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32]


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    gu.bind(product.dll)
    return gt.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def close_all(srcs):
    for s in {id(s): s for s in srcs}.values():
        s.close()


def mixed_states(level, bits, seed):
    """planted states that are not uniform (a level-0 block always is)"""
    return next(s for s in (cu.planted_states(level, bits, k) for k in range(seed, seed + 40)) if level == 0 or s.min() != s.max())


def per_primitive(r):
    """what each primitive of a result (model or download) reads: its special entry, or the level, format and bytes of its block"""
    blocks = [(int(l), int(f), r["array"][int(o):int(o) + max(1, 4 ** int(l) * int(f) // 8)].tobytes()) for o, l, f in r["descs"]]
    return [int(e) if e < 0 else blocks[int(e)] for e in r["index"]]


# ---- the copy ----
@pytest.fixture(scope="module")
def blocks_to_level_8():
    return [(mixed_states(level, bits, 100 + level), level, bits) for level in range(8, -1, -1) for bits in (2, 1)]


@pytest.mark.parametrize("misalignment", range(16))
def test_every_level_at_every_misalignment(dll, hip, baker, blocks_to_level_8, misalignment):
    """one block per level 8..0 in both formats, packed without gaps behind `misalignment` bytes: every block of 16 bytes and more lies at that
    misalignment (the array itself is 16-byte aligned), the smaller ones at whatever follows; the last block ends with the array, which ends the
    allocation.  No block is uniform and no two are equal, so every block comes out as it went in, in the order of the tail"""
    table = cu.table_of_blocks(blocks_to_level_8, first_offset=misalignment)
    assert all(o % 16 == misalignment for o, l, f in table[1].tolist() if f * 4 ** l >= 128)
    src = cu.Source(hip, *table, np.arange(len(blocks_to_level_8))[::-1], ot.IDX_U8, array_align=16)
    try:
        ref = gt.gather_and_check(dll, hip, baker, [src])
        assert ref["info"]["referencedBlocks"] == 18 and ref["info"]["uniformBlocks"] == 2 and ref["info"]["duplicateBlocks"] == 0   # (the two of level 0)
        assert ref["descs"][:, 1].tolist()[:4] == [8, 8, 7, 7] and len(ref["array"]) == len(table[0]) - misalignment - 2
    finally:
        src.close()


@pytest.fixture(scope="module")
def blocks_above_level_8():
    return [(mixed_states(12, 2, 7), 12, 2)] + [(mixed_states(level, bits, 200 + level), level, bits) for level in (11, 10, 9) for bits in (2, 1)]


@pytest.mark.parametrize("misalignment", [0, 5])
def test_levels_9_to_12(dll, hip, baker, blocks_above_level_8, misalignment):
    """blocks of many units (16 KiB each): level 12 in the 4-state format -- 256 units -- once, at an odd address; levels 9..11 in both formats at an
    aligned and at an odd address"""
    blocks = blocks_above_level_8[0 if misalignment else 1:]
    src = cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=misalignment), np.arange(len(blocks)), ot.IDX_U16, array_align=16)
    try:
        ref = gt.gather_and_check(dll, hip, baker, [src])
        assert ref["info"]["descArrayCount"] == len(blocks) and ref["descs"][0, 1] == (12 if misalignment else 11)
    finally:
        src.close()


@pytest.mark.parametrize("array_align", [1, 4, 16, 256])
def test_a_block_that_ends_with_the_allocation(dll, hip, baker, array_align):
    """the array is the tail of its allocation and its last block ends with it: blocks of 1 byte, 16 bytes, 1 KiB and 16 KiB + an odd lead"""
    for level, bits, lead in ((0, 2, 0), (3, 2, 3), (6, 2, 7), (8, 2, 1)):
        blocks = [(mixed_states(2, 2, 3), 2, 2), (mixed_states(level, bits, 5), level, bits)]
        table = cu.table_of_blocks(blocks, first_offset=lead)
        assert table[1][-1, 0] + su.block_bytes(level, bits) == len(table[0])
        src = cu.Source(hip, *table, [1, 0, 1], ot.IDX_U32, array_align=array_align)
        try:
            ref = gt.gather_and_check(dll, hip, baker, [src], flags=gt.NO_SPECIAL)
            assert ref["info"]["descArrayCount"] == 2
        finally:
            src.close()


def test_one_byte_blocks_with_garbage(dll, hip, baker):
    """levels 0 and 1 (and level 1 in the 4-state format, whose byte is full) with ones in the unused bits of their byte: they merge with their clean
    twin in another source, they are promoted when their used bits are uniform, and the output byte has zeros in the unused bits"""
    shapes = [(0, 1), (0, 2), (1, 1), (1, 2)]
    clean = [(np.array(s, np.uint8), l, b) for (l, b), s in zip(shapes, ([1], [2], [1, 0, 1, 1], [1, 3, 0, 2]))]
    uniform = [(np.full(4 ** l, 1, np.uint8), l, b) for l, b in shapes]
    table, descs = cu.table_of_blocks(clean + uniform, first_offset=5, gap=2)
    dirty = table.copy()
    for o, l, f in descs.tolist():
        dirty[o] |= (0xFF << (f * 4 ** l)) & 0xFF
    assert (dirty != table).sum() == 6                                                    # (the level-1 4-state bytes have no unused bits)
    index = list(range(8)) + [-2, 3]
    srcs = [cu.Source(hip, dirty, descs, index, ot.IDX_U8, array_align=1), cu.Source(hip, table, descs, index[::-1], ot.IDX_U16, array_align=16)]
    try:
        ref = gt.gather_and_check(dll, hip, baker, srcs)
        # of the 16 items the four of level 0 and the eight uniform ones are promoted; levels 1 of both formats stay: two blocks, two duplicates
        assert ref["info"]["referencedBlocks"] == 16 and ref["info"]["uniformBlocks"] == 12 and ref["info"]["duplicateBlocks"] == 2
        assert sorted(ref["array"].tolist()) == sorted([0x0D, 0x8D]) and ref["index"][:8].tolist() == [-2, -3, 0, 1, -2, -2, -2, -2]
        kept = gt.gather_and_check(dll, hip, baker, srcs, flags=gt.NO_SPECIAL)
        assert kept["info"]["descArrayCount"] == 7 and kept["info"]["duplicateBlocks"] == 9      # (the uniform level-0 2-state block is the clean one's twin)
        assert all(kept["array"][o] >> (f * 4 ** l) == 0 for o, l, f in kept["descs"].tolist())
        both = gt.gather_and_check(dll, hip, baker, srcs[:1], flags=gt.NO_SPECIAL | gt.NO_DEDUP)
        assert both["info"]["descArrayCount"] == 8 and all(both["array"][o] >> (f * 4 ** l) == 0 for o, l, f in both["descs"].tolist() if f * 4 ** l < 8)
    finally:
        close_all(srcs)


def test_one_two_and_many_units(dll, hip, baker):
    """blocks of one unit (16 KiB), two and sixteen: a twin that differs in ONE bit of the last word of the last unit is not merged; an equal twin at
    another misalignment in another source is -- the digest is summed over the units of a block, whichever workgroups took them"""
    shapes = [(8, 2), (9, 1), (10, 2)]
    blocks = [(mixed_states(l, b, 300 + l), l, b) for l, b in shapes]
    near = []
    for states, l, b in blocks:
        s = states.copy()
        s[-1] ^= 1                                                                        # the last field: the top bits of the last word
        near.append((s, l, b))
    srcs = [cu.Source(hip, *cu.table_of_blocks(blocks + near, first_offset=0), [0, 1, 2, 3, 4, 5], ot.IDX_U8, array_align=16),
            cu.Source(hip, *cu.table_of_blocks(blocks[::-1], first_offset=11, gap=3), [2, 1, 0], ot.IDX_U8, array_align=16)]
    try:
        ref = gt.gather_and_check(dll, hip, baker, srcs)
        assert ref["info"]["referencedBlocks"] == 9 and ref["info"]["duplicateBlocks"] == 3 and ref["info"]["descArrayCount"] == 6
        assert ref["index"].tolist() == [4, 2, 0, 5, 3, 1, 4, 2, 0] and ref["descs"][:, 1].tolist() == [10, 10, 9, 9, 8, 8]
        twin = gt.gather_and_check(dll, hip, baker, srcs[::-1])                           # the representative is the lower (source, descriptor)
        assert twin["index"].tolist() == [4, 2, 0, 4, 2, 0, 5, 3, 1]
    finally:
        close_all(srcs)


# ---- the selection ----
def tiny_sources(hip, rng, count, formats=FORMATS):
    """`count` distinct sources of 0..3 primitives over 1..3 blocks of levels 0..3; every fifth has no primitive, some have one"""
    pool = [(mixed_states(level, bits, 400 + 7 * j), level, bits) for level in range(4) for bits in (1, 2) for j in range(3)]
    srcs = []
    for k in range(count):
        blocks = [pool[int(j)] for j in rng.integers(0, len(pool), int(rng.integers(1, 4)))]
        T = 0 if k % 5 == 0 else 1 if k % 5 == 1 else int(rng.integers(2, 4))
        srcs.append(cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=k % 4, gap=k % 3), rng.integers(-4, len(blocks), T), formats[k % len(formats)],
                              array_align=16 if k % 2 else 1))
    return srcs


@pytest.mark.parametrize("count", [1, 2, 3, 17])
def test_the_concatenation_of_a_few_sources(dll, hip, baker, count):
    """the NULL selection over K = 1, 2, 3 and 17 sources with mixed 8/16/32-bit index formats: sources without primitives at the front, in the
    middle and at the end, sources of one primitive, a source given twice"""
    rng = np.random.default_rng(70 + count)
    body = tiny_sources(hip, rng, max(count - 5, 1))
    empty = cu.Source(hip, *cu.table_of_blocks([(mixed_states(2, 2, 1), 2, 2)]), [], ot.IDX_U16)
    big = cu.Source(hip, *cu.table_of_blocks([(mixed_states(l, 1 + l % 2, 9), l, 1 + l % 2) for l in range(7)], first_offset=9), rng.integers(-4, 7, 300), ot.IDX_U8)
    srcs = {1: [big], 2: [empty, big], 3: [big, empty, big]}.get(count) or [empty] + body[:8] + [empty, big] + body[8:] + [body[3], empty]
    srcs = srcs[:count] if count != 17 else srcs
    try:
        assert len(srcs) == count
        ref = gt.gather_and_check(dll, hip, baker, srcs)
        assert ref["info"]["primitiveCount"] == sum(s.rd.indexCount for s in srcs) >= 300
    finally:
        close_all(srcs + body + [empty, big])


def test_4096_sources(dll, hip, baker):
    """the most sources: 300 tiny ones given 4096 times in a seeded order, empty ones first and last; every equal block of the 4096 is one block"""
    rng = np.random.default_rng(75)
    distinct = tiny_sources(hip, rng, 300)
    order = rng.integers(0, 300, gt.MAX_SOURCES)
    order[[0, 1, -1]] = [0, 5, 10]                                                        # (every fifth has no primitive)
    srcs = [distinct[int(k)] for k in order]
    try:
        unpacked = {}
        ref = gt.gather_and_check(dll, hip, baker, srcs, unpacked=unpacked)
        assert ref["info"]["primitiveCount"] > 4096 and ref["info"]["descArrayCount"] <= 24 and ref["info"]["duplicateBlocks"] > 1000
        picks = np.stack([rng.integers(0, gt.MAX_SOURCES + 1, 5000), rng.integers(0, 4, 5000)], 1)
        ref = gt.gather_and_check(dll, hip, baker, srcs, picks.tolist(), unpacked=unpacked)
        assert ref["info"]["skippedPrimitives"] > 500 and ref["info"]["referencedBlocks"] > 500
        r, _, _ = gt.gather(dll, baker, [s.rd for s in srcs] + [srcs[0].rd], want_result=False)
        assert r == ot.INVALID_ARGUMENT                                                   # 4097
    finally:
        close_all(distinct)


@pytest.fixture(scope="module")
def three_sources(hip):
    rng = np.random.default_rng(80)
    made = []
    for k, fmt in enumerate(FORMATS):
        blocks = [(mixed_states(level, 1 + (level + k) % 2, 500 + 10 * k), level, 1 + (level + k) % 2) for level in range(1, 7)]
        blocks.append((np.full(64, k, np.uint8), 3, 2))                                   # uniform
        made.append(cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=3 * k, gap=k), np.concatenate([np.arange(7), rng.integers(-4, 7, 33)]), fmt,
                              array_align=1 if k == 1 else 16))
    yield made
    close_all(made)


def test_explicit_selections(dll, hip, baker, three_sources):
    """repeats, the reversed concatenation, a selection of specials only, and references that name no primitive: source == resultCount,
    primitive == indexCount, 0xFFFFFFFF in either field and in both -- each of those is -4 and counted once"""
    srcs = three_sources
    everything = [(k, p) for k in range(3) for p in range(40)]
    ref = gt.gather_and_check(dll, hip, baker, srcs, everything[::-1])
    forward = gt.gather_and_check(dll, hip, baker, srcs)
    assert per_primitive(ref) == per_primitive(forward)[::-1] and np.array_equal(ref["array"], forward["array"]) and ref["info"] == forward["info"]
    repeats = [(1, 5)] * 300 + [(0, 2), (1, 5), (2, 6), (0, 2)] * 10
    ref = gt.gather_and_check(dll, hip, baker, srcs, repeats)
    assert ref["info"]["referencedBlocks"] == 3 and ref["info"]["uniformBlocks"] == 1 and len(set(ref["index"][:300].tolist())) == 1
    specials = [(k, p) for k, s in enumerate(srcs) for p in np.nonzero(s.host[2] < 0)[0].tolist()]
    ref = gt.gather_and_check(dll, hip, baker, srcs, specials)
    assert len(specials) > 20 and ref["info"] == dict(dict.fromkeys(gt.INFO_FIELDS, 0), primitiveCount=len(specials))
    assert ref["index"].tolist() == [int(srcs[k].host[2][p]) for k, p in specials]
    nowhere = [(3, 0), (0, 40), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (2, 40), (4096, 1), (0x80000000, 0x80000000)]
    ref = gt.gather_and_check(dll, hip, baker, srcs, nowhere + [(0, 1)] + nowhere)
    assert ref["info"]["skippedPrimitives"] == 16 and ref["info"]["referencedBlocks"] == 1 and (np.delete(ref["index"], 8) == -4).all()
    ref = gt.gather_and_check(dll, hip, baker, srcs, nowhere)
    assert ref["info"] == dict(dict.fromkeys(gt.INFO_FIELDS, 0), primitiveCount=8, skippedPrimitives=8)


@pytest.mark.parametrize("index_format", FORMATS)
def test_bounds_table(dll, hip, baker, index_format):
    """lookup_util.bounds_table between two well-formed sources: an entry below -4, an entry at or beyond descArrayCount, level 13, formats 0 and 3, a
    block one byte past arrayDataSize -- each is -4, counted once, and never read through: the arrays are followed by padding that looks valid
    (Source(declared=...): it declares less than it owns), so a kernel that reads past a declared size answers differently"""
    tb = lu.bounds_table(index_format)
    rows = [r for r in tb["rows"] if r[2]]
    index = [r[0] for r in rows] + [0] * 64
    descs = list(tb["descs"]) + [(0, 3, 2)] * 70000
    array_data = np.concatenate([tb["array"], np.full((4 << 20) + 64, 0x6D, np.uint8)])
    good = cu.Source(hip, *cu.table_of_blocks([(mixed_states(level, 2, 60), level, 2) for level in (2, 4)]), [0, 1, -3], ot.IDX_U16)
    bad = cu.Source(hip, array_data, descs, index, index_format, array_align=16, declared=(len(tb["array"]), len(tb["descs"]), len(rows)))
    none = cu.Source(hip, array_data, descs, index, index_format, array_align=16, declared=(0, len(tb["descs"]), len(rows)))
    try:
        invalid = [i for i, r in enumerate(rows) if r[1] == lu.INVALID]
        ref = gt.gather_and_check(dll, hip, baker, [good, bad, good], flags=gt.NO_SPECIAL)
        assert ref["info"]["skippedPrimitives"] == len(invalid) > 8 and (ref["index"][3:3 + len(rows)][invalid] == -4).all()
        assert ref["info"]["referencedBlocks"] == 6 and ref["info"]["duplicateBlocks"] == 2
        beyond = [(1, len(rows)), (1, len(rows) + 63), (1, len(index))]                   # primitives the source owns but does not declare
        ref = gt.gather_and_check(dll, hip, baker, [good, bad], [(1, i) for i in invalid] * 2 + beyond + [(1, 0), (0, 1)])
        assert ref["info"]["skippedPrimitives"] == 2 * len(invalid) + 3 and ref["index"][-2:].tolist() == [1, 0]
        ref = gt.gather_and_check(dll, hip, baker, [none, good])
        assert ref["info"]["skippedPrimitives"] == len(rows) - 4 and ref["info"]["referencedBlocks"] == 2      # arrayDataSize 0: only the specials remain
    finally:
        close_all([good, bad, none])


# ---- the wiring to the tail ----
def test_duplicates_and_flags(dll, hip, baker):
    """equal blocks within one source and across sources are one block; the representative is the lowest (source, descriptor) and the order within a
    size class is the representative's; equal states at another level or in another format are not merged; both flags and their combination; the
    invariant on the info holds with default flags"""
    a, b, c = mixed_states(4, 2, 21), mixed_states(4, 2, 25), mixed_states(6, 2, 23)
    one = np.array([1, 0, 1, 1], np.uint8)
    first = [(b, 4, 2), (a, 4, 2), (a, 4, 2), (np.repeat(a, 4), 5, 2), (one, 1, 1), (np.full(256, 3, np.uint8), 4, 2)]
    second = [(c, 6, 2), (a, 4, 2), (np.array([1, 3, 0, 0], np.uint8), 1, 2), (b, 4, 2), (np.full(256, 3, np.uint8), 4, 2), (one, 1, 1)]
    srcs = [cu.Source(hip, *cu.table_of_blocks(first, gap=3), [2, 1, 0, 3, 4, 5, -1, 2], ot.IDX_U16),
            cu.Source(hip, *cu.table_of_blocks(second, first_offset=5), [0, 1, 2, 3, 4, 5, 1], ot.IDX_U8, array_align=1)]
    try:
        ref = gt.gather_and_check(dll, hip, baker, srcs)
        assert ref["info"]["referencedBlocks"] == 12 and ref["info"]["uniformBlocks"] == 2 and ref["info"]["duplicateBlocks"] == 4
        # level 6 (source 1's 0), 5 (3), 4: b (0) before a (1), then the one-byte blocks: 2-state (4) before 4-state (source 1's 2)
        assert ref["descs"][:, 1:].tolist() == [[6, 2], [5, 2], [4, 2], [4, 2], [1, 1], [1, 2]]
        assert ref["index"].tolist() == [3, 3, 2, 1, 4, -4, -1, 3, 0, 3, 5, 2, -4, 4, 3]
        assert np.array_equal(ref["array"][ref["descs"][2, 0]:][:64], lu.pack(b, 2))
        flipped = gt.gather_and_check(dll, hip, baker, srcs[::-1])
        assert flipped["index"].tolist() == [0, 2, 4, 3, -4, 5, 2, 2, 2, 3, 1, 5, -4, -1, 2]
        keep = gt.gather_and_check(dll, hip, baker, srcs, flags=gt.NO_SPECIAL)
        assert keep["info"]["descArrayCount"] == 7 and keep["info"]["duplicateBlocks"] == 5 and keep["info"]["uniformBlocks"] == 2 and (keep["index"] >= -1).all()
        apart = gt.gather_and_check(dll, hip, baker, srcs, flags=gt.NO_DEDUP)
        assert apart["info"]["descArrayCount"] == 10 and apart["info"]["duplicateBlocks"] == 0 and apart["index"][0] == apart["index"][7] != apart["index"][1]
        raw = gt.gather_and_check(dll, hip, baker, srcs, flags=gt.NO_SPECIAL | gt.NO_DEDUP)
        assert raw["info"]["descArrayCount"] == 12 and sorted(raw["index"][raw["index"] >= 0].tolist()) == [0, 1, 2, 3, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11]
    finally:
        close_all(srcs)


def test_many_blocks_on_a_stream(dll, hip, baker):
    """20 000 descriptors in each of three sources and 2^17 + 17 selected primitives on a caller's stream: every per-primitive and per-descriptor
    kernel over many workgroups, every size class up to level 5 in the partition; two calls return the same bytes"""
    rng = np.random.default_rng(8)
    protos = [(cu.planted_states(level, bits, seed), level, bits) for level in range(6) for bits in (1, 2) for seed in range(12)]
    srcs = []
    for k, fmt in enumerate((ot.IDX_U32, ot.IDX_U16, ot.IDX_U32)):
        table, pdescs = cu.table_of_blocks(protos, first_offset=2 + k, gap=k)
        srcs.append(cu.Source(hip, table, pdescs[rng.integers(0, len(protos), 20000)], rng.integers(-6, 20002, 30000), fmt, array_align=16 if k else 1))
    picks = np.stack([rng.integers(0, 3, (1 << 17) + 17), rng.integers(0, 30001, (1 << 17) + 17)], 1)
    stream = hip.stream_create(non_blocking=True)
    try:
        unpacked = {}
        ref, h1 = gt.gather_and_check(dll, hip, baker, srcs, gt.refs(picks), stream=stream, unpacked=unpacked, keep=True)
        try:
            assert ref["info"]["duplicateBlocks"] > 20000 and 20 < ref["info"]["descArrayCount"] <= len(protos) and ref["info"]["skippedPrimitives"] > 0
            d_sel = hip.upload(gt.refs(picks))
            r, info, h2 = gt.gather(dll, baker, [s.rd for s in srcs], d_sel, len(picks))
            hip.free(d_sel)
            assert (r, info) == (ot.SUCCESS, ref["info"])
            try:
                cu.assert_same(cu.download_result(dll, hip, h2), cu.download_result(dll, hip, h1))
            finally:
                assert dll.ommxDestroyDeviceBakeResult(h2) == ot.SUCCESS
        finally:
            assert dll.ommxDestroyDeviceBakeResult(h1) == ot.SUCCESS
        ref = gt.gather_and_check(dll, hip, baker, srcs, flags=gt.NO_DEDUP, stream=stream, unpacked=unpacked)
        assert ref["info"]["descArrayCount"] > 20000 and ref["info"]["primitiveCount"] == 90000
    finally:
        hip.stream_destroy(stream)
        close_all(srcs)


# ---- cross-checks that do not use the model ----
def _hits_for(rng, levels, prims):
    """interior hits in random micro-triangles of each primitive's own level"""
    micro = (rng.random(len(prims)) * (4.0 ** levels)).astype(np.int64)
    u, v = lu.interior_points(rng, lu.micro_vertices(micro, levels))
    hits = np.empty(len(prims), lu.HIT)
    hits["prim"], hits["u"], hits["v"] = prims, u, v
    return hits


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_one_source_equals_a_coarsening_that_keeps_every_level(dll, hip, baker, flags):
    """K = 1 with the NULL selection against ommxCoarsenMicromap at cap 12 with the same flags, both on the device: arrayData, descArray, the index
    values, the histograms and the shared info fields are equal.  Levels 0..9 in both formats at odd addresses, a duplicate pair, a uniform block,
    specials, and entries that fail the bounds rule"""
    blocks = [(mixed_states(level, 1 + level % 2, 70), level, 1 + level % 2) for level in range(10)]
    blocks += [blocks[5], (np.ones(4 ** 4, np.uint8), 4, 2)]
    array_data, descs = cu.table_of_blocks(blocks, first_offset=3, gap=1)
    descs = np.concatenate([descs, [(len(array_data) - 1, 3, 2)]])                        # descriptor 12: its block ends behind the array
    index = list(range(13)) + [-1, -2, -3, -4, 10, 3, 5, -7, 11, 0, 9, 12]
    src = cu.Source(hip, array_data, descs, index, ot.IDX_U8, array_align=1)
    try:
        r, coarse_info, coarse = cu.coarsen(dll, baker, src.rd, 12, 3, flags)
        assert r == ot.SUCCESS
        try:
            r, info, gathered = gt.gather(dll, baker, [src.rd], flags=flags)
            assert r == ot.SUCCESS
            try:
                a, b = cu.download_result(dll, hip, coarse), cu.download_result(dll, hip, gathered)
                assert (a["index_format"], b["index_format"]) == (ot.IDX_U8, ot.IDX_U32)
                assert np.array_equal(a["array"], b["array"]) and np.array_equal(a["descs"], b["descs"]) and len(a["descs"]) >= 9
                assert np.array_equal(a["index"].astype(np.int64), b["index"].astype(np.int64))
                assert a["array_hist"] == b["array_hist"] and a["index_hist"] == b["index_hist"]
                for field in ("descArrayCount", "arrayDataSize", "referencedBlocks", "uniformBlocks", "duplicateBlocks", "skippedPrimitives"):
                    assert coarse_info[field] == info[field], field
                assert info["skippedPrimitives"] == 3 and info["primitiveCount"] == len(index)
            finally:
                assert dll.ommxDestroyDeviceBakeResult(gathered) == ot.SUCCESS
        finally:
            assert dll.ommxDestroyDeviceBakeResult(coarse) == ot.SUCCESS
    finally:
        src.close()


def test_lookups_chains_and_the_other_entries(dll, hip, baker, three_sources):
    """without the model: for every output primitive ommxLookupOpacity on the output at a handful of hits equals the lookup on source k at primitive p,
    with Force2State off and on; two calls give the same bytes; the output fed back as a source changes nothing; the statistics, geometry (count
    only), coarsen and combine entries accept it"""
    srcs = three_sources
    rng = np.random.default_rng(90)
    picks = np.stack([rng.integers(0, 3, 500), rng.integers(0, 40, 500)], 1)
    picks = picks[[srcs[k].host[2][p] >= -4 for k, p in picks.tolist()]]                  # (the sources hold no malformed entry anyway)
    d_sel = hip.upload(gt.refs(picks))
    made = []
    try:
        r, info, h = gt.gather(dll, baker, [s.rd for s in srcs], d_sel, len(picks))
        assert r == ot.SUCCESS and info["skippedPrimitives"] == 0
        made.append(h)
        out = cu.download_result(dll, hip, h)
        # each output primitive's own level, from the sources' host copies
        levels = np.array([srcs[k].host[1][srcs[k].host[2][p], 1] if srcs[k].host[2][p] >= 0 else 0 for k, p in picks.tolist()], np.int64)
        for flags in (0, 1):                                                              # ommxLookupFlags_Force2State
            for _ in range(4):
                hits = _hits_for(rng, levels, np.arange(len(picks), dtype=np.uint32))
                got = lu.lookup_device(dll, hip, out["rdesc"], hits, flags)
                for k, s in enumerate(srcs):
                    mine = picks[:, 0] == k
                    theirs = hits[mine].copy()
                    theirs["prim"] = picks[mine, 1]
                    assert np.array_equal(got[mine], lu.lookup_device(dll, hip, s.rd, theirs, flags)), (k, flags)
                assert (got < 4).all() and (flags == 0 or (got < 2).all())
        r, info2, h2 = gt.gather(dll, baker, [s.rd for s in srcs], d_sel, len(picks))
        assert r == ot.SUCCESS and info2 == info
        made.append(h2)
        cu.assert_same(cu.download_result(dll, hip, h2), out)
        # fed back: alone it is reproduced; beside a source it is an ordinary source
        r, info3, h3 = gt.gather(dll, baker, [out["rdesc"]])
        assert r == ot.SUCCESS and info3["referencedBlocks"] == info3["descArrayCount"] == info["descArrayCount"] and info3["duplicateBlocks"] == 0
        made.append(h3)
        cu.assert_same(cu.download_result(dll, hip, h3), out)
        r, info4, h4 = gt.gather(dll, baker, [srcs[0].rd, out["rdesc"], srcs[0].rd])
        assert r == ot.SUCCESS and info4["primitiveCount"] == 80 + len(picks) and info4["skippedPrimitives"] == 0
        made.append(h4)
        chained = cu.download_result(dll, hip, h4)
        assert per_primitive(chained)[40:40 + len(picks)] == per_primitive(out) and per_primitive(chained)[:40] == per_primitive(chained)[-40:]
        # the other entries accept it
        want = su.reference_stats(out["array"], out["descs"], out["index"])
        assert cu.device_stats(dll, baker, out["rdesc"]) == (want["fields"], 0)
        counts, skipped = (C.c_uint64 * 4)(), C.c_uint32(7)
        assert dll.ommxExtractMicroGeometry(baker, C.byref(out["rdesc"]), C.byref(gu.c_desc(gu.IDENTITY)), None, counts, C.byref(skipped), None) == ot.SUCCESS
        assert sum(counts) > 0 and skipped.value == 0
        r, cinfo, hc = cu.coarsen(dll, baker, out["rdesc"], 2, 3)
        assert r == ot.SUCCESS and cinfo["coarsenedBlocks"] > 0 and cinfo["skippedPrimitives"] == 0
        made.append(hc)
        r, minfo, hm = mu.combine(dll, baker, [out["rdesc"], out["rdesc"]], 2, 3)
        assert r == ot.SUCCESS and minfo["skippedPrimitives"] == 0 and minfo["combinedTuples"] == info["descArrayCount"]
        made.append(hm)
    finally:
        hip.free(d_sel)
        for h in made:
            assert dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS


# ---- real bakes ----
def test_real_bakes(product, dll, hip):
    """two small ommxBakeDevice results (tests/workloads.py: 200 triangles of foliage cards, 500 triangles over value noise) -- special indices and
    blocks both occur.  Their concatenation and then a strided subset of it equal the model, on a caller's stream and on the null stream; the subset
    taken from the concatenation reads what the subset taken from the bakes reads"""
    b = product.create_baker()
    bakes, textures, made = [], [], []
    stream = hip.stream_create(non_blocking=True)
    try:
        for kind, tris in (("cards", 200), ("c1", 500)):
            tex, uv, ix, lv, kw = wl.workload(kind, tris)
            level = kw.pop("level")
            textures.append(product.create_texture(b, [tex], alpha_cutoff=0.5))
            d = ot.make_desc(textures[-1], uv, ix, level, levels=lv, **kw)
            bakes.append(lu.DeviceBake(product, hip, b, d, uv, ix, lv))
        rds = [k.rdesc for k in bakes]
        host = [(k.host.array_data, k.host.descs, k.host.index, None) for k in bakes]
        every = np.concatenate([k.host.index for k in bakes])
        assert (every < 0).any() and (every >= 0).any() and all(len(k.host.descs) for k in bakes)
        total = len(every)
        strided = np.arange(1, total, 3)
        first = bakes[0].rdesc.indexCount
        pairs = np.stack([strided >= first, np.where(strided >= first, strided - first, strided)], 1).astype(np.int64)
        for s in (stream, None):
            ref = gt.restate_gather(host)
            r, info, h = gt.gather(dll, b, rds, want_result=False, stream=s)
            assert (r, info, h) == (ot.SUCCESS, ref["info"], None)
            r, info, h = gt.gather(dll, b, rds, stream=s)
            assert r == ot.SUCCESS
            made.append(h)
            cat = gt.check_result(dll, hip, b, h, info, ref)
            assert info["primitiveCount"] == total and info["skippedPrimitives"] == 0
            # a strided subset of the concatenation, and the same primitives straight from the bakes
            d_sel = hip.upload(gt.refs(np.stack([np.zeros(len(strided), np.int64), strided], 1)))
            try:
                sub_ref = gt.restate_gather([(ref["array"], ref["descs"], ref["index"], None)], np.stack([np.zeros(len(strided), np.int64), strided], 1))
                r, info, h = gt.gather(dll, b, [cat["rdesc"]], d_sel, len(strided), stream=s)
                assert r == ot.SUCCESS
                made.append(h)
                sub = gt.check_result(dll, hip, b, h, info, sub_ref)
                assert info["descArrayCount"] < ref["info"]["descArrayCount"]             # descriptors that are no longer referenced have left
            finally:
                hip.free(d_sel)
            d_sel = hip.upload(gt.refs(pairs))
            try:
                r, info, h = gt.gather(dll, b, rds, d_sel, len(pairs), stream=s)
                assert r == ot.SUCCESS
                made.append(h)
                direct = gt.check_result(dll, hip, b, h, info, gt.restate_gather(host, pairs))
                assert per_primitive(direct) == per_primitive(sub) and info["arrayDataSize"] == sub_ref["info"]["arrayDataSize"]
            finally:
                hip.free(d_sel)
    finally:
        hip.stream_destroy(stream)
        for h in made:
            assert dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS
        for k in bakes:
            k.close()
        for t in textures:
            product.destroy_texture(b, t)
        product.destroy_baker(b)
