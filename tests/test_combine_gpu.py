"""ommxCombineMicromaps on the GPU.  Every case compares arrayData, descArray, the index buffer, both histograms (as mappings) and the info fields with
tests/combine_util.py's restate_combine byte for byte -- there is no tolerance anywhere.  The shapes are the edges of the streaming pass (a source at
the output's level, one to three levels above it within a word, further above as a broadcast, several units per block, blocks below a lane's share and
at odd addresses), not a workload."""
import ctypes as C
import itertools
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import combine_util as mu
import geometry_util as gu
import kat_cases
import kat_runner

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    gu.bind(product.dll)
    return mu.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def close_all(srcs):
    for s in {id(s): s for s in srcs}.values():
        s.close()


def output_states(ref):
    seen = set()
    for o, l, f in ref["descs"]:
        seen |= set(cu.block_states(ref["array"], int(o), int(l), int(f)).tolist())
    return seen | {-(int(e) + 1) for e in ref["index"] if e < 0}


# ---- every level pair ----
@pytest.mark.parametrize("fmt", [1, 2], ids=["to_2state", "to_4state"])
@pytest.mark.parametrize("bits_b", [1, 2], ids=["b_2state", "b_4state"])
@pytest.mark.parametrize("bits_a", [1, 2], ids=["a_2state", "a_4state"])
def test_every_level_pair_up_to_9(dll, hip, baker, bits_a, bits_b, fmt):
    """one block per level 0..9 in each of two sources and 100 primitives, one per (L_a, L_b), in one call, under both mixedState values: states with
    planted uniform and one-sided regions at every scale, so agreeing, one-sided and mixed micro-triangles occur at every scale of the repetition.
    Every state the output format can express occurs."""
    blocks_a = [(cu.planted_states(level, bits_a, seed=11), level, bits_a) for level in range(10)]
    blocks_b = [(cu.planted_states(level, bits_b, seed=12), level, bits_b) for level in range(10)]
    pairs = np.arange(100)
    srcs = [cu.Source(hip, *cu.table_of_blocks(blocks_a), pairs // 10, ot.IDX_U8, array_align=16),
            cu.Source(hip, *cu.table_of_blocks(blocks_b), pairs % 10, ot.IDX_U16, array_align=16)]
    try:
        seen, unpacked = set(), {}
        for mixed in (2, 3):
            ref = mu.combine_and_check(dll, hip, baker, srcs, fmt, mixed, unpacked=unpacked)
            assert ref["info"]["combinedTuples"] == 100 and ref["info"]["refinedTuples"] == 90 and ref["info"]["skippedPrimitives"] == 0
            seen |= output_states(ref)
        assert seen == ({0, 1} if fmt == 1 else {0, 1, 2, 3})
    finally:
        close_all(srcs)


# ---- level 12: repetition within a word, across words, and the broadcast ----
@pytest.fixture(scope="module")
def level_12_block():
    return cu.planted_states(12, 2, seed=5)


@pytest.mark.parametrize("partner", [0, 3, 5, 8, 11, 12, -1, -2, -3, -4])
def test_level_12(dll, hip, baker, level_12_block, partner):
    """a level-12 block (256 units) against a partner of level 0, 3, 5, 8, 11 or 12 -- broadcast, repetition across words and within a word, none --
    and against each special index; the partner first or second"""
    bits = 1 + (partner & 1)
    other = (cu.planted_states(max(partner, 0), bits, seed=6), max(partner, 0), bits)
    srcs = [cu.Source(hip, *cu.table_of_blocks([(level_12_block, 12, 2)]), [0], ot.IDX_U32, array_align=256),
            cu.Source(hip, *cu.table_of_blocks([other], first_offset=16 * (partner & 1)), [min(partner, 0)], ot.IDX_U8, array_align=16)]
    try:
        ref = mu.combine_and_check(dll, hip, baker, srcs if partner % 3 else srcs[::-1], 2, 2 + (partner & 1))
        assert ref["descs"].tolist() == [[0, 12, 2]] and ref["info"]["combinedTuples"] == 1 and ref["info"]["refinedTuples"] == (0 <= partner < 12)
    finally:
        close_all(srcs)


# ---- source counts ----
def test_one_source_is_a_format_change(dll, hip, baker):
    """K = 1: 4-state to 2-state is & 1 of every state, 2-state to 4-state keeps every state; uniform blocks are promoted on the way"""
    for bits, fmt in ((2, 1), (1, 2), (2, 2)):
        blocks = [(cu.planted_states(level, bits, seed=20 + level), level, bits) for level in (0, 1, 2, 3, 4, 6, 8, 9)]
        blocks.append((np.array([2, 0, 2, 2] * 4, np.uint8) if bits == 2 else np.zeros(16, np.uint8), 2, bits))       # T and UT: uniform once & 1 is taken
        index = list(range(len(blocks))) + [-1, -3, -4, 2]
        src = cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=3, gap=1), index, ot.IDX_U16, array_align=1)
        try:
            ref = mu.combine_and_check(dll, hip, baker, [src], fmt)
            assert ref["info"]["refinedTuples"] == 0 and ref["index"][-4:-1].tolist() == ([-1, -1, -2] if fmt == 1 else [-1, -3, -4])
            last = int(ref["index"][len(blocks) - 1])             # T and UT: a block in the 4-state format, FullyTransparent in the 2-state format
            assert (last >= 0) == (bits == 2 and fmt == 2) and (last >= 0 or last == -1) and ref["index"][-1] == ref["index"][2]
            for i, (states, level, _) in enumerate(blocks):
                e = int(ref["index"][i])
                want = states & 1 if fmt == 1 else states
                got = np.full(len(want), -(e + 1)) if e < 0 else cu.block_states(ref["array"], *(int(x) for x in ref["descs"][e]))
                assert np.array_equal(got, want), (bits, fmt, i)
        finally:
            src.close()


def _related_sources(hip, rng, K, T, formats, levels, slots=6):
    """K sources that mostly agree, as bakes of one mesh under slightly different alpha tests do: per slot one picture (planted states of level 6); source
    k holds it at a level of its own (a coarser level takes every 4^n-th state) in a format of its own, with a few states of its own on top; primitive i
    selects its slot's block in most sources and something else in the others"""
    pictures = [cu.planted_states(6, 2, seed=300 + j) for j in range(slots)]
    slot = rng.integers(0, slots, T)
    srcs = []
    for k in range(K):
        blocks = []
        for j in range(slots):
            level, bits = int(rng.choice(list(levels))), int(rng.integers(1, 3))
            states = pictures[j][::4 ** (6 - level)].copy()
            own = rng.random(len(states)) < 0.03
            states[own] = rng.integers(0, 4, int(own.sum()))
            blocks.append(((states & 1 if bits == 1 else states).astype(np.uint8), level, bits))
        index = np.where(rng.random(T) < 0.85, slot, rng.integers(-4, slots, T))
        table = cu.table_of_blocks(blocks, first_offset=k % 5, gap=k % 3)
        srcs.append(cu.Source(hip, *table, index, formats[k % len(formats)], array_align=1 if k % 2 else 16))
    return srcs


def test_three_sources_with_mixed_index_formats(dll, hip, baker):
    """K = 3, index buffers of 8, 16 and 32 bits over the same 300 primitives, both output formats"""
    srcs = _related_sources(hip, np.random.default_rng(31), 3, 300, [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32], levels=range(7))
    try:
        for fmt, mixed in ((2, 3), (1, 2)):
            ref = mu.combine_and_check(dll, hip, baker, srcs, fmt, mixed)
            assert ref["info"]["combinedTuples"] > 50 and ref["info"]["refinedTuples"] > 25 and ref["info"]["descArrayCount"] > 25
    finally:
        close_all(srcs)


def test_sixteen_sources(dll, hip, baker):
    """K = 16 (the most), one source given twice"""
    srcs = _related_sources(hip, np.random.default_rng(32), 15, 200, [ot.IDX_U32, ot.IDX_U8], levels=range(4, 7), slots=3)
    srcs.insert(7, srcs[2])
    try:
        for fmt, mixed in ((2, 2), (1, 3)):
            ref = mu.combine_and_check(dll, hip, baker, srcs, fmt, mixed)
            assert ref["info"]["combinedTuples"] > 100 and ref["info"]["descArrayCount"] > 20 and len(output_states(ref)) == 2 * fmt
        r, _, _ = mu.combine(dll, baker, [s.rd for s in srcs] + [srcs[0].rd], 2, want_result=False)
        assert r == ot.INVALID_ARGUMENT                                                             # 17
    finally:
        close_all(srcs)


# ---- odd offsets and the bounds rule ----
@pytest.mark.parametrize("fmt,mixed", [(1, 2), (2, 3)], ids=["to_2state", "to_4state"])
def test_statistics_table_twice(dll, hip, baker, fmt, mixed):
    """stats_util's table as two sources under different orders of its index entries: levels 0 - 3 in both formats at odd offsets with random bytes
    (garbage in the unused bits of the one-byte blocks), a level-7 and a level-9 block at odd addresses, and every way to fail the bounds rule -- level
    13, formats 0 and 3, a block one byte past the array, -5, -100, descArrayCount and beyond -- in the first source, the second, or both: such a
    primitive is skipped once"""
    array_data, descs, index, _ = su.table_arrays()
    perm = np.random.default_rng(4).permutation(len(index))
    srcs = [cu.Source(hip, array_data, descs, index, ot.IDX_U8, array_align=1), cu.Source(hip, array_data, descs, index[perm], ot.IDX_U16, array_align=16)]
    try:
        ref = mu.combine_and_check(dll, hip, baker, srcs, fmt, mixed)
        bad = lambda e: (e < -4) | (e >= su.TABLE_WELL_FORMED)
        either, both = bad(index) | bad(index[perm]), bad(index) & bad(index[perm])
        assert ref["info"]["skippedPrimitives"] == int(either.sum()) > 8 and both.any() and (ref["index"][either] == -4).all()
        small = ref["descs"][ref["descs"][:, 1] <= 1]                     # one-byte blocks: unused bits are zero
        assert len(small) >= 2 and all(ref["array"][o] >> (f * 4 ** l) == 0 for o, l, f in small.tolist())
    finally:
        close_all(srcs)


@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U32])
def test_bounds_table(dll, hip, baker, index_format):
    """lookup_util.bounds_table beside a well-formed source: malformed descriptors are skipped and never read through -- the arrays are followed by
    padding that looks valid, so a kernel that reads past a declared size answers differently"""
    tb = lu.bounds_table(index_format)
    rows = [r for r in tb["rows"] if r[2]]
    index = [r[0] for r in rows] + [0] * 64
    descs = list(tb["descs"]) + [(0, 3, 2)] * 70000
    array_data = np.concatenate([tb["array"], np.full((4 << 20) + 64, 0x6D, np.uint8)])
    good = [(cu.planted_states(level, 2, 60 + level), level, 2) for level in (2, 4)]
    srcs = [cu.Source(hip, array_data, descs, index, index_format, array_align=16, declared=(len(tb["array"]), len(tb["descs"]), len(rows))),
            cu.Source(hip, *cu.table_of_blocks(good), np.arange(len(rows)) % 2, ot.IDX_U16)]
    try:
        invalid = [i for i, r in enumerate(rows) if r[1] == lu.INVALID]
        for order in (srcs, srcs[::-1]):
            ref = mu.combine_and_check(dll, hip, baker, order, 2, 2)
            assert ref["info"]["skippedPrimitives"] == len(invalid) > 8 and (ref["index"][invalid] == -4).all()
    finally:
        close_all(srcs)


# ---- specials ----
@pytest.mark.parametrize("fmt", [1, 2], ids=["to_2state", "to_4state"])
def test_all_pairs_of_specials(dll, hip, baker, fmt):
    """the 16 pairs of special indices (and the four alone): no block is made, the entry is the rule's answer"""
    pairs = list(itertools.product((-1, -2, -3, -4), repeat=2))
    empty = (np.zeros(0, np.uint8), np.zeros((0, 3), np.int64))
    srcs = [cu.Source(hip, *empty, [p[0] for p in pairs], ot.IDX_U8), cu.Source(hip, *empty, [p[1] for p in pairs], ot.IDX_U32)]
    try:
        for mixed in (2, 3):
            ref = mu.combine_and_check(dll, hip, baker, srcs, fmt, mixed)
            assert ref["info"] == dict.fromkeys(mu.INFO_FIELDS, 0)
            assert ref["index"].tolist() == [-(mu.brute_join([-(a + 1), -(b + 1)], fmt, mixed) + 1) for a, b in pairs]
            alone = mu.combine_and_check(dll, hip, baker, srcs[:1], fmt, mixed)
            assert alone["index"].tolist() == [-(((-(a + 1)) & 1 if fmt == 1 else -(a + 1)) + 1) for a, _ in pairs]
    finally:
        close_all(srcs)


# ---- promotion ----
def test_promotion(dll, hip, baker):
    """a block against its complement is mixed everywhere: no block, -3 or -4 by mixedState (format 1: -1 or -2); blocks that agree on a side become
    uniform through the unknown bit; a block against the special of its only state stays uniform"""
    rng = np.random.default_rng(41)
    a5, a9 = rng.integers(0, 2, 4 ** 5).astype(np.uint8), rng.integers(0, 2, 4 ** 9).astype(np.uint8)
    half = (np.arange(64) % 2).astype(np.uint8)
    blocks_a = [(a5, 5, 1), (a9, 9, 2), ((2 * half).astype(np.uint8), 3, 2), (np.ones(16, np.uint8), 2, 1), (a5, 5, 1)]
    blocks_b = [(1 - a5, 5, 2), (1 - a9, 9, 1), ((2 - 2 * half).astype(np.uint8), 3, 2), (np.full(1, 1, np.uint8), 0, 2), (a5, 5, 1)]
    srcs = [cu.Source(hip, *cu.table_of_blocks(blocks_a, first_offset=1), [0, 1, 2, 3, 4, 3], ot.IDX_U8, array_align=1),
            cu.Source(hip, *cu.table_of_blocks(blocks_b), [0, 1, 2, 3, 4, -2], ot.IDX_U8)]
    try:
        for fmt in (1, 2):
            for mixed in (2, 3):
                ref = mu.combine_and_check(dll, hip, baker, srcs, fmt, mixed)
                m = -((mixed & 1 if fmt == 1 else mixed) + 1)
                assert ref["index"].tolist() == [m, m, -1 if fmt == 1 else -3, -2, 0, -2] and ref["info"]["uniformBlocks"] == 5
                assert ref["info"]["descArrayCount"] == 1 and ref["info"]["combinedTuples"] == 6
    finally:
        close_all(srcs)


# ---- duplicates ----
def test_duplicates(dll, hip, baker):
    """different tuples whose outputs have equal bytes are one block; the representative is the tuple whose lowest primitive is lowest, and the order
    within a size class is that primitive's; equal states at another level are not merged"""
    a, b, c = cu.planted_states(4, 2, 21), cu.planted_states(4, 2, 22), cu.planted_states(6, 2, 23)
    one = np.array([1, 3, 0, 0], np.uint8)
    blocks_a = [(a, 4, 2), (a, 4, 2), (np.repeat(a, 4), 5, 2), (c, 6, 2), (one, 1, 2), (np.repeat(one, 4), 2, 2), (b, 4, 2)]
    blocks_b = [(b, 4, 2), (b, 4, 2), (c, 6, 2)]
    # primitive 0: c with c.  1, 2, 4, 9: a with b through four pairs of descriptors.  3: a one level down, with b.  5, 6: one picture at levels 1 and 2
    # with the special T.  7, 11: b with b through two pairs.  8: T with b.  10: c with the special UT.
    index_a = [3, 1, 0, 2, 1, 4, 5, 6, -1, 0, 3, 6]
    index_b = [2, 1, 0, 0, 0, -1, -1, 0, 0, 1, -3, 1]
    srcs = [cu.Source(hip, *cu.table_of_blocks(blocks_a, gap=3), index_a, ot.IDX_U16), cu.Source(hip, *cu.table_of_blocks(blocks_b, first_offset=5), index_b, ot.IDX_U8)]
    try:
        ref = mu.combine_and_check(dll, hip, baker, srcs, 2, 3)
        assert ref["info"]["combinedTuples"] == 12 and ref["info"]["duplicateBlocks"] == 4 and ref["info"]["uniformBlocks"] == 0
        # size descending, then the lowest primitive of the representative: level 6 (primitives 0, 10), 5 (3), 4 (1, 7, 8), 2 (6), 1 (5)
        assert ref["index"].tolist() == [0, 3, 3, 2, 3, 7, 6, 4, 5, 3, 1, 4]
        assert ref["descs"][:, 1].tolist() == [6, 6, 5, 4, 4, 4, 2, 1] and ref["info"]["refinedTuples"] == 1
        assert np.array_equal(cu.block_states(ref["array"], *(int(x) for x in ref["descs"][2])), np.repeat(cu.block_states(ref["array"], *(int(x) for x in ref["descs"][3])), 4))
    finally:
        close_all(srcs)


# ---- scale, stream, purity ----
def test_a_million_primitives_on_a_stream(dll, hip, baker):
    """20 000 distinct tuples over 2^20 primitives on a caller's stream: every per-primitive and per-tuple kernel over many workgroups, tuples of many
    primitives in the hash table; two calls return equal bytes; the info-only call returns the full call's info"""
    rng = np.random.default_rng(50)
    T, M = 1 << 20, 20000
    srcs = []
    for k, fmt in enumerate((ot.IDX_U32, ot.IDX_U16)):
        protos = [(cu.planted_states(level, bits, seed + 40 * k), level, bits) for level in range(6) for bits in (1, 2) for seed in range(12)]
        table, pdescs = cu.table_of_blocks(protos, first_offset=2 * k, gap=k)
        descs = pdescs[rng.integers(0, len(protos), 300)]
        srcs.append((table, descs, fmt))
    pool = np.stack([rng.integers(-4, 300, M), rng.integers(-4, 300, M)], 1)
    pick = np.concatenate([np.arange(M), rng.integers(0, M, T - M)])
    rng.shuffle(pick)
    srcs = [cu.Source(hip, table, descs, pool[pick, k], fmt, array_align=16) for k, (table, descs, fmt) in enumerate(srcs)]
    stream = hip.stream_create(non_blocking=True)
    try:
        ref = mu.combine_and_check(dll, hip, baker, srcs, 2, 3, stream=stream)
        assert 15000 < ref["info"]["combinedTuples"] <= M and ref["info"]["duplicateBlocks"] > 1000 and ref["info"]["skippedPrimitives"] == 0
        rds = [s.rd for s in srcs]
        r1, info1, h1 = mu.combine(dll, baker, rds, 2, 3, stream=stream)
        r2, info2, h2 = mu.combine(dll, baker, rds, 2, 3)
        r0, info0, none = mu.combine(dll, baker, rds, 2, 3, want_result=False, stream=stream)
        try:
            assert (r0, r1, r2) == (ot.SUCCESS,) * 3 and none is None and info0 == info1 == info2 == ref["info"]
            cu.assert_same(cu.download_result(dll, hip, h1), cu.download_result(dll, hip, h2))
        finally:
            assert dll.ommxDestroyDeviceBakeResult(h1) == ot.SUCCESS and dll.ommxDestroyDeviceBakeResult(h2) == ot.SUCCESS
    finally:
        hip.stream_destroy(stream)
        close_all(srcs)


def test_commutative_and_idempotent(dll, hip, baker):
    """every permutation of three sources returns the same bytes; a source combined with itself in its own format reproduces its states block for block"""
    srcs = _related_sources(hip, np.random.default_rng(61), 3, 400, [ot.IDX_U16, ot.IDX_U8, ot.IDX_U32], levels=range(7), slots=8)
    try:
        first = None
        for order in itertools.permutations(range(3)):
            r, info, h = mu.combine(dll, baker, [srcs[k].rd for k in order], 2, 2)
            assert r == ot.SUCCESS
            try:
                got = cu.download_result(dll, hip, h)
                got.pop("rdesc")
                if first is None:
                    first = (got, info)
                    mu.check_result(dll, hip, baker, h, info, mu.restate_combine(mu.host_sources(srcs), 2, 2))
                cu.assert_same(got, first[0])
                assert info == first[1]
            finally:
                assert dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS
    finally:
        close_all(srcs)
    for bits in (1, 2):
        blocks = []
        for level in range(10):                                       # (planted states may be uniform as they are: take the first seed where they are not)
            states = next(s for s in (cu.planted_states(level, bits, seed) for seed in range(70, 90)) if level == 0 or s.min() != s.max())
            blocks.append((states, level, bits))
        blocks[3] = (np.full(64, bits, np.uint8), 3, bits)            # uniform: promoted
        index = list(range(10)) + [-1, -2, 4]
        src = cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=7), index, ot.IDX_U8, array_align=1)
        try:
            ref = mu.combine_and_check(dll, hip, baker, [src, src], bits, 3)
            assert ref["index"][3] == -(bits + 1) and ref["index"][10:12].tolist() == [-1, -2] and ref["index"][12] == ref["index"][4]
            for i, (states, level, _) in enumerate(blocks):
                e = int(ref["index"][i])
                if e < 0:                                             # (blocks 0 and 3)
                    assert (states == -(e + 1)).all()
                else:
                    o, l, f = (int(x) for x in ref["descs"][e])
                    assert (l, f) == (level, bits) and np.array_equal(cu.block_states(ref["array"], o, l, f), states)
            assert (ref["index"][:10] >= 0).sum() == 8
        finally:
            src.close()


# ---- the two callers of the shared tail ----
@pytest.mark.parametrize("fmt", [1, 2], ids=["2state", "4state"])
def test_one_source_equals_a_coarsening_that_keeps_every_level(dll, hip, baker, fmt):
    """ommxCoarsenMicromap with cap 12 and ommxCombineMicromaps of the one source into its own format both keep every block as it is and then run the
    same tail, so they return the same result.  Blocks are ordered by size class descending and, within a class, by source descriptor (coarsen) or
    by lowest primitive (combine): the two coincide because descriptors first appear in ascending order in the index buffer.  One table of levels
    0..9 in one format with an exact duplicate pair, a uniform block, special entries and entries that fail the bounds rule."""
    blocks = []
    for level in range(10):
        states = next(s for s in (cu.planted_states(level, fmt, seed) for seed in range(70, 90)) if level == 0 or s.min() != s.max())
        blocks.append((states, level, fmt))
    blocks.append(blocks[5])                                          # descriptor 10: the bytes of descriptor 5 again
    blocks.append((np.ones(4 ** 4, np.uint8), 4, fmt))                # descriptor 11: uniform
    array_data, descs = cu.table_of_blocks(blocks, first_offset=3, gap=1)
    descs = np.concatenate([descs, [(len(array_data) - 1, 3, fmt)]])  # descriptor 12: its block ends behind the array
    specials = [-1, -2] if fmt == 1 else [-1, -2, -3, -4]             # (the 2-state format has no unknown states to keep)
    index = list(range(13)) + specials + [10, 3, 5, -7, 11, 0, 9, 12]
    src = cu.Source(hip, array_data, descs, index, ot.IDX_U8, array_align=1)
    try:
        ref = src.model(12)
        assert ref["info"]["duplicateBlocks"] == 1 and ref["info"]["uniformBlocks"] == 2 and ref["info"]["descArrayCount"] == 9
        assert ref["info"]["skippedPrimitives"] == 3 and ref["descs"][:, 1].tolist() == [9, 8, 7, 6, 5, 4, 3, 2, 1]
        r, coarse_info, coarse = cu.coarsen(dll, baker, src.rd, 12)
        assert r == ot.SUCCESS
        try:
            r, info, combined = mu.combine(dll, baker, [src.rd], fmt)
            assert r == ot.SUCCESS
            try:
                a, b = cu.download_result(dll, hip, coarse), cu.download_result(dll, hip, combined)
                assert (a["index_format"], b["index_format"]) == (ot.IDX_U8, ot.IDX_U32)
                assert np.array_equal(a["array"], b["array"]) and np.array_equal(a["descs"], b["descs"])
                assert np.array_equal(a["index"].astype(np.int64), b["index"].astype(np.int64))
                assert a["array_hist"] == b["array_hist"] and a["index_hist"] == b["index_hist"]
                for field in ("descArrayCount", "arrayDataSize", "uniformBlocks", "duplicateBlocks", "skippedPrimitives"):
                    assert coarse_info[field] == info[field] == ref["info"][field], field
                b["index"] = b["index"].astype(a["index"].dtype)
                cu.assert_same(b, ref)
            finally:
                assert dll.ommxDestroyDeviceBakeResult(combined) == ot.SUCCESS
        finally:
            assert dll.ommxDestroyDeviceBakeResult(coarse) == ot.SUCCESS
    finally:
        src.close()


# ---- real bakes ----
def _level9_hits(rng, num_prims, count):
    """random hits inside level-9 micro-triangles: interior to their ancestors at every coarser level"""
    prims = rng.integers(0, num_prims, count)
    micro = rng.integers(0, 4 ** 9, count)
    u, v = lu.interior_points(rng, lu.micro_vertices(micro, np.full(count, 9, np.int64)))
    hits = np.empty(count, lu.HIT)
    hits["prim"], hits["u"], hits["v"] = prims, u, v
    return hits


def _known_fraction(dll, hip, baker, rd):
    out = hip.alloc(4 * rd.indexCount)
    try:
        o = su.DeviceStatsOutputs(None, None, out)
        st, skipped = ot.DebugStats(), C.c_uint32(77)
        assert dll.ommxDebugGetStatsDevice(baker, C.byref(rd), None, C.byref(o), C.byref(st), C.byref(skipped), None) == ot.SUCCESS and skipped.value == 0
        return hip.download(out, 4 * rd.indexCount, np.float32)
    finally:
        hip.free(out)


def test_real_bakes(product, dll, hip):
    """ommxBakeDevice of a known-answer case (tests/kat_cases.py) at level 7, at level 9 and at level 9 under a second alpha cut-off.  For 100 000 random
    hits, every one compared: ommxLookupOpacity on the combined result equals the rule applied to the sources' lookups; the format-1 output is & 1 of
    that; combining in two steps answers as combining at once; the output equals the model; the statistics, geometry and coarsening entries accept it;
    no primitive's known share exceeds any source's"""
    c = next(k for k in kat_cases.CASES if k["name"] == "Mandelbrot3")
    b = product.create_baker()
    tex = product.create_texture(b, [kat_runner.texture_array(c["tex"], c["size"], c["param"])])
    uv, ix = np.array(c["uv"], np.float32), np.array(c["ix"], np.uint32)
    rng = np.random.default_rng(77)
    bakes, made = [], []
    try:
        for level, cutoff in ((7, 0.5), (9, 0.5), (9, 0.3)):
            d = ot.make_desc(tex, uv, ix, level, alpha_cutoff=cutoff, fmt=ot.FMT_4STATE, promo=ot.PROMO_NEAREST)
            bakes.append(lu.DeviceBake(product, hip, b, d, uv, ix))
        rds = [k.rdesc for k in bakes]
        assert all(len(k.host.descs) >= 1 for k in bakes) and not np.array_equal(bakes[1].host.array_data, bakes[2].host.array_data)
        hits = _level9_hits(rng, rds[0].indexCount, 100000)
        looked = np.stack([lu.lookup_device(dll, hip, rd, hits) for rd in rds])
        host = [(k.host.array_data, k.host.descs, k.host.index, None) for k in bakes]
        for mixed in (2, 3):
            want = mu.join_states(looked, 2, mixed)
            assert len(set(want.tolist())) == 4
            r, info, h = mu.combine(dll, baker=b, rds=rds, fmt=2, mixed=mixed)
            assert r == ot.SUCCESS
            made.append(h)
            full = mu.check_result(dll, hip, b, h, info, mu.restate_combine(host, 2, mixed))
            assert info["refinedTuples"] > 0
            assert np.array_equal(lu.lookup_device(dll, hip, full["rdesc"], hits), want)
            r, _, h1 = mu.combine(dll, b, rds, 1, mixed)
            assert r == ot.SUCCESS
            made.append(h1)
            assert np.array_equal(lu.lookup_device(dll, hip, cu.result_desc_of(dll, h1), hits), want & 1)
            # (A, B) then C
            r, _, hab = mu.combine(dll, b, rds[:2], 2, mixed)
            assert r == ot.SUCCESS
            made.append(hab)
            r, _, habc = mu.combine(dll, b, [cu.result_desc_of(dll, hab), rds[2]], 2, mixed)
            assert r == ot.SUCCESS
            made.append(habc)
            assert np.array_equal(lu.lookup_device(dll, hip, cu.result_desc_of(dll, habc), hits), want)
            # the other entries accept it
            counts, skipped = (C.c_uint64 * 4)(), C.c_uint32(7)
            assert dll.ommxExtractMicroGeometry(b, C.byref(full["rdesc"]), C.byref(gu.c_desc(gu.IDENTITY)), None, counts, C.byref(skipped), None) == ot.SUCCESS
            assert sum(counts) > 0 and skipped.value == 0
            r, cinfo, hc = cu.coarsen(dll, b, full["rdesc"], 5, mixed)
            assert r == ot.SUCCESS and cinfo["coarsenedBlocks"] > 0 and cinfo["skippedPrimitives"] == 0
            made.append(hc)
            share = _known_fraction(dll, hip, b, full["rdesc"])
            for rd in rds:
                assert (share <= _known_fraction(dll, hip, b, rd)).all()
    finally:
        for h in made:
            assert dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS
        for k in bakes:
            k.close()
        product.destroy_texture(b, tex)
        product.destroy_baker(b)
