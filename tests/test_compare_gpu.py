"""ommxCompareMicromaps on the GPU.  Every case compares the relations, the levels, the matrices and the info with tests/compare_util.py's
restate_compare byte for byte -- there is no tolerance anywhere.  The shapes are the edges of the streaming pass (a side at the pair's level, one to
three levels above it within a word, further above as a broadcast, several units per pair, blocks below a lane's share, at odd addresses and at the end
of their allocation), not a workload.  The last tests hold the derived entries to what they promise about their source, which is what the entry is
for."""
import ctypes as C
import itertools
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import combine_util as mu
import compare_util as pu
import fit_util as ft
import gather_util as gt
import reorient_util as rt
import kat_cases
import kat_runner

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    for m in (lu, ft, gt, rt):
        m.bind(product.dll)
    return pu.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def close_all(srcs):
    for s in {id(s): s for s in srcs}.values():
        s.close()


def cells_of(ref):
    return {(sa, sb) for sa in range(4) for sb in range(4) if ref["info"]["totals"][sa][sb]}


def relation_bits(ref):
    bits = 0
    for r in ref["relations"].tolist():
        bits |= r
    return bits


# ---- every level pair ----
@pytest.mark.parametrize("bits_b", [1, 2], ids=["b_2state", "b_4state"])
@pytest.mark.parametrize("bits_a", [1, 2], ids=["a_2state", "a_4state"])
def test_every_level_pair_up_to_9(dll, hip, baker, bits_a, bits_b):
    """one block per level 0..9 in each source and 100 primitives, one per (L_a, L_b), in one call, with and without Force2State: states with planted
    uniform and one-sided regions at every scale.  Every cell the two formats can express occurs, and with two 4-state sources all four relation bits"""
    blocks_a = [(cu.planted_states(level, bits_a, seed=11), level, bits_a) for level in range(10)]
    blocks_b = [(cu.planted_states(level, bits_b, seed=12), level, bits_b) for level in range(10)]
    pairs = np.arange(100)
    srcs = [cu.Source(hip, *cu.table_of_blocks(blocks_a), pairs // 10, ot.IDX_U8, array_align=16),
            cu.Source(hip, *cu.table_of_blocks(blocks_b), pairs % 10, ot.IDX_U16, array_align=16)]
    try:
        unpacked = {}
        for force2 in (False, True):
            ref = pu.compare_and_check(dll, hip, baker, srcs[0], srcs[1], force2, unpacked=unpacked)
            i = ref["info"]
            assert (i["comparedPairs"], i["refinedPairs"], i["skippedPrimitives"]) == (100, 90, 0)
            assert ref["levels"].tolist() == np.maximum(pairs // 10, pairs % 10).tolist()
            assert (ref["confusion"].reshape(100, 16).sum(axis=1) == 4 ** ref["levels"].astype(np.int64)).all()
            assert sum(sum(i["totals"], [])) == 100 * pu.UNIT
            top_a, top_b = (2 if bits_a == 1 or force2 else 4), (2 if bits_b == 1 or force2 else 4)
            assert cells_of(ref) == set(itertools.product(range(top_a), range(top_b)))
            want = pu.CONFLICT | (0 if force2 else (pu.A_WEAKER if bits_a == 2 else 0) | (pu.B_WEAKER if bits_b == 2 else 0) | (pu.HINT if bits_a == bits_b == 2 else 0))
            assert relation_bits(ref) == want
            for bit, field in ((pu.CONFLICT, "conflictPrimitives"), (pu.A_WEAKER, "aWeakerPrimitives"), (pu.B_WEAKER, "bWeakerPrimitives"), (pu.HINT, "hintPrimitives")):
                assert (i[field] > 0) == bool(want & bit)
    finally:
        close_all(srcs)


# ---- level 12: repetition within a word, across words, and the broadcast ----
@pytest.fixture(scope="module")
def level_12(hip):
    """a level-12 4-state block as a source of one primitive: at a 256-byte aligned address and at an odd one; what was unpacked of them"""
    states = cu.planted_states(12, 2, seed=5)
    srcs = dict(aligned=cu.Source(hip, *cu.table_of_blocks([(states, 12, 2)]), [0], ot.IDX_U32, array_align=256),
                odd=cu.Source(hip, *cu.table_of_blocks([(states, 12, 2)], first_offset=3), [0], ot.IDX_U32, array_align=1), unpacked={})
    yield srcs
    srcs["aligned"].close()
    srcs["odd"].close()


@pytest.mark.parametrize("partner", [0, 3, 5, 8, 11, 12, -1, -2, -3, -4])
def test_level_12(dll, hip, baker, level_12, partner):
    """a level-12 4-state block (256 units) against a partner of level 0, 3, 5, 8, 11 or 12 -- broadcast, repetition across words and within a word,
    none -- and against each special index; the partner as B and as A; against the level-5 partner the big block sits at an odd byte address"""
    bits = 1 + (partner & 1)
    other = (cu.planted_states(max(partner, 0), bits, seed=6), max(partner, 0), bits)
    big = level_12["odd" if partner == 5 else "aligned"]
    small = cu.Source(hip, *cu.table_of_blocks([other], first_offset=16 * (partner & 1)), [min(partner, 0)], ot.IDX_U8, array_align=16)
    try:
        for a, b in ((big, small), (small, big)):
            ref = pu.compare_and_check(dll, hip, baker, a, b, unpacked=level_12["unpacked"])
            i = ref["info"]
            assert ref["levels"].tolist() == [12] and (i["comparedPairs"], i["refinedPairs"]) == (1, int(partner != 12))
            assert int(ref["confusion"].sum()) == 4 ** 12 == sum(sum(i["totals"], []))
            assert i["totals"] == ref["confusion"][0].tolist()                                     # level 12: the units of the totals
    finally:
        small.close()


# ---- one-byte blocks ----
def test_one_byte_blocks_ignore_their_unused_bits(dll, hip, baker):
    """levels 0 and 1 in both formats (1, 2, 4 and 8 bits of a byte) against each other and against a level-3 block, with garbage in the unused bits
    on both sides: every answer equals that of the same blocks with zeros there"""
    rng = np.random.default_rng(21)
    blocks = [(cu.planted_states(level, bits, seed=30 + 2 * level + bits), level, bits) for level in (0, 1) for bits in (1, 2)]
    blocks.append((cu.planted_states(3, 2, seed=39), 3, 2))
    clean, descs = cu.table_of_blocks(blocks, first_offset=1, gap=2)
    index = np.array(list(itertools.product(range(5), repeat=2)))
    refs = []
    for garbage in (False, True):
        arrays = []
        for side in range(2):
            a = clean.copy()
            if garbage:
                for o, l, f in descs.tolist():
                    if 4 ** l * f < 8:
                        a[o] |= (int(rng.integers(1, 256)) << (4 ** l * f)) & 0xFF
                assert not np.array_equal(a, clean)
            arrays.append(a)
        srcs = [cu.Source(hip, arrays[0], descs, index[:, 0], ot.IDX_U8, array_align=1), cu.Source(hip, arrays[1], descs, index[:, 1], ot.IDX_U32, array_align=16)]
        try:
            for force2 in (False, True):
                refs.append(pu.compare_and_check(dll, hip, baker, srcs[0], srcs[1], force2))
        finally:
            close_all(srcs)
    for clean_ref, dirty_ref in zip(refs[:2], refs[2:]):
        pu.assert_outputs(dirty_ref, clean_ref)
        assert dirty_ref["info"] == clean_ref["info"]
    diagonal = index[:, 0] == index[:, 1]
    assert (refs[2]["relations"][diagonal] == 0).all() and refs[2]["info"]["comparedPairs"] == 25


# ---- addresses ----
def _placed(blocks, residues, filler=0xA5):
    """blocks: [(states, level, bits)] -> (array_data, descs): block k at the next offset that is residues[k] modulo 16"""
    parts, descs, at = [], [], 0
    for (states, level, bits), m in zip(blocks, residues):
        pad = (m - at) % 16
        b = lu.pack(states, bits)
        parts += [np.full(pad, filler, np.uint8), b]
        descs.append((at + pad, level, bits))
        at += pad + len(b)
    return np.concatenate(parts), np.array(descs, np.int64).reshape(-1, 3)


def test_every_misalignment(dll, hip, baker):
    """blocks of levels 8, 7, 6 and 4 at every address 0..15 modulo 16 on both sides: the 16-byte loads of an aligned block and the byte loads of the
    others give the same counts.  Pairs at equal and at different misalignments, at equal levels and one to four levels apart"""
    levels = (8, 7, 6, 4)
    blocks_a = [(cu.planted_states(levels[m % 4], 2, seed=100 + m), levels[m % 4], 2) for m in range(16)]
    blocks_b = [(cu.planted_states(levels[(m // 4) % 4], 1 + m % 2, seed=120 + m), levels[(m // 4) % 4], 1 + m % 2) for m in range(16)]
    table_a, table_b = _placed(blocks_a, range(16)), _placed(blocks_b, [(5 * m + 3) % 16 for m in range(16)])
    assert sorted(o % 16 for o in table_a[1][:, 0]) == sorted(o % 16 for o in table_b[1][:, 0]) == list(range(16))
    ia, ib = np.repeat(np.arange(16), 16), np.tile(np.arange(16), 16)
    srcs = [cu.Source(hip, *table_a, ia, ot.IDX_U8, array_align=16), cu.Source(hip, *table_b, ib, ot.IDX_U16, array_align=16)]
    try:
        ref = pu.compare_and_check(dll, hip, baker, srcs[0], srcs[1])
        assert ref["info"]["comparedPairs"] == 256 and ref["info"]["refinedPairs"] == 192 and relation_bits(ref) == 0x0F
        same = pu.compare_and_check(dll, hip, baker, srcs[0], srcs[0])
        assert same["info"]["identicalPrimitives"] == 256 and same["info"]["comparedPairs"] == 16
    finally:
        close_all(srcs)


@pytest.mark.parametrize("array_align", [1, 4, 16, 256])
def test_a_block_that_ends_with_the_allocation(dll, hip, baker, array_align):
    """the array is the tail of its allocation and its last block ends with it: blocks of 1 byte, 16 bytes, 1 KiB and 16 KiB behind an odd lead, as A
    and as B, against a finer and a coarser partner"""
    for level, bits, lead in ((0, 2, 0), (3, 2, 3), (6, 2, 7), (8, 2, 1)):
        blocks = [(cu.planted_states(2, 2, 3), 2, 2), (cu.planted_states(level, bits, 5), level, bits)]
        table = cu.table_of_blocks(blocks, first_offset=lead)
        assert table[1][-1, 0] + su.block_bytes(level, bits) == len(table[0])
        last = cu.Source(hip, *table, [1, 0, 1, 1], ot.IDX_U32, array_align=array_align)
        partner = cu.Source(hip, *cu.table_of_blocks([(cu.planted_states(l, 1, 7), l, 1) for l in (1, 7)]), [0, 0, 1, -2], ot.IDX_U8)
        try:
            for a, b in ((last, partner), (partner, last)):
                ref = pu.compare_and_check(dll, hip, baker, a, b)
                assert ref["info"]["comparedPairs"] == 4 and ref["levels"].tolist() == [max(level, 1), 2, max(level, 7), level]
        finally:
            last.close()
            partner.close()


def test_bounds_table(dll, hip, baker):
    """lookup_util.bounds_table beside a well-formed source, as A and as B: malformed descriptors are skipped and never read through -- the arrays are
    followed by padding that looks valid (Source(declared=...)), so a kernel that reads past a declared size answers differently"""
    tb = lu.bounds_table(ot.IDX_U16)
    rows = [r for r in tb["rows"] if r[2]]
    index = [r[0] for r in rows] + [0] * 64
    descs = list(tb["descs"]) + [(0, 3, 2)] * 70000
    array_data = np.concatenate([tb["array"], np.full((4 << 20) + 64, 0x6D, np.uint8)])
    good = [(cu.planted_states(level, 2, 60 + level), level, 2) for level in (2, 4)]
    srcs = [cu.Source(hip, array_data, descs, index, ot.IDX_U16, array_align=16, declared=(len(tb["array"]), len(tb["descs"]), len(rows))),
            cu.Source(hip, *cu.table_of_blocks(good), np.arange(len(rows)) % 2, ot.IDX_U8)]
    try:
        invalid = [i for i, r in enumerate(rows) if r[1] == lu.INVALID]
        for a, b in (srcs, srcs[::-1]):
            ref = pu.compare_and_check(dll, hip, baker, a, b)
            assert ref["info"]["skippedPrimitives"] == len(invalid) > 8 and (ref["relations"][invalid] == pu.SKIPPED).all()
            assert (ref["levels"][invalid] == 0xFF).all() and not ref["confusion"][invalid].any()
    finally:
        close_all(srcs)


# ---- pair bookkeeping ----
def test_pair_bookkeeping(dll, hip, baker):
    """stats_util's table as both sources under different orders of its index entries -- levels 0 - 3 in both formats at odd offsets, a level-7 and a
    level-9 block, and every way to fail the bounds rule in A, in B or in both: such a primitive is skipped once -- then one pair under 3000
    primitives and 10 pairs under one descriptor"""
    array_data, descs, index, _ = su.table_arrays()
    perm = np.random.default_rng(4).permutation(len(index))
    many = np.full(3000, 8)
    ia = np.concatenate([index, many, np.full(10, 3)])
    ib = np.concatenate([index[perm], many + 1, np.arange(10)])
    srcs = [cu.Source(hip, array_data, descs, ia, ot.IDX_U8, array_align=1), cu.Source(hip, array_data, descs, ib, ot.IDX_U16, array_align=16)]
    try:
        for force2 in (False, True):
            ref = pu.compare_and_check(dll, hip, baker, srcs[0], srcs[1], force2)
            bad = lambda e: (e < -4) | (e >= su.TABLE_WELL_FORMED)
            either, both = bad(ia) | bad(ib), bad(ia) & bad(ib)
            assert ref["info"]["skippedPrimitives"] == int(either.sum()) > 8 and both.any() and (ref["relations"][either] == pu.SKIPPED).all()
            assert sum(sum(ref["info"]["totals"], [])) == (len(ia) - int(either.sum())) * pu.UNIT
            block = ref["confusion"][len(index):len(index) + 3000]
            assert (block == block[0]).all() and block[0].sum() == 4 ** int(ref["levels"][len(index)])
            tail = ref["relations"][-10:]
            assert tail[3] == 0 and ref["info"]["comparedPairs"] >= 11
    finally:
        close_all(srcs)


@pytest.mark.parametrize("force2", [False, True], ids=["states", "force_2state"])
def test_all_pairs_of_specials(dll, hip, baker, force2):
    """the 16 pairs of special indices, four times over: no pair is streamed, T is 0 and the one field is in its cell"""
    pairs = list(itertools.product((-1, -2, -3, -4), repeat=2)) * 4
    empty = (np.zeros(0, np.uint8), np.zeros((0, 3), np.int64))
    srcs = [cu.Source(hip, *empty, [p[0] for p in pairs], ot.IDX_U8), cu.Source(hip, *empty, [p[1] for p in pairs], ot.IDX_U32)]
    try:
        ref = pu.compare_and_check(dll, hip, baker, srcs[0], srcs[1], force2)
        i = ref["info"]
        assert (i["comparedPairs"], i["refinedPairs"], i["skippedPrimitives"]) == (0, 0, 0) and not ref["levels"].any()
        assert i["identicalPrimitives"] == (32 if force2 else 16) and i["conflictPrimitives"] == (32 if force2 else 8) and i["firstConflictPrimitive"] == 1
        assert (i["aWeakerPrimitives"], i["bWeakerPrimitives"], i["hintPrimitives"]) == ((0, 0, 0) if force2 else (16, 16, 8))
        for k, (a, b) in enumerate(pairs):
            sa, sb = (-(a + 1), -(b + 1)) if not force2 else (-(a + 1) & 1, -(b + 1) & 1)
            assert ref["confusion"][k, sa, sb] == 1 and ref["confusion"][k].sum() == 1 and ref["relations"][k] == pu.cell_relation(sa, sb)
    finally:
        close_all(srcs)


# ---- scale, stream, purity ----
def test_many_primitives_on_a_stream(dll, hip, baker):
    """2^17 + 17 primitives over 3000 descriptors per side and 6000 distinct pairs on a caller's stream: every per-primitive and per-pair kernel over
    many workgroups, pairs of many primitives in the hash table; two calls return the same bytes"""
    rng = np.random.default_rng(50)
    T, M = (1 << 17) + 17, 6000
    tables = []
    for k in range(2):
        protos = [(cu.planted_states(level, bits, seed + 40 * k), level, bits) for level in range(6) for bits in (1, 2) for seed in range(12)]
        table, pdescs = cu.table_of_blocks(protos, first_offset=2 * k, gap=k)
        tables.append((table, pdescs[rng.integers(0, len(protos), 3000)]))
    pool = np.stack([rng.integers(-4, 3000, M), rng.integers(-4, 3000, M)], 1)
    pick = np.concatenate([np.arange(M), rng.integers(0, M, T - M)])
    rng.shuffle(pick)
    srcs = [cu.Source(hip, table, descs, pool[pick, k], fmt, array_align=16) for k, ((table, descs), fmt) in enumerate(zip(tables, (ot.IDX_U32, ot.IDX_U16)))]
    stream = hip.stream_create(non_blocking=True)
    try:
        ref = pu.compare_and_check(dll, hip, baker, srcs[0], srcs[1], stream=stream)
        i = ref["info"]
        assert 5000 < i["comparedPairs"] <= M and i["skippedPrimitives"] == 0 and sum(sum(i["totals"], [])) == T * pu.UNIT
        assert i["firstConflictPrimitive"] == int(np.nonzero(ref["relations"] & pu.CONFLICT)[0][0])
        got = []
        for _ in range(2):
            out = pu.Outputs(hip, T)
            try:
                r, info = pu.compare(dll, baker, srcs[0].rd, srcs[1].rd, 0, out, stream=stream)
                assert r == ot.SUCCESS and info == i
                got.append(out.download())
            finally:
                out.close()
        assert all(got[0][k].tobytes() == got[1][k].tobytes() for k in got[0])
    finally:
        hip.stream_destroy(stream)
        close_all(srcs)


# ---- detection ----
def test_one_flipped_micro_triangle_is_found(dll, hip, baker):
    """two level-9 blocks that differ in ONE micro-triangle (Transparent in A, Opaque in B), under primitives 37 and 41 of 50: exactly those two have
    CONFLICT, their matrices have one micro-triangle off the diagonal, and firstConflictPrimitive is 37"""
    states = np.random.default_rng(77).integers(0, 4, 4 ** 9).astype(np.uint8)
    at = int(np.nonzero(states == 0)[0][1234])
    flipped = states.copy()
    flipped[at] = 1
    table = cu.table_of_blocks([(states, 9, 2), (flipped, 9, 2)], first_offset=5)
    ia, ib = np.zeros(50, np.int64), np.zeros(50, np.int64)
    ib[[37, 41]] = 1
    srcs = [cu.Source(hip, *table, ia, ot.IDX_U8, array_align=1), cu.Source(hip, *table, ib, ot.IDX_U8, array_align=16)]
    try:
        ref = pu.compare_and_check(dll, hip, baker, srcs[0], srcs[1])
        i = ref["info"]
        assert np.nonzero(ref["relations"])[0].tolist() == [37, 41] and (ref["relations"][[37, 41]] == pu.CONFLICT).all()
        assert (i["conflictPrimitives"], i["identicalPrimitives"], i["firstConflictPrimitive"], i["comparedPairs"]) == (2, 48, 37, 2)
        off = ref["confusion"][37].copy()
        off[range(4), range(4)] = 0
        assert off.sum() == 1 and off[0, 1] == 1 and i["totals"][0][1] == 2 * 4 ** 3 and i["totals"][1][0] == 0
    finally:
        close_all(srcs)


# ---- what the derived entries promise ----
@pytest.fixture(scope="module")
def bakes(product, dll, hip):
    """ommxBakeDevice of a known-answer case (tests/kat_cases.py) at level 7 under two alpha cut-offs"""
    c = next(k for k in kat_cases.CASES if k["name"] == "Mandelbrot3")
    b = product.create_baker()
    tex = product.create_texture(b, [kat_runner.texture_array(c["tex"], c["size"], c["param"])])
    uv, ix = np.array(c["uv"], np.float32), np.array(c["ix"], np.uint32)
    made = []
    try:
        for cutoff in (0.5, 0.3):
            d = ot.make_desc(tex, uv, ix, 7, alpha_cutoff=cutoff, fmt=ot.FMT_4STATE, promo=ot.PROMO_NEAREST)
            made.append(lu.DeviceBake(product, hip, b, d, uv, ix))
        yield b, made
    finally:
        for k in made:
            k.close()
        product.destroy_texture(b, tex)
        product.destroy_baker(b)


def _compare_handles(dll, hip, baker, rd_a, rd_b):
    out = pu.Outputs(hip, rd_a.indexCount)
    try:
        r, info = pu.compare(dll, baker, rd_a, rd_b, 0, out)
        assert r == ot.SUCCESS and info["skippedPrimitives"] == 0
        return info, out.download()
    finally:
        out.close()


def test_derived_results_keep_their_promises(dll, hip, bakes):
    """on a real bake X: a coarsening, a fit into a quarter of the bytes and a combine with a bake at another cut-off claim nothing that X does not (no
    CONFLICT, no B_WEAKER), and each does lose something (A_WEAKER); a gather of every primitive and a rotation followed by its inverse are identical
    to X; the rows of a primitive's matrix add up to the statistics entry's stateCounts of A's block, scaled to the pair's level"""
    b, (X, Y) = bakes
    x = X.rdesc
    assert x.descArrayCount >= 1 and not np.array_equal(X.host.array_data, Y.host.array_data)
    made = []
    try:
        r, _, coarse = cu.coarsen(dll, b, x, 4)
        made.append(coarse)
        r2, _, _, fitted = ft.fit(dll, hip, b, x, x.arrayDataSize // 4)
        made.append(fitted)
        r3, _, joined = mu.combine(dll, b, [x, Y.rdesc], 2, 3)
        made.append(joined)
        assert (r, r2, r3) == (ot.SUCCESS,) * 3
        for h in (coarse, fitted, joined):
            info, got = _compare_handles(dll, hip, b, cu.result_desc_of(dll, h), x)
            assert not (got["relations"] & (pu.CONFLICT | pu.B_WEAKER)).any() and info["conflictPrimitives"] == info["bWeakerPrimitives"] == 0
            assert info["aWeakerPrimitives"] > 0 and info["firstConflictPrimitive"] == pu.NO_CONFLICT
            assert sum(info["totals"][sa][sb] for sa in (0, 1) for sb in range(4) if sa != sb) == 0
        # the other way round X claims more than the coarsening: B_WEAKER, never CONFLICT
        info, _ = _compare_handles(dll, hip, b, x, cu.result_desc_of(dll, coarse))
        assert info["bWeakerPrimitives"] > 0 and info["conflictPrimitives"] == info["aWeakerPrimitives"] == 0
        r, _, gathered = gt.gather(dll, b, [x])
        made.append(gathered)
        r2, _, once = rt.reorient(dll, b, x, orientation=1)
        made.append(once)
        r3, _, back = rt.reorient(dll, b, cu.result_desc_of(dll, once), orientation=2)
        made.append(back)
        assert (r, r2, r3) == (ot.SUCCESS,) * 3
        for h in (gathered, back):
            info, got = _compare_handles(dll, hip, b, cu.result_desc_of(dll, h), x)
            assert not got["relations"].any() and info["identicalPrimitives"] == x.indexCount
        info, _ = _compare_handles(dll, hip, b, cu.result_desc_of(dll, once), x)
        assert info["identicalPrimitives"] < x.indexCount                                           # (a rotation alone is seen)
        # row sums against the statistics of A = the coarsening, B = X
        a = cu.result_desc_of(dll, coarse)
        counts = hip.alloc(16 * max(a.descArrayCount, 1))
        try:
            o = su.DeviceStatsOutputs(counts, None, None)
            st = ot.DebugStats()
            assert dll.ommxDebugGetStatsDevice(b, C.byref(a), None, C.byref(o), C.byref(st), None, None) == ot.SUCCESS
            state_counts = hip.download(counts, 16 * a.descArrayCount, np.uint32).reshape(-1, 4).astype(np.int64)
        finally:
            hip.free(counts)
        _, got = _compare_handles(dll, hip, b, a, x)
        host = cu.download_result(dll, hip, coarse)
        checked = 0
        for i, e in enumerate(host["index"].tolist()):
            rows = got["confusion"][i].astype(np.int64).sum(axis=1)
            if e >= 0:
                scale = 4 ** (int(got["levels"][i]) - int(host["descs"][e, 1]))
                assert rows.tolist() == (state_counts[e] * scale).tolist(), i
                checked += 1
            else:
                assert rows[-(e + 1)] == 4 ** int(got["levels"][i]) == rows.sum()
        assert checked > 0
    finally:
        for h in made:
            if h is not None:
                assert dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS
