"""ommxMergeSimilarMicromaps on the GPU.  Every case compares the result arrays, the histograms, the info and the roots with tests/merge_util.py's
restate_merge byte for byte -- there is no tolerance anywhere.  The shapes are the edges of the kernels (a lane's blocks of 1, 4, 16, 64 and 256
bytes, a wave's of 1 KiB, of one full step of 4 KiB and of several steps, member lists from 1 to 1025, blocks at odd addresses and at the end of
their allocation), not a workload; tests/README_merge.md says which level stands on which side of which switch."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import compare_util as pu
import merge_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    cu.bind(product.dll)
    return gu.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def limit_for(level, percent=4):
    """`percent` of a block, and one micro-triangle at the least"""
    return max(gu.UNIT * percent // 100, 4 ** (12 - level))


def families(level, counts, share, seed):
    """near-copy families of `level` with a 2-state and a level-0 block between them, interleaved so that no family is contiguous"""
    fams = [gu.near_copies(level, n, share, seed + 10 * k) for k, n in enumerate(counts)]
    blocks = [(cu.planted_states(3, 1, seed), 3, 1), (np.array([seed & 3], np.uint8), 0, 2)]
    for j in range(max(counts)):
        blocks += [f[j] for f in fams if j < len(f)]
    return blocks


# ---- every level on either side of a switch, both mixed states ----
@pytest.mark.parametrize("mixed", [2, 3])
@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_near_copies_at_every_level(dll, hip, baker, level, mixed):
    """two families of planted near-copies (1..3 % of the fields set to another state) at odd byte addresses, every block under two primitives"""
    blocks = families(level, (9, 6) if level < 8 else (6, 3), 0.03, 40 + level)
    table = cu.table_of_blocks(blocks, first_offset=2, gap=2 * (level & 1))
    index = np.concatenate([np.arange(len(blocks)), np.arange(len(blocks))[::-1], [-1, -3]])
    src = cu.Source(hip, *table, index, ot.IDX_U8, array_align=1)
    try:
        assert any(o % 2 == 1 for o in table[1][2:, 0])
        ref = gu.merge_and_check(dll, hip, baker, src, limit_for(level), mixed=mixed, seed=level)
        i = ref["info"]
        assert i["candidateBlocks"] == len(blocks) - 2 and 0 < i["absorbedBlocks"] <= i["candidateBlocks"] - 2, i
        assert ref["roots"][:2].tolist() == [0, 1] and (ref["roots"] <= np.arange(len(blocks))).all()
        gu.lost_known_fields(ref, table[1], index)
    finally:
        src.close()


# ---- member lists ----
def _bucket_source(level, members, samples, seed, distinct=False):
    """one family per entry of `members`: a base whose sampled fields spell the family's number, and members that differ from it in one field that is
    not sampled in round 0 -> (blocks in memory order, the family of each block).  distinct: no two members of a family are equal (draws that repeat
    an earlier member are drawn again; a family then holds at most 1 + 3 * (4^level - samples) blocks)"""
    at = [gu.pos(seed, level, 0, j) for j in range(samples)]
    assert len(set(at)) == samples
    free = [f for f in range(4 ** level) if f not in at]
    rng = np.random.default_rng(seed)
    blocks, family = [], []
    for k, m in enumerate(members):
        base = rng.integers(0, 4, 4 ** level).astype(np.uint8)
        for j, p in enumerate(at):
            base[p] = (k >> (2 * j)) & 3
        blocks.append((base, level, 2))
        family.append(k)
        seen = {base.tobytes()}
        assert not distinct or m <= 3 * len(free)
        while len(seen) <= m:
            s = base.copy()
            f = free[int(rng.integers(0, len(free)))]
            s[f] = (s[f] + int(rng.integers(1, 4))) & 3
            if distinct and s.tobytes() in seen:
                continue
            seen.add(s.tobytes() if distinct else len(seen))
            blocks.append((s, level, 2))
            family.append(k)
    return blocks, family


def test_member_lists_of_every_size(dll, hip, baker):
    """one round at level 2: leaders with 1, 2, 63, 64, 65, 257 and 1025 members, every one absorbed in round 0 and joined in one pass.  The blocks sit
    at odd byte addresses; the descriptor of the LAST block in arrayData -- which ends with its allocation -- comes first, so it leads its family"""
    members = (1, 2, 63, 64, 65, 257, 1024)
    blocks, family = _bucket_source(2, members, 4, seed=3)
    blocks.append(blocks[family.index(6)])                                            # a copy of the last family's base: with it, 1025 members
    array, descs = cu.table_of_blocks(blocks, first_offset=1)
    descs = np.concatenate([descs[-1:], descs[:-1]])                                  # descriptor 0: the last block of the array
    assert descs[0, 0] + 4 == len(array) and all(o % 2 == 1 for o in descs[:, 0])
    index = np.concatenate([np.arange(len(descs)), [0, 0, -2]])
    src = cu.Source(hip, array, descs, index, ot.IDX_U16, array_align=1)
    try:
        for mixed in (2, 3):
            ref = gu.merge_and_check(dll, hip, baker, src, limit_for(2), rounds=1, samples=4, seed=3, mixed=mixed)
            i = ref["info"]
            assert i["absorbedPerRound"][0] == i["absorbedBlocks"] == sum(members) + 1 and i["candidateBlocks"] == len(descs)
            assert int((ref["roots"] == 0).sum()) == 1026 and len(set(ref["roots"].tolist())) == len(members)
            sizes = sorted(np.bincount(ref["roots"])[sorted(set(ref["roots"].tolist()))] - 1)
            assert sizes == [1, 2, 63, 64, 65, 257, 1025]
    finally:
        src.close()


def test_a_wide_leader_with_65_members(dll, hip, baker):
    """level 6: a wave's leader takes 65 members in, beside one with a single member; the last block ends with the allocation"""
    blocks, _ = _bucket_source(6, (65, 1), 6, seed=9)
    table = cu.table_of_blocks(blocks, first_offset=3)
    src = cu.Source(hip, *table, np.arange(len(blocks)), ot.IDX_U32, array_align=1)
    try:
        for mixed in (2, 3):
            ref = gu.merge_and_check(dll, hip, baker, src, limit_for(6), rounds=1, samples=6, seed=9, mixed=mixed)
            assert ref["info"]["absorbedBlocks"] == 66 and sorted(set(ref["roots"].tolist())) == [0, 66]
    finally:
        src.close()


# ---- the parameters at their ends ----
@pytest.fixture(scope="module")
def mixed_source(hip):
    """families at levels 2 to 6 side by side, 2-state and level-0 blocks, specials and a bad entry: 300 primitives over 70 descriptors"""
    blocks = []
    for level in (2, 3, 4, 5, 6):
        blocks += families(level, (7, 5), 0.04, 70 + level)
    rng = np.random.default_rng(6)
    table = cu.table_of_blocks(blocks, first_offset=5, gap=1)
    index = np.concatenate([np.arange(len(blocks)), rng.integers(-4, len(blocks), 300 - len(blocks))])
    index[-1] = len(blocks) + 3
    src = cu.Source(hip, *table, index, ot.IDX_U16, array_align=16)
    yield src
    src.close()


@pytest.mark.parametrize("samples,rounds", [(1, 1), (1, 32), (28, 1), (28, 32), (0, 0)])
def test_samples_rounds_limits_and_seeds(dll, hip, baker, mixed_source, samples, rounds):
    """samples 1 and 28, rounds 1 and 32 and the defaults, under maxDistance 0, 5 % and 4^12 and two seeds; DisableSpecialIndices with the last"""
    absorbed = []
    for limit in (0, gu.UNIT // 20, gu.UNIT):
        for seed in (0, 0xFFFFFFFF):
            flags = gu.NO_SPECIAL if limit == gu.UNIT else 0
            ref = gu.merge_and_check(dll, hip, baker, mixed_source, limit, rounds=rounds, samples=samples, seed=seed, mixed=2 + (seed & 1), flags=flags)
            absorbed.append(ref["info"]["absorbedBlocks"])
            assert ref["info"]["skippedPrimitives"] == 1 and ref["info"]["candidateBlocks"] == 60
    assert absorbed[0] == absorbed[1] <= absorbed[2] and absorbed[2] > 0 and absorbed[4] >= absorbed[2]   # (no distance: equal blocks only, whatever the seed)
    if samples == 1 and rounds == 32:
        assert absorbed[4] > 40                                                       # (one sample, every distance allowed: few blocks are left per level)


def test_two_calls_on_a_stream_return_the_same_bytes(dll, hip, baker, mixed_source):
    stream = hip.stream_create(non_blocking=True)
    try:
        ref = gu.merge_and_check(dll, hip, baker, mixed_source, gu.UNIT // 10, stream=stream, seed=3)
        got = []
        for _ in range(2):
            r, info, handle, roots = gu.merge(dll, hip, baker, mixed_source.rd, gu.UNIT // 10, seed=3, stream=stream)
            assert r == ot.SUCCESS and info == ref["info"]
            try:
                out = cu.download_result(dll, hip, handle)
                got.append([out["array"].tobytes(), out["descs"].tobytes(), out["index"].tobytes(), roots.tobytes(), repr((out["array_hist"], out["index_hist"]))])
            finally:
                assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
        assert got[0] == got[1] and ref["info"]["absorbedBlocks"] > 0
    finally:
        hip.stream_destroy(stream)


@pytest.mark.parametrize("flags", [0, gu.NO_SPECIAL])
def test_no_distance_is_the_coarsening_at_cap_12(dll, hip, baker, mixed_source, flags):
    """maxDistance == 0 against ommxCoarsenMicromap at maxSubdivisionLevel 12 on the same source, device against device: the same arrays"""
    twice = cu.Source(hip, mixed_source.host[0], np.concatenate([mixed_source.host[1]] * 2), mixed_source.host[2] + 70 * (np.arange(300) % 2) * (mixed_source.host[2] >= 0),
                      ot.IDX_U16, array_align=16)
    try:
        r, info, merged, _ = gu.merge(dll, hip, baker, twice.rd, 0, flags=flags)
        r2, cinfo, coarse = cu.coarsen(dll, baker, twice.rd, 12, 3, flags)
        assert (r, r2) == (ot.SUCCESS, ot.SUCCESS)
        try:
            cu.assert_same(cu.download_result(dll, hip, merged), cu.download_result(dll, hip, coarse))
            assert info["absorbedBlocks"] > 0 and (info["arrayDataSize"], info["descArrayCount"]) == (cinfo["arrayDataSize"], cinfo["descArrayCount"])
        finally:
            assert dll.ommxDestroyDeviceBakeResult(merged) == ot.SUCCESS and dll.ommxDestroyDeviceBakeResult(coarse) == ot.SUCCESS
    finally:
        twice.close()


def test_a_source_without_candidates(dll, hip, baker):
    """2-state blocks of levels 0 to 7 and 4-state blocks of level 0, equal ones among them: nothing takes part, the output is the coarsening at cap 12"""
    blocks = [(cu.planted_states(level, 1, 5), level, 1) for level in range(8)] * 2 + [(np.array([s], np.uint8), 0, 2) for s in (0, 3, 3)]
    src = cu.Source(hip, *cu.table_of_blocks(blocks, first_offset=1), np.arange(len(blocks)), ot.IDX_U8, array_align=1)
    try:
        ref = gu.merge_and_check(dll, hip, baker, src, gu.UNIT, rounds=32, samples=28)
        assert ref["info"]["candidateBlocks"] == 0 and ref["info"]["absorbedBlocks"] == 0 and ref["roots"].tolist() == list(range(len(blocks)))
        cu.assert_same(ref, src.model(12))
    finally:
        src.close()


@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U32])
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
        ref = gu.merge_and_check(dll, hip, baker, src, gu.UNIT, mixed=2, flags=gu.NO_SPECIAL)
        assert ref["info"]["skippedPrimitives"] == len(invalid) > 8 and (ref["index"][invalid] == -4).all() and ref["info"]["referencedBlocks"] == 2
        assert int((ref["roots"] != gu.NONE).sum()) == 2
    finally:
        src.close()


# ---- a bake of near-copies ----
BAKE_LIMITS = (gu.UNIT * 2 // 100, gu.UNIT * 5 // 100, gu.UNIT * 10 // 100)


@pytest.fixture(scope="module")
def near_copy_bake(product, dll, hip):
    """ommxBakeDevice at level 5, 4-state, of 60 triangles over a foliage texture, each 40 times with Gaussian jitter of 0.3 texel on every vertex; the
    model's answers at 2, 5 and 10 % (computed once)"""
    tex_data = ot.foliage_texture(3, 1024, 1024, 64)
    base, _ = ot.random_triangles(5, 60, 0.08, 0.1, 0.9)
    uv = np.repeat(base.reshape(60, 3, 2), 40, axis=0)
    uv = (uv + np.random.default_rng(5).normal(0.0, 0.3 / 1024, uv.shape)).astype(np.float32).reshape(-1, 2)
    ix = np.arange(len(uv), dtype=np.uint32)
    b = product.create_baker()
    tex = product.create_texture(b, [tex_data])
    d = ot.make_desc(tex, uv, ix, 5, alpha_cutoff=0.5, fmt=ot.FMT_4STATE)
    bake = lu.DeviceBake(product, hip, b, d, uv, ix)
    try:
        a, raw, index = bake.host_arrays
        raw = raw.view(cu.RAW_DESC)
        host = (a, np.stack([raw["o"], raw["l"], raw["f"]], 1).astype(np.int64).reshape(-1, 3),
                index.view(su.INDEX_DTYPE[bake.rdesc.indexFormat]).astype(np.int64))
        unpacked = {}
        refs = [gu.restate_merge(*host, bake.rdesc.indexFormat, limit, unpacked=unpacked) for limit in BAKE_LIMITS]
        yield b, bake, host, refs
    finally:
        bake.close()
        product.destroy_texture(b, tex)
        product.destroy_baker(b)


@pytest.mark.parametrize("k", [0, 1, 2], ids=["2_percent", "5_percent", "10_percent"])
def test_a_bake_of_near_copies(dll, hip, near_copy_bake, k):
    """2400 triangles at level 5: the output equals the model, which absorbs blocks at every limit; ommxCompareMicromaps(output, source) shows neither
    CONFLICT nor B_WEAKER and loses exactly the model's known fields; the lookup, the statistics and a second merge accept the output"""
    b, bake, host, refs = near_copy_bake
    ref, limit = refs[k], BAKE_LIMITS[k]
    print("limit %d: %s" % (limit, {f: v for f, v in ref["info"].items() if f != "absorbedPerRound"}), ref["info"]["absorbedPerRound"][:8])
    assert ref["info"]["absorbedBlocks"] >= 1 and ref["info"]["candidateBlocks"] > 100           # the case is not vacuous
    if k:
        assert ref["info"]["absorbedBlocks"] >= refs[k - 1]["info"]["absorbedBlocks"] and ref["info"]["arrayDataSize"] <= refs[k - 1]["info"]["arrayDataSize"]
    r, info, handle, roots = gu.merge(dll, hip, b, bake.rdesc, limit)
    assert (r, info) == (ot.SUCCESS, ref["info"]), (info, ref["info"])
    try:
        got = cu.download_result(dll, hip, handle)
        cu.assert_same(got, ref)
        assert np.array_equal(roots, ref["roots"])
        out_rd = got["rdesc"]
        # what was lost, by the entry that is for it
        lost, kept = gu.lost_known_fields(ref, host[1], host[2])
        outputs = pu.Outputs(hip, out_rd.indexCount, ("relations",))
        try:
            r, cmp_info = pu.compare(dll, b, out_rd, bake.rdesc, 0, outputs)
            relations = outputs.download()["relations"]
        finally:
            outputs.close()
        assert r == ot.SUCCESS and not (relations & (pu.CONFLICT | pu.B_WEAKER | pu.SKIPPED)).any()
        t = cmp_info["totals"]
        assert cmp_info["conflictPrimitives"] == cmp_info["bWeakerPrimitives"] == cmp_info["skippedPrimitives"] == 0
        assert sum(sum(t, [])) == out_rd.indexCount * pu.UNIT
        known_specials = int(((host[2] == -1) | (host[2] == -2)).sum()) * pu.UNIT
        assert sum(t[sa][sb] for sa in (2, 3) for sb in (0, 1)) == lost > 0 and t[0][0] + t[1][1] == kept + known_specials
        # the consumers
        T = out_rd.indexCount
        hits = np.zeros(T, lu.HIT)
        hits["prim"], hits["u"], hits["v"] = np.arange(T), 0.3, 0.3
        after, before = lu.lookup_device(dll, hip, out_rd, hits), lu.lookup_device(dll, hip, bake.rdesc, hits)
        assert ((after == before) | (after >= 2)).all() and (after <= 3).all()
        stats, skipped = cu.device_stats(dll, b, out_rd)
        assert skipped == 0
        r, again, _, roots2 = gu.merge(dll, hip, b, out_rd, limit, want_result=False)
        assert r == ot.SUCCESS and again["referencedBlocks"] == info["descArrayCount"] and again["skippedPrimitives"] == 0
        assert (roots2 != gu.NONE).all()
    finally:
        assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
