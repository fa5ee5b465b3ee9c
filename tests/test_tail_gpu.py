"""The tail of a bake on the device (omm_amd/csrc/tail_kernels.hip: tail_summarize, dedup_insert, tail_emit, tail_rank_place / tail_place, tail_indices; the
digest kernels of bake_kernels.hip) at its digest, sort-key and placement edges: HIP library vs oracle on full result arrays, statistics included, plus
the library's own descriptors, offsets, arrayData, index buffer, index format and histograms against the numpy restatement of tests/tail_cases.py, plus
the direct statements of each family -- the order inside tie groups, special values, multisets of item digests.  tests/test_tail_reference.py holds the
restatement to the oracle on the same cases without a GPU and proves what the families cover.  No tolerances anywhere."""
import ctypes as C
from collections import Counter
import numpy as np
import pytest
import ommtest as ot
import tail_cases as tc
from test_gpu_parity import both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


def on_product(product, case, run):
    """run(baker, desc) on a fresh baker of the HIP library with the case's texture and desc"""
    b = product.create_baker()
    t = product.create_texture(b, [case["tex"]], alpha_cutoff=0.5)
    d = ot.make_desc(t, case["uv"], case["ix"], case["gmax"], **tc.desc_kw(case))
    try:
        return run(b, d)
    finally:
        product.destroy_texture(b, t)
        product.destroy_baker(b)


def triple(product, oracle, case, raw=None, hip=None):
    """both libraries bake the case, full arrays equal (test_gpu_parity.both); the library's result equals the restatement from the oracle's states under
    RAW_FLAGS; with `hip`, the device-resident entry point gives the same arrays.  Returns (library result, restatement, tail inputs)"""
    raw = raw or case.get("raw") or tc.bake(oracle, case, flags=tc.RAW_FLAGS, rejection=0.0)
    r = both(product, oracle, [case["tex"]], case["uv"], case["ix"], case["gmax"], **tc.desc_kw(case))
    inp = tc.tail_inputs(case, raw)
    rs = tc.restate_tail(inp, case["flags"], case["rejection"])
    tc.check_result(case, r, rs)
    if hip is not None:
        dev = on_product(product, case, lambda b, d: ot.bake_device(product, hip, b, d, case["uv"], case["ix"], case["levels"]))
        assert dev.same_as(r), (case["name"], dev.diff(r))
    return r, rs, inp


# ---- family K: the sort key ----
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_centroids_on_cell_edges(product, oracle, hip, fmt):
    """8192 c at k and the floats either side for k = 0, 1, 2, 4095, 4096, 8191, 8192, 8193 and their negatives, on u and on v; c inside the
    double-width cell around 0"""
    triple(product, oracle, tc.k1_case(fmt), hip=hip)


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_centroids_a_wrong_rounding_would_move(product, oracle, hip, fmt):
    """240 triangles whose cell differs under sum * (1 / 3.f), p0 + (p1 + p2) or a single rounding from double, each tied with a witness in its cell"""
    triple(product, oracle, tc.k2_case(fmt), hip=hip)


@pytest.mark.parametrize("padded", [False, True], ids=["counting-path", "sort-path"])
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_ties_are_broken_by_descending_item_index(product, oracle, hip, fmt, padded):
    case = tc.k3_case(fmt, padded)
    r, rs, inp = triple(product, oracle, case, hip=hip)
    order = np.zeros(len(r.descs), np.int64)
    order[r.index.astype(np.int64)] = np.arange(len(r.index))          # no duplicates, no special indices: descriptor -> its one triangle
    tc.tie_groups_hold(case, order, inp)
    assert (len(r.descs) > tc.RANK_MAX) == padded


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_level_leads_the_key_and_offsets_are_running_sums(product, oracle, hip, fmt):
    case = tc.k4_case(fmt)
    r, rs, inp = triple(product, oracle, case, hip=hip)
    sizes = tc.block_bytes(r.descs[:, 1], inp["bits"])
    assert np.all(np.diff(r.descs[:, 1]) <= 0) and np.array_equal(r.descs[:, 0], np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    assert r.array_data.size == sizes.sum() and (sizes < 16).sum() == rs["small"]


# ---- family P: placement counts ----
@pytest.mark.parametrize("n", tc.P_COUNTS)
def test_every_candidate_emitted_at_tile_chunk_and_path_edges(product, oracle, n):
    for fmt in tc.FORMATS:
        for mode in tc.LEVEL_MODES:
            r, rs, inp = triple(product, oracle, tc.p_all_case(n, mode, fmt))
            assert len(r.descs) == n


@pytest.mark.parametrize("fmt", tc.FORMATS)
@pytest.mark.parametrize("n,emitted", tc.P_PARTIAL)
def test_more_candidates_than_the_counting_path_takes_but_few_emitted(product, oracle, n, emitted, fmt):
    """the path choice compares the candidate bound (active items + 64, tail_kernels.hip run_tail), not the emitted count: the sort path on 1, 1024 and
    16384 keys"""
    import bench
    for mode in tc.LEVEL_MODES:
        for kind in tc.PARTIAL_KINDS:
            case = tc.p_partial_case(oracle, n, emitted, mode, fmt, kind)
            r, rs, inp = triple(product, oracle, case)
            assert len(r.descs) == emitted
            active = on_product(product, case, lambda b, d: (product.bake(b, d, want_stats=False), bench.get_timings(product, b).activeItems)[1])
            print("%s: %d active items" % (case["name"], active))
            if kind == "duplicates":
                assert active == n                                  # every candidate is non-uniform: the bound is n, beyond the counting path


# ---- family R: promotion ----
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_rejection_threshold_at_known_fractions(product, oracle, fmt):
    """rejectionThreshold on float32(k / N) of six items, one float below and above, and 1.0, 1.5, a denormal, -0.0, -1 and NaN, with and without
    special indices"""
    base4 = tc.r1_case(ot.FMT_4STATE)
    inp4 = tc.tail_inputs(base4, tc.bake(oracle, base4, flags=tc.RAW_FLAGS))
    pairs = tc.r1_pairs(tc.restate_tail(inp4, base4["flags"]), inp4["level"])
    raw = tc.bake(oracle, tc.r1_case(fmt), flags=tc.RAW_FLAGS)
    for t, pair in tc.r1_thresholds(pairs):
        for flags in tc.R1_FLAGS:
            case = tc.r1_case(fmt, flags, t)
            r, rs, inp = triple(product, oracle, case, raw)
            if pair and fmt == ot.FMT_4STATE and not flags & ot.FLAG_NO_SPECIAL:
                on = np.nonzero(~rs["uniform"] & (rs["frac"] == np.float32(t)))[0]
                tri = np.nonzero(np.isin(inp["tri_item"], on))[0]
                assert len(tri) and (r.index[tri] >= 0).all()                                   # on the threshold: kept
                tri = np.nonzero(np.isin(inp["tri_item"], np.nonzero(rs["rejected"])[0]))[0]
                assert len(tri) and (r.index[tri] == ot.SPECIAL_FUT).all()                      # below: fully unknown transparent


@pytest.mark.parametrize("first_at", tc.R2_FIRST_AT)
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_uniform_items_of_every_state_and_level(product, oracle, fmt, first_at):
    """uniform items at levels 0 - 8 in every state of the format, all-UT next to all-UO in both orders, the first of them in the last lane of a
    workgroup, the first lane of the next, or beyond work item 65 536: special values, one block per level and state class without special indices,
    every later triangle carrying the first one's value"""
    for le, gt in tc.r2_states(fmt, first_at):
        raw = None
        for flags in tc.R1_FLAGS:
            case = tc.r2_case(fmt, le, gt, first_at, flags)
            raw = raw or tc.bake(oracle, case, flags=tc.RAW_FLAGS)
            r, rs, inp = triple(product, oracle, case, raw)
            tc.r2_statements(case, r.index, rs)


# ---- family D: digests ----
def item_meta(product, hip, case):
    """[mask | known | digest lo | digest hi] x active items of the four-phase sharded API with one rank (tail_kernels.hip: shard_pack_meta)"""
    import omm_amd.sharded as sh
    dll = sh.bind(product.dll)

    def run(b, d):
        bufs = [hip.upload(case["uv"]), hip.upload(case["ix"].astype(np.int32))]
        dd = ot.BakeInputDesc.from_buffer_copy(d)
        dd.texCoords, dd.indexBuffer = bufs[0], bufs[1]
        if case["levels"] is not None:
            bufs.append(hip.upload(case["levels"]))
            dd.subdivisionLevels = bufs[2]
        h = C.c_void_p()
        assert dll.ommxShardedBegin(b, C.byref(dd), 0, 1, C.byref(h)) == ot.SUCCESS
        w, nw = C.c_void_p(), C.c_uint64()
        assert dll.ommxShardedGetMeta(h, C.byref(w), C.byref(nw)) == ot.SUCCESS
        words = hip.download(w, 4 * nw.value, np.uint32).reshape(4, -1).copy()
        assert dll.ommxShardedDestroy(h) == ot.SUCCESS
        for p in bufs:
            hip.free(p)
        return words
    return on_product(product, case, run)


def digests_hold(words, want, level=None):
    """the multiset of the digests of items with more than one state equals the multiset of XXH64 over the oracle's non-uniform blocks; the digest of
    an active item with one state is XXH64 over 4^level bytes of it"""
    mask = words[0]
    dg = words[2].astype(np.uint64) | (words[3].astype(np.uint64) << np.uint64(32))
    mixed = (mask & (mask - 1)) != 0
    got = Counter(dg[mixed].tolist())
    assert got == want, "%d digests missing, %d unexpected, of %d" % (sum((want - got).values()), sum((got - want).values()), sum(want.values()))
    if level is not None:
        for m, g in zip(mask[~mixed].tolist(), dg[~mixed].tolist()):
            assert m in (1, 2, 4, 8)
            assert g == tc.digest_of_states(np.full(4 ** level, m.bit_length() - 1, np.uint8)), (m, g)
    return int(mixed.sum()), int((~mixed).sum())


D1_IDS = ["L%d-fmt%d-%d" % c for c in tc.D1_CASES]


@pytest.mark.parametrize("level,fmt,n", tc.D1_CASES, ids=D1_IDS)
def test_item_digests_of_every_form(product, oracle, hip, level, fmt, n):
    """digest_items with its 8-, 4- and 1-byte tails (streams of 1, 4, 16 ... 1024 bytes), digest_items_lds on either side of a 64-item workgroup,
    digest_items_chain on either side of a 16-item workgroup and of the 2048-item choice between the two"""
    case = tc.d1_case(oracle, level, fmt, n)
    want, rs = tc.block_digests(case["raw"], case)
    words = item_meta(product, hip, case)
    mixed, one_state = digests_hold(words, want, level)
    print("%s: %d active items, %d of one state" % (case["name"], words.shape[1], one_state))
    if level >= 5:
        assert words.shape[1] == n == mixed                # every item non-uniform: this is the count the choice of the form sees
    elif level == 0:
        assert one_state >= 30 and mixed == 0              # the 1-byte stream is digested on the device only here: by active items of one state
    else:
        assert mixed >= 30
    triple(product, oracle, case)


def test_item_digests_of_four_levels_in_one_bake(product, oracle, hip):
    """levels 3, 5, 6, 7 and 8 at once: the small form, two segments of the multi-level LDS launch (level 6 has more than 2048 active items) and two of
    the multi-level chain launch, each with its blockStart search"""
    case = tc.d1_multi_level_case()
    raw = tc.bake(oracle, case, flags=tc.RAW_FLAGS)
    want, rs = tc.block_digests(raw, case)
    mixed, one_state = digests_hold(item_meta(product, hip, case), want)
    assert mixed == sum(want.values()) > 2048 + 200
    triple(product, oracle, case, raw)


# ---- near twins and true twins ----
def streamed_too(product, case, r, to_the_end=True):
    """the streamed result of ommCpuBake forced to 1, 3 and 7 ranges (levels >= 6 stream): the digests then come from the range-by-range forms.
    to_the_end: the bake must finish as a streamed one (duplicates across ranges may make it fall back to the ordinary gather, having streamed).
    Returns the timings of the three bakes"""
    import bench
    seen = []
    if case["gmax"] >= 6:
        for chunks in (1, 3, 7):
            s = tc.bake(product, case, knobs=[(ot.KNOB_STREAM_CHUNKS, chunks)], inspect=lambda b: seen.append(bench.get_timings(product, b)))
            assert s.same_as(r), (case["name"], chunks, s.diff(r))
        print("%s: ranges %r, early items %r, streamed bytes %r" % (case["name"], [t.streamChunks for t in seen], [t.streamEarlyItems for t in seen], [t.streamedBytes for t in seen]))
        assert all(t.streamedBytes > 0 for t in seen)          # the bake did stream
        assert not to_the_end or [t.streamChunks for t in seen] == [1, 3, 7]
    return seen


TWIN_IDS = ["L%d-fmt%d-part%d" % c for c in tc.TWIN_CASES]


@pytest.mark.parametrize("level,fmt,part", tc.TWIN_CASES, ids=TWIN_IDS)
def test_near_twins_keep_a_descriptor_each(product, oracle, hip, level, fmt, part):
    """work items whose blocks differ in one micro-triangle and nowhere else -- in every packed byte (levels to 5 / 6), every 16 bytes (6, 7), the first
    and last 16 bytes of every 256-byte (8) and 1 KiB (9) chunk: a digest that drops or repeats a piece of its stream merges two of them"""
    orders = ("untouched", "moved") if level <= 7 else (("untouched", "moved")[part % 2],)
    for first in orders:
        case = tc.twin_case(level, fmt, part, tc.twin_parts(level), first=first)
        r, rs, inp = triple(product, oracle, case, hip=hip)
        n = len(case["uv"]) // 3
        assert len(r.descs) == n and sorted(r.index.tolist()) == list(range(n))
        streamed_too(product, case, r)


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_true_twins_merge_into_the_first(product, oracle, hip, fmt):
    for level in [L for L in tc.TWIN_LEVELS[fmt] if L <= 7]:
        case = tc.twin_case(level, fmt, true_twins=True)
        r, rs, inp = triple(product, oracle, case, hip=hip)
        assert len(r.descs) == 1 and (r.index == 0).all() and np.array_equal(r.array_data, tc.pack_states(inp["groups"][level][1][:1], inp["bits"])[0])
        streamed_too(product, case, r, to_the_end=False)


def test_blocks_that_differ_only_by_ut_against_uo_merge_into_the_first(product, oracle, hip):
    case = tc.ut_uo_case(oracle)
    r, rs, inp = triple(product, oracle, case, hip=hip)
    assert len(case["pairs"]) >= 8
    for a, b in case["pairs"]:
        assert r.index[a] == r.index[b] >= 0
        off, L = r.descs[r.index[a]][:2]
        states = tc.unpack_block(r.array_data[None, off:off + int(tc.block_bytes(L, 2))], 4 ** L, 2)[0]
        ids, S = inp["groups"][int(L)]
        assert np.array_equal(states, S[np.nonzero(ids == a)[0][0]])          # the bytes of the lower work item, UT and UO as it has them


def test_near_twins_that_share_their_preview_reach_the_early_list(product, oracle, hip):
    """four level-6 items equal at level 5 and different in one level-6 micro-triangle each: a streamed bake of several ranges classifies them early
    (their digests come from the early list of a range) and must still give each its own descriptor"""
    case = tc.early_twin_case(oracle)
    r, rs, inp = triple(product, oracle, case, hip=hip)
    n = len(case["uv"]) // 3
    assert len(r.descs) == n and len(set(r.index[case["twins"]].tolist())) == 4
    seen = streamed_too(product, case, r)
    assert all(t.streamEarlyItems >= 4 for t in seen[1:])


def test_streamed_blocks_that_differ_only_by_ut_against_uo_merge_into_the_first(product, oracle, hip):
    """seven level-6 items of one digest whose blocks hold T, UT and UO and differ by UT against UO in one micro-triangle each, three of them early
    with the untouched one: the range-by-range digest forms fold UT into UO like every other, the first triangle of the input keeps the block
    with its own bytes, through ommCpuBake, the device-resident path and the streamed result in 1, 3 and 7 ranges"""
    case = tc.ut_uo_streamed_case(oracle)
    r, rs, inp = triple(product, oracle, case, hip=hip)
    twins = case["twins"]
    assert twins[0] == 0 and len(set(r.index[twins].tolist())) == 1 and r.index[0] >= 0
    assert len(r.descs) == len(case["uv"]) // 3 - len(twins) + 1
    off = int(r.descs[r.index[0]][0])
    assert np.array_equal(tc.unpack_block(r.array_data[None, off:off + 1024], 4 ** tc.EARLY_LEVEL, 2)[0], inp["groups"][tc.EARLY_LEVEL][1][0])
    seen = streamed_too(product, case, r, to_the_end=False)
    assert all(t.streamEarlyItems >= 4 for t in seen[1:])
