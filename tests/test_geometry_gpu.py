"""ommxExtractMicroGeometry / ommxExpandMicroNodes on the GPU.  Every case compares all four record arrays, the primitive offsets, the counts and the
skipped count with tests/geometry_util.py's restate_cut byte for byte, and every byte of the arena outside the outputs must be unchanged.  The shapes are
the tier edges of the cut (a lane's word, part of a wave, one tile, a word of tiles, 4096 tiles), not a workload."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import geometry_util as gu
import workloads as wl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    return gu.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


# ---- block levels ----
@pytest.mark.parametrize("bits", [1, 2], ids=["2state", "4state"])
@pytest.mark.parametrize("level", [0, 1, 2, 3, 4, 5, 6, 7, 9])
def test_block_levels(dll, hip, baker, level, bits):
    """one block per pattern (uniform in each state, one odd micro-triangle at the word / tile edges, alternation per 1 / 4 / 64 / 4096, random with 1 % and
    50 % minority, four quarters) plus the specials and a block selected twice; the array at an odd address (byte path) and at a 16-byte aligned one"""
    array_data, descs, index = gu.pattern_table(level, bits, gu.ALL_PATTERNS)
    gu.extract_and_check(dll, hip, baker, array_data, descs, index, ot.IDX_U16, gu.IDENTITY, array_align=1)
    gu.extract_and_check(dll, hip, baker, array_data, descs, index, ot.IDX_U16, gu.IDENTITY, array_align=16)
    gu.extract_and_check(dll, hip, baker, array_data, descs, index, ot.IDX_U8, gu.PRESET, array_align=16)


@pytest.mark.parametrize("bits", [1, 2], ids=["2state", "4state"])
def test_level_10(dll, hip, baker, bits):
    """256 tiles: four words of tiles under a partial top word"""
    array_data, descs, index = gu.pattern_table(10, bits, gu.BIG_PATTERNS)
    gu.extract_and_check(dll, hip, baker, array_data, descs, index, ot.IDX_U32, gu.IDENTITY, array_align=16)


def test_level_12(dll, hip, baker):
    """4096 tiles, all four tiers full: two blocks, one of each format (the 2-state one at an odd address)"""
    rng = np.random.default_rng(12)
    sparse = np.ones(4 ** 12, np.uint8)          # 2000 odd micro-triangles: tens of thousands of records, not millions
    sparse[rng.integers(0, 4 ** 12, 2000)] = rng.integers(0, 4, 2000)
    blocks = [(sparse, 12, 2), (gu.pattern("except:4096", 12, 1), 12, 1)]
    array_data, descs = gu.table_of_blocks(blocks, first_offset=16, gap=1)
    gu.extract_and_check(dll, hip, baker, array_data, descs, [0, 1, -2, 0], ot.IDX_U32, gu.GDesc((0, 1, 2, 2), 0, 0xFFFFFFFF), array_align=16)
    uniform = [(gu.pattern("uniform:1", 12, 2), 12, 2), (gu.pattern("quarters", 12, 2), 12, 2)]
    array_data, descs = gu.table_of_blocks(uniform)
    ref = gu.extract_and_check(dll, hip, baker, array_data, descs, [0, 1], ot.IDX_U32, gu.IDENTITY, array_align=16)
    assert ref["counts"] == [1, 2, 1, 1] and ref["nodes"][1]["node"].tolist() == [0, (1 << 24) | 1]   # a whole block is one level-0 node


# ---- maxEmitLevel ----
@pytest.mark.parametrize("mixed", [1, 3, gu.DROP], ids=["mixed_shared", "mixed_own", "mixed_drop"])
@pytest.mark.parametrize("level,bits", [(7, 1), (7, 2), (9, 2)])
def test_max_emit_level(dll, hip, baker, level, bits, mixed):
    array_data, descs, index = gu.pattern_table(level, bits, gu.ALL_PATTERNS, first_offset=3)
    for emit in sorted({0, 1, level - 7, level - 6, level - 5, level - 3, level - 1, level, 12, 0xFFFFFFFF}):
        gu.extract_and_check(dll, hip, baker, array_data, descs, index, ot.IDX_U16, gu.GDesc((0, 1, 2, 2), mixed, emit), array_align=1 if emit & 1 else 16)


# ---- listOfState ----
MAPPINGS = {"identity": gu.IDENTITY, "one_list": gu.GDesc((2, 2, 2, 2), 2, 12), "preset": gu.PRESET, "preset_whole": gu.PRESET_WHOLE,
            "unknowns_merged": gu.GDesc((0, 1, 2, 2), 3, 12), "force_2state": gu.GDesc((gu.DROP, 0, gu.DROP, 0), 1, 12)}


@pytest.mark.parametrize("name", sorted(MAPPINGS))
def test_list_mappings(dll, hip, baker, name):
    for level in (5, 7):
        array_data, descs, index = gu.pattern_table(level, 2, gu.ALL_PATTERNS, first_offset=1, gap=3)
        gu.extract_and_check(dll, hip, baker, array_data, descs, index, ot.IDX_U32, MAPPINGS[name])


def test_every_state_dropped(dll, hip, baker):
    """zero counts, and with outputs of capacity 0 nothing but the offsets (all zero) is written"""
    array_data, descs, index = gu.pattern_table(7, 2, gu.ALL_PATTERNS)
    ref = gu.extract_and_check(dll, hip, baker, array_data, descs, index, ot.IDX_U16, gu.GDesc((gu.DROP,) * 4, gu.DROP, 12), slack=2)
    assert ref["counts"] == [0, 0, 0, 0] and ref["skipped"] == 0


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
    declared = (len(tb["array"]), len(tb["descs"]), len(rows))
    ref = gu.extract_and_check(dll, hip, baker, array_data, descs, index, index_format, gu.IDENTITY, declared=declared)
    assert ref["skipped"] == sum(1 for r in rows if r[1] == lu.INVALID) > 8
    ref = gu.extract_and_check(dll, hip, baker, array_data, descs, index, index_format, gu.PRESET_WHOLE, declared=(0, len(tb["descs"]), len(rows)))
    assert ref["skipped"] == len(rows) - 4          # arrayDataSize 0: only the specials are answered


@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32])
def test_statistics_table(dll, hip, baker, index_format):
    """stats_util's table: levels 0 - 3 in both formats at odd offsets with random bytes (garbage in the unused bits of the one-byte blocks), a level-7 and
    a level-9 block at odd addresses, level 13, formats 0 and 3, a block one byte past the array, the specials, -5 and descArrayCount, a block three times"""
    array_data, descs, index, _ = su.table_arrays()
    for g in (gu.IDENTITY, gu.PRESET, gu.GDesc((0, 1, 0, 1), 2, 2)):
        ref = gu.extract_and_check(dll, hip, baker, array_data, descs, index, index_format, g)
        assert ref["skipped"] == 8


def test_shared_blocks(dll, hip, baker):
    """a block shared by 1, 3 and 300 primitives: cut once, written per primitive"""
    blocks = [(gu.pattern("random:50", 4, 2), 4, 2), (gu.pattern("random:1", 7, 2), 7, 2), (gu.pattern("alternate:4", 6, 1), 6, 1)]
    array_data, descs = gu.table_of_blocks(blocks, first_offset=5, gap=2)
    index = [0] + [1] * 3 + [-1] + [2] * 300
    gu.extract_and_check(dll, hip, baker, array_data, descs, index, ot.IDX_U8, gu.IDENTITY)
    gu.extract_and_check(dll, hip, baker, array_data, descs, index[::-1], ot.IDX_U16, gu.PRESET)


# ---- launch shapes ----
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097, (1 << 18) + 17])
def test_launch_shapes(dll, hip, baker, count):
    """level-2 blocks, many primitives: the primitive scans across many workgroups, on a caller's stream"""
    rng = np.random.default_rng(count)
    blocks = [(rng.integers(0, 4, 16).astype(np.uint8) * (rng.random(16) < 0.5), 2, 2) for _ in range(40)]
    array_data, descs = gu.table_of_blocks(blocks, first_offset=1, gap=1)
    index = rng.integers(-6, 42, count)          # the specials, -5, -6 and two entries beyond descArrayCount among them
    stream = hip.stream_create(non_blocking=True)
    try:
        gu.extract_and_check(dll, hip, baker, array_data, descs, index, ot.IDX_U8, gu.PRESET, stream=stream)
    finally:
        hip.stream_destroy(stream)


def test_behind_a_kernel_that_writes_the_index_buffer(dll, hip, baker):
    """the index buffer is filled on the caller's non-blocking stream (a memset kernel) and the extraction is enqueued behind it without a wait between"""
    count = (1 << 18) + 17
    blocks = [(gu.pattern("alternate:%d" % (1 + 3 * (k % 2)), 2, 2), 2, 2) for k in range(8)]
    array_data, descs = gu.table_of_blocks(blocks)
    ref = gu.restate_cut(array_data, descs, np.full(count, 5), gu.IDENTITY)
    call = gu.Call(hip, array_data, descs, np.full(count, 0x7F), ot.IDX_U8, ref["counts"])
    stream = hip.stream_create(non_blocking=True)
    try:
        hip.rt.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        assert hip.rt.hipMemsetAsync(call.im.ptr("index"), 5, count, stream) == 0
        at = call.im.parts["index"][0]
        call.im.before[at:at + count] = 5
        r, counts, skipped = call.run(dll, baker, gu.IDENTITY, stream)
        assert (r, counts, skipped) == (ot.SUCCESS, ref["counts"], 0)
        call.check(ref)
    finally:
        hip.stream_destroy(stream)
        call.free()


# ---- count-only and capacity ----
def test_capacity_and_optional_outputs(product, dll, hip):
    array_data, descs, index = gu.pattern_table(7, 2, gu.ALL_PATTERNS, first_offset=1)
    g = gu.IDENTITY
    ref = gu.restate_cut(array_data, descs, index, g)
    assert all(c > 1 for c in ref["counts"])
    msgs = []
    lib = ot.Lib("product")      # (a Lib keeps one callback alive: this baker gets a Lib of its own)
    b = lib.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    try:
        gu.extract_and_check(dll, hip, b, array_data, descs, index, ot.IDX_U16, g, slack=0)         # capacity exact
        for short in range(4):                                                                       # one short on one list
            call = gu.Call(hip, array_data, descs, index, ot.IDX_U16, [c - (k == short) for k, c in enumerate(ref["counts"])])
            r, counts, skipped = call.run(dll, b, g)
            assert (r, counts, skipped) == (gu.INSUFFICIENT, ref["counts"], 0) and len(msgs) == short + 1 and "capacity" in msgs[-1][1]
            call.check(ref, written=False)
            call.free()
        # nodes[k] == NULL for some lists only (their capacity does not matter); offsets for others only
        call = gu.Call(hip, array_data, descs, index, ot.IDX_U16, [None, ref["counts"][1], None, ref["counts"][3] + 5], offsets=(True, False, False, True))
        r, counts, _ = call.run(dll, b, g)
        assert (r, counts) == (ot.SUCCESS, ref["counts"])
        call.check(ref)
        call.free()
        # only primitiveOffsets
        call = gu.Call(hip, array_data, descs, index, ot.IDX_U16, [None] * 4)
        r, counts, _ = call.run(dll, b, g)
        assert (r, counts) == (ot.SUCCESS, ref["counts"])
        call.check(ref)
        call.free()
        assert len(msgs) == 4
    finally:
        lib.destroy_baker(b)


# ---- real results ----
def real_cases():
    yield "c0_4state", "c0", None, ot.FMT_4STATE
    yield "c1_4state", "c1", 3000, ot.FMT_4STATE
    yield "cards_4state", "cards", 200, ot.FMT_4STATE
    yield "cards_2state", "cards", 200, ot.FMT_2STATE


@pytest.mark.parametrize("name,kind,tris,fmt", list(real_cases()), ids=[c[0] for c in real_cases()])
def test_real_results(product, dll, hip, name, kind, tris, fmt):
    """ommxBakeDevice results, first preset: the extraction equals restate_cut of the downloaded arrays; for 10^5 interior hits the list of the one node
    that contains the hit is listOfState[ommxLookupOpacity(hit)]; a caller-filled desc over device copies of the ommCpuBake result gives the same
    records; two calls give identical bytes; a handle that is no baker is refused"""
    tex, uv, ix, lv, kw = wl.workload(kind, tris)
    kw = dict(kw, fmt=fmt)
    level = kw.pop("level")
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    g = gu.PRESET
    try:
        d = ot.make_desc(t, uv, ix, level, levels=lv, **kw)
        bake = lu.DeviceBake(product, hip, b, d, uv, ix, lv)
        try:
            res = bake.host
            ref = gu.restate_cut(res.array_data, res.descs, res.index, g)
            print(name, "triangles", len(res.index), "blocks", len(res.descs), "records", ref["counts"], "skipped", ref["skipped"])
            assert ref["skipped"] == 0 and ref["counts"][0] > 0 and (fmt == ot.FMT_2STATE or ref["counts"][1] > 0)
            first = gu.extract_device(dll, hip, b, bake.rdesc, g, ref)
            again = gu.extract_device(dll, hip, b, bake.rdesc, g, ref)
            assert all(np.array_equal(x, y) for x, y in zip(first, again))
            # the two consumers agree
            rng = np.random.default_rng(5)
            plevel, has = lu.prim_levels(res)
            prims = rng.integers(0, len(res.index), 100000)
            micro = (rng.random(len(prims)) * (4.0 ** plevel[prims])).astype(np.int64)
            u, v = lu.interior_points(rng, lu.micro_vertices(micro, plevel[prims]))
            hits = np.empty(len(prims), lu.HIT)
            hits["prim"], hits["u"], hits["v"] = prims, u, v
            states = lu.lookup_device(dll, hip, bake.rdesc, hits)
            assert (states < 4).all() and np.array_equal(states, lu.numpy_states(res, prims, micro))
            nodes = [x.view(gu.NODE) for x in first]
            got = gu.list_of_hits(nodes, plevel, prims, micro)
            assert np.array_equal(got, np.array(g.list_of_state, np.int64)[states])
            # the ommCpuBake result of the same desc, copied to the device by the caller
            host = product.bake(b, d)
            copy = lu.DeviceResult(hip, *lu.host_arrays_of(host), host.index_format)
            try:
                assert host.same_as(res), host.diff(res)
                mine = gu.extract_device(dll, hip, b, copy.rdesc, g, ref)
                assert all(np.array_equal(x, y) for x, y in zip(first, mine))
            finally:
                copy.close()
            counts = (C.c_uint64 * 4)()
            assert dll.ommxExtractMicroGeometry(t, C.byref(bake.rdesc), C.byref(gu.c_desc(g)), None, counts, None, None) == ot.INVALID_ARGUMENT
        finally:
            bake.close()
    finally:
        product.destroy_texture(b, t)
        product.destroy_baker(b)


# ---- ommxExpandMicroNodes ----
CANARY = 256


def expand(dll, hip, nodes, count, mesh, want_bary=True, want_pos=True, stream=None):
    """-> (barycentric bytes as uint32 (count, 3, 2), position bytes as uint32 (count, 3, 3)); the canaries around both outputs must be intact"""
    d_nodes = hip.upload(nodes if len(nodes) else np.zeros(1, gu.NODE))
    bufs = [hip.upload(np.full(4 * n * count + 2 * CANARY, 0xAB, np.uint8)) if want else None for n, want in ((6, want_bary), (9, want_pos))]
    try:
        r = dll.ommxExpandMicroNodes(d_nodes, count, C.byref(mesh) if mesh is not None else None,
                                     C.c_void_p(bufs[0].value + CANARY) if bufs[0] else None, C.c_void_p(bufs[1].value + CANARY) if bufs[1] else None, stream)
        assert r == ot.SUCCESS, r
        lu.sync(hip)
        out = []
        for p, n in zip(bufs, (6, 9)):
            if p is None:
                out.append(None)
                continue
            raw = hip.download(p, 4 * n * count + 2 * CANARY)
            assert (raw[:CANARY] == 0xAB).all() and (raw[CANARY + 4 * n * count:] == 0xAB).all(), "bytes outside an output were written"
            out.append(raw[CANARY:CANARY + 4 * n * count].copy().view(np.uint32).reshape(count, 3, n // 3))
        return out
    finally:
        hip.free(d_nodes)
        for p in bufs:
            if p is not None:
                hip.free(p)


@pytest.fixture(scope="module")
def expand_records():
    """the records of a cut with nodes of every level 0..6 over 40 primitives, then malformed nodes and primitives past the mesh's 40 triangles"""
    rng = np.random.default_rng(21)
    blocks = [(gu.pattern(name, level, 2, seed=level), level, 2) for level in range(7) for name in ("random:1", "random:50", "uniform:1", "quarters", "alternate:4")]
    array_data, descs = gu.table_of_blocks(blocks)
    ref = gu.restate_cut(array_data, descs, list(range(35)) + [-2, -4, 7, 7, 33], gu.IDENTITY)
    good = np.concatenate(ref["nodes"])
    bad = np.zeros(8, gu.NODE)
    bad["prim"] = [0, 1, 2, 3, 40, 41, 0xFFFFFFFF, 5]
    bad["node"] = [13 << 24, (2 << 24) | 16, (11 << 24) | (1 << 22), 0xFF000000, 0, (3 << 24) | 5, 0, (0 << 24) | 1]
    nodes = np.concatenate([good, bad, good[:50]])
    assert set((good["node"] >> 24).tolist()) == set(range(7))
    pos = (rng.random((100, 3)).astype(np.float32) - np.float32(0.5)) * np.float32(37.0)
    tri = rng.integers(0, 100, (40, 3))
    return nodes, len(good), pos, tri


@pytest.mark.parametrize("index_format,stride", [(ot.IDX_U8, 12), (ot.IDX_U16, 16), (ot.IDX_U32, 28), (ot.IDX_U32, 0)])
def test_expand(dll, hip, expand_records, index_format, stride):
    nodes, n_good, pos, tri = expand_records
    step = stride or 12
    raw = np.full((len(pos), step), 0xCD, np.uint8)
    raw[:, :12] = pos.view(np.uint8).reshape(len(pos), 12)
    d_pos, d_tri = hip.upload(raw), hip.upload(tri.astype({ot.IDX_U8: np.uint8, ot.IDX_U16: np.uint16, ot.IDX_U32: np.uint32}[index_format]).reshape(-1))
    try:
        mesh = gu.MicroMeshDesc(d_pos, stride, d_tri, index_format, len(tri))
        want_bary, want_pos = gu.expand_reference(nodes, pos, tri, len(tri))
        bary, got = expand(dll, hip, nodes, len(nodes), mesh)
        assert np.array_equal(bary, want_bary.view(np.uint32)) and np.array_equal(got, want_pos.view(np.uint32))
        bad = slice(n_good, n_good + 8)
        assert (bary[bad] == gu.NAN_BITS).all() and (got[bad] == gu.NAN_BITS).all() and not (bary[:n_good] == gu.NAN_BITS).any()
        # without a mesh only the node decides: primitives 40, 41 and 0xFFFFFFFF have barycentrics
        only_bary, none = expand(dll, hip, nodes, len(nodes), None, want_pos=False)
        assert none is None and np.array_equal(only_bary, gu.expand_reference(nodes)[0].view(np.uint32)) and not (only_bary[n_good + 4] == gu.NAN_BITS).any()
        # corner vertices equal the mesh's bits
        roots = np.nonzero(nodes["node"][:n_good] == 0)[0]
        assert len(roots) >= 3
        assert np.array_equal(got[roots], pos[tri[nodes["prim"][roots]]].view(np.uint32))
        # vertices shared by nodes of one primitive are bit-identical: group every vertex by (primitive, u, v)
        key = np.stack([np.repeat(nodes["prim"][:n_good], 3), bary[:n_good, :, 0].reshape(-1), bary[:n_good, :, 1].reshape(-1)], 1).astype(np.int64)
        order = np.lexsort(key.T[::-1])
        k, p = key[order], got[:n_good].reshape(-1, 3)[order]
        same = (k[1:] == k[:-1]).all(axis=1)
        assert same.sum() > 1000 and (p[1:][same] == p[:-1][same]).all()
        # positions only
        none, only_pos = expand(dll, hip, nodes, len(nodes), mesh, want_bary=False)
        assert none is None and np.array_equal(only_pos, got)
    finally:
        hip.free(d_pos)
        hip.free(d_tri)


@pytest.mark.parametrize("count", [0, 1, 65, (1 << 20) + 3])
def test_expand_counts(dll, hip, expand_records, count):
    """0 (no launch), 1, 65 and 2^20 + 3 records (the grid strides), on a caller's stream, canaries around both outputs"""
    nodes, n_good, pos, tri = expand_records
    many = np.tile(nodes, count // len(nodes) + 1)[:count]
    d_pos, d_tri = hip.upload(pos), hip.upload(tri.astype(np.uint32).reshape(-1))
    stream = hip.stream_create(non_blocking=True)
    try:
        mesh = gu.MicroMeshDesc(d_pos, 12, d_tri, ot.IDX_U32, len(tri))
        bary, got = expand(dll, hip, many, count, mesh, stream=stream)
        want_bary, want_pos = gu.expand_reference(many, pos, tri, len(tri))
        assert np.array_equal(bary, want_bary.view(np.uint32).reshape(count, 3, 2)) and np.array_equal(got, want_pos.view(np.uint32).reshape(count, 3, 3))
    finally:
        hip.stream_destroy(stream)
        hip.free(d_pos)
        hip.free(d_tri)
