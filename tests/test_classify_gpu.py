"""The classification's work distribution on the device (omm_amd/csrc/bake_kernels.hip: triage_items, triage_tiles, triage_groups, classify_tiles,
classify_generic) at its tile, group and chunk edges.  Every case of tests/classify_cases.py goes through both libraries (full result arrays and
statistics equal, test_gpu_parity.both); the counters of ommxBakeTimings are then held to the restated schedule in the three modes of a case (classify_cases' docstring) --
"table" (Linear with DisableLevelLineIntersection: the schedule is exactly the table's), "nearest" (nothing is triaged: everything is open, exactly)
and "linear" (the hot path: between the restatement's bounds) --; the join and window cases also go through ommxBakeDevice and through
ommCpuBake streamed in 1, 3 and 7 ranges (asserted to have streamed: sections cut the queue, windows are per section), byte-identical to the
unstreamed result under the same flags.
tests/test_classify_reference.py proves without a GPU what each case covers.  No tolerances anywhere."""
import numpy as np
import pytest
import bench
import ommtest as ot
import classify_cases as cc
from classify_cases import tc
from test_gpu_parity import both

pytestmark = pytest.mark.gpu
MODES = cc.MODES
STREAM_RANGES = [1, 3, 7]


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


def parity(product, oracle, case, knobs=()):
    return both(product, oracle, case.get("mips") or [case["tex"]], case["uv"], case["ix"], case["gmax"], knobs=knobs, **tc.desc_kw(case))


def on_product(product, case, run, knobs=()):
    b = product.create_baker()
    for k, v in knobs:
        product.set_knob(b, k, v)
    t = product.create_texture(b, case.get("mips") or [case["tex"]], alpha_cutoff=0.5)
    d = ot.make_desc(t, case["uv"], case["ix"], case["gmax"], **tc.desc_kw(case))
    try:
        return run(b, d)
    finally:
        product.destroy_texture(b, t)
        product.destroy_baker(b)


def baked_with_timings(product, case, knobs=()):
    return on_product(product, case, lambda b, d: (product.bake(b, d), bench.get_timings(product, b)), knobs)


def counters(tm):
    return dict(activeItems=tm.activeItems, openTiles=tm.openTiles, openTileMicroTriangles=tm.openTileMicroTriangles, fineMicroTriangles=tm.fineMicroTriangles)


def scheduled(product, oracle, case, r, knobs=()):
    """the library's counters against the restated schedule of the case; r = the result both libraries agreed on"""
    s = cc.restate_schedule(case, exact_fine=True)
    r2, tm = baked_with_timings(product, case, knobs)
    assert r2.same_as(r), (case["name"], r2.diff(r))
    got = counters(tm)
    print(case["name"], got, s["fineExact"])
    want = {k: s[k] for k in got}
    if case["mode"] == "nearest":
        assert got == want, (case["name"], got, want)
    elif case["mode"] == "table":
        fine = got.pop("fineMicroTriangles")
        assert got == {k: s[k] for k in got} and s["fineLower"] <= fine <= s["fineMicroTriangles"], (case["name"], got, fine, want, s["fineLower"])
        if s["fineExact"] is not None:      # (Wrap, and no micro-triangle's rectangle edge within 1e-3 texel of a rounding step)
            assert fine == s["fineExact"], (case["name"], fine, s["fineExact"])
    else:
        lo, hi = cc.linear_bounds(case, s, cc.oracle_states(oracle, case))      # (they coincide but for dead records: test_classify_reference.py)
        assert lo <= got["openTiles"] <= hi and got["activeItems"] <= s["activeItems"], (case["name"], got, lo, hi)
        assert got["openTileMicroTriangles"] == (1024 if s["small"] else 4096) * got["openTiles"] and not (s["small"] and s["records"])
    return s


def every_entry_point(product, oracle, hip, case, r):
    """ommxBakeDevice, and ommCpuBake streamed in 1, 3 and 7 ranges.  A bake streams only with special indices enabled and without
    DisableLevelLineIntersection (omm_host.cpp: the plain path handles the others), so the streamed bakes -- and the oracle's and the unstreamed bake
    they are compared with -- run under FLAG_THREADS | FLAG_NO_DEDUP in the linear and nearest modes, and each is asserted to have streamed.  A range
    ends on a work item, so only bakes of several items are really cut: `items`, `four`, `level6`, `level6-plus7`."""
    dev = on_product(product, case, lambda b, d: ot.bake_device(product, hip, b, d, case["uv"], case["ix"], case["levels"]))
    assert dev.same_as(r), (case["name"], "ommxBakeDevice", dev.diff(r))
    if case["mode"] == "table" or case["gmax"] < 6:
        return
    c = dict(case, flags=ot.FLAG_THREADS | ot.FLAG_NO_DEDUP)
    ref = parity(product, oracle, c)
    seen = []
    for k in STREAM_RANGES:
        st, tm = baked_with_timings(product, c, knobs=[(ot.KNOB_STREAM_CHUNKS, k)])
        assert st.same_as(ref), (case["name"], "streamed in %d" % k, st.diff(ref))
        seen.append((tm.streamChunks, tm.streamedBytes, tm.streamEarlyItems))
    print(case["name"], "ranges, streamed bytes, early items:", seen, "blocks:", len(ref.descs))
    if len(ref.descs):          # (a bake whose items are all uniform has no block to stream)
        assert [x[0] for x in seen] == STREAM_RANGES and all(x[1] > 0 for x in seen), (case["name"], seen)


# ---- family J: the chunk join ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", cc.J_NAMES)
def test_chunk_join(product, oracle, hip, name, mode):
    for fp32 in (False, True):
        case = cc.variant(cc.j_case(name), mode=mode, fp32=fp32)
        r = parity(product, oracle, case)
        scheduled(product, oracle, case, r)
        if not fp32:
            every_entry_point(product, oracle, hip, case, r)
    parity(product, oracle, cc.variant(cc.j_case(name), mode=mode, fmt=ot.FMT_2STATE))


# ---- family W: the LDS window ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", cc.W_NAMES)
def test_lds_window(product, oracle, hip, name, mode):
    for fp32 in (False, True):
        case = cc.variant(cc.w_case(name), mode=mode, fp32=fp32)
        r = parity(product, oracle, case)
        scheduled(product, oracle, case, r)
        if fp32:
            every_entry_point(product, oracle, hip, case, r)


# ---- family M: the sums through what reads them ----
@pytest.mark.parametrize("mode", MODES)
def test_dead_tile_of_a_uniform_item(product, oracle, mode):
    """the defect lies in the box of a hypotenuse tile, outside the item: an open tile without an open group; the mask of its 64 settled groups alone
    makes the item uniform"""
    case = cc.variant(cc.m_dead_case(), mode=mode)
    r = parity(product, oracle, case)
    assert r.index.tolist() == [ot.SPECIAL_FO] and len(r.descs) == 0
    s = scheduled(product, oracle, case, r)
    assert mode == "nearest" or [x["open"] for x in s["records"]] == [0]


@pytest.mark.parametrize("fp32", [False, True], ids=["u8", "fp32"])
def test_known_count_of_three_sources_at_the_rejection_threshold(product, oracle, fp32):
    """rejectionThreshold at float32(known / 4^N), the float below and the float above: kept, kept, rejected -- known counted by triage_tiles, by
    triage_groups and by classify_tiles"""
    base = cc.m_threshold_case(fp32, 0.0)
    st = cc.oracle_states(oracle, base)
    tiles, groups, rest, known = cc.m_sources(cc.restate_schedule(base), st)
    assert tiles > 0 and groups > 0 and rest > 0 and known < st[0].size
    for t, kept in cc.m_thresholds(known, st[0].size):
        r = parity(product, oracle, cc.m_threshold_case(fp32, t))
        assert (r.index[0] >= 0) == kept, (t, kept, r.index)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", cc.M5_COUNTS)
def test_level_5_items(product, oracle, hip, n, mode):
    """the 1024-tile queue: 16 groups per tile, four tiles per wave of triage_groups; patterns none / all 16 / group 0 / group 15 / alternating in cells
    above and below the cut-off in turn"""
    for fp32 in (False, True):
        case = cc.m5_case(n, fp32=fp32, mode=mode)
        r = parity(product, oracle, case)
        s = scheduled(product, oracle, case, r)
        assert got_small(s, n)
    every_entry_point(product, oracle, hip, case, r)
    parity(product, oracle, cc.m5_case(n, mode=mode, fmt=ot.FMT_2STATE))


def got_small(s, n):
    return len(s["small"]) == n and not s["records"] and s["openTileMicroTriangles"] == 1024 * n


@pytest.mark.parametrize("n", [n for n in cc.M5_COUNTS if n >= 3])
def test_level_5_known_count_at_the_rejection_threshold(product, oracle, n):
    base = cc.m5_case(n, mode="linear")
    st = cc.oracle_states(oracle, base)
    item = cc.m5_threshold_item(n)
    tiles, groups, rest, known = cc.m_sources(cc.restate_schedule(base), st, item)
    assert tiles == 0 and rest > 0 and known < 1024 and (groups > 0) == (n >= 5)
    for t, kept in cc.m_thresholds(known, 1024):
        r = parity(product, oracle, cc.m5_case(n, mode="linear", rejection=t))
        assert (r.index[item] >= 0) == kept, (t, kept, r.index[item])


# ---- family S: the unsliced launches ----
@pytest.mark.parametrize("level,count", cc.S_CASES)
def test_unsliced_levels_at_tile_edges(product, oracle, level, count):
    n = count + count // 2
    for fmt in cc.FORMATS:
        for fp32, mode in ((False, "table"), (True, "linear"), (True, "nearest")):
            case = cc.s_case(level, count, fmt, fp32, mode=mode)
            r = parity(product, oracle, case)
            assert len(r.index) == n
            r2, tm = baked_with_timings(product, case)
            assert r2.same_as(r) and tm.openTiles == 0, (case["name"], tm.openTiles)
            # table: the culled items are exactly the uniform ones; nearest: nothing is culled; linear: a triangle with a block of its own in the
            # result both libraries agree on has two states, so it cannot have been culled
            blocks = int((r.index[[p for p in range(n) if p % 3 != 2]] >= 0).sum())
            lo, hi = {"table": (count, count), "nearest": (n, n), "linear": (blocks, n)}[mode]
            assert lo <= tm.activeItems <= hi, (case["name"], tm.activeItems, lo, hi)


# ---- family B: micro-triangles of several texels ----
@pytest.mark.parametrize("generic_pass", [1, 2])
@pytest.mark.parametrize("name", cc.B_NAMES)
def test_join_with_micro_triangles_of_several_texels(product, oracle, name, generic_pass):
    knobs = [(ot.KNOB_GENERIC_PASS, generic_pass)]
    for mode in ("linear", "table"):
        case = cc.b_case(name, mode)
        r = parity(product, oracle, case, knobs=knobs)
        scheduled(product, oracle, case, r, knobs=knobs)
        r2, tm = baked_with_timings(product, case, knobs=knobs)
        assert r2.same_as(r) and (tm.genericMicroTriangles > 0) == (generic_pass == 2), (mode, generic_pass, tm.genericMicroTriangles)


@pytest.mark.parametrize("generic_pass", [1, 2])
def test_degenerate_item_and_mip_chain_in_the_deferred_pass(product, oracle, generic_pass):
    case = cc.b_mips_case()
    knobs = [(ot.KNOB_GENERIC_PASS, generic_pass)]
    r = parity(product, oracle, case, knobs=knobs)
    r2, tm = baked_with_timings(product, case, knobs=knobs)
    assert r2.same_as(r) and (tm.genericMicroTriangles > 0) == (generic_pass == 2), (generic_pass, tm.genericMicroTriangles)


# ---- above the deterministic size ----
@pytest.mark.parametrize("mode", MODES)
def test_level_10_item_three_times_on_one_baker(product, oracle, mode):
    """256 tiles = four waves of triage_tiles appending through an atomic: whatever order they took (a follower's tile may precede its head's), each
    result is the oracle's.  No layout is asserted."""
    case = cc.t_case(mode)
    ref = tc.bake(oracle, case)
    s = cc.restate_schedule(case)

    def run(b, d):
        out = []
        for _ in range(3):
            out.append((product.bake(b, d), counters(bench.get_timings(product, b))))
        return out

    for r, got in on_product(product, case, run):
        assert r.same_as(ref), r.diff(ref)
        if mode == "nearest":
            assert got == {k: s[k] for k in got}, got
        elif mode == "table":
            fine = got.pop("fineMicroTriangles")
            assert got == {k: s[k] for k in got} and s["fineLower"] <= fine <= s["fineMicroTriangles"], (got, fine)
