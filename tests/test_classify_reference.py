"""No GPU: tests/classify_cases.py held to the oracle, and what its families cover proved on the restated schedule.

Every sub-triangle the restatement calls settled -- inactive items, settled tiles, settled groups of open tiles -- has exactly that state on all its
micro-triangles in the oracle's decode of the same input, in every mode; the coverage tests assert on `restate_schedule` that the join is crossed
from both sides, that every member count, rectangle size and window case exists, that the M item draws its known count from all three sources and that
every S count is met.  A case the seeded search cannot place raises: it fails, it does not skip.  The oracle's side of every test is printed and bounded."""
import time
import numpy as np
import pytest
import ommtest as ot
import classify_cases as cc

ORACLE_SECONDS_PER_TEST = 3.0
SPENT = [0.0, 0]
MODES = cc.MODES


@pytest.fixture(autouse=True)
def oracle_time_of_this_test(request):
    SPENT[:] = [0.0, 0]
    yield
    if SPENT[1]:
        print("oracle side of %s: %d bakes, %.2f s" % (request.node.name, SPENT[1], SPENT[0]))
    assert SPENT[0] < ORACLE_SECONDS_PER_TEST, (request.node.name, SPENT)


def decode(oracle, case):
    t0 = time.perf_counter()
    st = cc.oracle_states(oracle, case)
    SPENT[0] += time.perf_counter() - t0
    SPENT[1] += 1
    return st


def held(oracle, case):
    s = cc.restate_schedule(case)
    st = decode(oracle, case)
    cc.check_against_decode(case, s, st)
    if case["mode"] == "linear":
        lo, hi = cc.linear_bounds(case, s, st)
        print("%s: open tiles between %d and %d" % (case["name"], lo, hi))
        assert lo <= hi
    return s, st


# ---- the restatement against the oracle ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", cc.J_NAMES)
def test_join_cases_hold_to_the_oracle(oracle, name, mode):
    for fp32 in (False, True):
        held(oracle, cc.variant(cc.j_case(name), mode=mode, fp32=fp32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", cc.W_NAMES)
def test_window_cases_hold_to_the_oracle(oracle, name, mode):
    held(oracle, cc.variant(cc.w_case(name), mode=mode))


@pytest.mark.parametrize("mode", MODES)
def test_dead_tile_of_a_uniform_item(oracle, mode):
    c = cc.variant(cc.m_dead_case(), mode=mode)
    s, st = held(oracle, c)
    if mode != "nearest":
        assert [(r["tile"], r["open"]) for r in s["records"]] == [(44, 0)] and s["chunks"] == [] and s["activeItems"] == 1
    assert set(st[0].tolist()) == {ot.O}                                  # the defect lies outside the item: one state
    t0 = time.perf_counter()
    r = cc.tc.bake(oracle, c)
    SPENT[0] += time.perf_counter() - t0
    assert r.index.tolist() == [ot.SPECIAL_FO] and len(r.descs) == 0      # ... and its special index


@pytest.mark.parametrize("fp32", [False, True], ids=["u8", "fp32"])
def test_known_count_of_three_sources_at_the_rejection_threshold(oracle, fp32):
    base = cc.m_threshold_case(fp32, 0.0)
    s, st = held(oracle, base)
    tiles, groups, rest, known = cc.m_sources(s, st)
    print("known micro-triangles: %d of settled tiles, %d of settled groups, %d classified, %d of %d" % (tiles, groups, rest, known, st[0].size))
    assert tiles > 0 and groups > 0 and rest > 0 and known < st[0].size
    for t, kept in cc.m_thresholds(known, st[0].size):
        t0 = time.perf_counter()
        r = cc.tc.bake(oracle, cc.m_threshold_case(fp32, t))
        SPENT[0] += time.perf_counter() - t0
        assert (r.index[0] >= 0) == kept, (t, kept, r.index)


@pytest.mark.parametrize("mode", ["table", "linear"])
@pytest.mark.parametrize("name", cc.B_NAMES)
def test_big_micro_triangle_cases_hold_to_the_oracle(oracle, name, mode):
    c = cc.b_case(name, mode)
    sched, st = held(oracle, c)
    leg = 768.0 / 2 ** 7
    want = cc.B_WANTS[name]
    assert 4 <= leg <= 16 and [(r["tile"], r["open"]) for r in sched["records"]] == sorted(want.items())
    assert not any(k["lds"] for k in sched["chunks"])
    members = [len(k["members"]) for k in sched["chunks"]]
    assert members == {"sum-62": [2], "sum-64": [2], "sum-65": [1, 1], "members-4": [4], "dead": [2], "tail-3": [3]}[name]
    if name == "dead":
        assert sched["records"][0]["open"] == 0 and sched["chunks"][0]["dead"] == [2]


def test_degenerate_item_and_mip_chain_case(oracle):
    c = cc.b_mips_case()
    assert len(c["mips"]) == 2 and c["mips"][1].shape == (512, 512)
    p = np.asarray(c["uv"], np.float64).reshape(-1, 3, 2)[1]
    assert abs((p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[2, 0] - p[0, 0]) * (p[1, 1] - p[0, 1])) < 1e-9      # the second triangle has no area
    t0 = time.perf_counter()
    b = oracle.create_baker()
    t = oracle.create_texture(b, c["mips"], alpha_cutoff=0.5)
    r = oracle.bake(b, ot.make_desc(t, c["uv"], c["ix"], c["gmax"], **cc.tc.desc_kw(c)))
    oracle.destroy_texture(b, t)
    oracle.destroy_baker(b)
    SPENT[0] += time.perf_counter() - t0
    SPENT[1] += 1
    assert len(r.index) == 2


@pytest.mark.parametrize("mode", MODES)
def test_level_10_case_is_beyond_one_wave_of_tiles(oracle, mode):
    c = cc.t_case(mode)
    s, st = held(oracle, c)
    opens = [r["open"] for r in s["records"]]
    print("%d open tiles, %.1f open groups each" % (len(opens), np.mean(opens)))
    if mode == "nearest":
        assert len(opens) == 256 and set(opens) == {64} and all(len(k["members"]) == 1 for k in s["chunks"])      # nothing is triaged
        return
    assert not s["deterministic"] and len(opens) > 100 and 0 < np.mean(opens) < 8
    assert any(len(k["members"]) > 1 for k in s["chunks"])      # (in enumeration order; the device's order may differ)


def test_linear_bounds_coincide_on_every_tile_a_case_is_about(oracle):
    """every wanted tile with an open group holds two states in the oracle's Linear decode (the placement search keeps nothing else), so the bounds of
    openTiles differ by the dead records alone -- tiles whose every group the table settles, which the curve test may or may not settle as tiles.
    Named exceptions, by construction: `clamp-over` (one alpha value under Clamp: nothing is mixed)."""
    loose = {}
    for names, maker in ((cc.J_NAMES, cc.j_case), (cc.W_NAMES, cc.w_case), (["dead"], lambda n: cc.m_dead_case())):
        for n in names:
            c = cc.variant(maker(n), mode="linear")
            s = cc.restate_schedule(c)
            t0 = time.perf_counter()
            st = cc.oracle_states(oracle, c)
            assert time.perf_counter() - t0 < ORACLE_SECONDS_PER_TEST            # (31 bakes in this test: each is bounded, as everywhere else)
            lo, hi = cc.linear_bounds(c, s, st)
            dead = sum(1 for r in s["records"] if r["open"] == 0)
            assert c.get("loose", []) == [] and hi == len(s["records"])
            if n == "clamp-over":
                assert lo == 0
                continue
            assert lo == hi - dead, (n, lo, hi, dead)
            if dead:
                loose[n] = dead
    assert loose == {"members-4": 4, "members-5": 3, "union": 2, "dead": 1}, loose


# ---- M at level 5 ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", cc.M5_COUNTS)
def test_level_5_items_hold_to_the_oracle(oracle, n, mode):
    c = cc.m5_case(n, mode=mode)
    s, st = held(oracle, c)
    assert s["records"] == [] and s["chunks"] == [] and len(s["small"]) == n and s["openTileMicroTriangles"] == 1024 * n and s["activeItems"] == n
    if mode == "nearest":
        assert [r["open"] for r in s["small"]] == [16] * n
        return
    assert [r["open"] for r in s["small"]] == [bin(cc.M5_PATTERNS[k % 5][1]).count("1") for k in range(n)]
    for k in range(n):
        gv = s["items"][k]["group_verdict"][0]
        assert sum(1 << g for g in range(16) if gv[g] < 0) == cc.M5_PATTERNS[k % 5][1]
        assert set(gv[gv >= 0].tolist()) <= {ot.O if k % 2 == 0 else ot.T}          # neighbours in a wave settle to different states
        if k % 5 == 0:
            assert set(st[k].tolist()) == {ot.O if k % 2 == 0 else ot.T}              # "none": a dead tile, a uniform item


@pytest.mark.parametrize("n", [n for n in cc.M5_COUNTS if n >= 3])
def test_level_5_known_count_at_the_rejection_threshold(oracle, n):
    base = cc.m5_case(n, mode="linear")
    s, st = held(oracle, base)
    item = cc.m5_threshold_item(n)
    tiles, groups, rest, known = cc.m_sources(s, st, item)
    print("item %d: %d known of settled groups, %d classified, %d of 1024" % (item, groups, rest, known))
    assert tiles == 0 and rest > 0 and known < 1024 and (groups > 0) == (n >= 5)
    for t, kept in cc.m_thresholds(known, 1024):
        t0 = time.perf_counter()
        r = cc.tc.bake(oracle, cc.m5_case(n, mode="linear", rejection=t))
        SPENT[0] += time.perf_counter() - t0
        assert (r.index[item] >= 0) == kept, (t, kept, r.index[item])


# ---- coverage, on the restated schedule alone ----
def scheds(names, maker):
    return {n: cc.restate_schedule(maker(n)) for n in names}


def test_join_family_covers_what_it_claims():
    S = scheds(cc.J_NAMES, cc.j_case)
    for n, s in S.items():
        assert s["deterministic"] and s["window"] == (1 if n == "level6" else 8), n
    # the bound hOpen + open <= 64 from both sides, on unrelated boxes and on the two halves of one square
    for s_, names in [(v, "sum-%d" % v) for v in cc.J_SUMS] + [(v, "pair-%d" % v) for v in cc.J_PAIR_SUMS]:
        r = S[names]["records"]
        assert len(r) == 2 and r[0]["open"] + r[1]["open"] == s_ and r[0]["item"] == r[1]["item"]
        assert [len(k["members"]) for k in S[names]["chunks"]] == ([2] if s_ <= 64 else [1, 1]), names
    assert sorted({r["open"] + r2["open"] for n in S if n.startswith("sum-") for r, r2 in [S[n]["records"]]}) == [62, 63, 64, 65, 66]
    chunks = [k for s in S.values() for k in s["chunks"]]
    assert any(k["total"] == 64 and len(k["members"]) == 1 for k in S["head64"]["chunks"])
    f1 = S["follower1"]
    assert [r["open"] for r in f1["records"]][-1] == 1 and f1["chunks"][0]["members"][-1] == len(f1["records"]) - 1 and f1["chunks"][0]["slots"][-1] == 20
    # every member count; 5 reaches the second pass of the slot tables, 8 fills the mask
    assert {len(k["members"]) for k in chunks} >= {1, 2, 4, 5, 8}
    for m in cc.J_MEMBERS:
        assert [len(k["members"]) for k in S["members-%d" % m]["chunks"]] == [m], m
    assert S["members-8"]["chunks"][0]["mask"] == 0x7F and S["members-8"]["chunks"][0]["total"] == 64
    # dead records between a head and a follower, a window whose first record is dead
    assert any(k["dead"] for k in S["members-5"]["chunks"]) and S["members-5"]["records"][0]["open"] > 0
    m4 = S["members-4"]
    assert m4["records"][0]["open"] == 0 and m4["chunks"][0]["head"] == 1 and m4["chunks"][0]["dead"]
    # a join refused for the item alone
    it = S["items"]
    r = it["records"]
    assert [x["item"] for x in r] == [0, 0, 1, 1] and [x["level"] for x in r] == [8, 8, 7, 7] and sum(x["open"] for x in r) <= 64
    assert [k["members"] for k in it["chunks"]] == [[0, 1], [2, 3]]
    # four items in one wave of tiles: a chunk per item, eight records that a streamed bake cuts between the items
    f4 = S["four"]
    assert [x["item"] for x in f4["records"]] == [0, 0, 1, 1, 2, 2, 3, 3] and [k["members"] for k in f4["chunks"]] == [[0, 1], [2, 3], [4, 5], [6, 7]]
    # windows cut by the tail
    for n in cc.J_TAILS:
        s = S["tail-%d" % n]
        assert len(s["records"]) == n and all(x["open"] for x in s["records"])
        assert [len(k["members"]) for k in s["chunks"]] == ([n] if n <= 8 else [8, n - 8])
    # level 6 on top: no window; a level-7 item behind them in the input comes first in the queue and brings the window back
    assert [len(k["members"]) for k in S["level6"]["chunks"]] == [1] * len(cc.J_LEVEL6) and S["level6"]["window"] == 1
    p7 = S["level6-plus7"]
    assert [x["level"] for x in p7["records"]] == [7, 7] + [6] * len(cc.J_LEVEL6) and p7["records"][0]["item"] == len(cc.J_LEVEL6)
    assert [len(k["members"]) for k in p7["chunks"]] == [2] + [1] * len(cc.J_LEVEL6)
    # micro-triangles below a texel, tile legs of 30 texels or less
    leg = float(cc.J_TRI[1, 0] - cc.J_TRI[0, 0]) * cc.SIZE
    assert leg / 8 <= 30 and leg / 2 ** 9 < 1


def test_window_family_covers_what_it_claims():
    S = scheds(cc.W_NAMES, cc.w_case)
    size = cc.SIZE
    wh = [(r["rect"][2] - r["rect"][0] + 1, r["rect"][3] - r["rect"][1] + 1) for n in ("sizes-a", "sizes-b") for r in S[n]["records"]]
    print("tile rectangles:", sorted(set(wh)))
    assert {w for w, h in wh} >= {31, 32, 33} and {h for w, h in wh} >= {31, 32, 33}
    # members that each fit while their union does not
    u = S["union"]["chunks"]
    assert len(u) == 1 and len(u[0]["members"]) == 2 and not u[0]["lds"] and u[0]["ok"]
    for m in u[0]["members"]:
        sx, sy, ex, ey = S["union"]["records"][m]["rect"]
        assert ex - sx + 1 <= cc.WIN and ey - sy + 1 <= cc.WIN
    lds = [k["lds"] for s in S.values() for k in s["chunks"]]
    assert any(lds) and not all(lds)
    # rectangles from texel 0 and to the last texel, on each axis, in a chunk that loads the window
    o = S["origin"]["chunks"][0]
    assert o["rect"][:2] == (0, 0) and o["lds"]
    e = S["end"]["records"]
    assert e[0]["rect"][2] == size - 1 and e[1]["rect"][3] == size - 1
    assert any(r["rect"][2] == size - 1 for r in e) and any(r["rect"][3] == size - 1 for r in e)
    # a whole period away: the rectangle is translated, the schedule is the one of the item at home
    for n, k in (("wrap+1", 1), ("wrap-2", -2)):
        c = cc.w_case(n)
        g = cc._geometry(np.ascontiguousarray(c["uv"], np.float32).reshape(-1, 6)[0].tobytes(), 9, size, size, ot.WRAP)["tiles"]
        assert g["ok"].all() and (g["X0"] - g["sx"] == k * size).all() and (g["Y1"] - g["ey"] == k * size).all()
    # over the edge under Clamp and Border: no rectangle, no window, groups that cannot be asked
    for n in ("clamp-over", "border-over"):
        r = S[n]["records"]
        assert any(not x["ok"] for x in r) and all(not k["lds"] for k in S[n]["chunks"] if not k["ok"]) and any(not k["ok"] for k in S[n]["chunks"])
        assert max(x["open"] for x in r) >= 49


@pytest.mark.parametrize("level,count", cc.S_CASES)
def test_unsliced_cases_have_their_counts(level, count):
    per = 1024 // 4 ** level
    assert count == 1 or any(count == k * per + d for k in (1, 2) for d in (-1, 0, 1))
    c = cc.s_case(level, count, ot.FMT_4STATE, False)
    s = cc.restate_schedule(c)
    n = len(c["uv"]) // 3
    assert cc.restate_schedule(cc.s_case(level, count, ot.FMT_4STATE, False, mode="nearest"))["activeItems"] == n
    assert s["activeItems"] == count and n == count + count // 2 and (count < 2 or n > count)
    act = s["active"]
    assert count < 3 or (not act[2] and act[0] and act[1] and act[3])         # the culled items lie between the active ones


def test_unsliced_counts_are_the_tile_edges():
    for L in range(5):
        per = 1024 // 4 ** L
        assert set(cc.s_counts(L)) == {1} | {k * per + d for k in (1, 2) for d in (-1, 0, 1)} - {0}
