"""No GPU: the numpy restatement of the tail of a bake (tests/tail_cases.py: promotion, digest, exact duplicates, spatial sort, serialisation) against the
oracle on every case of families K (sort key), P (placement counts), R (promotion) and D (digests), and the conditions the families must meet for a
comparison of the HIP library on them to mean something -- cell edges hit from both sides, enough triangles on which a wrong rounding of the centroid
shows, tie groups of the intended sizes, item counts on both sides of every threshold of the device's kernels, known fractions exactly on the
rejection threshold.  Run with -s for the counts recorded in tests/README.md."""
import ctypes as C
import importlib.util
import os
import time
import numpy as np
import pytest
import ommtest as ot
import tail_cases as tc

ORACLE_SECONDS_PER_TEST = 3.0      # the bound on the oracle's side of one test, as in test_setup_reference.py
SPENT = [0.0, 0]


@pytest.fixture(autouse=True)
def oracle_time_of_this_test(request):
    SPENT[:] = [0.0, 0]
    yield
    if SPENT[1]:
        print("oracle side of %s: %d bakes, %.2f s" % (request.node.name, SPENT[1], SPENT[0]))
    assert SPENT[0] < ORACLE_SECONDS_PER_TEST, (request.node.name, SPENT)


def timed(f, *a, **kw):
    t0 = time.perf_counter()
    r = f(*a, **kw)
    SPENT[0] += time.perf_counter() - t0
    SPENT[1] += 1
    return r


def check(oracle, case, raw=None):
    """oracle bake of the case == restatement from the oracle's own states under RAW_FLAGS; returns (restatement, inputs)"""
    raw = raw or case.get("raw") or timed(tc.bake, oracle, case, flags=tc.RAW_FLAGS, rejection=0.0)
    res = timed(tc.bake, oracle, case)
    inp = tc.tail_inputs(case, raw)
    rs = tc.restate_tail(inp, case["flags"], case["rejection"])
    tc.check_result(case, res, rs)
    return rs, inp


def orc_digest(oracle, row):
    oracle.dll.orc_xxh64.restype, oracle.dll.orc_xxh64.argtypes = C.c_uint64, [C.c_char_p, C.c_size_t, C.c_uint64]
    raw = np.where(row == ot.UT, ot.UO, row).astype(np.uint8).tobytes()
    return int(oracle.dll.orc_xxh64(raw, len(raw), 42))


def orc_key(oracle, p, level):
    oracle.dll.orc_sort_key.restype, oracle.dll.orc_sort_key.argtypes = C.c_uint64, [C.POINTER(C.c_float), C.c_uint32]
    return np.array([oracle.dll.orc_sort_key((C.c_float * 6)(*[float(v) for v in t]), int(l)) for t, l in zip(p, level)], np.uint64)


# ---- the restatement's parts on their own ----
def test_restated_digest_is_orc_xxh64(oracle):
    """every stream length of levels 0 - 6 (1, 4, 16 bytes: the short-stream tails; 32-byte stripes and their remainders), all four states"""
    rng = np.random.default_rng(42)
    for n in [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 255, 256, 1024, 4096]:
        for _ in range(4):
            row = rng.integers(0, 4, n).astype(np.uint8)
            assert tc.digest_of_states(row) == orc_digest(oracle, row), n
    a, b = np.full(64, ot.UT, np.uint8), np.full(64, ot.UO, np.uint8)
    assert tc.digest_of_states(a) == tc.digest_of_states(b) != tc.digest_of_states(np.full(64, ot.O, np.uint8))


def test_restated_key_is_orc_sort_key(oracle):
    """the edge triangles, the searched ones, random ones, and centroids far outside [0, 1)"""
    tris = [np.array([t[0] for t in tc.k1_edge_triangles()], np.float32)] + list(tc.k2_rounding_triangles().values())
    tris.append(tc.cheap_triangles(3, 2000, extent=0.01, lo=-3.0, hi=3.0))
    tris.append(tc.cheap_triangles(4, 200, extent=1000.0, lo=-4e5, hi=4e5))
    p = np.concatenate(tris)
    level = np.arange(len(p)) % 13
    assert np.array_equal(tc.sort_key(p, level), orc_key(oracle, p, level))
    far = np.array([[3e5, 0.1, 3e5, 0.2, 3e5, 0.4], [np.nan, 0.1, 0.2, 0.2, 0.3, 0.4]], np.float32)       # 8192 c beyond the int range, and NaN
    assert np.array_equal(tc.sort_key(far, [1, 1]), orc_key(oracle, far, [1, 1]))
    assert not np.array_equal(tc.sort_key(far, [1, 1], "sat"), tc.sort_key(far, [1, 1]))                       # the `sat` variant shows only there


# ---- family K ----
EDGES_WITH_A_STEP = {1, 2, 4095, 4096, 8191, -2, -4096, -8191, -8192}     # (0, -1: one double-width cell; 8192, 8193, -8193: clamped)


def test_k1_reaches_every_cell_edge_from_both_sides():
    tris = tc.k1_edge_triangles()
    for axis in (0, 1):
        mine = [t for t in tris if t[1] == axis]
        p = np.array([t[0] for t in mine], np.float32)
        got = tc.cell(p[:, axis], p[:, 2 + axis], p[:, 4 + axis])
        assert got.tolist() == [tc.expected_cell(t[4]) for t in mine]
        by_k = {}
        for t, g in zip(mine, got.tolist()):
            if t[3] != 2:
                by_k.setdefault(t[2], {})[t[3]] = g
        assert set(by_k) == set(tc.EDGE_K) and all(set(v) == {-1, 0, 1} for v in by_k.values())
        for k, v in by_k.items():
            assert (len(set(v.values())) == 2) == (k in EDGES_WITH_A_STEP), (axis, k, v)
        for k in (0, -1):
            assert set(by_k[k].values()) == {0}
        assert by_k[8192] == by_k[8193] == {-1: 8191, 0: 8191, 1: 8191} and by_k[-8193] == {-1: 8191, 0: 8191, 1: 8191}
        inside = [g for t, g in zip(mine, got.tolist()) if t[3] == 2]
        assert len(inside) == 6 and set(inside) == {0}                  # both halves of the cell around 0
        other = tc.cell(p[:, 1 - axis], p[:, 3 - axis], p[:, 5 - axis])
        assert len(set(other.tolist())) <= 12                           # the other Morton lane stays put: only this lane's bits order the triangles


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_k1_edges_against_the_oracle(oracle, fmt):
    case = tc.k1_case(fmt)
    rs, inp = check(oracle, case)
    assert len(rs["order"]) == len(inp["level"])


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_k2_rounding_against_the_oracle_and_the_wrong_variants(oracle, fmt):
    case = tc.k2_case(fmt)
    found = tc.k2_rounding_triangles()
    print("triangles whose key differs under a wrong variant:", {v: len(t) for v, t in found.items()})
    assert len(found["recip"]) >= 50 and len(found["reorder"]) >= 50 and len(found["fused"]) >= 20
    for v, t in found.items():
        assert (tc.sort_key(t, np.zeros(len(t)), v) != tc.sort_key(t, np.zeros(len(t)))).all()
    rs, inp = check(oracle, case)
    for v in ("recip", "reorder", "fused"):
        wrong = tc.restate_tail(inp, case["flags"], variant=v)
        moved = int((wrong["order"] != rs["order"]).sum())
        print("variant %s moves %d of %d descriptors" % (v, moved, len(rs["order"])))
        assert moved >= 20 and not np.array_equal(wrong["index"], rs["index"])


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_k3_ties_against_the_oracle_on_both_placement_paths(oracle, fmt):
    counts = []
    for padded in (False, True):
        case = tc.k3_case(fmt, padded)
        rs, inp = check(oracle, case)
        tc.tie_groups_hold(case, rs["order"], inp)
        counts.append(len(rs["order"]))
    assert counts[0] <= tc.RANK_MAX < counts[1]
    a, b = tc.k3_case(fmt, False), tc.k3_case(fmt, True)
    assert np.array_equal(b["uv"][:len(a["uv"])], a["uv"])       # the same input, padded


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_k4_level_leads_against_the_oracle(oracle, fmt):
    case = tc.k4_case(fmt)
    rs, inp = check(oracle, case)
    bits = inp["bits"]
    d = rs["descs"]
    assert set(d[:, 1].tolist()) == {0, 1, 2, 3, 4, 5} and np.all(np.diff(d[:, 1]) <= 0)
    sizes = tc.block_bytes(d[:, 1], bits)
    assert sorted(set(sizes.tolist())) == ([1, 2, 8, 32, 128] if bits == 1 else [1, 4, 16, 64, 256])
    assert np.array_equal(d[:, 0], np.concatenate([[0], np.cumsum(sizes)[:-1]])) and len(rs["array"]) == sizes.sum()
    assert rs["small"] == (d[:, 1] <= (3 if bits == 1 else 2)).sum() and 0 < rs["small"] < len(d)
    assert (case["levels"] == 0xF).sum() > 20 and (inp["level"][case["levels"] == 0xF] == 4).all()


# ---- family P ----
def test_p_counts_stand_on_every_threshold():
    """numpy alone: 32 lanes per key, look-back tiles of 1024, LDS chunks of 4096 and the path choice at 16384 are stood on from both sides by the emitted
    counts; the partial cases have more candidates than the counting path takes and at most that many emitted keys, one of them a single key, one ending on a tile"""
    c = set(tc.P_COUNTS)
    for edge in (32, tc.PLACE_TILE, tc.RANK_CHUNK, tc.RANK_MAX):
        assert {edge - 1, edge, edge + 1} <= c, edge
    assert {2047, 2049, 8191, 8193} <= c                                        # either side of the second tile / chunk edge
    assert {17 * tc.PLACE_TILE, 17 * tc.PLACE_TILE + 1, 32769} <= c             # the sort path: a list that ends on a tile, one key into the next tile, many tiles
    assert all(n > tc.RANK_MAX >= e for n, e in tc.P_PARTIAL)
    assert {e for n, e in tc.P_PARTIAL} == {1, tc.PLACE_TILE, tc.RANK_MAX}
    spec = importlib.util.spec_from_file_location("stress_tail_paths", os.path.join(os.path.dirname(os.path.abspath(__file__)), "scripts", "stress_tail_paths.py"))
    st = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(st)
    assert min(st.COUNTS) > 65536 and not set(st.COUNTS) & c          # the script keeps only what the suite does not run


@pytest.mark.parametrize("n", tc.P_COUNTS)
def test_p_all_candidates_emitted_against_the_oracle(oracle, n):
    for fmt in tc.FORMATS:
        for mode in tc.LEVEL_MODES:
            case = tc.p_all_case(n, mode, fmt)
            rs, inp = check(oracle, case)
            assert len(rs["order"]) == n == len(inp["level"])
            if mode == "stepped" and n > 2000:
                assert set(inp["level"].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("fmt", tc.FORMATS)
@pytest.mark.parametrize("n,emitted", tc.P_PARTIAL)
def test_p_partly_emitted_against_the_oracle(oracle, n, emitted, fmt):
    timed(tc.p_picks, oracle, fmt, 3)
    timed(tc.p_picks, oracle, fmt, 4)
    for mode in tc.LEVEL_MODES:
        for kind in tc.PARTIAL_KINDS:
            case = tc.p_partial_case(oracle, n, emitted, mode, fmt, kind)
            rs, inp = check(oracle, case)
            assert len(inp["level"]) == n and len(rs["order"]) == emitted         # n candidates (no two triangles share coordinates), `emitted` blocks
            if kind == "duplicates":
                assert not rs["uniform"].any() and (rs["rep"] != np.arange(n)).sum() == n - emitted
            else:
                assert (rs["special"] < 0).sum() == n - emitted
            if mode == "stepped" and emitted > 1000:
                assert set(inp["level"][rs["order"]].tolist()) == {3, 4}


# ---- family R ----
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_r1_rejection_at_the_boundary_against_the_oracle(oracle, fmt):
    base4 = tc.r1_case(ot.FMT_4STATE)
    inp4 = tc.tail_inputs(base4, timed(tc.bake, oracle, base4, flags=tc.RAW_FLAGS))
    rs4 = tc.restate_tail(inp4, base4["flags"])
    pairs = tc.r1_pairs(rs4, inp4["level"])
    print("(k, N) on the threshold:", pairs)
    assert len(pairs) == 6 and {n for k, n in pairs} == {16, 64, 256, 1024}
    base = tc.r1_case(fmt)
    raw = timed(tc.bake, oracle, base, flags=tc.RAW_FLAGS)
    for t, pair in tc.r1_thresholds(pairs):
        for flags in tc.R1_FLAGS:
            case = tc.r1_case(fmt, flags, t)
            rs, inp = check(oracle, case, raw)
            mixed = ~rs["uniform"]
            if pair and fmt == ot.FMT_4STATE:
                on = mixed & (rs["frac"] == np.float32(t))
                assert on.any() and not rs["rejected"][on].any() and (mixed & (rs["frac"] < np.float32(t))).any() and rs["rejected"].any()
                if not flags & ot.FLAG_NO_SPECIAL:
                    assert (rs["special"][rs["rejected"]] == ot.SPECIAL_FUT).all() and (rs["special"][on] == 0).all()
                below = tc.restate_tail(inp, flags, float(np.nextafter(np.float32(t), np.float32(-1))))
                above = tc.restate_tail(inp, flags, float(np.nextafter(np.float32(t), np.float32(2))))
                assert np.array_equal(below["rejected"], rs["rejected"]) and np.array_equal(above["rejected"], rs["rejected"] | on)
            if not t > 0:
                assert not rs["rejected"].any()
            if t == 1.5:
                assert rs["rejected"][mixed].all()
            if fmt == ot.FMT_2STATE and t <= 1.0:
                assert not rs["rejected"].any()                     # every state of a 2-state item is known: its fraction is 1


@pytest.mark.parametrize("first_at", tc.R2_FIRST_AT)
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_r2_uniform_items_of_every_state_against_the_oracle(oracle, fmt, first_at):
    """levels 0 - 8, every state the format can produce, both input orders of the two states of a level; the first uniform items at work items 255 and 256
    (a workgroup edge of the device's hash build) or beyond 65 536"""
    states = set()
    for le, gt in tc.r2_states(fmt, first_at):
        raw = None
        for flags in tc.R1_FLAGS:
            case = tc.r2_case(fmt, le, gt, first_at, flags)
            raw = raw or timed(tc.bake, oracle, case, flags=tc.RAW_FLAGS)
            rs, inp = check(oracle, case, raw)
            u = case["side"] >= 0
            assert len(inp["level"]) == len(u) and rs["uniform"][u].all() and not rs["uniform"][~u].any()
            assert np.nonzero(u)[0][:2].tolist() == [first_at, first_at + 1] and set(inp["level"][u].tolist()) == set(range(9))
            classes, values = tc.r2_statements(case, rs["index"], rs)
            assert classes == (9 if {le, gt} == {ot.UT, ot.UO} else 18)
            if {le, gt} == {ot.UT, ot.UO} and not flags & ot.FLAG_NO_SPECIAL:
                assert {ot.SPECIAL_FUT, ot.SPECIAL_FUO} <= set(values)       # the first of a level is UT at some levels and UO at others: it keeps its own value
                assert 0 in values                                             # level 1: an earlier non-uniform item of UT and UO shares the digest and keeps the block
            first_sides = [case["side"][case["levels"] == L][case["side"][case["levels"] == L] >= 0][0] for L in range(9)]
            assert set(first_sides) == {0, 1}
            states |= {le, gt}
    assert states == ({ot.T, ot.O} if fmt == ot.FMT_2STATE else {ot.T, ot.O, ot.UT, ot.UO}) and len(tc.R2_STATES[fmt]) == (2 if fmt == ot.FMT_2STATE else 4)


# ---- family D ----
def test_d1_shapes_stand_on_every_digest_threshold():
    """numpy alone: streams of 1, 4 and 16 bytes (and 64, 256, 1024: the small form's stripes); blocks below, at and above 256 and 1024 packed bytes;
    16- and 64-item workgroups and the 2048-item choice between the chain and the LDS form from both sides"""
    size = lambda L, f: int(tc.block_bytes(L, 2 if f == ot.FMT_4STATE else 1))
    assert {4 ** L for L, f, n in tc.D1_SMALL} == {1, 4, 16, 64, 256, 1024}
    assert all(size(L, f) < 256 for L, f, n in tc.D1_SMALL) and max(size(L, f) for L, f, n in tc.D1_SMALL) == 128
    assert {size(L, f) for L, f, n in tc.D1_LDS} == {256, 512} and {n for L, f, n in tc.D1_LDS} == {1, 63, 64, 65, 129}
    assert {size(L, f) for L, f, n in tc.D1_CHAIN} == {1024, 2048} and {n for L, f, n in tc.D1_CHAIN} == {1, 15, 16, 17, 2047, 2048, 2049}


D1_GROUPS = sorted({(L, f, n >= 1000) for L, f, n in tc.D1_CASES})


@pytest.mark.parametrize("level,fmt,big", D1_GROUPS, ids=["L%d-fmt%d-%s" % (l, f, "many" if b else "few") for l, f, b in D1_GROUPS])
def test_d1_block_digests_against_orc_xxh64(oracle, level, fmt, big):
    for L, f, n in tc.D1_CASES:
        if (L, f, n >= 1000) != (level, fmt, big):
            continue
        case = timed(tc.d1_case, oracle, L, f, n)
        counter, rs = tc.block_digests(case["raw"], case)
        inp = tc.tail_inputs(case, case["raw"], tc.RAW_FLAGS)
        ids, S = inp["groups"][L]
        step = max(1, len(ids) // 40)
        for i in range(0, len(ids), step):
            assert int(rs["digest"][ids[i]]) == orc_digest(oracle, S[i])
        if L >= 5:
            assert sum(counter.values()) == n == len(ids)           # every item non-uniform: the device's active list of the level holds n
        elif L >= 1:
            assert sum(counter.values()) >= 30
        if n <= 150 or (n == 2049 and L == 6):          # (2049 items of level 7 would double the slowest test: the 17-item case holds the restatement to the oracle there)
            check(oracle, case)


def test_d1_multi_level_against_the_oracle(oracle):
    """by the oracle's decode the bake has non-uniform items on the small form (level 3), on two segments of the multi-level LDS launch (level 5, and
    level 6 with more than 2048 of them) and on two segments of the chain launch (levels 7 and 8, at most 2048 each)"""
    case = tc.d1_multi_level_case()
    rs, inp = check(oracle, case)
    mixed = {L: int((~rs["uniform"][ids]).sum()) for L, (ids, S) in inp["groups"].items()}
    print("non-uniform items per level:", mixed)
    assert set(mixed) == {3, 5, 6, 7, 8} and min(mixed.values()) >= 25 and mixed[6] > 2048 and max(tc.D1_MULTI_COUNTS[7], tc.D1_MULTI_COUNTS[8]) <= 2048


TWIN_IDS = ["L%d-fmt%d-part%d" % c for c in tc.TWIN_CASES]


def test_d2_units_cover_every_chunk_of_every_digest_form():
    """numpy alone: the swept units are every packed byte to level 5 (4-state) / 6 (2-state), every 16 bytes at levels 6 and 7, the first and the last
    16 bytes of every 256-byte chunk at level 8 and of every 1 KiB chunk at level 9; the parts of a level make up all its units"""
    for fmt in tc.FORMATS:
        bits = 2 if fmt == ot.FMT_4STATE else 1
        assert tc.TWIN_LEVELS[fmt] == ([2, 3, 4, 5, 6, 7, 8, 9] if bits == 2 else [3, 4, 5, 6, 7, 8])
        for L in tc.TWIN_LEVELS[fmt]:
            nbytes = 4 ** L * bits // 8
            byte_of = sorted({u * bits // 8 for u in tc.twin_units(L, fmt)})
            if L <= (5 if bits == 2 else 6):
                assert byte_of == list(range(nbytes))
            elif L <= 7:
                assert byte_of == list(range(0, nbytes, 16))
            else:
                chunk = 256 if L == 8 else 1024
                assert byte_of == sorted({c + o for c in range(0, nbytes, chunk) for o in (0, chunk - 16)})
            parts = [tc.twin_targets(L, fmt)[p::tc.twin_parts(L)] for p in range(tc.twin_parts(L))]
            assert sorted(sum(parts, [])) == sorted(tc.twin_targets(L, fmt)) and (L, fmt, tc.twin_parts(L) - 1) in tc.TWIN_CASES


@pytest.mark.parametrize("level,fmt,part", tc.TWIN_CASES, ids=TWIN_IDS)
def test_d2_near_twins_against_the_oracle(oracle, level, fmt, part):
    """by the oracle's decode: every moved copy differs from the untouched triangle in 1 - 4 micro-triangles (here: exactly the one aimed at), none is
    dropped, none is equal, the differing micro-triangles lie in every unit of this part; neither block is uniform; every copy keeps a descriptor"""
    for first in ("untouched", "moved"):
        case = tc.twin_case(level, fmt, part, tc.twin_parts(level), first=first)
        rs, inp = check(oracle, case)
        diffs = tc.twin_differences(case, inp)
        assert len(diffs) == len(case["targets"]) >= 1 and all(1 <= len(d) <= 4 for d in diffs)
        assert [d.tolist() for d in diffs] == [[j] for j in case["targets"]]
        unit = tc.twin_unit(level, fmt)
        assert sorted({int(d[0]) // unit * unit for d in diffs}) == sorted(tc.twin_units(level, fmt)[part::tc.twin_parts(level)])
        assert not rs["uniform"].any() and len(rs["order"]) == len(diffs) + 1 and len(set(rs["digest"].tolist())) == len(diffs) + 1
        if level >= 8:
            break                                                  # (the other input order runs on the device; here it would double the slowest cases)


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_d3_true_twins_against_the_oracle(oracle, fmt):
    for level in [L for L in tc.TWIN_LEVELS[fmt] if L <= 7]:
        case = tc.twin_case(level, fmt, true_twins=True)
        rs, inp = check(oracle, case)
        n = len(inp["level"])
        assert n >= 4 and len(rs["order"]) == 1 and rs["order"][0] == 0 and (rs["rep"] == 0).all() and (rs["index"] == 0).all()
        assert not rs["uniform"].any()


def test_d3_ut_against_uo_twins_against_the_oracle(oracle):
    case = timed(tc.ut_uo_case, oracle)
    print("pairs that differ only by UT against UO:", len(case["pairs"]))
    assert len(case["pairs"]) >= 8
    rs, inp = check(oracle, case)
    rows = {}
    for L, (ids, S) in inp["groups"].items():
        rows.update(zip(ids.tolist(), S))
    for a, b in case["pairs"]:                                      # (no two triangles share coordinates: item = triangle)
        assert a < b and rs["rep"][b] == rs["rep"][a] == a and rs["index"][a] == rs["index"][b] >= 0
        d = rows[a] != rows[b]
        assert d.any() and set(rows[a][d].tolist()) | set(rows[b][d].tolist()) == {ot.UT, ot.UO}
        off, L = rs["descs"][rs["index"][a]][:2]
        assert np.array_equal(tc.unpack_block(rs["array"][None, off:off + int(tc.block_bytes(L, 2))], 4 ** L, 2)[0], rows[a])    # the first one's bytes
    assert any(case["levels"][a] == 1 for a, b in case["pairs"]) and any(case["levels"][a] == 2 for a, b in case["pairs"])


def test_d2_near_twins_that_share_their_preview_against_the_oracle(oracle):
    """the copies differ from the untouched triangle in exactly the micro-triangle aimed at; at level 5 (the preview of a streamed bake) all four are equal and mixed"""
    case = timed(tc.early_twin_case, oracle)
    rs, inp = check(oracle, case)
    ids, S = inp["groups"][tc.EARLY_LEVEL]
    a = S[case["twins"][0]]
    assert [np.nonzero(S[t] != a)[0].tolist() for t in case["twins"][1:]] == [[u] for u in case["targets"]]
    assert len(set(rs["digest"].tolist())) == len(ids) == len(rs["order"]) and not rs["uniform"].any()
    coarse = dict(case, gmax=5, name="early-twins-preview")
    S5 = tc.tail_inputs(coarse, timed(tc.bake, oracle, coarse, flags=tc.RAW_FLAGS), tc.RAW_FLAGS)["groups"][5][1]
    assert all(np.array_equal(S5[t], S5[case["twins"][0]]) for t in case["twins"]) and len(set(S5[case["twins"][0]].tolist())) > 1


def test_d3_ut_against_uo_twins_that_stream_against_the_oracle(oracle):
    """level 6: every copy differs from the untouched triangle in exactly the micro-triangle aimed at, UO there against UT; the block holds T, UT and UO;
    one digest, the first triangle of the input (a copy) keeps the block with its own bytes; at level 5 three copies equal the untouched triangle"""
    case = timed(tc.ut_uo_streamed_case, oracle)
    rs, inp = check(oracle, case)
    ids, S = inp["groups"][tc.EARLY_LEVEL]
    home = case["twins"][case["targets"].index(None)]
    for t, u in zip(case["twins"], case["targets"]):
        d = np.nonzero(S[t] != S[home])[0].tolist()
        assert d == ([] if u is None else [u]) and (u is None or (S[home][u], S[t][u]) == (ot.UO, ot.UT))
    assert set(S[home].tolist()) == {ot.T, ot.UT, ot.UO}
    first = case["twins"][0]
    assert first == 0 and case["targets"][0] is not None and (rs["rep"][case["twins"]] == 0).all() and len(set(rs["index"][case["twins"]].tolist())) == 1
    off = rs["descs"][rs["index"][0]][0]
    assert np.array_equal(tc.unpack_block(rs["array"][None, off:off + 1024], 4 ** tc.EARLY_LEVEL, 2)[0], S[0])
    assert len(rs["order"]) == len(ids) - len(case["twins"]) + 1
    coarse = dict(case, gmax=5, name="ut-uo-streamed-preview")
    S5 = tc.tail_inputs(coarse, timed(tc.bake, oracle, coarse, flags=tc.RAW_FLAGS), tc.RAW_FLAGS)["groups"][5][1]
    same = [bool(np.array_equal(S5[t], S5[home])) for t, u in zip(case["twins"], case["targets"]) if u is not None]
    assert sum(same) == 3 and len(same) == 6 and len(set(S5[home].tolist())) > 1
