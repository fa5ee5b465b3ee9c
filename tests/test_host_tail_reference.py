"""No GPU: omm_amd/csrc/host_tail.cpp -- the serial tail behind ommCpuBakeFlags_EnableNearDuplicateDetection (LSH, or brute force with the internal bit
10) and maxArrayDataSize -- compiled unchanged with ASan + UBSan into tests/native/host_tail_check.cpp and run on the work items of the oracle's decode of a
bake; what it returns must equal the oracle's own result of that bake with the reducers on, byte for byte.  Every item goes through twice: uniform items as
(state, level), the form the device hands them over in, and with explicit packed states.  The families are those of tests/host_tail_cases.py, and every
claim a family makes -- this pair merges, that one is compared and left, these items drop that many levels, the keys of the budget walk are pairwise
different -- is asserted here with the oracle alone.  Run with -s for the counts recorded in tests/README.md."""
import os
import subprocess
import time
import numpy as np
import pytest
import ommtest as ot
import tail_cases as tc
import host_tail_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SECONDS_PER_TEST = 3.0      # the bound on the oracle's side of one test, as in test_tail_reference.py
SPENT = [0.0, 0, 0]
FOUR, TWO = ot.FMT_4STATE, ot.FMT_2STATE


@pytest.fixture(autouse=True)
def oracle_time_of_this_test(request):
    SPENT[:] = [0.0, 0, 0]
    yield
    print("oracle side of %s: %d bakes, %.2f s; %d cases through the program" % (request.node.name, SPENT[1], SPENT[0], SPENT[2]))
    assert SPENT[0] < ORACLE_SECONDS_PER_TEST, (request.node.name, SPENT)


def timed(f, *a, **kw):
    t0 = time.perf_counter()
    r = f(*a, **kw)
    SPENT[0] += time.perf_counter() - t0
    SPENT[1] += 1
    return r


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """host_tail.cpp as it is, under both sanitizers"""
    exe = str(tmp_path_factory.mktemp("host_tail") / "host_tail_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-o", exe,
                        os.path.join(ROOT, "tests", "native", "host_tail_check.cpp"), os.path.join(ROOT, "omm_amd", "csrc", "host_tail.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def run_program(program, tmp_path, blobs):
    """the program on the encoded cases -> one TailResult each; any sanitizer report fails the run"""
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(src, "wb") as f:
        f.write(b"".join(blobs))
    r = subprocess.run([program, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok %d" % len(blobs), r.stdout[-4000:]
    SPENT[2] += len(blobs)
    with open(dst, "rb") as f:
        return hc.read_results(f.read(), len(blobs))


def check(oracle, program, tmp_path, case, variants=({},), decoded=None, expect=ot.SUCCESS):
    """per variant (keywords of hc.knobs_of): the oracle's result of the case with 32-bit indices, and the program's on the oracle's decode, in both forms of
    the uniform items, equal to it.  -> the oracle's results, the decode"""
    items, tri_item = decoded or timed(hc.decode, oracle, case)
    T = len(tri_item)
    refs, blobs = [], []
    for v in variants:
        flags = hc.knobs_of(case, **v)[0]
        refs.append(timed(hc.bake, oracle, case, **dict(v, flags=flags | ot.FLAG_FORCE32), expect=expect))
        assert decoded or not flags & ot.FLAG_NO_DEDUP, "a bake without duplicate detection groups its triangles differently: pass decode_for's items"
        blobs += [hc.encode_case(case, items, T, uniform_form=u, **v) for u in (True, False)]
    got = run_program(program, tmp_path, blobs)
    for k, ref in enumerate(refs):
        for u in (0, 1):
            g = got[2 * k + u]
            name = (case["name"], variants[k], "uniform as (state, level)" if u == 0 else "uniform as packed states")
            if expect == ot.SUCCESS:
                assert g.rc == 0, name
                hc.same(name, g, ref)
            else:
                assert g.rc == 1, name
    return refs, (items, tri_item)


def decode_for(oracle, case, flags):
    """the decode grouped as the bake under `flags` groups its triangles"""
    raw = timed(hc.bake, oracle, case, flags=tc.RAW_FLAGS, budget=hc.NO_BUDGET, rejection=0.0)
    return hc.work_items(case, raw, flags)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the restated parts, against the painted tiles
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_painted_tiles_decode_as_painted(oracle, fmt):
    """every base, legs of unequal length, levels 0 - 6, items of two triangles: the states the oracle decodes are the painted ones; the distance of two
    tiles is the size of the difference of their defect sets"""
    rng = np.random.default_rng(1)
    tiles = []
    for L in range(7):
        room = int(hc.clear_micro(L).sum())
        a = hc.pick(rng, L, min(room, 3))
        tiles += [hc.tile(L, a), hc.tile(L, a[:1]), hc.tile(L, hc.pick(rng, L, min(4 ** L, 2), "O"), "O", 7, 9), hc.tile(L, hc.pick(rng, L, min(4 ** L, 2), "T"), "T", 11, 6, tris=2)]
    case = hc.painted("painted-fmt%d" % fmt, tiles, fmt, shuffle=3)
    items, tri_item = timed(hc.decode, oracle, case)
    hc.tiles_decode_as_painted(case, items, tri_item)
    assert len(items) == len(tiles) and sorted(len(it["prims"]) for it in items).count(2) == 7
    if fmt == FOUR:
        for L in range(1, 7):
            a, b = items[hc.item_of_tile(case, tri_item, 4 * L)], items[hc.item_of_tile(case, tri_item, 4 * L + 1)]
            assert hc.distance(a["states"], b["states"]) == len(tiles[4 * L]["defects"]) - 1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# T0: the host tail that reduces nothing
# ---------------------------------------------------------------------------------------------------------------------------------------------
T0 = [{"budget": hc.NO_REDUCTION}]


def t0_check(oracle, program, tmp_path, case, raw=None):
    """budget 0xFFFFFFFE: the program's result == the oracle's == the oracle's without a budget (the device tail's answer) == tail_cases.restate_tail"""
    raw = raw or timed(hc.bake, oracle, case, flags=tc.RAW_FLAGS, budget=hc.NO_BUDGET, rejection=0.0)
    (ref,), _ = check(oracle, program, tmp_path, case, T0, decoded=hc.work_items(case, raw))
    plain = timed(hc.bake, oracle, case, flags=case["flags"] | ot.FLAG_FORCE32)
    hc.same(case["name"], plain, ref)
    rs = tc.restate_tail(tc.tail_inputs(case, raw), case["flags"] | ot.FLAG_FORCE32, case["rejection"])
    tc.check_result(case, ref, rs)
    return ref, rs


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_t0_sort_key_edges_ties_and_levels(oracle, program, tmp_path, fmt):
    """families K of tail_cases: centroids on cell edges; tie groups of 2 / 63 / 64 / 65 / 300; per-triangle levels 0 - 5 and 0xF"""
    for case in (tc.k1_case(fmt), tc.k3_case(fmt, False), tc.k4_case(fmt)):
        ref, rs = t0_check(oracle, program, tmp_path, case)
        print(case["name"], "descriptors:", len(ref.descs), "levels:", sorted(set(ref.descs[:, 1].tolist())))
    assert set(ref.descs[:, 1].tolist()) == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_t0_rejection_thresholds(oracle, program, tmp_path, fmt):
    """family R1: the six float32(k / N) thresholds, with and without special indices"""
    base4 = tc.r1_case(FOUR)
    inp4 = tc.tail_inputs(base4, timed(tc.bake, oracle, base4, flags=tc.RAW_FLAGS))
    pairs = tc.r1_pairs(tc.restate_tail(inp4, base4["flags"]), inp4["level"])
    assert len(pairs) == 6
    raw = timed(tc.bake, oracle, tc.r1_case(fmt), flags=tc.RAW_FLAGS)
    rejected = 0
    for k, n in pairs:
        for flags in tc.R1_FLAGS:
            ref, rs = t0_check(oracle, program, tmp_path, tc.r1_case(fmt, flags, float(np.float32(k) / np.float32(n))), raw)
            rejected += int(rs["rejected"].sum())
    assert (rejected > 0) == (fmt == FOUR)                               # (every state of a 2-state block is known)


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_t0_uniform_items_of_every_state_and_level(oracle, program, tmp_path, fmt):
    """family R2: uniform items of every state the format has at levels 0 - 8 (a 4-state level-0 item is one field of a byte), UT and UO sharing a digest"""
    for le, gt in tc.r2_states(fmt, 255):
        raw = None
        for flags in tc.R1_FLAGS:
            case = tc.r2_case(fmt, le, gt, 255, flags)
            raw = raw or timed(hc.bake, oracle, case, flags=tc.RAW_FLAGS, budget=hc.NO_BUDGET, rejection=0.0)
            ref, rs = t0_check(oracle, program, tmp_path, case, raw)
            u = case["side"] >= 0
            assert rs["uniform"][u].all() and set(np.asarray(case["levels"])[u].tolist()) == set(range(9))


def test_t0_placement_counts_and_ut_uo_twins(oracle, program, tmp_path):
    """family P up to 4097 items in both formats; blocks that differ only by UT against UO (one keeps its bytes), here also with the near-duplicate flag on"""
    for n in (1, 2, 33, 1025, 4097):
        for fmt in tc.FORMATS:
            t0_check(oracle, program, tmp_path, tc.p_all_case(n, "stepped" if n > 1000 else "one-level", fmt))
    case = timed(tc.ut_uo_case, oracle)
    assert len(case["pairs"]) >= 8
    ref, rs = t0_check(oracle, program, tmp_path, case)
    near, _ = check(oracle, program, tmp_path, case, [{"flags": case["flags"] | ot.FLAG_NEAR_DUP}, {"flags": case["flags"] | ot.FLAG_NEAR_DUP | hc.BRUTE}])
    for a, b in case["pairs"]:
        assert ref.index[a] == ref.index[b] >= 0 and near[0].index[a] == near[0].index[b] and near[1].index[a] == near[1].index[b]


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_t0_invalid_triangles_and_no_triangles(oracle, program, tmp_path, fmt):
    """some triangles invalid (no work item: they keep unresolvedTriState), all of them invalid, and no triangle at all (the program alone: the ABI refuses
    an index count of 0)"""
    rng = np.random.default_rng(5)
    tiles = [hc.tile(L, hc.pick(rng, L, 1)) for L in (0, 1, 2, 3, 1, 2)]
    case = hc.painted("t0-invalid-fmt%d" % fmt, tiles, fmt)
    uv = case["uv"].reshape(-1, 6).copy()
    uv[1, 2], uv[4, 5] = np.nan, np.inf
    case["uv"] = uv.reshape(-1, 2)
    for v in (T0, [{"flags": hc.NEAR, "budget": 1}]):
        (ref,), (items, tri_item) = check(oracle, program, tmp_path, case, v)
        assert len(items) == 4 and (tri_item[[1, 4]] == -1).all() and (ref.index[[1, 4]] == ot.SPECIAL_FUO).all()
    uv[:, 0] = np.nan
    case["uv"] = uv.reshape(-1, 2)
    (ref,), (items, _) = check(oracle, program, tmp_path, case, T0)
    assert items == [] and len(ref.descs) == 0 and (ref.index == ot.SPECIAL_FUO).all()
    empty, = run_program(program, tmp_path, [hc.encode_case(case, [], 0, budget=hc.NO_REDUCTION)])
    assert empty.rc == 0 and empty.array_data.size == 0 and len(empty.descs) == 0 and empty.index.tolist() == [ot.SPECIAL_FUO] and not empty.array_hist and not empty.index_hist


# ---------------------------------------------------------------------------------------------------------------------------------------------
# N: near-duplicate merging by LSH
# ---------------------------------------------------------------------------------------------------------------------------------------------
N_FACTORS = [(1, 0.15), (2, 0.15), (3, 0.15), (4, 0.15), (5, 0.15), (6, 0.15), (1, 0.25), (2, 0.125), (3, 0.0625)]


@pytest.mark.parametrize("level,factor", N_FACTORS)
def test_n_distances_around_the_radius(oracle, program, tmp_path, level, factor):
    """near copies at d = 1, the largest d below r = factor * 4^level, d = r where r is whole, and the smallest d above.  Below r the oracle merges the pair
    (a seeded search for a placement whose pair shares a bucket).  At and above r it leaves the pair -- and merges the same pair of the same bake under a
    factor just large enough for d, whose LSH has the same table count and sample count and so draws the same bits: the pair was compared, and only
    `dist < r` kept it apart"""
    r = hc.radius(level, factor)
    below, at, above = hc.around(r)
    base = "O" if level <= 3 else "cols"
    room = 4 ** level if base == "O" else int(hc.clear_micro(level).sum())
    print("level %d factor %r: r = %r, distances %r" % (level, factor, float(r), (1, below, at, above)))
    assert (at is not None) == (factor != 0.15)
    done = []
    for d in sorted({1, below, above} | ({at} if at else set())):
        if d < 1 or d > room - 2:
            continue
        merges = d < r
        hi = np.float32(d) / np.float32(4 ** level)                     # the smallest factor whose radius lies above d
        while not hc.radius(level, hi) > d:
            hi = np.nextafter(hi, np.float32(np.inf))
        hi = float(hi)
        far = int(np.ceil(max(r, hc.radius(level, hi))))
        sizes = [n for n in range(0, 14) if merges or hc.lsh_k(2 + n, level, factor) == hc.lsh_k(2 + n, level, hi) > 0]   # batches at which both factors give the same k
        proof = bool(sizes)                                             # (level 2, r = 2, d = 3: no batch size gives both factors the same k; d = 2 carries the proof there)
        sizes = sizes or [3]
        for seed in range(120):
            try:
                case = hc.pair_case("n-L%d-f%r-d%d-s%d" % (level, factor, d, seed), level, d, seed, sizes[(seed // 2) % len(sizes)], far, base, factor=factor)
            except AssertionError:
                continue                                                # (the lowest levels have no room for every filler count)
            decoded = timed(hc.decode, oracle, case)
            hc.tiles_decode_as_painted(case, *decoded)
            a, b = (decoded[0][hc.item_of_tile(case, decoded[1], k)] for k in (0, 1))
            assert hc.distance(a["states"], b["states"]) == d
            ref = timed(hc.bake, oracle, case, flags=hc.NEAR | ot.FLAG_FORCE32)
            if merges and not hc.merged_with(ref, case, decoded[1], 0, 1):
                continue                                                # no shared bucket in this placement
            if not merges:
                assert not hc.merged_with(ref, case, decoded[1], 0, 1), (case["name"], "merged at distance %d, r = %r" % (d, float(r)))
                wide = timed(hc.bake, oracle, case, flags=hc.NEAR | ot.FLAG_FORCE32, factor=hi)
                if proof and not hc.merged_with(wide, case, decoded[1], 0, 1):
                    continue                                            # never compared
                assert not proof or len(wide.descs) == len(ref.descs) - 1   # (and the fillers stay apart under both factors)
            check(oracle, program, tmp_path, case, [{}] + ([] if merges else [{"factor": hi}]), decoded)
            done.append((d, merges, seed, merges or proof))
            break
        else:
            raise AssertionError("no placement for level %d factor %r d %d" % (level, factor, d))
    print("placed (d, merges, seed, shown to be compared):", done)
    assert any(not m and p for d, m, s, p in done) and (level == 1 or any(m for d, m, s, p in done))
    assert at is None or any(d == at and p for d, m, s, p in done)


def test_n_degenerate_factors(oracle, program, tmp_path):
    """factor 0 (r = 0: k converts from +inf to 0, the level is skipped), a negative factor (k = ceil(-ln(n) / 4) = -0 -> 0: skipped), both merging nothing;
    factor 1.0 (r = 4^level: blocks that differ in all but one micro-triangle merge); NaN (every comparison false)"""
    rng = np.random.default_rng(11)
    near = hc.pick(rng, 2, 3)
    tiles = [hc.tile(2, near), hc.tile(2, near[:2]), hc.tile(2, (), "T"), hc.tile(2, (3,), "T"), hc.tile(2, (3, 7), "O", 7, 7), hc.tile(2, (3, 9), "T", 8, 8)]
    case = hc.painted("n-degenerate", tiles, flags=hc.NEAR)
    decoded = timed(hc.decode, oracle, case)
    hc.tiles_decode_as_painted(case, *decoded)
    assert hc.lsh_k(5, 2, 0.0) == 0 and hc.lsh_k(5, 2, -1.0) == 0 and hc.lsh_k(5, 2, 1.0) == 1
    refs, _ = check(oracle, program, tmp_path, case, [{"factor": f} for f in (0.0, -1.0, float("nan"), 0.15, 1.0)], decoded)
    plain = timed(hc.bake, oracle, case, flags=ot.FLAG_THREADS | ot.FLAG_FORCE32)
    for ref in refs[:3]:
        hc.same("nothing merges", ref, plain)
    assert hc.merged_with(refs[3], case, decoded[1], 0, 1) and hc.merged_with(refs[3], case, decoded[1], 3, 5) and len(refs[3].descs) == 3
    assert len(refs[4].descs) < 3                                        # factor 1: an opaque-based and a transparent-based block merge as well
    merged = refs[4].array_data
    assert ((merged >> 0) & 3 == ot.UO).any() or ((merged >> 2) & 3 == ot.UO).any()   # known against known gave UnknownOpaque beside the bake's UnknownTransparent


BATCHES = [1, 2, 16, 17, 81, 82, 256, 257]


@pytest.mark.parametrize("n", BATCHES)
def test_n_batch_sizes_at_the_steps_of_the_table_count(oracle, program, tmp_path, n):
    """n mergeable level-3 items of one batch (near pairs at d = 1 .. 3, the pairs far from each other): L = ceil(n^0.25) steps at 16 / 17, 81 / 82 and
    256 / 257; a batch of 1 has k = 0 and draws nothing"""
    rng = np.random.default_rng(n)
    tiles = []
    while len(tiles) < n:
        a = hc.pick(rng, 3, int(rng.integers(18, 40)), "O")
        tiles.append(hc.tile(3, a, "O"))
        if len(tiles) < n:
            tiles.append(hc.tile(3, a + hc.pick(rng, 3, 1 + len(tiles) % 3, "O", avoid=a), "O"))
    case = hc.painted("n-batch-%d" % n, tiles, flags=hc.NEAR, shuffle=n)
    (ref,), (items, tri_item) = check(oracle, program, tmp_path, case)
    assert len(items) == n and all(not (it["states"] == it["states"][0]).all() for it in items)
    want_L = {1: 1, 2: 2, 16: 2, 17: 3, 81: 3, 82: 4, 256: 4, 257: 5}[n]
    assert hc.lsh_tables(n) == want_L and (hc.lsh_k(n, 3, 0.15) > 0) == (n > 1)
    pairs = sum(hc.merged_with(ref, case, tri_item, k, k + 1) for k in range(0, n - 1, 2))
    print("batch %d: L = %d, k = %d, %d of %d pairs merged, %d descriptors" % (n, want_L, hc.lsh_k(n, 3, 0.15), pairs, n // 2, len(ref.descs)))
    assert pairs >= (n // 2) * 3 // 4 and len(ref.descs) <= n - pairs


def test_n_mixed_levels_one_stream_of_draws(oracle, program, tmp_path):
    """levels 1 - 6 shuffled over the input, one level with exactly one non-special item between two levels with many, one level with none: the one stream
    of std::mt19937(42) is consumed level by level and a skipped level draws nothing.  That the outcome at the levels above depends on where the stream
    stands is shown with the oracle alone: with a second item at level 2 (the level then draws L * k values) other blocks merge at levels 3 - 6"""
    found = None
    for seed in range(20):
        case = hc.painted("n-mixed-s%d" % seed, hc.mixed_levels_tiles(seed), flags=hc.NEAR, shuffle=seed)
        other = hc.painted("n-mixed-two-s%d" % seed, hc.mixed_levels_tiles(seed, lone=2), flags=hc.NEAR, shuffle=seed)
        ref, ref2 = (timed(hc.bake, oracle, c, flags=hc.NEAR | ot.FLAG_FORCE32) for c in (case, other))
        high = lambda c, r: sorted((int(c["tile_of"][t]) - (1 if c is other and c["tile_of"][t] > 6 else 0), int(r.index[t])) for t in range(len(r.index)) if c["tiles"][c["tile_of"][t]]["level"] >= 3)
        groups = lambda c, r: sorted(tuple(sorted(k for k, v in high(c, r) if v == w)) for w in {v for k, v in high(c, r)})
        if groups(case, ref) != groups(other, ref2):
            found = seed
            break
    assert found is not None
    print("seed %d: the merges at levels 3 - 6 change when level 2 draws" % found)
    for c in (case, other):
        (r,), (items, tri_item) = check(oracle, program, tmp_path, c)
        hc.tiles_decode_as_painted(c, items, tri_item)
        levels = [it["level"] for it in items if not (it["states"] == it["states"][0]).all()]
        assert sorted(set(levels)) == [1, 2, 3, 5, 6] and levels.count(2) == (1 if c is case else 2) and len(r.descs) < len(levels)
        assert np.any(np.diff([it["level"] for it in items]) < 0)


@pytest.mark.parametrize("brute", [0, hc.BRUTE])
def test_n_two_state_bakes_merge_nothing(oracle, program, tmp_path, brute):
    """OC1_2_State items never enter a batch: with the flag the result is the one without"""
    tiles = hc.mixed_levels_tiles(3)
    case = hc.painted("n-two-state", tiles, TWO, flags=hc.NEAR | brute, shuffle=1)
    (ref, t0), _ = check(oracle, program, tmp_path, case, [{}, {"flags": ot.FLAG_THREADS, "budget": hc.NO_REDUCTION}])
    hc.same("2-state", ref, t0)


@pytest.mark.parametrize("promo", [ot.PROMO_FORCE_TRANSPARENT, ot.PROMO_FORCE_OPAQUE])
@pytest.mark.parametrize("brute", [0, hc.BRUTE])
def test_n_uniform_items_that_are_not_special(oracle, program, tmp_path, promo, brute):
    """DisableSpecialIndices: uniform T / O / UT (UO with ForceOpaque) items stay ordinary items and meet near-uniform ones (one defect) as merge target
    (the uniform item comes first) and as merge source (it comes second), at levels 1 (through a factor of 0.3), 2 and 3, also under a budget"""
    tiles = []
    for L in (2, 3, 1):
        full = tuple(range(4 ** L))
        tiles += [hc.tile(L, (), "O"), hc.tile(L, (1,), "O", 7, 7), hc.tile(L, (2,), "T", 8, 6), hc.tile(L, (), "T", 9, 6),
                  hc.tile(L, full, "O", 6, 8), hc.tile(L, full[1:], "O", 6, 9), hc.tile(L, full[:-1], "T", 6, 10), hc.tile(L, full, "T", 6, 11)]
    flags = hc.NEAR | ot.FLAG_NO_SPECIAL | brute
    case = hc.painted("n-uniform-promo%d" % promo, tiles, flags=flags, promo=promo, factor=0.3)
    refs, (items, tri_item) = check(oracle, program, tmp_path, case, [{}, {"budget": 1}])   # (1: everything ends at level 0 in every order; budgets between meet the uniform items' tied keys)
    hc.tiles_decode_as_painted(case, items, tri_item)
    assert sum((it["states"] == it["states"][0]).all() for it in items) == 12
    ref = refs[0]
    known = case["tile_of"] % 8 < 4
    assert (ref.index[known] >= 0).all()
    # The all-unknown group at the LSH shows how the reference treats an item that was merged away: it keeps its states and still enters the second
    # DeduplicateExact.  The uniform item takes the near-uniform one, is itself taken by the other near-uniform one later in the same pass, and that one,
    # now all-unknown, is then found a duplicate of the dead uniform item, which comes first: every triangle of the group ends at the dead item's marker,
    # -1, the value of FullyTransparent.  The oracle restates that, and so does the host tail.
    assert ((ref.index[~known] == -1).all() if not brute else (ref.index[~known] >= 0).all()), ref.index
    merged = [hc.merged_with(ref, case, tri_item, k, k + 1) for k in range(0, 24, 2)]
    print("uniform / near-uniform pairs merged:", merged)
    assert all(merged[k] for k in (0, 1, 4, 5)) and [merged[8], merged[9]] == [not brute] * 2   # (brute force: 1 / 16 and 1 / 64 lie below 0.1, 1 / 4 does not)


def test_n_merge_to_all_unknown_and_rejection_of_the_merged_item(oracle, program, tmp_path):
    """a level-1 pair [U U O U] / [O U U U] under factor 0.75 (r = 3 > 2) merges to all-unknown, which the second promotion turns into a special index; a
    level-2 pair of 9 / 16 known each merges to 8 / 16 and is rejected under a threshold of 0.55, which rejects neither alone"""
    for seed in range(40):
        rng = np.random.default_rng(seed)
        case = hc.painted("n-all-unknown", [hc.tile(1, (0, 1, 3), "O"), hc.tile(1, (1, 2, 3), "O", 7, 7)] + [hc.tile(1, hc.pick(rng, 1, 2, "T"), "T", 8 + k, 6) for k in range(seed % 3)],
                          flags=hc.NEAR, factor=0.75)
        ref = timed(hc.bake, oracle, case, flags=hc.NEAR | ot.FLAG_FORCE32)
        if ref.index[0] == ref.index[1] == ot.SPECIAL_FUT:
            break
    else:
        raise AssertionError("the level-1 pair never shares a bucket")
    check(oracle, program, tmp_path, case)
    plain = timed(hc.bake, oracle, case, flags=ot.FLAG_THREADS | ot.FLAG_FORCE32)
    assert plain.index[0] >= 0 and plain.index[1] >= 0 and plain.index[0] != plain.index[1]
    for seed in range(40):
        rng = np.random.default_rng(100 + seed)
        x = hc.pick(rng, 2, 6, "O")
        a, b = hc.pick(rng, 2, 2, "O", avoid=x)
        case = hc.painted("n-rejected", [hc.tile(2, x + (a,), "O"), hc.tile(2, x + (b,), "O", 7, 7)], flags=hc.NEAR, rejection=0.55)
        ref = timed(hc.bake, oracle, case, flags=hc.NEAR | ot.FLAG_FORCE32)
        if ref.index[0] == ref.index[1] == ot.SPECIAL_FUT:
            break
    else:
        raise AssertionError("the level-2 pair never shares a bucket")
    (ref, kept), _ = check(oracle, program, tmp_path, case, [{}, {"rejection": 0.5}])
    assert kept.index[0] == kept.index[1] >= 0 and len(kept.descs) == 1
    plain = timed(hc.bake, oracle, case, flags=ot.FLAG_THREADS | ot.FLAG_FORCE32)
    assert len(plain.descs) == 2


def test_n_no_reducer_runs_without_duplicate_detection(oracle, program, tmp_path):
    """DisableDuplicateDetection: every triangle keeps a block of its own, exact duplicates included, and the budget still applies.  Together with the
    near-duplicate flag the ABI answers INVALID_ARGUMENT; the program, which takes the flags as they are, then merges nothing"""
    rng = np.random.default_rng(2)
    a = hc.pick(rng, 3, 20, "O")
    tiles = [hc.tile(3, a, "O", tris=2), hc.tile(3, a + hc.pick(rng, 3, 1, "O", avoid=a), "O", 7, 8), hc.tile(2, (1, 2), "O", tris=3), hc.tile(2, (1, 2), "O", 9, 7)]
    flags = hc.NEAR | ot.FLAG_NO_DEDUP
    case = hc.painted("n-no-dedup", tiles, flags=flags, shuffle=4)
    decoded = decode_for(oracle, case, flags)
    items, tri_item = decoded
    assert len(items) == 7
    for f in (flags, flags | hc.BRUTE):                                 # the ABI refuses the combination (ValidateDesc), in the oracle as in the reference
        assert timed(hc.bake, oracle, case, flags=f, expect=ot.INVALID_ARGUMENT) is None
    plain = ot.FLAG_THREADS | ot.FLAG_NO_DEDUP
    refs, _ = check(oracle, program, tmp_path, case, [{"flags": plain, "budget": hc.NO_REDUCTION}, {"flags": plain, "budget": 1}], decoded)
    assert len(refs[0].descs) == 7 and len(set(refs[0].index.tolist())) == 7 and len(refs[1].descs) == 0 and (refs[1].index < 0).all()   # (budget 1: everything ends at level 0 and is promoted)
    got = run_program(program, tmp_path, [hc.encode_case(case, items, len(tri_item), flags=f, budget=b) for f in (flags, flags | hc.BRUTE) for b in (hc.NO_BUDGET, 1)])
    for k, g in enumerate(got):                                         # host_tail.cpp itself, should the flags ever reach it: no reducer runs
        hc.same("no-dedup %d" % k, g, refs[k % 2])


def test_n_items_of_several_triangles(oracle, program, tmp_path):
    """work items of 2 and 5 triangles, their triangles interleaved in the input: a merge appends the source's triangles to the target's, and every
    triangle of both ends at the target's descriptor"""
    for seed in range(30):
        rng = np.random.default_rng(seed)
        a, c = hc.pick(rng, 3, 20, "O"), hc.pick(rng, 4, 100, "O")
        tiles = [hc.tile(3, a, "O", tris=2), hc.tile(3, a + hc.pick(rng, 3, 2, "O", avoid=a), "O", 7, 8, tris=5),
                 hc.tile(4, c, "O", tris=5), hc.tile(4, c + hc.pick(rng, 4, 3, "O", avoid=c), "O", 7, 8, tris=2), hc.tile(3, hc.pick(rng, 3, 30, "O"), "O", 9, 9, tris=3)]
        case = hc.painted("n-several-s%d" % seed, tiles, flags=hc.NEAR, shuffle=seed)
        (ref,), (items, tri_item) = check(oracle, program, tmp_path, case)
        if hc.merged_with(ref, case, tri_item, 0, 1) and hc.merged_with(ref, case, tri_item, 2, 3):
            break
    else:
        raise AssertionError("no placement")
    assert sorted(len(it["prims"]) for it in items) == [2, 2, 3, 5, 5] and len(ref.descs) == 3
    for k in (0, 2):
        t = np.nonzero((case["tile_of"] == k) | (case["tile_of"] == k + 1))[0]
        assert len(t) == 7 and len(set(ref.index[t].tolist())) == 1 and np.any(np.diff(case["tile_of"][t]) < 0)
    assert sorted(ref.index_hist) == [(7, 4, 2), (10, 3, 2)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# B: brute force
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,d_in,d_out", [(2, 1, 2), (3, 6, 7), (4, 25, 26)])
def test_b_distances_around_a_tenth(oracle, program, tmp_path, level, d_in, d_out):
    """dist / n < 0.1f: 1 / 16, 6 / 64 and 25 / 256 merge, 2 / 16, 7 / 64 and 26 / 256 do not (every pair inside the window is compared)"""
    assert np.float32(d_in) / np.float32(4 ** level) < np.float32(0.1) <= np.float32(d_out) / np.float32(4 ** level)
    for d, merges in ((d_in, True), (d_out, False)):
        for seed in (0, 1):                                            # both orders of the fuller block
            case = hc.pair_case("b-L%d-d%d-s%d" % (level, d, seed), level, d, seed, 0, 0, base="O", flags=hc.NEAR | hc.BRUTE)
            (ref,), (items, tri_item) = check(oracle, program, tmp_path, case)
            assert hc.distance(items[0]["states"], items[1]["states"]) == d and hc.merged_with(ref, case, tri_item, 0, 1) == merges



def window_case(gap):
    """2 100 level-2 items, every one an even number of unknown micro-triangles (any two differ in two or more: 2 / 16 is no merge), and one near pair: item
    20 + gap is item 20 with one more, three or more away from every other item"""
    rng = np.random.default_rng(2048)
    words = rng.permutation(1 << 16)
    even = [w for w in words.tolist() if bin(w).count("1") % 2 == 0 and 2 <= bin(w).count("1") <= 12][:2100]
    family = set(even)
    for x in range(16):
        p = even[20] | (1 << x)
        if p != even[20] and all((p ^ (1 << y)) not in family or (p ^ (1 << y)) == even[20] for y in range(16)):
            break
    else:
        raise AssertionError("no partner")
    family.discard(even[20 + gap])
    even[20 + gap] = p
    assert len(set(even)) == 2100
    tiles = [hc.tile(2, [j for j in range(16) if w >> j & 1], "O") for w in even]
    return hc.painted("b-window-%d" % gap, tiles, flags=hc.NEAR | hc.BRUTE)


@pytest.mark.parametrize("gap", [2048, 2049])
def test_b_window_of_2048_items(oracle, program, tmp_path, gap):
    """a near pair 2048 positions apart lies inside the window of the earlier item, 2049 apart outside: the only merge of the bake, or none"""
    case = window_case(gap)
    (ref,), (items, tri_item) = check(oracle, program, tmp_path, case)
    assert len(items) == 2100 and hc.distance(items[20]["states"], items[20 + gap]["states"]) == 1
    assert hc.merged_with(ref, case, tri_item, 20, 20 + gap) == (gap == 2048) and len(ref.descs) == (2099 if gap == 2048 else 2100)


def test_b_partner_already_taken_and_mixed_levels(oracle, program, tmp_path):
    """A, C, B in input order with B one away from both: A takes B; C, which looks forward only, finds B gone and stays alone although A is two away.
    Then levels 1 - 6 in one bake"""
    rng = np.random.default_rng(9)
    x = hc.pick(rng, 3, 20, "O")
    a, c = hc.pick(rng, 3, 2, "O", avoid=x)
    case = hc.painted("b-taken", [hc.tile(3, x + (a,), "O"), hc.tile(3, x + (c,), "O", 7, 7), hc.tile(3, x, "O", 8, 8)], flags=hc.NEAR | hc.BRUTE)
    (ref,), (items, tri_item) = check(oracle, program, tmp_path, case)
    assert hc.merged_with(ref, case, tri_item, 0, 2) and not hc.merged_with(ref, case, tri_item, 1, 2) and len(ref.descs) == 2
    case = hc.painted("b-mixed", hc.mixed_levels_tiles(4), flags=hc.NEAR | hc.BRUTE, shuffle=4)
    (ref,), (items, tri_item) = check(oracle, program, tmp_path, case)
    plain = timed(hc.bake, oracle, case, flags=ot.FLAG_THREADS | ot.FLAG_FORCE32)
    assert len(ref.descs) < len(plain.descs) and len({int(l) for o, l, f in ref.descs}) >= 4


# ---------------------------------------------------------------------------------------------------------------------------------------------
# C: the budget
# ---------------------------------------------------------------------------------------------------------------------------------------------
def active_items(case, items, tri_item, flags):
    """the items that enter the budget walk of a bake without a near-duplicate merge: not special, the first of their digest, with the triangles of their
    exact duplicates"""
    rs = tc.restate_tail(tc.tail_inputs(case, case["raw"], flags), flags, case["rejection"])
    out = []
    for i in rs["emitted"].tolist():
        if items[i]["level"] > 0:
            out.append(dict(states=items[i]["states"], level=items[i]["level"], area=hc.area_of(items[i]["uv"]), nprims=int((rs["rep"][tri_item] == i).sum()), item=i))
    return out


def levels_hold(case, ref, active, walk, tri_item, special=True):
    """the oracle's result has every item at the level the restated walk leaves it at (a special index where its states ended all equal)"""
    for a, L, s in zip(active, walk["levels"], walk["states"]):
        v = int(ref.index[np.nonzero(tri_item == a["item"])[0][0]])
        if special and (s == s[0]).all():
            assert v == -int(s[0]) - 1, (case["name"], a["item"], v, s)
        else:
            assert v >= 0 and ref.descs[v, 1] == L, (case["name"], a["item"], v, L)


def budgets_of(S, deep=False):
    return [S + 1, S, S - 1, S // 2, S // 8] + ([S // 32] if deep else [])


def drawn_budget_case(oracle, name, levels, count, fmt, must_pin, deep=False):
    """the first draw whose restated walk is pinned under the budgets of budgets_of(S) numbered in must_pin"""
    for seed in range(40):
        case = hc.painted("%s-fmt%d-s%d" % (name, fmt, seed), hc.budget_tiles(seed, levels, count), fmt, shuffle=seed)
        case["raw"] = timed(hc.bake, oracle, case, flags=tc.RAW_FLAGS, budget=hc.NO_BUDGET, rejection=0.0)
        items, tri_item = hc.work_items(case, case["raw"])
        active = active_items(case, items, tri_item, case["flags"])
        S = hc.budget_walk(active, hc.NO_REDUCTION)["S"]
        walks = [hc.budget_walk(active, b, need_pinned=False) for b in budgets_of(S, deep)]
        if all(walks[k]["pinned"] for k in must_pin):
            return case, items, tri_item, active, S, walks, seed
    raise AssertionError("no draw with a pinned walk")


def compare_budgets(oracle, program, tmp_path, case, items, tri_item, active, S, walks, deep=False):
    """the pinned budgets, and 1 and 0, against the oracle; the others through the program alone.  -> (budget, items that dropped, most levels dropped,
    rounds, steps back) per pinned budget"""
    hc.tiles_decode_as_painted(case, items, tri_item)
    pinned = [(b, w) for b, w in zip(budgets_of(S, deep), walks) if w["pinned"]]
    budgets = [b for b, w in pinned] + [1, 0]
    refs, _ = check(oracle, program, tmp_path, case, [{"budget": b} for b in budgets], (items, tri_item))
    start = np.array([a["level"] for a in active])
    summary = []
    for (b, w), ref in zip(pinned, refs):
        levels_hold(case, ref, active, w, tri_item)
        drops = start - np.array(w["levels"])
        summary.append((b, int((drops > 0).sum()), int(drops.max()), w["rounds"], w["revisits"]))
        assert w["total"] < b or not any(w["levels"])
    for ref in refs[-2:]:
        assert len(ref.descs) == 0 or (ref.descs[:, 1] == 0).all()
    rest = [b for b, w in zip(budgets_of(S, deep), walks) if not w["pinned"]]
    for g in run_program(program, tmp_path, [hc.encode_case(case, items, len(tri_item), budget=b, uniform_form=u) for b in rest for u in (True, False)]):
        hc.invariants_hold(case["name"], g, case["fmt"], len(tri_item))
    return summary, rest


@pytest.mark.parametrize("fmt", tc.FORMATS)
@pytest.mark.parametrize("levels", [(4,), (3,), (1, 2, 3, 4, 5, 3, 4, 2, 3, 4, 5, 6, 2, 3, 4, 3)], ids=["level4", "level3", "mixed"])
def test_c_budgets_against_the_oracle(oracle, program, tmp_path, levels, fmt):
    """40 - 72 items of pairwise different areas; budgets S + 1 (untouched), S and S - 1 (the item of the lowest key drops), S / 2, S / 8, then 1 and 0
    (everything ends at level 0 in whatever order the walk goes, so these two are compared although several level-1 keys are +inf on the way).  The
    generator re-draws until the restated walk is pinned (host_tail_cases.budget_walk) under the first four budgets.  With this many items two keys
    area * coverage / bytes meet somewhere among the items that S / 8 reaches in every draw tried; where they do, S / 8 goes through the program alone"""
    count = {(4,): 60, (3,): 40}.get(levels, 72)
    case, items, tri_item, active, S, walks, seed = drawn_budget_case(oracle, "c-" + "".join(map(str, levels[:6])), levels, count, fmt, (0, 1, 2, 3))
    summary, rest = compare_budgets(oracle, program, tmp_path, case, items, tri_item, active, S, walks)
    print("seed %d, %d active items, S = %d; (budget, items that dropped, most levels dropped, rounds, steps back):" % (seed, len(active), S), summary, "program alone:", rest)
    assert summary[0][1] == 0 and summary[1][1] >= 1 and summary[2][1] >= 1 and summary[3][1] > summary[1][1]
    assert len([a for a in active if a["level"] == 1]) <= 1
    assert len({float(a["area"]) for a in active}) == len(active) and (fmt == TWO or any(a["nprims"] > 1 for a in active))


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_c_deep_drop_beside_an_item_that_keeps_its_level(oracle, program, tmp_path, fmt):
    """a level-5 item that loses next to nothing by dropping (one unknown micro-triangle) beside a small level-2 item that loses much: with S = 260 the
    walk takes the level-5 item down one, two and three levels, stepping back onto it each time (the `i--`: its new key stays below the neighbour's), and
    the level-2 item keeps its level.  The totals on the way are 68 and 20: budgets of 69 / 68 / 67 and 21 / 20 / 19 put `total < maxArrayDataSize` at
    the exact size and one either side"""
    base, promo = ("O", ot.PROMO_FORCE_TRANSPARENT) if fmt == FOUR else ("T", ot.PROMO_FORCE_OPAQUE)
    case = hc.painted("c-deep-fmt%d" % fmt, [hc.tile(5, (5,), base), hc.tile(2, (0, 5, 10), base, 9, 9)], fmt, promo=promo)
    case["raw"] = timed(hc.bake, oracle, case, flags=tc.RAW_FLAGS, budget=hc.NO_BUDGET, rejection=0.0)
    items, tri_item = hc.work_items(case, case["raw"])
    hc.tiles_decode_as_painted(case, items, tri_item)
    active = active_items(case, items, tri_item, case["flags"])
    budgets = [261, 260, 69, 68, 67, 21, 20, 19]                       # (total < budget: 68 and 20 are totals the walk passes through)
    walks = [hc.budget_walk(active, b) for b in budgets]
    assert walks[0]["S"] == 260 and [w["levels"][0] for w in walks] == [5, 4, 4, 3, 3, 3, 2, 2] and [w["revisits"] for w in walks] == [0, 0, 0, 1, 1, 1, 2, 2]
    assert all(w["levels"][1] == 2 for w in walks)
    refs, _ = check(oracle, program, tmp_path, case, [{"budget": b} for b in budgets], (items, tri_item))
    for w, ref in zip(walks, refs):
        levels_hold(case, ref, active, w, tri_item)


def test_c_two_state_parents_of_mixed_children(oracle, program, tmp_path):
    """OC1_2_State: a level-3 item over a transparent base with one opaque child under parents 0, 3 and 7 drops to level 2 under a budget of its own size
    (16: the walk counts 4-state bytes).  The three parents become UnknownOpaque (3), which the serialiser ORs in as 3 << lane: lanes 0 and 1, 3 and 4, and
    bit 7 of the first byte"""
    case = hc.painted("c-two-state", [hc.tile(3, (1, 13, 29), "T"), hc.tile(2, (), "T", 7, 7)], TWO, promo=ot.PROMO_FORCE_OPAQUE)
    refs, (items, tri_item) = check(oracle, program, tmp_path, case, [{"budget": 17}, {"budget": 16}])
    hc.tiles_decode_as_painted(case, items, tri_item)
    assert refs[0].descs.tolist() == [[0, 3, TWO]] and refs[1].descs.tolist() == [[0, 2, TWO]]
    assert refs[1].array_data.tolist() == [0x9B, 0x00] and hc.parent_states(items[0]["states"]).tolist()[:8] == [3, 0, 0, 3, 0, 0, 0, 3]


def test_c_uniform_items_that_are_not_special(oracle, program, tmp_path):
    """DisableSpecialIndices: uniform O / T / UT items of levels 1 - 4 enter the walk beside mixed ones (a uniform known item loses nothing by dropping: key 0
    for all of them, so the compared cases hold one such item; more of them go through the program alone)"""
    flags = ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL
    rng = np.random.default_rng(3)
    mixed = [hc.tile(L, hc.pick(rng, L, 4 ** L // 3 + k, "O"), "O", 6 + L, 7 + k) for k, L in enumerate((2, 3, 4, 3))]
    compared = 0
    for k, uni in enumerate([hc.tile(3, (), "O", 9, 9), hc.tile(2, (), "T", 9, 9), hc.tile(4, tuple(range(256)), "O", 9, 9)]):
        case = hc.painted("c-uniform-%d" % k, mixed[:2] + [uni] + mixed[2:], flags=flags)
        case["raw"] = timed(hc.bake, oracle, case, flags=tc.RAW_FLAGS, budget=hc.NO_BUDGET, rejection=0.0)
        items, tri_item = hc.work_items(case, case["raw"])
        active = active_items(case, items, tri_item, flags)
        assert len(active) == 5
        S = hc.budget_walk(active, hc.NO_REDUCTION)["S"]
        walks = [(b, hc.budget_walk(active, b, need_pinned=False)) for b in (S, S - 8, S * 3 // 4, S // 2, S // 4)]
        budgets = [b for b, w in walks if w["pinned"]]                  # (once the uniform item reaches level 1 its key is 0 / 0)
        print("uniform item %d: S = %d, (budget, pinned):" % (k, S), [(b, w["pinned"]) for b, w in walks])
        compared += len(budgets)
        if not budgets:
            continue
        refs, _ = check(oracle, program, tmp_path, case, [{"budget": b} for b in budgets], (items, tri_item))
        for (b, w), ref in zip([bw for bw in walks if bw[1]["pinned"]], refs):
            levels_hold(case, ref, active, w, tri_item, special=False)
        assert budgets[0] != S or walks[0][1]["levels"][2] == uni["level"] - 1   # key 0, below the mixed items': the uniform item drops first
    assert compared >= 2
    many = hc.painted("c-uniform-many", mixed + [hc.tile(L, (), b, 8 + L, 9) for L in (1, 2, 3, 4) for b in "OT"] + [hc.tile(2, tuple(range(16)), "O", 13, 13)], flags=flags)
    items, tri_item = timed(hc.decode, oracle, many)
    got = run_program(program, tmp_path, [hc.encode_case(many, items, len(tri_item), budget=b, uniform_form=u) for b in (200, 60, 20, 1) for u in (True, False)])
    for g in got:
        hc.invariants_hold(many["name"], g, FOUR, len(tri_item))
    for k in range(0, len(got), 2):
        assert got[k].array_data.size == got[k + 1].array_data.size


def test_c_budget_and_near_duplicates_together(oracle, program, tmp_path):
    """merge, promotion, budget walk and the second DeduplicateExact in one bake: C and C' merge at the LSH; A and B, 24 apart (r = 9.6), have their unknown
    micro-triangles under the same six parents, so they are equal blocks only after both dropped a level, and the second DeduplicateExact merges them"""
    rng = np.random.default_rng(8)
    parents = rng.choice(16, 6, replace=False)
    c = hc.pick(rng, 3, 20, "O")
    tiles = [hc.tile(3, [4 * p + k for p in parents for k in (0, 1)], "O"), hc.tile(3, [4 * p + k for p in parents for k in (2, 3)], "O", 7, 8),
             hc.tile(3, c, "O", 9, 9), hc.tile(3, c + hc.pick(rng, 3, 1, "O", avoid=c), "O", 8, 10), hc.tile(4, hc.pick(rng, 4, 90, "O"), "O", 6, 9)]
    case = hc.painted("c-near", tiles, flags=hc.NEAR)
    items, tri_item = timed(hc.decode, oracle, case)
    assert hc.distance(items[0]["states"], items[1]["states"]) == 24 and np.array_equal(hc.parent_states(items[0]["states"]), hc.parent_states(items[1]["states"]))
    merged = np.where((items[2]["states"] != items[3]["states"]), ot.UT, items[2]["states"])
    active = [dict(states=it["states"], level=it["level"], area=hc.area_of(it["uv"]), nprims=1) for it in (items[0], items[1])]
    active += [dict(states=merged, level=3, area=hc.area_of(items[2]["uv"]), nprims=2), dict(states=items[4]["states"], level=4, area=hc.area_of(items[4]["uv"]), nprims=1)]
    S = hc.budget_walk(active, hc.NO_REDUCTION)["S"]
    assert S == 16 * 3 + 64
    found = None
    for b in range(S, 8, -1):
        w = hc.budget_walk(active, b, need_pinned=False)
        if w["pinned"] and w["levels"][0] == w["levels"][1] == 2:
            found = b
            break
    assert found
    refs, _ = check(oracle, program, tmp_path, case, [{}, {"budget": found}], (items, tri_item))
    assert len(refs[0].descs) == 4 and refs[0].index[2] == refs[0].index[3] and refs[0].index[0] != refs[0].index[1]
    assert refs[1].index[2] == refs[1].index[3] and refs[1].index[0] == refs[1].index[1] >= 0 and refs[1].descs[refs[1].index[0], 1] == 2
    print("budget %d of S = %d: levels %r" % (found, S, w["levels"]))


def test_c_tied_and_nan_keys_through_the_program_alone(oracle, program, tmp_path):
    """not compared with the oracle, because the reference leaves the order open: several level-1 items (memDelta == 0: keys +inf), level-1 and level-2 items
    without a known micro-triangle before and after (0 / 0: NaN keys; UT beside UO, states no bake of one promotion yields), equal items of equal area
    (tied keys), and the smallest budget that leaves an item above level 0.  Held to: the call returns, no sanitizer report, offsets are the running sum of
    the sizes, every triangle points at a descriptor or a special index, the histograms sum to the descriptors"""
    rng = np.random.default_rng(12)
    uv = lambda k: [0.01 * k, 0.0, 0.01 * k + 0.004 + 0.0001 * (k % 3), 0.0, 0.01 * k, 0.003]
    items = []
    for k in range(24):
        L = (1, 1, 2, 1, 3, 2)[k % 6]
        s = rng.integers(0, 4, 4 ** L).astype(np.uint8)
        if k % 4 == 1:
            s = rng.integers(2, 4, 4 ** L).astype(np.uint8)           # no known micro-triangle: NaN
            s[:2] = [ot.UT, ot.UO]
        if k % 8 == 2:
            s = items[-2]["states"].copy() if items[-2]["level"] == L else s
        items.append(dict(level=L, uv=np.array(uv(k), np.float32), prims=np.array([2 * k, 2 * k + 1][:1 + k % 2], np.uint32), states=s))
    case = dict(fmt=FOUR, flags=ot.FLAG_THREADS, rejection=0.0, name="c-unpinned")
    total = sum(max(1, 4 ** it["level"] // 4) for it in items)
    blobs, names = [], []
    for flags in (ot.FLAG_THREADS, ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL, hc.NEAR, ot.FLAG_THREADS | ot.FLAG_NO_DEDUP):
        for b in (total + 1, total, total - 1, total // 2, len(items) + 2, len(items) + 1, len(items), 1, 0):
            for u in (True, False):
                blobs.append(hc.encode_case(case, items, 48, flags=flags, budget=b, uniform_form=u))
                names.append((flags, b, u))
    for name, g in zip(names, run_program(program, tmp_path, blobs)):
        hc.invariants_hold(name, g, FOUR, 48)
        assert (g.index[[2 * k + 1 for k in range(24) if k % 2 == 0]] == ot.SPECIAL_FUO).all()     # the triangles of no item stay unresolved
    # the smallest budget that leaves an item above level 0, located by running every budget up to the total: below it no descriptor is above level 0, at
    # it one is, and it lies above the number of items that enter the walk (each of them counts a byte at least, whatever its level)
    flags = ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL | ot.FLAG_NO_DEDUP          # every item keeps a descriptor: its level is the item's
    scan = run_program(program, tmp_path, [hc.encode_case(case, items, 48, flags=flags, budget=b) for b in range(total + 2)])
    above = [int((g.descs[:, 1] > 0).sum()) for g in scan]
    for b, g in enumerate(scan):
        hc.invariants_hold(("scan", b), g, FOUR, 48)
        assert len(g.descs) == len(items)
    smallest = next(b for b, n in enumerate(above) if n)
    print("smallest budget that leaves an item above level 0: %d (%d items above), %d items, total %d" % (smallest, above[smallest], len(items), total))
    assert len(items) < smallest <= total and above[smallest - 1] == 0 and above[smallest] >= 1 and above[total + 1] == len(items) and above[0] == above[1] == 0
