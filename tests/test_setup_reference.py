"""No GPU: the numpy restatement of SetupWorkItems' arithmetic (tests/setup_cases.py) against the oracle on every case of families 1, 2, 3, 5 and 6, and
the conditions the case families must meet for a comparison of the HIP library on them to mean something -- boundaries hit from both sides, enough triangles on which a
fused multiply-add or a reciprocal multiplication shows, tile edges crossed by duplicates, chunks holding every level.  The comparison goes through the
oracle's results: descriptor levels (every case carries DisableSpecialIndices), the index buffer (invalid triangles, shared descriptors), error codes
and log strings (the workload figure), and the per-triangle areas behind ommDebugGetStats2.  Run with -s for the counts recorded in tests/README.md."""
import time
import numpy as np
import pytest
import ommtest as ot
import setup_cases as sc

ALL_SCALES = sc.POW2_SCALES + sc.ROUNDED_SCALES
ORACLE_SECONDS_PER_TEST = 3.0      # the bound on the oracle's side of one test; a test above it is sliced
SPENT = [0.0, 0]                   # oracle seconds and bakes of the running test


@pytest.fixture(autouse=True)
def oracle_time_of_this_test(request):
    """every test of this file mirrors one device test bake for bake: the oracle's share of its time is measured here, printed and bounded"""
    SPENT[:] = [0.0, 0]
    yield
    if SPENT[1]:
        print("oracle side of %s: %d bakes, %.2f s" % (request.node.name, SPENT[1], SPENT[0]))
    assert SPENT[0] < ORACLE_SECONDS_PER_TEST, (request.node.name, SPENT)


def check(oracle, case, dedup=True):
    """oracle bake of a case == restatement: validity, levels, first occurrences, areas; returns (setup, oracle result)"""
    t0 = time.perf_counter()
    r = sc.run(oracle, case, want_areas=True)
    SPENT[0] += time.perf_counter() - t0
    SPENT[1] += 1
    s = sc.setup(case)
    first = sc.first_occurrence(s["p"], s["level"], s["invalid"], dedup)
    sc.check_result_against_restatement(case, r["result"], s, first)
    assert np.array_equal(r["areas"].view(np.uint32), s["area"].view(np.uint32)), case["name"]
    return s, r


def test_half_and_unorm_fetch_of_every_pattern():
    """all 65 536 patterns: binary16 against numpy's own float16 (NaN payloads aside), unorm16 against the float64 quotient rounded once"""
    h = np.arange(65536, dtype=np.uint32)
    got = sc.half_to_float(h)
    want = h.astype(np.uint16).view(np.float16).astype(np.float32)
    fin = np.isfinite(want)
    assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32))
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert (~fin).sum() == 2 * 1024 and np.isnan(want).sum() == 2 * 1023
    assert np.array_equal(got[~fin].view(np.uint32), ((h[~fin] & 0x8000) << 16) | 0x7F800000 | ((h[~fin] & 0x3FF) << 13))
    u = h.astype(np.float32) * sc.UNORM_SCALE
    assert np.abs(u.astype(np.float64) - h / 65535.0).max() <= 2.0 ** -24 and u[65535] == np.float32(1.0)


def test_conversions_and_level_of_count():
    f = np.float32
    assert sc.cvt_u32(np.array([0.99, 1.0, 4294967296.0, 4294967808.0, 2.0 ** 63, np.nan, np.inf, -1.0, 9.2233715e18], f)).tolist() == \
        [0, 1, 0, 512, 0, 0, 0, 0xFFFFFFFF, (2 ** 63 - 2 ** 39) & 0xFFFFFFFF]
    assert sc.cvt_i32(np.array([1.999, -1.999, 2147483648.0, np.nan, -2147483648.0], f)).tolist() == [1, -1, -2147483648, -2147483648, -2147483648]
    v = [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 2 ** 31 - 128, 2 ** 31, 2 ** 31 + 256, 512]
    assert sc.level_of_count(np.array(v, np.uint64)).tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 15, 15, 0, 4]


def test_family1_reaches_every_boundary():
    """numpy alone: every count k that a few-texel triangle reaches at a scale -- the listed ones, the real level steps 2 * 4^L + 1, the floats around 2^24,
    2^31, 2^32 (with 2^32 + 512) and 2^63 -- has a triangle whose quotient is the float below k and one above it, and k itself wherever some area
    divides to it (always with an exact division).  A search that finds no triangle drops a boundary: this is where that shows"""
    big = {}
    for scale in ALL_SCALES:
        by_k = {}
        for p, shape, k, side in sc.family1_triangles(scale):
            by_k.setdefault(k, set()).add(side)
        want = {k for k in sc.ALL_K if sc.reachable(k, scale)}
        assert want and want == set(by_k), (scale, sorted(want ^ set(by_k)))
        for k in sorted(by_k):
            assert by_k[k] == {-1, 0, 1} if scale in sc.POW2_SCALES else {-1, 1} <= by_k[k], (scale, k, by_k[k])
        for k in sc.BIG_K + [2.0 ** 32 + 512]:
            if k in by_k:
                big.setdefault(k, []).append(scale)
    assert all(len(big.get(k, [])) >= 1 for k in sc.BIG_K + [2.0 ** 32 + 512]), big
    assert {2.0 ** -16, 1e-5} <= set(big[2.0 ** 31]) & set(big[2.0 ** 32]) & set(big[2.0 ** 32 + 512]) and 1e-9 in big[2.0 ** 63], big


FAMILY1_TESTS = [(s, v) for s in ALL_SCALES for v in sc.FAMILY1_VARIANTS]


@pytest.mark.parametrize("scale,variant", FAMILY1_TESTS, ids=["%g-%s" % sv for sv in FAMILY1_TESTS])
def test_family1_boundaries_against_the_oracle(oracle, scale, variant):
    """the levels either side of a real step (count 2 * 4^L -> 2 * 4^L + 1, and 2 -> 3) differ where the global maximum allows; 2^32 + 512 wraps to level 4;
    the oracle agrees with the restatement on every triangle"""
    cases = sc.family1_cases(scale, variant)
    assert cases
    steps = [float(x) for x in sc.STEP_K + [3]]
    for case in cases:
        s, r = check(oracle, case)
        lv = s["level"]
        if case["levels"] is None:
            for k in {b[0] for b in case["boundary"]}:
                below = [lv[i] for i, b in enumerate(case["boundary"]) if b == (k, -1)]
                at = [lv[i] for i, b in enumerate(case["boundary"]) if b[0] == k and b[1] >= 0]
                if k in steps and below and at:      # (the search may serve a side on another texture shape only; test_family1_reaches_every_boundary counts them)
                    count_level = lambda c: min(int(sc.level_of_count(np.array([c], np.uint64))[0]), case["gmax"])
                    assert (set(below) != set(at)) == (count_level(int(k)) != count_level(int(k) - 1)), (case["name"], k, below, at)
                if k == 2.0 ** 32 + 512:
                    assert [lv[i] for i, b in enumerate(case["boundary"]) if b == (k, 0)] == [min(4, case["gmax"])] * sum(1 for b in case["boundary"] if b == (k, 0))


FAMILY1_COUNTS = {}


def test_family1_odd_scales_against_the_oracle(oracle):
    for case in sc.family1_odd_scale_cases():
        s, _ = check(oracle, case)
        want = 0 if np.float32(case["scale"]) > 0 else case["gmax"]       # scale^2 = 0 or inf: quotient inf or 0, count 0, level 0; not positive: the global level
        assert set(s["level"].tolist()) == {want}, case["name"]


def test_family1_and_2_notice_wrong_arithmetic(oracle):
    """>= 5 % of family 1 changes level under approx-div; >= 50 triangles of families 1 and 2 change level or degenerate flag under fused"""
    for scale in ALL_SCALES:
        n = a = f = 0
        for case in sc.family1_cases(scale, "max6"):
            lv = sc.setup(case)["level"]
            n, a, f = n + len(lv), a + int((sc.setup(case, approx_div=True)["level"] != lv).sum()), f + int((sc.setup(case, fused=True)["level"] != lv).sum())
        FAMILY1_COUNTS[scale] = (n, a, f)
        print("family 1 scale %g: %d triangles, approx-div changes %d levels, fused changes %d" % (scale, n, a, f))
    n, a, f1 = (sum(v[i] for v in FAMILY1_COUNTS.values()) for i in range(3))
    exact, flips = sc.family2_threshold_triangles()
    both = np.concatenate([exact, flips])
    f2 = int((sc.degenerate(both) != sc.degenerate(both, fused=True)).sum())
    f2e = 0
    for case in sc.family2_edge_cases():
        f2e += int((sc.setup(case, fused=True)["level"] != sc.setup(case)["level"]).sum())
    print("family 1: %d triangles, approx-div changes %d (%.1f %%), fused changes %d; family 2: fused flips `degenerate` of %d of %d threshold triangles and "
          "the level of %d edge-heuristic triangles" % (n, a, 100.0 * a / n, f1, f2, len(both), f2e))
    assert a >= 0.05 * n
    assert f1 + f2 + f2e >= 50


def test_family2_threshold_against_the_oracle(oracle):
    exact, flips = sc.family2_threshold_triangles()
    a = sc.area0(exact).astype(np.float64)
    assert (a < 1e-9).sum() == 8 and (a >= 1e-9).sum() == 6              # float32(1e-9) and below: degenerate; from its successor on: not
    mags = np.abs(flips[:, 0])
    assert ((mags > 50) & (mags <= 4000)).sum() >= 60 and (mags < 1).sum() >= 10, mags
    for case in sc.family2_threshold_cases():
        s, _ = check(oracle, case)
        if case["flags"] & sc.FLAG_DEGENERATE_INVALID:
            assert np.array_equal(s["invalid"], s["degenerate"]) and 10 < s["invalid"].sum() < len(s["invalid"]) - 10


def test_family2_edge_heuristic_against_the_oracle(oracle):
    total = dropped = 0
    for scale in sc.EDGE_SCALES:
        tris, d = sc.family2_edge_triangles(scale)
        total, dropped = total + len(tris) + d, dropped + d
        lv = sc.edge_level(tris, 64, 32, scale, 7)
        e = sc.edge_emax(tris, 64, 32).astype(np.float64)
        assert (e < 1e-6).sum() >= 2 and ((e >= 1e-6) & (e < 1.0001e-6)).sum() >= 1, scale
        assert len(set(lv.tolist())) >= 3, (scale, lv)
    print("edge heuristic: %d inputs, %d dropped for a log2f disagreement" % (total, dropped))
    assert dropped <= 0.01 * total
    assert sum(1 for s in sc.EDGE_SCALES if np.log2(s) != np.round(np.log2(s))) >= 2, sc.EDGE_SCALES
    for case in sc.family2_edge_cases():
        check(oracle, case)


@pytest.mark.parametrize("count", sc.PENDING_COUNTS)
def test_family2_pending_lists_against_the_oracle(oracle, count):
    case = sc.family2_pending_case(count)
    s, r = check(oracle, case)
    pend = s["degenerate"] & (case["levels"] == 0xF)
    assert pend.sum() == count
    if count >= 255:
        assert set(s["level"][pend].tolist()) == {0, 1, 2, 3}
    first = sc.first_occurrence(s["p"], s["level"], s["invalid"])
    copies = np.nonzero(case["levels"] != 0xF)[0][-80:] if count >= 40 else np.nonzero(case["levels"] <= 4)[0][-2 * min(count, 40):]
    merged = [t for t in copies if first[t] != t and pend[first[t]]]
    assert len(merged) >= min(count, 40) // 2 or count == 1 and len(merged) == 1, (count, len(merged))
    if count == 8192:
        check(oracle, sc.family2_pending_case(count, threads=False))


@pytest.mark.parametrize("uv_format,axis,lo", sc.family3_sweeps(), ids=["%s-%s-%d" % ("half" if f == ot.UV16_FLOAT else "unorm", "uv"[a], lo) for f, a, lo in sc.family3_sweeps()])
def test_family3_every_16_bit_pattern_against_the_oracle(oracle, uv_format, axis, lo):
    case = sc.family3_sweep_case(uv_format, axis, lo)
    s, _ = check(oracle, case)
    if uv_format == ot.UV16_FLOAT:
        pat = np.arange(lo, lo + sc.SLICE + 1) & 0xFFFF
        special = (pat & 0x7C00) == 0x7C00
        assert np.array_equal(s["invalid"], special[:-1] | special[1:])            # exactly the triangles that touch an inf / NaN pattern
    else:
        assert not s["invalid"].any()


def test_family3_strides_and_index_formats_against_the_oracle(oracle):
    cases = sc.family3_stride_cases() + sc.family3_index_cases()
    assert {c["stride"] for c in cases if c["uv_format"] != ot.UV32_FLOAT} == {0, 4, 8, 12, 16, 5, 6, 7}
    assert any(c["uv_format"] == ot.UV32_FLOAT and (c["stride"] % 4 or c["offset"] % 4) for c in cases)
    for case in cases:
        check(oracle, case)


@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_family4_small_counts_against_the_oracle(oracle, pattern):
    """first occurrences, levels and invalid triangles of every pattern at the 17 counts to 4097"""
    for n in sc.SMALL_COUNTS:
        check(oracle, sc.family4_case(pattern, n), dedup=not pattern.endswith("nodedup"))


BIG_PATTERNS = ["unique", "every1024", "nan-edges", "levels"]


@pytest.mark.parametrize("n", sc.BIG_COUNTS)
@pytest.mark.parametrize("pattern", BIG_PATTERNS)
def test_family4_many_tiles_against_the_oracle(oracle, pattern, n):
    """66 561 and 262 145 triangles: the only cases allowed to be the slowest; their oracle time is printed and bounded like every other"""
    check(oracle, sc.family4_case(pattern, n))


def test_family4_patterns_cover_their_edges():
    """numpy alone.  For every count >= 1024 every inner 1024-triangle tile edge (1024 itself has none) is crossed by a duplicate pair in the patterns
    built for it; for every count every chunk of 4096 work items of every pattern that has that many holds every level; NaN triangles sit on both sides
    of every tile edge and at both ends"""
    chunked = set()
    for n in sc.COUNTS:
        for pattern in ("equal", "every1024", "last-lane"):
            key, nan, level = sc.family4_keys(pattern, n)
            for e in range(1024, n, 1024):
                assert np.intersect1d(key[e - 1024:e], key[e:e + 1024]).size, (pattern, n, e)      # equal triangles in the tiles either side
        for pattern in sc.PATTERNS:
            key, nan, level = sc.family4_keys(pattern, n)
            live = np.nonzero(~nan)[0]
            _, idx = np.unique(key[live] * 4 + level[live], return_index=True)        # work items = first occurrences of (coordinates, level)
            items = level[live][np.sort(idx)] if not pattern.endswith("nodedup") else level[live]
            if len(items) >= 4096:
                chunked.add((pattern, n))
                for c0 in range(0, len(items), 4096):
                    if len(items) - c0 >= 4:       # (a last chunk of one to three items cannot hold four levels: 4097 unique triangles end in one)
                        assert set(items[c0:c0 + 4096].tolist()) == {0, 1, 2, 3}, (pattern, n, c0)
        key, nan, level = sc.family4_keys("nan-edges", n)
        assert nan[0] and nan[n - 1]
        for e in range(1024, n, 1024):
            assert nan[e - 1] and nan[e]
        assert n < 8 or not nan.all()
    assert {p for p, n in chunked if n == 4096} >= {"unique", "every4096", "runs31-nodedup"} and {p for p, n in chunked if n == 262145} >= set(sc.PATTERNS) - {"equal", "every1024", "every4096", "abab"}, chunked


def test_family5_workload_against_the_oracle(oracle):
    """the restated figure is the limit at which the oracle starts to refuse; wrapped boxes only in bakes that are refused (EnableAABBTesting without
    DisableLevelLineIntersection is refused right behind the workload validation, after the warning that carries the figure)"""
    mesh = sc.family5_mesh()
    s = sc.setup(mesh)
    first = sc.first_occurrence(s["p"], s["level"], s["invalid"])
    w = sc.workload(s["p"], first, s["invalid"], 64, 64)
    everything = sc.workload(s["p"], np.arange(len(first)), s["invalid"], 64, 64)      # duplicates counted again
    assert 0 < w < everything
    print("workload figure of the mesh: %d (%d with its duplicates counted again)" % (w, everything))
    sc.run(oracle, sc.with_limit(mesh, w))
    sc.run(oracle, sc.with_limit(mesh, w - 1), expect=ot.WORKLOAD_TOO_BIG)
    for case in sc.family5_wrap_cases():
        s = sc.setup(case)
        first = sc.first_occurrence(s["p"], s["level"], s["invalid"])
        w = sc.workload(s["p"], first, s["invalid"], 64, 64)
        plain = sum(int(x) for x in (sc.cvt_i32((s["p"][:, 0::2].max(1) - s["p"][:, 0::2].min(1)) * np.float32(64)) * sc.cvt_i32((s["p"][:, 1::2].max(1) - s["p"][:, 1::2].min(1)) * np.float32(64))).tolist())
        assert w != plain                                                             # the product did wrap
        r = sc.run(oracle, sc.with_limit(case, w - 1, sc.FLAG_AABB), expect=ot.WORKLOAD_TOO_BIG, validation=True)
        r = sc.run(oracle, sc.with_limit(case, w, sc.FLAG_AABB), expect=ot.INVALID_ARGUMENT, validation=True)
        if w > 1 << 27:
            assert any("consists of %d work items" % (w - (1 << 64) if w >> 63 else w) in m for m in r["messages"]), r["messages"]
