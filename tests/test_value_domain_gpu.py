"""HIP library vs oracle, full result arrays (test_gpu_parity.both), on texel values, cut-offs and UV coordinates outside the range the rest of the suite
stays in: signed-distance and HDR values, values whose bilinear sums overflow, denormals with a denormal cut-off, plateaus of the cut-off and its two
neighbours (-0.0 against +0.0), NaN / +inf / -inf texels, UNORM8 texels equal to the cut-off, +-0 and denormal UVs, and pixel coordinates beyond the int
range.  The kernels evaluate LESS than the reference in curve_excluded / cell_excluded (classify_device.h), region_curve.h and the FINITE fast paths, each
with an argument why such numbers are safe ("NaN / Inf operands compare false and take the exact path", bounds scaled by S = |ha| + |hb| + |hc| + |hd|,
cvt_trunc_x86, std_min / std_max); these tests are where those arguments meet data.  The case list is tests/value_domain_cases.py; the two CPU audits
run the exclusion predicates over the same inputs.

Pixel coordinates beyond the int range (regime b of value_domain_cases.overflow_cases: every float -> int conversion of the bake answers INT_MIN, the x86
"integer indefinite").  Read before the first run, per call site of cvt_trunc_x86 that these bakes reach, why loops are bounded and addresses stay inside
the texture.  Common to all: the case module asserts in float64 that no triangle has pixel coordinates on both sides of +-2^31 in an axis, and every
micro-triangle vertex is a convex combination of its triangle's vertices up to a few ulp, so a bound pair is (INT_MIN, INT_MIN), never (valid, INT_MIN);
tex_coord() maps INT_MIN and INT_MIN + 1 into the texture for the three modes used: Wrap -> (uint32) x & (size - 1) or % size, in [0, size);
Clamp -> clampi(x, 0, size - 1) = 0 (and 0 for INT_MIN + 1); Border -> x < 0 -> the sentinel, which load_texel_border() answers with borderAlpha
without an address.  Mirror / MirrorOnce are not run: the reference negates / abs()es INT_MIN there (undefined), DESIGN.md "documented fences".
  * classify_device.h raster_micro_triangle (minx .. maxy, :649-650): min == max == INT_MIN in both axes, `for (y = miny; y < maxy; ++y)` runs zero times.
  * raster_micro_segment (:688-702) is for degenerate items (UV area < 1e-9); the overflow triangles have grid areas of at least 1/2 ulp^2 >= 32 UV^2 and
    are not degenerate.  (Were one to reach it: x = xMin = xMax = INT_MIN, likewise y; the first step leaves the range, one visit.)
  * coarse_state (:718-727): INT_MIN == INT_MIN passes the tile test; sx = sy = tex(INT_MIN), ex = ey = tex(INT_MIN + 1): Wrap (0, 1), Clamp (0, 0), Border
    (sentinel: fails `sx >= 0`, returns -1).  The rectangle handed to sat_sum is [0, 1]^2 or [0, 0]^2, inside every texture of two texels or more; the
    checks of :725-727 stand between any other value and the table.
  * bilinear (:289): ix = iy = INT_MIN; fetch_cell addresses (INT_MIN, INT_MIN + 1) through tex_coord as above: texels 0 / 1 or the border value.
  * region_rect (:780) and rc_frame (region_curve.h) return before their conversions: maxAbs > 16384.  The single-texel pass (fine_single_texel,
    coarse_state_finite: plain (int) conversions) is reached only by items with every |uv| <= 16384, which regimes (a) and (b) are built to exceed.
  * bake_kernels.hip raster_box (:840-847): w = h = 0 in 64-bit arithmetic, cnt64 = 0, the box is "empty": xend = minx + 1, yend = miny; the owner is
    exhausted (cy >= yend) before it offers a texel, no visit enters a ring.
  * tail_kernels.hip spatial_key30 (:127-130): qx = INT_MIN, (float) qx + 0.5f = -2^31, |.| = 2^31 -> INT_MIN again -> clampi(.., 0, 8191) = 0: a sort key,
    no address.
Regime (a) stays below 2^31 - 2^16 in magnitude: every conversion is exact, boxes are a few hundred texels."""
import time
import numpy as np
import pytest
import ommtest as ot
import value_domain_cases as vd
from test_gpu_parity import both

INPUTS = vd.inputs()
UV_CASES = vd.uv_cases()


@pytest.fixture(scope="module")
def oracle_results(oracle):
    """oracle alone, every bake of the case list once: {(case name, bake name): (BakeResult, seconds)}"""
    out = {}
    for inp in INPUTS:
        for b in vd.bakes_of(inp):
            t0 = time.perf_counter()
            r = vd.oracle_bake(oracle, inp["mips"], b["uv"], b["ix"], b["level"], b["sat"], inp["cutoff"], **b["kw"])
            out[(inp["name"], b["path"])] = (r, time.perf_counter() - t0)
    tex = vd.uv_texture()
    for c in UV_CASES:
        t0 = time.perf_counter()
        r = vd.oracle_bake(oracle, [tex], c["uv"], c["ix"], c["level"], c["sat"], vd.UV_CUTOFF, levels=c["levels"], **c["kw"])
        out[("uv", c["name"])] = (r, time.perf_counter() - t0)
    return out


def test_case_list_coverage(oracle_results):
    """no GPU: what the rotation of the options reaches, that no case is vacuous, and the rules of the overflow cases"""
    families = ["sdf", "hdr", "huge", "denormal", "plateau", "nonfinite", "unorm8"]
    assert sorted({i["family"] for i in INPUTS}) == sorted(families)
    names = [i["name"] for i in INPUTS]
    assert len(set(names)) == len(names)
    n_bakes = len(INPUTS) * len(vd.PATHS) + len(UV_CASES)
    assert n_bakes <= 200, n_bakes
    # ---- the inputs are what they say ----
    by_name = {i["name"]: i for i in INPUTS}
    for i in INPUTS:
        assert all(32 <= m.shape[0] <= 128 and 32 <= m.shape[1] <= 128 for m in i["mips"][:1]) and i["mips"][0].dtype in (np.float32, np.uint8)
    assert (96, 80) in {(i["mips"][0].shape[1], i["mips"][0].shape[0]) for i in INPUTS}
    sdf = by_name["sdf-c0"]["mips"][0]
    assert sdf.min() < -40 and sdf.max() > 40 and by_name["sdf-c0"]["cutoff"] == 0.0 and by_name["sdf-c0"]["sat"] is True and by_name["sdf-neg"]["cutoff"] == -3.0
    assert by_name["hdr"]["mips"][0].max() > 9000 and by_name["hdr"]["cutoff"] == 100.0
    huge = by_name["huge"]["mips"][0]
    assert np.all(np.isfinite(huge)) and huge.max() > 2.9e38 and huge.min() < -2.9e38      # a - b of two such texels overflows
    den = by_name["denormal"]["mips"][0]
    assert 0 < den.max() < 1.2e-38 and by_name["denormal"]["cutoff"] == float(np.float32(5e-41)) and 0 < by_name["denormal"]["cutoff"] < 1.2e-38
    for name, c in (("plateau-0.5", np.float32(0.5)), ("plateau-0.0", np.float32(0.0))):
        t = by_name[name]["mips"][0].view(np.uint32)
        words = [np.array([v], np.float32).view(np.uint32)[0] for v in [c, vd.su.ulp_up(c), vd.su.ulp_down(c)] + ([np.float32(-0.0)] if c == 0 else [])]
        for a in words:
            # whole cells with four equal corners, and a horizontal or vertical edge with every other plateau value
            assert np.any((t[:-1, :-1] == a) & (t[:-1, 1:] == a) & (t[1:, :-1] == a) & (t[1:, 1:] == a))
            for b2 in words:
                assert a == b2 or any(np.any((t[:, :-1] == p) & (t[:, 1:] == q)) or np.any((t[:-1, :] == p) & (t[1:, :] == q)) for p, q in ((a, b2), (b2, a))), (name, a, b2)
        ordinary = ~np.isin(t, words)
        assert 0.1 < ordinary.mean() < 0.4
    for name, c in (("hdr-plateau", np.float32(100.0)), ("sdf-plateau", np.float32(0.0))):
        # cells with a corner at the cut-off, one ulp off it, 1e-3 and 0.03 off it whose S = |ha| + |hb| + |hc| + |hd| is thousands (HDR) / at least 50 (SDF)
        t = by_name[name]["mips"][0].astype(np.float64)
        assert by_name[name]["cutoff"] == float(c) and by_name[name]["family"] == "plateau"
        g00, g10, g01, g11 = t[:-1, :-1], t[:-1, 1:], t[1:, :-1], t[1:, 1:]
        S = np.abs(g00 - float(c)) + np.abs(g10 - g00) + np.abs(g01 - g00) + np.abs(g00 + g11 - g01 - g10)
        near = np.minimum(np.minimum(np.abs(g00 - float(c)), np.abs(g10 - float(c))), np.minimum(np.abs(g01 - float(c)), np.abs(g11 - float(c))))
        big = S > (1000.0 if name == "hdr-plateau" else 50.0)          # (texels to +-1e4 around 100, to +-100 around 0)
        for lo, hi in ((0.0, 0.0), (1e-45, float(np.spacing(c)) if c else 2e-45), (5e-4, 2e-3), (0.02, 0.04)):
            assert np.sum(big & (near >= lo) & (near <= hi)) >= 20, (name, lo, hi)
    for vname, test in (("nan", np.isnan), ("pinf", lambda a: a == np.inf), ("ninf", lambda a: a == -np.inf)):
        for arr in ("single", "row", "col", "block"):
            t = by_name["%s-%s" % (vname, arr)]["mips"][0]
            m = test(t)
            assert m.any() and not m.all() and np.isfinite(t[~m]).all()
            if arr == "row":
                assert m[0].all() and not m[1:].any()
            if arr == "col":
                assert m[:, -1].all() and not m[:, :-1].any()
            if arr == "block":
                assert m[0:2, 0:2].all() and m.sum() == 20
            if arr == "single":
                assert 0.01 < m.mean() < 0.06
    bits = set(by_name["nan-bits"]["mips"][0].view(np.uint32).ravel().tolist())
    assert {vd.QNAN, vd.SNAN, vd.NEG_NAN} <= bits
    assert np.isnan(by_name["all-nan"]["mips"][0]).all() and [i["name"] for i in INPUTS if i["special_only"]] == ["all-nan"]
    mip = by_name["mip1-nonfinite"]["mips"]
    assert len(mip) == 2 and np.isfinite(mip[0]).all() and np.isnan(mip[1]).any() and (mip[1] == np.inf).any() and (mip[1] == -np.inf).any()
    u8 = [i for i in INPUTS if i["family"] == "unorm8"]
    assert [i["cutoff"] for i in u8] == [0.0, 1.0] + [float(np.float32(k) * np.float32(1 / 255)) for k in (1, 127, 128, 254)] + [1.5]
    for i, k in zip(u8[2:6], (1, 127, 128, 254)):
        t = i["mips"][0]
        assert t.dtype == np.uint8 and set(np.unique(t).tolist()) == {k - 1, k, k + 1}
        assert np.float32(k) * np.float32(1.0 / 255.0) == np.float32(i["cutoff"])          # texel == cut-off exactly, as Load() computes it
        w = t.shape[1]
        left, right = t[:, :w // 2 - 2], t[:, w // 2:]
        assert np.mean(left[:, 1:] == left[:, :-1]) > 0.7 and np.mean(right[:, 1:] == right[:, :-1]) < 0.45     # plateaus / 1-texel noise
    # ---- what the rotation reaches: every option value with every family and every path; every border value; SAT on and off per UNORM8 cut-off ----
    seen = set()
    border_kinds = set()
    for i in INPUTS:
        bakes = vd.bakes_of(i)
        assert [b["path"] for b in bakes] == vd.PATHS and [b["level"] for b in bakes] == [7, 5, 5, 0, 3]
        assert [b["knobs"] for b in bakes] == [(), ((ot.KNOB_GENERIC_PASS, 1),), ((ot.KNOB_GENERIC_PASS, 2),), (), ()]
        for b in bakes:
            assert 40 <= b["ix"].size // 3 <= 120
            kw = b["kw"]
            for key in (i["family"], b["path"]):
                seen |= {(key, "filter", kw["filt"]), (key, "format", kw["fmt"]), (key, "promo", kw["promo"]), (key, "addr", kw["addr"])}
            if i["sat"] is None:
                seen.add((i["family"], "sat", b["sat"]))
            if kw["addr"] == ot.BORDER:
                border_kinds.add(b["border_kind"])
                c = np.float32(i["cutoff"])
                assert np.float32(kw["border_alpha"]) in (c, vd.su.ulp_up(c), vd.su.ulp_down(c), np.float32(-2.0), np.float32(7.0))
        if i["family"] == "unorm8":
            assert {b["sat"] for b in bakes} == {True, False}, i["name"]
        # triangles reach over the texture's edge: a seam in every stream
        for b in bakes:
            t = b["uv"].reshape(-1, 3, 2)
            crosses = (t.min(axis=(1, 2)) < 0) | (t.max(axis=(1, 2)) > 1)
            assert crosses.mean() > 0.1, (i["name"], b["path"], crosses.mean())
    for key in families + vd.PATHS:
        for opt, values in (("filter", vd.FILTERS), ("format", vd.FORMATS), ("promo", vd.PROMOS), ("addr", vd.ADDRS)):
            for v in values:
                assert (key, opt, v) in seen, (key, opt, v)
    for fam in ("hdr", "huge", "denormal", "plateau", "nonfinite", "unorm8"):
        assert (fam, "sat", True) in seen and (fam, "sat", False) in seen, fam
    assert border_kinds == set(vd.BORDER_KINDS)
    # the micro-triangle sizes that choose the path: below a texel at level 7, 1 .. 4 texels across at level 5, most of the texture at levels 0 and 3
    for i in INPUTS:
        h, w = i["mips"][0].shape
        for b in vd.bakes_of(i):
            t = b["uv"].reshape(-1, 3, 2)
            ext = (t.max(axis=1) - t.min(axis=1)).max(axis=1) * max(w, h) / 2.0 ** b["level"]        # largest box side of a micro-triangle, texels
            if b["path"] == "fast7":
                assert ext.max() < 0.5
            elif b["path"].startswith("gen5"):
                assert np.median(ext) > 1.0 and ext.max() <= 4.0      # (more than half of them over a texel across: the generic pass)
            else:
                assert np.median(ext) * 2.0 ** b["level"] > 0.3 * max(w, h)
    # ---- UV cases ----
    groups = {c["group"] for c in UV_CASES}
    assert groups == {"zero", "tiny", "overflow-a", "overflow-b"}
    zero = [c for c in UV_CASES if c["group"] == "zero"]
    assert {(c["levels"] is None, bool(c["kw"]["flags"] & ot.FLAG_NO_DEDUP)) for c in zero} == {(a, b) for a in (True, False) for b in (True, False)}
    zu = zero[0]["uv"].reshape(-1, 2, 6)
    assert np.array_equal(zu[:, 0], zu[:, 1]) and all(not np.array_equal(np.signbit(p[0]), np.signbit(p[1])) for p in zu)     # equal as floats, different bits
    assert any(np.all(p[0].reshape(3, 2)[:, 0] == 0) or np.all(p[0].reshape(3, 2)[:, 1] == 0) for p in zu)                  # all three vertices on an axis
    lv = zero[2]["levels"].reshape(-1, 2)
    assert np.all(lv[:, 0] != lv[:, 1])
    tiny = [c for c in UV_CASES if c["group"] == "tiny"][0]["uv"].reshape(-1, 3, 2)
    a = np.abs(tiny)
    assert np.any((a > 0) & (a < 1.2e-38)) and np.any(a == np.float32(1e-30)) and np.sum(np.all(a <= 1e-30, axis=(1, 2))) == 10
    for regime in ("a", "b"):
        cs = [c for c in UV_CASES if c["group"] == "overflow-" + regime]
        assert {c["kw"]["addr"] for c in cs} == set(vd.ADDRS) and {c["level"] for c in cs} == {3, 4}
        assert {c["kw"]["filt"] for c in cs} == set(vd.FILTERS) and {c["sat"] for c in cs} == {True, False}
        for c in cs:
            vd.check_overflow_rules(c["uv"], regime, float(vd.OVERFLOW_SIZE))      # the straddle rule, in float64 (also asserted when the list is built)
            p = c["uv"].astype(np.float64) * vd.OVERFLOW_SIZE
            assert np.any(p > 0) or np.any(p < 0)
            t = c["uv"].astype(np.float64).reshape(-1, 3, 2)
            area2 = np.abs((t[:, 1, 0] - t[:, 0, 0]) * (t[:, 2, 1] - t[:, 0, 1]) - (t[:, 2, 0] - t[:, 0, 0]) * (t[:, 1, 1] - t[:, 0, 1]))
            assert area2.min() > 1e-3                                               # no degenerate item (UV area < 1e-9) among them
        signs = {(bool(np.all(c["uv"][:, 0] > 0)), bool(np.all(c["uv"][:, 1] > 0))) for c in cs}
        assert len(signs) >= 3                                                      # both signs, in both axes
    with pytest.raises(AssertionError):
        vd.check_overflow_rules(np.array([[2.0 ** 25 - 2, 0], [2.0 ** 25, 0], [2.0 ** 25 - 2, 4]], np.float32), "b", 64.0)     # the rule does catch a straddle
    # ---- the oracle's side: nothing vacuous, every state, the time caps ----
    states = {}
    for i in INPUTS:
        for b in vd.bakes_of(i):
            r, dt = oracle_results[(i["name"], b["path"])]
            assert dt < 1.0, (i["name"], b["path"], dt)
            assert r.index.size == b["ix"].size // 3
            if i["special_only"]:
                # the stated exception: no texel of an all-NaN texture is above the cut-off.  Within the texture every triangle is fully transparent (a special
                # index; at level 0, which runs with DisableSpecialIndices, one transparent block); only Border's borderAlpha can add anything else
                if b["kw"]["addr"] != ot.BORDER:
                    assert np.all(r.index == ot.SPECIAL_FT) or b["level"] == 0, (i["name"], b["path"])
                    assert vd.block_states(r) <= {(1, 0), (2, 0)}
                continue
            assert np.mean(r.index >= 0) >= 0.2, (i["name"], b["path"], float(np.mean(r.index >= 0)))
            states.setdefault(i["family"], set()).update(vd.block_states(r))
    for c in UV_CASES:
        r, dt = oracle_results[("uv", c["name"])]
        assert dt < 2.0, (c["name"], dt)
        assert np.mean(r.index >= 0) >= 0.2, (c["name"], float(np.mean(r.index >= 0)))
        states.setdefault(c["group"].split("-")[0], set()).update(vd.block_states(r))
    every = {(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3)}
    for fam in families + ["zero", "tiny", "overflow"]:
        assert states[fam] == every, (fam, sorted(every - states[fam]))
    # +-0 pairs are ONE work item, owned by the first: both triangles of a pair carry the same index when they have the same level
    r, _ = oracle_results[("uv", "zero-same-level")]
    ix = r.index.reshape(-1, 2)
    assert np.all(ix[:, 0] == ix[:, 1])


@pytest.mark.gpu
@pytest.mark.parametrize("inp", INPUTS, ids=[i["name"] for i in INPUTS])
def test_texel_values_and_cutoffs(product, oracle, inp):
    """one input along its five paths; filter, format, promotion, address mode, borderAlpha and SAT on / off rotating with the bake"""
    vd.run_input(both, product, oracle, inp)


@pytest.mark.gpu
@pytest.mark.parametrize("case", UV_CASES, ids=[c["name"] for c in UV_CASES])
def test_uv_values(product, oracle, case):
    """+-0 pairs (one work item, owned by the first), denormal and tiny coordinates, pixel coordinates beyond 16384 UV and beyond the int range"""
    vd.run_uv_case(both, product, oracle, case)
