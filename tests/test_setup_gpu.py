"""SetupWorkItems on the device (omm_amd/csrc/setup_kernels.hip, hash_build.h, scan_lookback.h and the host half in omm_host.cpp) at its rounding, format
and tile boundaries: HIP library vs oracle on full result arrays, bit for bit, plus direct assertions on the library's result against the numpy
restatement of tests/setup_cases.py -- the descriptor level of every valid triangle, the unresolved index of every invalid one, merged triangles
sharing their first occurrence's descriptor, and the per-triangle areas of ommxGetDeviceBakeResultTriangleAreas.  tests/test_setup_reference.py holds the
restatement to the oracle on the same cases without a GPU and proves what the families cover.  No tolerances anywhere."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import setup_cases as sc
from test_gpu_parity import both

pytestmark = pytest.mark.gpu
ALL_SCALES = sc.POW2_SCALES + sc.ROUNDED_SCALES


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


def pair(product, oracle, case, first=True, dedup=True):
    """both libraries bake the case; full arrays equal (as test_gpu_parity.both compares them, for descs with a stride and a base offset); then the
    library's own result against the restatement.  Returns (product result, setup)"""
    r = [sc.run(lib, case)["result"] for lib in (product, oracle)]
    assert r[0].same_as(r[1]), (case["name"], r[0].diff(r[1]))
    s = sc.setup(case)
    f = sc.first_occurrence(s["p"], s["level"], s["invalid"], dedup) if first else None
    sc.check_result_against_restatement(case, r[0], s, f)
    return r[0], s


def device_areas(product, hip, case):
    """ommxBakeDevice of the case, the areas it hands out"""
    su.bind(product.dll)
    b = product.create_baker()
    t = product.create_texture(b, [sc.texture(case["w"], case["h"], case["fp32"])], alpha_cutoff=0.5)
    d = sc.desc_of(case, t)
    bake = lu.DeviceBake(product, hip, b, d, case["buf"], case["ix"], case["levels"], uv_offset=case["offset"])
    try:
        T = len(case["ix"]) // 3
        p_areas = C.c_void_p()
        assert product.dll.ommxGetDeviceBakeResultTriangleAreas(bake.out, C.byref(p_areas)) == ot.SUCCESS and p_areas.value
        return hip.download(p_areas, 4 * T, np.float32).copy(), bake.host
    finally:
        bake.close()
        product.destroy_texture(b, t)
        product.destroy_baker(b)


def check_areas(product, hip, case, s, host_result):
    areas, dev = device_areas(product, hip, case)
    assert np.array_equal(areas.view(np.uint32), s["area"].view(np.uint32)), (case["name"], np.nonzero(areas.view(np.uint32) != s["area"].view(np.uint32))[0][:8])
    assert np.all(areas[s["invalid"]] == 0)
    assert dev.same_as(host_result), (case["name"], dev.diff(host_result))


# ---- family 1: level boundaries of the area heuristic (and family 6: their areas) ----
FAMILY1_TESTS = [(s, v) for s in ALL_SCALES for v in sc.FAMILY1_VARIANTS]


@pytest.mark.parametrize("scale,variant", FAMILY1_TESTS, ids=["%g-%s" % sv for sv in FAMILY1_TESTS])
def test_area_heuristic_level_boundaries(product, oracle, hip, scale, variant):
    """quotients at k and the floats either side for every count k a few-texel triangle reaches at this scale, square and non-square textures; the
    variants: a global maximum that does not clamp, one that does, per-triangle overrides"""
    cases = sc.family1_cases(scale, variant)
    assert cases
    for case in cases:
        r, s = pair(product, oracle, case)
        if variant != "max2":
            check_areas(product, hip, case, s, r)


def test_area_heuristic_scales_without_a_square(product, oracle, hip):
    """scale^2 underflows to 0 or overflows to inf (level 0), or the scale is NaN, negative, -0.0 (the global level)"""
    for case in sc.family1_odd_scale_cases():
        r, s = pair(product, oracle, case)
        check_areas(product, hip, case, s, r)


# ---- family 2: the degenerate threshold and the host's edge heuristic ----
def test_degenerate_threshold(product, oracle, hip):
    """area0 below, at and above float32(1e-9) and triangles a fused multiply-add would put on the other side (offsets to 4000 UV units): dynamic
    subdivision off, on, and either with degenerate triangles invalid"""
    for case in sc.family2_threshold_cases():
        r, s = pair(product, oracle, case)
        check_areas(product, hip, case, s, r)


def test_edge_heuristic_boundaries(product, oracle, hip):
    """eMax either side of 1e-6 and of every ceilf step of levels 0 - 7, degenerate triangles and bit 11, scales that are powers of two and not"""
    cases = sc.family2_edge_cases()
    assert len(cases) >= 8
    for case in cases:
        r, s = pair(product, oracle, case)
        check_areas(product, hip, case, s, r)


@pytest.mark.parametrize("count,threads", [(c, True) for c in sc.PENDING_COUNTS] + [(8192, False)], ids=lambda v: str(v))
def test_pending_triangles_on_the_host(product, oracle, count, threads):
    """`count` degenerate triangles under dynamic subdivision take the host's path (gather, log2f, scatter, rehash; four helper threads from 8192 on with
    EnableInternalThreads): levels vary with the position in the list, pending triangles repeat each other, and non-pending triangles with the same
    coordinates merge with them exactly when the rehash saw the host's level"""
    case = sc.family2_pending_case(count, threads)
    r, s = pair(product, oracle, case)
    assert (s["degenerate"] & (case["levels"] == 0xF)).sum() == count


# ---- family 3: every 16-bit coordinate, strides, index formats ----
@pytest.mark.parametrize("uv_format,axis,lo", sc.family3_sweeps(), ids=["%s-%s-%d" % ("half" if f == ot.UV16_FLOAT else "unorm", "uv"[a], lo) for f, a, lo in sc.family3_sweeps()])
def test_every_16_bit_coordinate(product, oracle, hip, uv_format, axis, lo):
    case = sc.family3_sweep_case(uv_format, axis, lo)
    r, s = pair(product, oracle, case)
    if lo in (0, 0x6000 // sc.SLICE * sc.SLICE, 0xE000 // sc.SLICE * sc.SLICE):       # (the slices with +-0 and denormals, and with inf / NaN)
        check_areas(product, hip, case, s, r)


def test_strides_base_offsets_and_index_formats(product, oracle, hip):
    for case in sc.family3_stride_cases() + sc.family3_index_cases():
        r, s = pair(product, oracle, case)
        check_areas(product, hip, case, s, r)


# ---- family 4: dedup, numbering and the level split at their tile edges ----
@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_dedup_numbering_and_split_at_small_counts(product, oracle, pattern):
    for n in sc.SMALL_COUNTS:
        case = sc.family4_case(pattern, n)
        pair(product, oracle, case, dedup=not pattern.endswith("nodedup"))


@pytest.mark.parametrize("n", sc.BIG_COUNTS)
@pytest.mark.parametrize("pattern", ["unique", "every1024", "every4096", "last-lane", "runs31", "abcabc", "nan-edges", "levels"])
def test_dedup_numbering_and_split_at_many_tiles(product, oracle, pattern, n):
    """66 561 triangles = 66 look-back tiles and 17 chunks; 262 145 = 257 tiles and 65 chunks, the second round of setup_split_scan"""
    pair(product, oracle, sc.family4_case(pattern, n))


def test_hot_keys(product, oracle):
    """tests/scripts/hot_keys.py at 20 000 triangles: one hot key in the UV-dedup table (one block), one hot key in the digest table (a few dozen)"""
    tex, cases = sc.hot_key_cases()
    for name, uv, expect in cases:
        ix = np.arange(len(uv), dtype=np.uint32)
        r = both(product, oracle, [tex], uv, ix, 6, addr=ot.WRAP, promo=ot.PROMO_FORCE_OPAQUE)
        assert expect(len(r.descs)), (name, len(r.descs))
        assert len(r.index) == len(uv) // 3


# ---- family 5: the workload figure ----
def test_workload_figure(product, oracle):
    """maxWorkloadSize at the restated figure: both bake; one below: both refuse.  Boxes whose 32-bit product wraps only in bakes both refuse: one below
    the wrapped total WORKLOAD_TOO_BIG, at it the refusal that follows the validation, behind the warning that carries the figure"""
    mesh = sc.family5_mesh()
    s = sc.setup(mesh)
    w = sc.workload(s["p"], sc.first_occurrence(s["p"], s["level"], s["invalid"]), s["invalid"], 64, 64)
    pair(product, oracle, sc.with_limit(mesh, w))
    out = [sc.run(lib, sc.with_limit(mesh, w - 1), expect=ot.WORKLOAD_TOO_BIG, validation=True) for lib in (product, oracle)]
    assert out[0]["messages"] == out[1]["messages"]
    for case in sc.family5_wrap_cases():
        s = sc.setup(case)
        w = sc.workload(s["p"], sc.first_occurrence(s["p"], s["level"], s["invalid"]), s["invalid"], 64, 64)
        for limit, expect in ((w - 1, ot.WORKLOAD_TOO_BIG), (w, ot.INVALID_ARGUMENT)):
            out = [sc.run(lib, sc.with_limit(case, limit, sc.FLAG_AABB), expect=expect, validation=True) for lib in (product, oracle)]
            assert out[0]["messages"] == out[1]["messages"], (case["name"], limit, out[0]["messages"], out[1]["messages"])
            if expect == ot.INVALID_ARGUMENT:
                assert len(out[0]["messages"]) == (2 if w > 1 << 27 else 1), out[0]["messages"]
