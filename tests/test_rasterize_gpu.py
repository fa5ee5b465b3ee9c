"""ommxRasterizeMicromap on the GPU.  Every case compares every output and the info with tests/rasterize_util.py's model byte for byte -- there is no
tolerance anywhere.  The shapes are the edges of the two passes (pixel centres on edges and vertices, triangles at and beyond the image's sides, boxes at
the thresholds between the three coverage kernels, images around a wave's and a block's worth of pixels, every kind of index entry), not a workload.  The
last tests hold a real bake to what the entry is for: a fresh 4-state bake contradicts its texture nowhere."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import coarsen_util as cu
import rasterize_util as ru

pytestmark = pytest.mark.gpu
UNIT = (0.0, 0.0, 1.0, 1.0)
LANE_BOX, WAVE_BOX = 64, 4096   # kRasterLaneBox, kRasterWaveBox of omm_amd/csrc/raster_kernels.hip
GRID_BLOCKS, GRID_TURNS, GRID_SHARE = 2048, 64, 4096   # kRasterGridBlocks, kRasterGridTurns, kRasterGridShare


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    cu.bind(lu.bind(product.dll))
    return ru.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def checker_texture(n=8, seed=1):
    return (np.random.default_rng(seed).integers(0, 2, (n, n)) * 255).astype(np.uint8)


def mixed_result(rng, prims, index_format=ot.IDX_U16, levels=(0, 1, 2, 3, 4)):
    """blocks of the given levels in both formats at odd addresses, random bytes between them and in the unused bits of one-byte blocks; an index of
    `prims` entries over them and the special indices"""
    blocks = [(rng.integers(0, 1 << bits, 4 ** level), level, bits) for level in levels for bits in (1, 2)]
    array, descs = cu.table_of_blocks(blocks, first_offset=1, gap=2)
    for o, l, f in descs.tolist():
        if 4 ** l * f < 8:
            array[o] |= (int(rng.integers(0, 256)) << (4 ** l * f)) & 0xFF
    return lu.Result(array, [tuple(d) for d in descs.tolist()], rng.integers(-4, len(descs), prims), index_format)


def tiles(n, cols, lo=0.0, size=1.0):
    """n triangles, one per cell of a grid of `cols` columns over [lo, lo + size]^2, well inside their cells -> (uv (3n, 2), ix)"""
    rows = (n + cols - 1) // cols
    i = np.arange(n)
    cx, cy = (i % cols) / cols, (i // cols) / rows
    shape = np.array([[0.1, 0.1], [0.9, 0.15], [0.2, 0.9]])
    uv = lo + size * (np.stack([cx, cy], 1)[:, None, :] + shape[None] / np.array([cols, rows]))
    return uv.reshape(-1, 2), np.arange(3 * n, dtype=np.uint32)


class Session:
    """scenes of one test, closed together"""

    def __init__(self, product, hip, baker):
        self.product, self.hip, self.baker, self.open = product, hip, baker, []

    def scene(self, *args, **kw):
        dev = ru.DeviceScene(self.product, self.hip, self.baker, ru.Scene(*args, **kw))
        self.open.append(dev)
        return dev

    def close(self):
        for d in self.open:
            d.close()


@pytest.fixture()
def make(product, hip, baker, dll):
    s = Session(product, hip, baker)
    yield s
    s.close()


# ---- tiny images, exact hits, winding ----
def test_one_pixel(dll, hip, make):
    """a 1 x 1 image with one triangle that holds / does not hold the centre"""
    res = lu.Result(lu.pack([2], 2), [(0, 0, 2)], [0], ot.IDX_U8)
    for uv, holds in (([[0.1, 0.1], [0.9, 0.2], [0.4, 0.9]], True), ([[0.0, 0.0], [0.45, 0.0], [0.0, 0.45]], False), ([[0.5, 0.5], [1, 0.5], [0.5, 1]], True)):
        dev = make.scene(checker_texture(), np.array(uv), np.arange(3, dtype=np.uint32), ru.HostResult.of(res))
        ref = ru.check(dll, hip, dev, UNIT, 1, 1)
        assert ref["info"]["coveredPixels"] == int(holds) and ref["info"]["drawnPrimitives"] == int(holds)
        assert ref["states"][0, 0] == (2 if holds else ru.STATE_NONE)


def test_centres_on_a_shared_edge_and_on_the_vertex_of_a_fan(dll, hip, make):
    """8 x 8 pixels over [0, 1]^2: centres at odd sixteenths.  Two triangles share the diagonal through eight centres; six triangles share the vertex
    (9/16, 9/16), a centre.  All coordinates are dyadic: the lowest index owns every such pixel, and no pixel of the square is left out"""
    s = 1 / 16
    quad = [[s, s], [15 * s, s], [15 * s, 15 * s], [s, s], [15 * s, 15 * s], [s, 15 * s]]
    res = mixed_result(np.random.default_rng(2), 8)
    dev = make.scene(checker_texture(), np.array(quad), np.arange(6, dtype=np.uint32), ru.HostResult.of(res))
    ref = ru.check(dll, hip, dev, UNIT, 8, 8)
    ids = ref["primitiveIds"]
    assert (ids.diagonal() == 0).all() and (ids != ru.NONE).all() and set(ids.reshape(-1).tolist()) == {0, 1}
    for first, owner in ((1, 1), (0, 0)):   # without primitive 0 the diagonal is primitive 1's
        assert (ru.check(dll, hip, dev, UNIT, 8, 8, first=first)["primitiveIds"].diagonal() == owner).all()
    c, ring = np.array([9 * s, 9 * s]), np.array([[1, 0], [0.5, 1], [-0.5, 1], [-1, 0], [-0.5, -1], [0.5, -1]]) * 0.25
    fan = np.concatenate([[c, c + ring[k], c + ring[(k + 1) % 6]] for k in range(6)])
    for order in (np.arange(6), np.array([3, 5, 1, 0, 4, 2])):
        uv = fan.reshape(6, 3, 2)[order].reshape(-1, 2)
        dev = make.scene(checker_texture(), uv, np.arange(18, dtype=np.uint32), ru.HostResult.of(res))
        ref = ru.check(dll, hip, dev, UNIT, 8, 8)
        assert ref["primitiveIds"][4, 4] == 0 and ref["info"]["drawnPrimitives"] >= 3


def test_winding_and_degenerate_triangles(dll, hip, make):
    """the same triangles clockwise and counter-clockwise own the same pixels; collinear, repeated-vertex, NaN and Inf triangles draw nothing and are
    counted"""
    rng = np.random.default_rng(3)
    uv, ix = tiles(6, 3)
    res = lu.Result(lu.pack([2, 2, 2, 2], 2), [(0, 1, 2)], [-1, -2, -3, -4, 0, 0], ot.IDX_U8)   # states that do not depend on the barycentrics' order
    flipped = uv.reshape(6, 3, 2)[:, [0, 2, 1]].reshape(-1, 2)
    a = ru.check(dll, hip, make.scene(checker_texture(), uv, ix, ru.HostResult.of(res)), UNIT, 63, 33)
    b = ru.check(dll, hip, make.scene(checker_texture(), flipped, ix, ru.HostResult.of(res)), UNIT, 63, 33)
    assert np.array_equal(a["primitiveIds"], b["primitiveIds"]) and np.array_equal(a["states"], b["states"]) and a["info"]["drawnPrimitives"] == 6
    bad = uv.astype(np.float32).reshape(6, 3, 2).copy()
    bad[0] = [[0.25, 0.25], [0.5, 0.5], [0.75, 0.75]]   # collinear
    bad[1, 1] = bad[1, 0]                          # a repeated vertex
    bad[2, 0, 0] = np.nan
    bad[3, 2, 1] = np.inf
    bad[4, 1] = [-np.inf, np.inf]
    dev = make.scene(checker_texture(), bad.reshape(-1, 2), ix, ru.HostResult.of(mixed_result(rng, 6)))
    ref = ru.check(dll, hip, dev, UNIT, 63, 33)
    assert ref["info"]["degeneratePrimitives"] == 5 and ref["info"]["drawnPrimitives"] == 1 and set(np.unique(ref["primitiveIds"]).tolist()) == {5, ru.NONE}


# ---- the image's sides ----
def test_triangles_outside_and_across_every_side_and_corner(dll, hip, make):
    """a triangle beyond each of the four sides (nothing drawn), and one across each side and each corner, in a 65 x 33 image of the view [0.25, 0.75]^2"""
    view = (0.25, 0.25, 0.75, 0.75)
    shape = np.array([[-0.06, -0.05], [0.07, -0.03], [0.0, 0.08]])
    outside = [(0.1, 0.5), (0.9, 0.5), (0.5, 0.1), (0.5, 0.9)]
    across = [(0.25, 0.5), (0.75, 0.5), (0.5, 0.25), (0.5, 0.75), (0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)]
    uv = np.concatenate([np.array(c) + shape for c in outside + across])
    res = mixed_result(np.random.default_rng(4), 12)
    dev = make.scene(checker_texture(), uv, np.arange(36, dtype=np.uint32), ru.HostResult.of(res))
    ref = ru.check(dll, hip, dev, view, 65, 33)
    assert set(np.unique(ref["primitiveIds"]).tolist()) == set(range(4, 12)) | {ru.NONE} and ref["info"]["drawnPrimitives"] == 8
    ids = ref["primitiveIds"]
    assert ids[0, 0] == 8 and ids[0, -1] == 9 and ids[-1, 0] == 10 and ids[-1, -1] == 11


@pytest.mark.parametrize("addr", [ot.WRAP, ot.CLAMP, ot.BORDER, ot.MIRROR], ids=["wrap", "clamp", "border", "mirror"])
def test_viewport_beyond_the_texture(dll, hip, make, addr):
    """[-0.5, 1.5]^2 under each addressing mode, Nearest and Linear: the alpha test, the contour and the grey follow the sampler beyond [0, 1]"""
    rng = np.random.default_rng(5)
    uv, ix = tiles(9, 3, lo=-0.5, size=2.0)
    seen = set()
    for filt, tex in ((ot.NEAREST, checker_texture(8, 6)), (ot.LINEAR, rng.integers(0, 256, (6, 5)).astype(np.uint8))):
        dev = make.scene(tex, uv, ix, ru.HostResult.of(mixed_result(rng, 9)), addr=addr, filt=filt, border=0.75)
        ref = ru.check(dll, hip, dev, (-0.5, -0.5, 1.5, 1.5), 64, 48)
        seen.add(ref["alphaTest"].tobytes())
        assert 0 < ref["info"]["alphaAbovePixels"] < 64 * 48 and (ref["rgba"][..., :3] == (255, 0, 0)).all(axis=2).any()
    assert len(seen) == 2


def test_viewport_inside_one_micro_triangle_of_level_12(dll, hip, make):
    """a view 2^-20 wide inside one micro-triangle of a level-12 block: every pixel reads the same micro-triangle, by fp64 sample points that fp32 could
    not tell apart"""
    rng = np.random.default_rng(6)
    block = rng.integers(0, 256, 4 ** 12 // 4, dtype=np.uint8)
    res = lu.Result(block, [(0, 12, 2)], [0], ot.IDX_U32)
    uv = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    dev = make.scene(checker_texture(), uv, np.arange(3, dtype=np.uint32), ru.HostResult.of(res))
    lo = (1228 + 0.25) / 4096
    ref = ru.check(dll, hip, dev, (lo, lo, lo + 2.0 ** -20, lo + 2.0 ** -20), 33, 17)
    micro = np.unique(ref["microTriangles"])
    assert len(micro) == 1 and micro[0] < 4 ** 12 and ref["info"]["coveredPixels"] == 33 * 17
    wide = ru.check(dll, hip, dev, (lo, lo, lo + 2.0 ** -9, lo + 2.0 ** -9), 33, 17)
    assert len(np.unique(wide["microTriangles"])) > 40


# ---- image sizes ----
@pytest.mark.parametrize("width", [1, 63, 64, 65, 257])
def test_image_sizes(dll, hip, make, width):
    """widths 1, 63, 64, 65 and 257 x heights 1, 2 and 65: rows that end inside a wave, at its end and behind it; pixel counts below a wave and beyond
    several blocks"""
    rng = np.random.default_rng(7)
    uv, ix = tiles(40, 8, lo=-0.1, size=1.2)
    dev = make.scene(checker_texture(16, 8), uv, ix, ru.HostResult.of(mixed_result(rng, 40)), addr=ot.WRAP)
    for height in (1, 2, 65):
        ref = ru.check(dll, hip, dev, UNIT, width, height)
        assert ref["primitiveIds"].shape == (height, width)


# ---- the three coverage kernels ----
def box_pixels(tri, view, width, height):
    """raster_box of omm_amd/csrc/raster_cover.h restated: the number of pixels of a triangle's clipped box"""
    n = 1
    for axis, size in ((0, width), (1, height)):
        step = (np.float64(np.float32(view[2 + axis])) - np.float64(np.float32(view[axis]))) / size
        c = np.asarray(tri, np.float32).astype(np.float64)[:, axis]
        first = min(max(np.floor((c.min() - np.float64(np.float32(view[axis]))) / step) - 1, 0), size)
        end = min(max(np.ceil((c.max() - np.float64(np.float32(view[axis]))) / step) + 1, 0), size)
        n *= max(int(end - first), 0)
    return n


def test_box_sizes_around_the_thresholds(dll, hip, make):
    """one triangle per call whose box has exactly kRasterLaneBox and kRasterWaveBox pixels, one pixel more and some more, and one whose box is the
    whole 257 x 65 image: a lane, a wave and the grid walk the same rule"""
    res = lu.Result(lu.pack(np.arange(16) % 4, 2), [(0, 2, 2)], [0], ot.IDX_U8)
    sizes = []
    # boxes of 8 x 8, 5 x 13, 8 x 9, 64 x 64, 241 x 17, 65 x 65 and 238 x 65 pixels: at, one above and further above either threshold
    for left, legs in ((20.3, (5.2, 5.2)), (20.3, (2.2, 10.2)), (20.3, (5.2, 6.2)), (20.3, (61, 61)), (2.3, (238.2, 14.2)), (20.3, (62, 62)), (20.3, (300, 300))):
        tri = np.array([[left, 1.4], [left + legs[0], 1.4], [left, 1.4 + legs[1]]]) / np.array([257.0, 65.0])
        sizes.append(box_pixels(tri, UNIT, 257, 65))
        dev = make.scene(checker_texture(), tri, np.arange(3, dtype=np.uint32), ru.HostResult.of(res))
        assert ru.check(dll, hip, dev, UNIT, 257, 65)["info"]["coveredPixels"] > 5
    assert sizes == [LANE_BOX, LANE_BOX + 1, LANE_BOX + 8, WAVE_BOX, WAVE_BOX + 1, 65 * 65, 257 * 65 - 19 * 65], sizes
    whole = np.array([[-3.0, -3.0], [5.0, -3.0], [-3.0, 5.0]])
    dev = make.scene(checker_texture(), whole, np.arange(3, dtype=np.uint32), ru.HostResult.of(res))
    assert box_pixels(whole, UNIT, 257, 65) == 257 * 65 and ru.check(dll, hip, dev, UNIT, 257, 65)["info"]["coveredPixels"] == 257 * 65
    # three large boxes in one call: the left half, everything, the lower half
    three = np.concatenate([[[-3.0, -3.0], [0.5, -3.0], [0.5, 9.0]], whole, [[-3.0, 0.5], [9.0, 0.5], [0.5, -9.0]]])
    dev = make.scene(checker_texture(), three, np.arange(9, dtype=np.uint32), ru.HostResult.of(lu.Result(lu.pack(np.arange(16) % 4, 2), [(0, 2, 2)], [0, -2, 0], ot.IDX_U8)))
    ids = ru.check(dll, hip, dev, UNIT, 257, 65)["primitiveIds"]
    assert set(np.unique(ids).tolist()) == {0, 1} and 0.3 < (ids == 0).mean() < 0.6
    assert set(np.unique(ru.check(dll, hip, dev, UNIT, 257, 65, first=1)["primitiveIds"]).tolist()) == {1}


def test_so_many_large_boxes_that_the_shares_grow(dll, hip, make):
    """120 000 large boxes -- three triangles, 40 000 times over -- hold more pixels than kRasterGridBlocks x kRasterGridTurns shares of
    kRasterGridShare, so the grid kernel walks larger shares; every copy lies under its original, so the call must answer what the first three
    primitives alone answer (those against the model)"""
    whole = np.array([[-3.0, -3.0], [5.0, -3.0], [-3.0, 5.0]])
    three = np.concatenate([[[-3.0, -3.0], [0.5, -3.0], [0.5, 9.0]], whole, [[-3.0, 0.5], [9.0, 0.5], [0.5, -9.0]]])
    copies = 40000
    assert copies * sum(box_pixels(three[3 * k:3 * k + 3], UNIT, 257, 65) for k in range(3)) > 2 * GRID_BLOCKS * GRID_TURNS * GRID_SHARE
    res = lu.Result(lu.pack(np.arange(16) % 4, 2), [(0, 2, 2)], [0, -2, 0] * copies, ot.IDX_U8)
    dev = make.scene(checker_texture(), three, np.tile(np.arange(9, dtype=np.uint32), copies), ru.HostResult.of(res))
    ref = ru.check(dll, hip, dev, UNIT, 257, 65, count=3)
    assert set(np.unique(ref["primitiveIds"]).tolist()) == {0, 1}
    assert ru.same(ru.rasterize(dll, hip, dev, UNIT, 257, 65), ref)
    assert ru.same(ru.rasterize(dll, hip, dev, UNIT, 257, 65, want=(), want_info=True), ref, ("info",))


def test_many_small_triangles_and_a_large_one_between_them(dll, hip, make):
    """3000 triangles of at most a pixel each, then a large triangle overlapped by small ones with lower and with higher indices: the lowest index owns
    a pixel whichever kernel claims it"""
    rng = np.random.default_rng(8)
    c = rng.random((3000, 1, 2))
    small = (c + (rng.random((3000, 3, 2)) - 0.5) / np.array([257.0, 65.0])).reshape(-1, 2)
    dev = make.scene(checker_texture(), small, np.arange(9000, dtype=np.uint32), ru.HostResult.of(mixed_result(rng, 3000)))
    ref = ru.check(dll, hip, dev, UNIT, 257, 65)
    assert 100 < ref["info"]["drawnPrimitives"] <= ref["info"]["coveredPixels"] < 3000
    big = np.array([[0.05, 0.05], [0.95, 0.1], [0.1, 0.95]])
    uv = np.concatenate([small[:300], big, small[300:600]])
    dev = make.scene(checker_texture(), uv, np.arange(len(uv), dtype=np.uint32), ru.HostResult.of(mixed_result(rng, 201, ot.IDX_U8, levels=(0, 2, 5))))
    ref = ru.check(dll, hip, dev, UNIT, 257, 65)
    ids = ref["primitiveIds"]
    assert (ids < 100).any() and (ids == 100).sum() > 3000 and not ((ids > 100) & (ids != ru.NONE) & (ru.model(dll, dev.sc, UNIT, 257, 65, 100, 1)["primitiveIds"] == 100)).any()
    assert ((ids > 100) & (ids != ru.NONE)).any() and ref["info"]["invalidPixels"] == 0


# ---- input formats ----
@pytest.mark.parametrize("case", ["unorm16", "fp16", "fp32", "fp32_stride9_offset1", "fp32_stride20_offset4", "index16", "index8"])
def test_input_formats(dll, hip, make, case):
    """the three texture-coordinate formats, strides and offsets that are no multiples of 4, and the three index widths over shared vertices"""
    rng = np.random.default_rng(9)
    uv, ix = tiles(12, 4)
    kw = {}
    if case in ("unorm16", "fp16"):
        kw["uv_format"] = ot.UV16_UNORM if case == "unorm16" else ot.UV16_FLOAT
    elif case.startswith("fp32_"):
        stride, offset = (9, 1) if "stride9" in case else (20, 4)
        raw, read = ru.strided_fp32(uv, stride, offset)
        kw.update(raw=raw, stride=stride, offset=offset, uv_read=read)
    elif case.startswith("index"):
        uv, ix = lu.grid_mesh(11, 5, 0.2, 0.05, np.uint16 if case == "index16" else np.uint8)
    dev = make.scene(checker_texture(), uv, ix, ru.HostResult.of(mixed_result(rng, len(ix) // 3)), **kw)
    ref = ru.check(dll, hip, dev, UNIT, 65, 64)
    assert ref["info"]["drawnPrimitives"] == len(ix) // 3


# ---- blocks ----
@pytest.mark.parametrize("bits", [1, 2], ids=["2state", "4state"])
def test_every_level(dll, hip, make, bits):
    """levels 0..12 at odd byte addresses, one-byte blocks with garbage in their unused bits, and the four special indices: states, micro-triangles and
    the darker inverted ones"""
    rng = np.random.default_rng(10 + bits)
    uv, ix = tiles(17, 5)
    blocks = [(rng.integers(0, 1 << bits, 4 ** level), level, bits) for level in range(13)]
    array, descs = cu.table_of_blocks(blocks, first_offset=3, gap=1)
    for o, l, f in descs.tolist():
        if 4 ** l * f < 8:
            array[o] |= (int(rng.integers(0, 256)) << (4 ** l * f)) & 0xFF
    assert sum(d[0] % 2 for d in descs.tolist()) >= 4
    res = lu.Result(array, [tuple(d) for d in descs.tolist()], list(range(13)) + [-1, -2, -3, -4], ot.IDX_U8)
    dev = make.scene(checker_texture(), uv, ix, ru.HostResult.of(res))
    ref = ru.check(dll, hip, dev, UNIT, 129, 97, flags=ru.NO_CONTOUR)
    assert ref["info"]["invalidPixels"] == 0 and ref["info"]["drawnPrimitives"] == 17
    for p in range(13):
        m = ref["microTriangles"][ref["primitiveIds"] == p]
        assert m.max() < 4 ** p and len(np.unique(m)) >= min(4 ** p, 30)
    assert (ref["microTriangles"][(ref["primitiveIds"] >= 13) & (ref["primitiveIds"] != ru.NONE)] == 0).all()
    assert [int(np.unique(ref["states"][ref["primitiveIds"] == 13 + k])[0]) for k in range(4)] == [0, 1, 2, 3]


@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32], ids=["u8", "u16", "u32"])
def test_bounds_rule(dll, hip, make, index_format):
    """every row of lookup_util.bounds_table that a device can hold, and primitives beyond the result's indexCount: state 0xFF, micro-triangle
    0xFFFFFFFF and the invalid colour; nothing is read outside the arrays"""
    table = lu.bounds_table(index_format)
    rows = [r for r in table["rows"] if r[2]]
    res = lu.Result(table["array"], table["descs"], [r[0] for r in rows], index_format)
    n = len(rows) + 3                                   # three primitives of the mesh have no entry
    uv, ix = tiles(n, 6)
    dev = make.scene(np.zeros((4, 4), np.uint8), uv, ix, ru.HostResult.of(res))
    ref = ru.check(dll, hip, dev, UNIT, 96, 64, flags=ru.NO_CONTOUR)
    for p in range(n):
        own = ref["primitiveIds"] == p
        want = rows[p][1] if p < len(rows) else lu.INVALID
        assert own.sum() > 20
        if want == lu.INVALID:
            assert (ref["states"][own] == ru.STATE_INVALID).all() and (ref["microTriangles"][own] == ru.NONE).all() and (ref["rgba"][own] == (128, 64, 0, 255)).all()
        else:
            assert (ref["states"][own] != ru.STATE_INVALID).all()
    assert ref["info"]["invalidPixels"] == int((ref["states"] == ru.STATE_INVALID).sum()) > 0


# ---- ranges, flags, outputs ----
def test_primitive_ranges(dll, hip, make):
    rng = np.random.default_rng(12)
    uv, ix = tiles(10, 4)
    dev = make.scene(checker_texture(), uv, ix, ru.HostResult.of(mixed_result(rng, 10)))
    for first, count, drawn in ((0, ru.ALL, 10), (0, 0, 0), (3, 4, 4), (9, 1, 1), (9, 5, 1), (10, 3, 0), (4, ru.ALL, 6), (0xFFFFFFF0, 0x20, 0), (2, 0xFFFFFFFE, 8)):
        ref = ru.check(dll, hip, dev, UNIT, 40, 30, first, count)
        assert ref["info"]["drawnPrimitives"] == drawn
        if drawn == 0:
            assert (ref["primitiveIds"] == ru.NONE).all() and (ref["states"] == ru.STATE_NONE).all()


def test_flags(dll, hip, make):
    """each flag alone and all together; HighlightReuse with one descriptor under three primitives, with the first of them in and out of the range"""
    rng = np.random.default_rng(13)
    uv, ix = tiles(8, 4)
    blocks = [(rng.integers(0, 4, 16), 2, 2), (rng.integers(0, 4, 64), 3, 2)]
    array, descs = cu.table_of_blocks(blocks)
    res = lu.Result(array, [tuple(d) for d in descs.tolist()], [0, 1, 0, -3, 0, 1, -3, 5], ot.IDX_U16)
    dev = make.scene(checker_texture(), uv, ix, ru.HostResult.of(res))
    pictures = {}
    for flags in (0, ru.NO_CONTOUR, ru.MONOCHROME_UNKNOWNS, ru.HIGHLIGHT_REUSE, 7):
        pictures[flags] = ru.check(dll, hip, dev, UNIT, 64, 32, flags=flags)["rgba"]
    assert len({p.tobytes() for p in pictures.values()}) == 5
    ids = ru.model(dll, dev.sc, UNIT, 64, 32)["primitiveIds"]
    halved = lambda first: {int(p) for p in np.unique(ids[(ru.check(dll, hip, dev, UNIT, 64, 32, first=first, flags=ru.NO_CONTOUR | ru.HIGHLIGHT_REUSE)["rgba"]
                                                          != ru.model(dll, dev.sc, UNIT, 64, 32, first, ru.ALL, ru.NO_CONTOUR)["rgba"]).any(axis=2)])}
    assert halved(0) == {2, 4, 5} and halved(1) == {4, 5} and halved(3) == set()


def test_each_output_alone_and_the_info(dll, hip, make):
    """each output member alone (the others keep their fill bytes), info only, outputs without info, two calls on a stream: the same bytes and the same
    info every time; the sources are unchanged afterwards"""
    rng = np.random.default_rng(14)
    uv, ix = tiles(20, 5, lo=-0.05, size=1.1)
    dev = make.scene(checker_texture(), uv, ix, ru.HostResult.of(mixed_result(rng, 18)), filt=ot.LINEAR)
    ref = ru.check(dll, hip, dev, UNIT, 65, 33, flags=ru.HIGHLIGHT_REUSE)
    for name in ru.OUTPUTS:
        got = ru.rasterize(dll, hip, dev, UNIT, 65, 33, flags=ru.HIGHLIGHT_REUSE, want=(name,))
        assert ru.same(got, ref, (name, "info"))
    assert ru.rasterize(dll, hip, dev, UNIT, 65, 33, flags=ru.HIGHLIGHT_REUSE, want=())["info"] == ref["info"]
    assert ru.same(ru.rasterize(dll, hip, dev, UNIT, 65, 33, flags=ru.HIGHLIGHT_REUSE, want_info=False), ref, ru.OUTPUTS)
    stream = hip.stream_create(non_blocking=True)
    try:
        a = ru.rasterize(dll, hip, dev, UNIT, 65, 33, flags=ru.HIGHLIGHT_REUSE, stream=stream)
        b = ru.rasterize(dll, hip, dev, UNIT, 65, 33, flags=ru.HIGHLIGHT_REUSE, stream=stream)
        assert ru.same(a, ref) and ru.same(b, ref)
    finally:
        hip.stream_destroy(stream)
    assert dev.sources_unchanged()


@pytest.mark.parametrize("fp32", [False, True], ids=["unorm8", "fp32"])
@pytest.mark.parametrize("filt", [ot.NEAREST, ot.LINEAR], ids=["nearest", "linear"])
def test_samplers(dll, hip, make, filt, fp32):
    """Nearest and Linear over UNORM8 and FP32 textures with a cut-off that equals a texel value (alphaTest is cutoff < alpha: that texel is below), and
    FP32 texels beyond [0, 1] and NaN for the grey"""
    rng = np.random.default_rng(15)
    tex = rng.integers(0, 256, (7, 9)).astype(np.uint8)
    tex[2, 3] = tex[5, 5] = 128
    cutoff = float(np.float32(128) * np.float32(1.0 / 255.0))
    if fp32:
        tex = rng.random((7, 9)).astype(np.float32)
        tex[2, 3] = tex[5, 5] = 0.5
        tex[0, 0], tex[1, 1], tex[3, 3] = -0.5, 1.5, np.nan
        cutoff = 0.5
    uv, ix = tiles(6, 3)
    dev = make.scene(tex, uv, ix, ru.HostResult.of(mixed_result(rng, 6)), filt=filt, addr=ot.MIRROR, cutoff=cutoff, le=ot.UT, gt=ot.O)
    ref = ru.check(dll, hip, dev, UNIT, 90, 70)
    assert 0 < ref["info"]["alphaAbovePixels"] < 90 * 70
    if filt == ot.NEAREST:
        assert ref["alphaTest"][int(2.5 / 7 * 70), int(3.5 / 9 * 90)] == 0


# ---- what the entry is for: a result against a texture ----
@pytest.fixture(scope="module")
def small_bake(product, hip, baker, dll):
    """a 32 x 32 texture of 0 / 1 texels and 20 triangles baked at level 4, 4-state, Nearest and Linear; the same mesh over the inverted texture"""
    rng = np.random.default_rng(16)
    tex = (ot.value_noise(16, 32, 32, octaves=2, base_cell=8) > 0.5).astype(np.uint8) * 255
    uv, ix = ot.random_triangles(21, 20, 0.3, lo=0.15, hi=0.85)
    placeholder = ru.HostResult.of(lu.Result(np.zeros(1, np.uint8), [], [-1] * 20, ot.IDX_U32))
    out = {}
    for name, texels, filt in (("nearest", tex, ot.NEAREST), ("inverted", 255 - tex, ot.NEAREST), ("linear", tex, ot.LINEAR)):
        dev = ru.DeviceScene(product, hip, baker, ru.Scene(texels, uv, ix, placeholder, filt=filt, addr=ot.CLAMP))
        out[name] = dev
    for name in ("nearest", "linear"):
        dev = out[name]
        desc = ot.make_desc(dev.tex, dev.sc.uv_read, ix, 4, filt=dev.sc.filt, addr=ot.CLAMP)
        bake = lu.DeviceBake(product, hip, baker, desc, dev.sc.uv_read, ix)
        out[name + "_bake"] = bake
    yield out
    for v in out.values():
        v.close()


def with_result(dev, host):
    sc = dev.sc
    return ru.Scene(sc.tex, None, sc.ix, host, filt=sc.filt, addr=sc.addr, raw=sc.raw, stride=sc.stride, offset=sc.offset, uv_read=sc.uv_read)


def check_against(dll, hip, dev, host, rdesc, width=96, height=96):
    ref = ru.model(dll, with_result(dev, host), UNIT, width, height)
    ru.same(ru.rasterize(dll, hip, dev, UNIT, width, height, rdesc=rdesc), ref)
    return ref


def test_a_fresh_bake_contradicts_its_texture_nowhere(dll, hip, baker, small_bake):
    """the Nearest bake at 96 x 96: contradictions equals the model and is 0, with known states on most of the covered pixels; against the inverted
    texture every known pixel contradicts; the coarsening at cap 2 of the same bake still has 0"""
    bake = small_bake["nearest_bake"]
    host = ru.HostResult.of_arrays(bake.host_arrays, bake.rdesc.indexFormat)
    ref = check_against(dll, hip, small_bake["nearest"], host, bake.rdesc)
    i = ref["info"]
    known = i["pixelsPerState"][0] + i["pixelsPerState"][1]
    assert i["contradictions"] == 0 and known > 0 and i["coveredPixels"] > 300 and i["invalidPixels"] == 0 and i["drawnPrimitives"] > 10
    inv = check_against(dll, hip, small_bake["inverted"], host, bake.rdesc)["info"]
    assert inv["contradictions"] == known > 0 and inv["pixelsPerState"] == i["pixelsPerState"]
    r, _, handle = cu.coarsen(dll, baker, bake.rdesc, 2)
    assert r == ot.SUCCESS
    try:
        got = cu.download_result(dll, hip, handle)
        coarse = ru.HostResult.of(lu.Result(got["array"] if len(got["array"]) else np.zeros(1, np.uint8), [tuple(d) for d in got["descs"].tolist()],
                                            got["index"].astype(np.int64), got["index_format"]))
        c = check_against(dll, hip, small_bake["nearest"], coarse, got["rdesc"])["info"]
        assert c["contradictions"] == 0 and c["coveredPixels"] == i["coveredPixels"]
        assert 0 < c["pixelsPerState"][0] + c["pixelsPerState"][1] < known
    finally:
        assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS


def test_a_linear_bake_is_held_to_the_model(dll, hip, small_bake):
    """the Linear-filter bake: contradictions is whatever the model counts (the classification of slivers may call a micro-triangle known against a
    bilinear value inside it), not 0 by decree"""
    bake = small_bake["linear_bake"]
    host = ru.HostResult.of_arrays(bake.host_arrays, bake.rdesc.indexFormat)
    ref = check_against(dll, hip, small_bake["linear"], host, bake.rdesc)
    assert ref["info"]["coveredPixels"] > 1000 and ref["info"]["contradictions"] <= ref["info"]["pixelsPerState"][0] + ref["info"]["pixelsPerState"][1]
