"""ommxCreateTextureDevice on the GPU: a texture made from one channel of an interleaved image in device memory (texture_kernels.hip) is the
texture ommCpuCreateTexture makes from the extracted channel -- equal serialized blobs with both compress flags, no tolerance -- and its tables
equal the numpy reference of tests/sat_util.py.  Every source is interleaved in numpy with a non-tight pitch, the complement of the alpha channel
(UNORM8) or NaN bit patterns (FP16 / FP32) in the other channels and the padding, at the widths and heights where the gather changes path: the
4 / 8 / 16-texel groups, the peeled texels in front of them (rows of the packed array that start off a group boundary), the ragged end of a row,
vector loads against per-texel loads (a base displaced by one pixel, a pitch that is only channel-aligned)."""
import ctypes as C
import numpy as np
import pytest
import blobfmt
import ommtest as ot
import sat_util as su
import texture_device_util as tu
import lookup_util as lu

pytestmark = pytest.mark.gpu

CUTOFF = 0.5


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


@pytest.fixture(scope="module")
def host_made():
    """blobs of the host-made textures, one per (format, shape, tiling): computed once, shared by the layouts, never changed"""
    return {}


def _one(product, baker, hip, host_made, layout, bits, disable_zorder, pad_elems, lead_pixels, cutoff=CUTOFF, key=None):
    fmt, stride, offset = layout
    h, w = bits.shape
    mips = [tu.texels_of(fmt, bits)]
    want = tu.host_blobs(product, baker, mips, cutoff, disable_zorder, host_made if key is not None else None, key)
    src = tu.Source(hip, fmt, stride, offset, bits, pad_elems, lead_pixels)
    try:
        tex = tu.create(product, baker, tu.make_desc(fmt, stride, offset, [src.mip], cutoff, disable_zorder))
    finally:
        src.free()
    try:
        tu.check_texture(product, baker, tex, mips, cutoff, disable_zorder, want,
                         "%s %dx%d zorder-off %d pad %d lead %d" % (tu.layout_id(layout), w, h, disable_zorder, pad_elems, lead_pixels))
    finally:
        product.destroy_texture(baker, tex)


@pytest.mark.parametrize("layout", tu.LAYOUTS, ids=[tu.layout_id(l) for l in tu.LAYOUTS])
def test_every_layout_at_every_shape(product, baker, hip, host_made, layout):
    """tight and padded pitch (3 channel-sized elements: rows lose their vector alignment), both tilings, base 16-byte aligned and displaced by one pixel"""
    fmt = layout[0]
    for (w, h) in tu.shapes():
        bits = tu.channel_bits(fmt, w, h, seed=1000 * w + h)
        for disable_zorder in su.tilings(w, h):
            for pad_elems in (0, 3):
                for lead_pixels in (0, 1):
                    _one(product, baker, hip, host_made, layout, bits, disable_zorder, pad_elems, lead_pixels, key=(fmt, w, h, disable_zorder))


def test_every_half_bit_pattern(product, baker, hip):
    """all 65 536 halves in one 256 x 256 FP16 texture, packed and as the A of RGBA16F: finite values and infinities by their bits, NaN by NaN-ness"""
    bits = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    want = bits.view(np.float16).astype(np.float32)
    for (stride, offset) in ((2, 0), (8, 6)):
        src = tu.Source(hip, tu.FP16, stride, offset, bits, pad_elems=1)
        tex = tu.create(product, baker, tu.make_desc(tu.FP16, stride, offset, [src.mip], CUTOFF, True))
        src.free()
        parsed = blobfmt.parse_blob(su.serialize_texture(product, baker, tex, 0))["inputs"][0]["texture"]
        product.destroy_texture(baker, tex)
        got = parsed["mips"][0]
        assert got.dtype == np.float32 and got.shape == (256, 256)
        nan = np.isnan(want)
        assert nan.sum() == 2 * 1023 and np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
        su.check_tables(parsed, [want], CUTOFF, True)


@pytest.mark.parametrize("disable_zorder", [True, False])
def test_fp32_special_values_through_rgba32f(product, baker, hip, disable_zorder):
    """NaN, +-inf, -0.0, denormals, texels at the cut-off and one ulp to either side, as the A of an RGBA32F image whose other channels are NaN"""
    for cutoff, tex in su.fp32_special_cases():
        _one(product, baker, hip, None, (tu.FP32, 16, 12), tex.view(np.uint32), disable_zorder, pad_elems=1, lead_pixels=1, cutoff=cutoff)


@pytest.mark.parametrize("disable_zorder", [True, False])
def test_unorm8_cutoffs_through_rgba8(product, baker, hip, disable_zorder):
    """every byte value against cut-offs k / 255 and one ulp to either side (one of them negative: no table), as the A of an RGBA8 image"""
    tex = ((np.arange(65)[None, :] * 7 + np.arange(67)[:, None] * 13) % 256).astype(np.uint8)
    for cutoff in su.unorm8_cutoffs():
        _one(product, baker, hip, None, (tu.UNORM8, 4, 3), tex, disable_zorder, pad_elems=2, lead_pixels=0, cutoff=cutoff)


MIP_SHAPES = [(257, 129), (64, 65), (1, 1)]


@pytest.mark.parametrize("layout", [(tu.UNORM8, 4, 3), (tu.FP16, 8, 6), (tu.FP32, 4, 0), (tu.UNORM8, 3, 1)], ids=tu.layout_id)
@pytest.mark.parametrize("disable_zorder", [True, False])
def test_three_mips_from_three_allocations(product, baker, hip, layout, disable_zorder):
    fmt, stride, offset = layout
    bits = [tu.channel_bits(fmt, w, h, seed=7 + w) for (w, h) in MIP_SHAPES]
    mips = [tu.texels_of(fmt, b) for b in bits]
    want = tu.host_blobs(product, baker, mips, CUTOFF, disable_zorder)
    srcs = [tu.Source(hip, fmt, stride, offset, b, pad_elems=k, lead_pixels=k & 1) for k, b in enumerate(bits)]
    tex = tu.create(product, baker, tu.make_desc(fmt, stride, offset, [s.mip for s in srcs], CUTOFF, disable_zorder))
    for s in srcs:
        s.free()
    tu.check_texture(product, baker, tex, mips, CUTOFF, disable_zorder, want, "three mips")
    product.destroy_texture(baker, tex)


@pytest.mark.parametrize("disable_zorder", [True, False])
def test_no_cutoff_no_table(product, baker, hip, disable_zorder):
    bits = tu.channel_bits(tu.UNORM8, 65, 63, seed=1)
    _one(product, baker, hip, None, (tu.UNORM8, 4, 3), bits, disable_zorder, pad_elems=4, lead_pixels=0, cutoff=-1.0)
    _one(product, baker, hip, None, (tu.FP16, 8, 6), tu.channel_bits(tu.FP16, 65, 63, seed=2), disable_zorder, pad_elems=0, lead_pixels=1, cutoff=-1.0)


def test_source_produced_on_the_callers_stream_without_synchronisation(product, baker, hip):
    """the image is written by device-to-device copies queued on a caller stream right before the call -- behind other copies that keep the stream busy --
    and nothing waits in between: the gather is ordered behind them by the stream alone"""
    hip.rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    layout = (tu.UNORM8, 4, 3)
    bits = tu.channel_bits(tu.UNORM8, 513, 257, seed=11)
    mips = [bits]
    want = tu.host_blobs(product, baker, mips, CUTOFF, True)
    staged = tu.Source(hip, *layout, bits, pad_elems=4)               # complete (uploaded with a blocking copy)
    target = hip.upload(np.full(staged.nbytes, 0x80, np.uint8))       # what the texture is made from: holds other bytes until the copy lands
    busy = [hip.alloc(32 << 20), hip.alloc(32 << 20)]
    for non_blocking in (False, True):
        hip.copy_htod(target, np.full(staged.nbytes, 0x80, np.uint8))
        assert hip.rt.hipDeviceSynchronize() == 0
        stream = hip.stream_create(non_blocking=non_blocking)
        for k in range(8):
            assert hip.rt.hipMemcpyAsync(busy[k & 1], busy[1 - (k & 1)], 32 << 20, 3, stream) == 0
        assert hip.rt.hipMemcpyAsync(target, staged.base, staged.nbytes, 3, stream) == 0
        w, h, pitch, ptr = staged.mip
        tex = tu.create(product, baker, tu.make_desc(*layout, [(w, h, pitch, target.value + (ptr - staged.base.value))], CUTOFF, True), stream=stream)
        tu.check_texture(product, baker, tex, mips, CUTOFF, True, want, "stream-ordered source")
        product.destroy_texture(baker, tex)
        hip.stream_destroy(stream)
    for p in busy + [target]:
        hip.free(p)
    staged.free()


def test_source_overwritten_and_freed_after_the_call(product, baker, hip):
    """the texture owns its texels when the call returns: the source is overwritten, then freed, and the texture is read afterwards"""
    for layout in ((tu.UNORM8, 4, 3), (tu.FP16, 8, 6)):
        fmt, stride, offset = layout
        bits = tu.channel_bits(fmt, 257, 65, seed=21)
        mips = [tu.texels_of(fmt, bits)]
        want = tu.host_blobs(product, baker, mips, CUTOFF, True)
        src = tu.Source(hip, fmt, stride, offset, bits, pad_elems=2)
        tex = tu.create(product, baker, tu.make_desc(fmt, stride, offset, [src.mip], CUTOFF, True))
        hip.copy_htod(src.base, np.full(src.nbytes, 0xFF, np.uint8))
        assert hip.rt.hipDeviceSynchronize() == 0
        src.free()
        tu.check_texture(product, baker, tex, mips, CUTOFF, True, want, "source gone")
        product.destroy_texture(baker, tex)


def test_pooled_scratch_reused_dirty(product, hip):
    """textures of different sizes back to back on one baker (the column pass's pooled scratch block is handed out as it was left), all above the cut-off
    before random ones, alive together, tables read afterwards"""
    b = product.create_baker()
    alive = []
    for n, (w, h, above) in enumerate([(513, 257, 1), (300, 129, 0), (257, 257, 0), (64, 65, 1), (513, 257, 0), (1, 200, 0)]):
        bits = np.full((h, w), 255, np.uint8) if above else tu.channel_bits(tu.UNORM8, w, h, seed=40 + n)
        src = tu.Source(hip, tu.UNORM8, 4, 3, bits, pad_elems=n)
        alive.append((bits, tu.create(product, b, tu.make_desc(tu.UNORM8, 4, 3, [src.mip], CUTOFF, True))))
        src.free()
    for bits, t in alive:
        su.check_tables(blobfmt.parse_blob(su.serialize_texture(product, b, t, 0))["inputs"][0]["texture"], [bits], CUTOFF, True)
    for bits, t in alive:
        product.destroy_texture(b, t)
    product.destroy_baker(b)


def test_bakes_and_hit_resolution_with_a_device_made_texture(product, baker, hip):
    """one 64 x 64 RGBA8 image, 300 small triangles at level 4: ommCpuBake and ommxBakeDevice give the results they give with the host-made texture, and
    ommxResolveHits answers 4096 hits with the same bytes"""
    lu.bind(product.dll)
    alpha = (ot.value_noise(5, 64, 64, octaves=3, base_cell=16) * 255).astype(np.uint8)
    uv, ix = ot.random_triangles(6, 300, 6.0 / 64)
    src = tu.Source(hip, tu.UNORM8, 4, 3, alpha, pad_elems=8)
    made = {"device": tu.create(product, baker, tu.make_desc(tu.UNORM8, 4, 3, [src.mip], CUTOFF)),
            "host": product.create_texture(baker, [alpha], alpha_cutoff=CUTOFF)}
    src.free()
    rng = np.random.RandomState(3)
    hits = np.zeros(4096, lu.HIT)
    hits["prim"] = rng.randint(0, 300, size=4096)
    hits["u"] = rng.rand(4096) * 0.5
    hits["v"] = rng.rand(4096) * 0.5
    got = {}
    for name, tex in made.items():
        d = ot.make_desc(tex, uv, ix, 4, addr=ot.WRAP, promo=ot.PROMO_FORCE_OPAQUE)
        host_bake = product.bake(baker, d)
        dev = lu.DeviceBake(product, hip, baker, d, uv, ix)
        resolved = [lu.resolve_device(product.dll, hip, baker, dev.ddesc, dev.rdesc, hits, flags) for flags in (0, lu.IGNORE_MICROMAP)]
        got[name] = (host_bake, dev.host, resolved)
        dev.close()
    for tex in made.values():
        product.destroy_texture(baker, tex)
    assert got["device"][0].same_as(got["host"][0]), got["device"][0].diff(got["host"][0])
    assert got["device"][1].same_as(got["host"][1]), got["device"][1].diff(got["host"][1])
    assert got["host"][0].array_data.size > 0 and got["host"][1].array_data.size > 0
    for a, b in zip(got["device"][2], got["host"][2]):
        assert np.array_equal(a, b)
    sampled = got["host"][2][1]                                  # IgnoreMicromap: every hit samples the texture; both answers occur
    assert (sampled != lu.INVALID).all() and (sampled & 8).all() and len(np.unique(sampled & 1)) == 2
