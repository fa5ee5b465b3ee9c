"""ommxCreateTextureBC / ommxCreateTextureBCDevice on the GPU: a texture made from BC1..BC5 blocks (block_kernels.hip) is the texture
ommCpuCreateTexture makes from the texels the numpy reference decoder of tests/block_texture_util.py gives for those blocks -- equal serialized blobs
with both compress flags, no tolerance -- and its tables equal the numpy reference of tests/sat_util.py.  Blocks are random in every byte, the ones
that must not matter included; shapes sit where the decode changes path: widths that are and are not multiples of 4 (one aligned store per block row
against per-texel stores), partial last block columns and rows, the 64 blocks of a wave and the 4 block rows of a workgroup."""
import ctypes as C
import numpy as np
import pytest
import blobfmt
import ommtest as ot
import sat_util as su
import texture_device_util as tu
import block_texture_util as bu
import lookup_util as lu

pytestmark = pytest.mark.gpu

CUTOFF = 0.5
FATAL = 3
IDENTITY_CODES = [0x88, 0xC6, 0xFA, 0x88, 0xC6, 0xFA]   # the 3-bit codes 0..7, 0..7


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def _made_and_checked(product, baker, desc, device, mips, cutoff, disable_zorder, want, what):
    tex = bu.create(product, baker, desc, device)
    try:
        tu.check_texture(product, baker, tex, mips, cutoff, disable_zorder, want, what)
    finally:
        product.destroy_texture(baker, tex)


@pytest.mark.parametrize("fc", bu.FORMATS, ids=bu.format_id)
def test_every_format_at_every_shape(product, baker, hip, fc):
    """tight pitch and one padded by 8 bytes of 0xFF, both tilings; device entry from hipMalloc memory at its base and 8 bytes behind it, one shape from
    pinned host memory; host entry from a numpy array 1 byte behind its start"""
    fmt, channel = fc
    for n, (w, h) in enumerate(bu.shapes()):
        blocks = bu.random_blocks(fmt, w, h, seed=1000 * w + h + 7 * fmt)
        mips = [bu.decode(fmt, channel, blocks, w, h)]
        for disable_zorder in su.tilings(w, h):
            want = tu.host_blobs(product, baker, mips, CUTOFF, disable_zorder)
            for pad in (0, 8):
                what = "%s %dx%d zorder-off %d pad %d" % (bu.format_id(fc), w, h, disable_zorder, pad)
                for lead in (0, 8):
                    src = bu.DeviceBlocks(hip, blocks, pad, lead)
                    try:
                        _made_and_checked(product, baker, bu.make_desc(fmt, channel, [src.mip(w, h)], CUTOFF, disable_zorder), True, mips, CUTOFF, disable_zorder, want,
                                          what + " device lead %d" % lead)
                    finally:
                        src.free()
                host = bu.HostBlocks(blocks, pad, lead=1)
                _made_and_checked(product, baker, bu.make_desc(fmt, channel, [host.mip(w, h)], CUTOFF, disable_zorder), False, mips, CUTOFF, disable_zorder, want, what + " host")
                if n == 20 and disable_zorder:
                    pinned = bu.PinnedBlocks(hip, blocks, pad)
                    try:
                        _made_and_checked(product, baker, bu.make_desc(fmt, channel, [pinned.mip(w, h)], CUTOFF, True), True, mips, CUTOFF, True, want, what + " pinned")
                    finally:
                        pinned.free()


def _texels_by_bits(product, baker, tex):
    parsed = blobfmt.parse_blob(su.serialize_texture(product, baker, tex, 0))["inputs"][0]["texture"]
    return parsed["mips"][0]


def test_every_endpoint_pair(product, baker, hip):
    """one 1024 x 1024 texture of 65 536 blocks, block (a0, a1) at block column a0, block row a1, its 16 codes going through all 8 values twice: as BC4 (device
    entry), as the second channel of BC5 (device entry) and as BC3 with random colour halves (host entry), every texel by its bits"""
    alpha = np.zeros((256, 256, 8), np.uint8)
    alpha[:, :, 0] = np.arange(256)[None, :]
    alpha[:, :, 1] = np.arange(256)[:, None]
    alpha[:, :, 2:] = IDENTITY_CODES
    want = bu.decode(bu.BC4, 0, alpha, 1024, 1024)
    assert want.dtype == np.float32 and want[4 * 100, 4 * 200] == np.float32(200) * (np.float32(1) / np.float32(255))   # code 0 of block (a0 = 200, a1 = 100)
    blobs = tu.host_blobs(product, baker, [want], CUTOFF, True)
    other = np.random.RandomState(5).randint(0, 256, size=(256, 256, 8)).astype(np.uint8)
    for fmt, channel, blocks, device in ((bu.BC4, 0, alpha, True), (bu.BC5, 1, np.concatenate([other, alpha], axis=2), True), (bu.BC3, 0, np.concatenate([alpha, other], axis=2), False)):
        assert np.array_equal(bu.decode(fmt, channel, blocks, 1024, 1024).view(np.uint32), want.view(np.uint32))
        src = bu.DeviceBlocks(hip, blocks) if device else bu.HostBlocks(blocks)
        tex = bu.create(product, baker, bu.make_desc(fmt, channel, [src.mip(1024, 1024)], CUTOFF, True), device)
        if device:
            src.free()
        try:
            got = _texels_by_bits(product, baker, tex)
            assert got.dtype == np.float32 and got.shape == (1024, 1024)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), bu.format_id((fmt, channel))
            tu.check_texture(product, baker, tex, [want], CUTOFF, True, blobs, bu.format_id((fmt, channel)) + " endpoint pairs")
        finally:
            product.destroy_texture(baker, tex)


def _bc2_complete():
    """64 x 4 texels, 16 blocks: nibble i of block b is (i + b) % 16 -- every value at every texel position; random colour halves"""
    blocks = np.random.RandomState(9).randint(0, 256, size=(1, 16, 16)).astype(np.uint8)
    for b in range(16):
        nib = [(i + b) % 16 for i in range(16)]
        blocks[0, b, :8] = [nib[2 * k] | (nib[2 * k + 1] << 4) for k in range(8)]
    return blocks


def _bc1_complete():
    """64 x 16 texels, 64 blocks.  The first 12: c0 <, ==, > c1, code of texel i = (i + b) % 4 for b = 0..3 -- every code at every position in each
    order; the rest random"""
    blocks = np.random.RandomState(10).randint(0, 256, size=(4, 16, 8)).astype(np.uint8)
    flat = blocks.reshape(64, 8)
    n = 0
    for c0, c1 in ((0x1234, 0x5678), (0x8421, 0x8421), (0x5678, 0x1234)):
        for b in range(4):
            codes = [(i + b) % 4 for i in range(16)]
            flat[n, :4] = [c0 & 255, c0 >> 8, c1 & 255, c1 >> 8]
            flat[n, 4:] = [sum(codes[4 * y + x] << (2 * x) for x in range(4)) for y in range(4)]
            n += 1
    return flat.reshape(4, 16, 8)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_bc2_and_bc1_complete(product, baker, hip, device):
    for fmt, blocks, w, h in ((bu.BC2, _bc2_complete(), 64, 4), (bu.BC1, _bc1_complete(), 64, 16)):
        mips = [bu.decode(fmt, 0, blocks, w, h)]
        if fmt == bu.BC2:
            assert all(sorted(mips[0][y, x::4].tolist()) == [17 * v for v in range(16)] for y in range(4) for x in range(4))
        else:
            holes = (mips[0][:4, :] == 0).reshape(4, 16, 4).transpose(1, 0, 2).reshape(16, 16)   # [block, texel] of the first row of blocks
            assert (holes[:8].sum(axis=0) == 2).all() and (holes[:8].sum(axis=1) == 4).all() and not holes[8:12].any()
        want = tu.host_blobs(product, baker, mips, CUTOFF, True)
        src = bu.DeviceBlocks(hip, blocks, lead=8) if device else bu.HostBlocks(blocks, lead=1)
        try:
            _made_and_checked(product, baker, bu.make_desc(fmt, 0, [src.mip(w, h)], CUTOFF, True), device, mips, CUTOFF, True, want, bu.NAMES[fmt] + " complete")
        finally:
            if device:
                src.free()


MIP_SHAPES = [(130, 66), (2, 2), (1, 1)]


@pytest.mark.parametrize("fmt", [bu.BC1, bu.BC3], ids=["bc1", "bc3"])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("disable_zorder", [True, False])
def test_three_mips_from_three_allocations(product, baker, hip, fmt, device, disable_zorder):
    blocks = [bu.random_blocks(fmt, w, h, seed=31 + w) for (w, h) in MIP_SHAPES]
    mips = [bu.decode(fmt, 0, b, w, h) for b, (w, h) in zip(blocks, MIP_SHAPES)]
    want = tu.host_blobs(product, baker, mips, CUTOFF, disable_zorder)
    srcs = [bu.DeviceBlocks(hip, b, pad=8 * (k & 1), lead=8 * (k >> 1)) if device else bu.HostBlocks(b, pad=8 * (k & 1), lead=k) for k, b in enumerate(blocks)]
    try:
        desc = bu.make_desc(fmt, 0, [s.mip(w, h) for s, (w, h) in zip(srcs, MIP_SHAPES)], CUTOFF, disable_zorder)
        _made_and_checked(product, baker, desc, device, mips, CUTOFF, disable_zorder, want, "three mips")
    finally:
        if device:
            for s in srcs:
                s.free()


def test_blocks_produced_on_the_callers_stream_and_overwritten_after_the_call(product, baker, hip):
    """the blocks reach device memory through hipMemcpyAsync from pinned memory on a non-blocking stream, behind copies that keep the stream busy; the call is
    made on that stream with nothing waiting in between, and the source is overwritten as soon as it returns"""
    hip.rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    w, h = 1024, 516
    blocks = bu.random_blocks(bu.BC3, w, h, seed=77)
    mips = [bu.decode(bu.BC3, 0, blocks, w, h)]
    want = tu.host_blobs(product, baker, mips, CUTOFF, True)
    pinned = bu.PinnedBlocks(hip, blocks)
    target = hip.upload(np.full(pinned.nbytes, 0x80, np.uint8))       # holds other bytes until the copy lands
    busy = [hip.alloc(32 << 20), hip.alloc(32 << 20)]
    assert hip.rt.hipDeviceSynchronize() == 0
    stream = hip.stream_create(non_blocking=True)
    for k in range(8):
        assert hip.rt.hipMemcpyAsync(busy[k & 1], busy[1 - (k & 1)], 32 << 20, 3, stream) == 0
    assert hip.rt.hipMemcpyAsync(target, pinned.base, pinned.nbytes, 1, stream) == 0
    tex = bu.create(product, baker, bu.make_desc(bu.BC3, 0, [(w, h, 0, target.value)], CUTOFF, True), True, stream=stream)
    hip.copy_htod(target, np.full(pinned.nbytes, 0xFF, np.uint8))     # the stream was synchronised by the call: the blocks are no longer needed
    assert hip.rt.hipDeviceSynchronize() == 0
    try:
        tu.check_texture(product, baker, tex, mips, CUTOFF, True, want, "stream-ordered blocks")
    finally:
        product.destroy_texture(baker, tex)
        hip.stream_destroy(stream)
        for p in busy + [target]:
            hip.free(p)
        pinned.free()


def _bake_both_ways(product, hip, baker, tex, uv, ix):
    d = ot.make_desc(tex, uv, ix, 4, addr=ot.WRAP, promo=ot.PROMO_FORCE_OPAQUE)
    host_bake = product.bake(baker, d)
    dev = lu.DeviceBake(product, hip, baker, d, uv, ix)
    device_bake = dev.host
    dev.close()
    return host_bake, device_bake


def _same_bakes(a, b):
    for x, y in zip(a, b):
        assert x.same_as(y), x.diff(y)
        assert x.array_data.size > 0


def test_bake_with_a_bc3_made_texture(product, baker, hip):
    """64 x 64, 300 triangles, level 4, 4-state, cut-off 0.5: ommCpuBake and ommxBakeDevice give, byte for byte, what they give with the host-made FP32 texture
    of the decoded texels"""
    lu.bind(product.dll)
    noise = ot.value_noise(5, 16, 16, octaves=2, base_cell=4) * 255
    blocks = np.random.RandomState(12).randint(0, 256, size=(16, 16, 16)).astype(np.uint8)   # random codes and colour halves
    blocks[:, :, 0] = np.clip(noise + 50, 0, 255)
    blocks[:, :, 1] = np.clip(noise - 50, 0, 255)
    texels = bu.decode(bu.BC3, 0, blocks, 64, 64)
    assert 0.2 < (texels > CUTOFF).mean() < 0.8
    uv, ix = ot.random_triangles(6, 300, 6.0 / 64)
    src = bu.DeviceBlocks(hip, blocks)
    made = {"blocks": bu.create(product, baker, bu.make_desc(bu.BC3, 0, [src.mip(64, 64)], CUTOFF), True),
            "texels": product.create_texture(baker, [texels], alpha_cutoff=CUTOFF)}
    src.free()
    try:
        got = {name: _bake_both_ways(product, hip, baker, tex, uv, ix) for name, tex in made.items()}
    finally:
        for tex in made.values():
            product.destroy_texture(baker, tex)
    _same_bakes(got["blocks"], got["texels"])


def test_integer_alpha_bc4_bakes_like_the_unorm8_texture(product, baker, hip):
    """a BC4 image whose blocks use only codes 0 and 1: every texel is one of its block's two endpoint bytes, and its fp32 value is the value the library gives
    that UNORM8 byte -- so a bake with it equals the bake with the UNORM8 texture of the same bytes"""
    lu.bind(product.dll)
    rng = np.random.RandomState(13)
    noise = ot.value_noise(8, 16, 16, octaves=2, base_cell=4) * 255
    a0 = np.clip(noise + rng.randint(-60, 60, size=(16, 16)), 0, 255).astype(np.uint8)
    a1 = np.clip(noise + rng.randint(-60, 60, size=(16, 16)), 0, 255).astype(np.uint8)
    codes = rng.randint(0, 2, size=(16, 16, 16))                                              # 0 or 1 per texel
    bits = sum(codes[:, :, i].astype(np.uint64) << np.uint64(3 * i) for i in range(16))
    blocks = np.zeros((16, 16, 8), np.uint8)
    blocks[:, :, 0], blocks[:, :, 1] = a0, a1
    for k in range(6):
        blocks[:, :, 2 + k] = ((bits >> np.uint64(8 * k)) & np.uint64(255)).astype(np.uint8)
    as_bytes = np.where(codes == 0, a0[:, :, None], a1[:, :, None]).astype(np.uint8).reshape(16, 16, 4, 4).transpose(0, 2, 1, 3).reshape(64, 64)
    texels = bu.decode(bu.BC4, 0, blocks, 64, 64)
    assert np.array_equal(texels, as_bytes.astype(np.float32) * (np.float32(1) / np.float32(255)))
    assert 0.2 < (texels > CUTOFF).mean() < 0.8
    uv, ix = ot.random_triangles(7, 300, 6.0 / 64)
    host = bu.HostBlocks(blocks)
    made = {"blocks": bu.create(product, baker, bu.make_desc(bu.BC4, 0, [host.mip(64, 64)], CUTOFF), False),
            "bytes": product.create_texture(baker, [as_bytes], alpha_cutoff=CUTOFF)}
    try:
        got = {name: _bake_both_ways(product, hip, baker, tex, uv, ix) for name, tex in made.items()}
    finally:
        for tex in made.values():
            product.destroy_texture(baker, tex)
    _same_bakes(got["blocks"], got["bytes"])


def test_memory_the_device_cannot_read_is_refused(product, hip):
    """pageable host memory and a pointer the runtime does not know on the device entry: INVALID_ARGUMENT with the line, the handle not written, and the
    device still healthy afterwards"""
    msgs = []
    b = product.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    bu.bind(product.dll)
    blocks = bu.random_blocks(bu.BC3, 64, 64, seed=3)
    pageable = np.zeros(blocks.size + 8, np.uint8)
    off = (-pageable.ctypes.data) % 8
    pageable[off:off + blocks.size] = blocks.reshape(-1)
    good = bu.DeviceBlocks(hip, blocks)
    try:
        for name, mips in (("pageable", [(64, 64, 0, pageable.ctypes.data + off)]), ("unknown", [(64, 64, 0, 0x10000)]),
                           ("pageable mip behind a good one", [good.mip(64, 64), (32, 32, 0, pageable.ctypes.data + off)])):
            del msgs[:]
            out = C.c_void_p(0x1234)
            r = product.dll.ommxCreateTextureBCDevice(b, C.byref(bu.make_desc(bu.BC3, 0, mips, CUTOFF)), None, C.byref(out))
            assert r == ot.INVALID_ARGUMENT and out.value == 0x1234, name
            assert len(msgs) == 1 and msgs[0][0] == FATAL and "is not memory the baker's device can read" in msgs[0][1], (name, msgs)
        assert hip.rt.hipDeviceSynchronize() == 0
        # the same baker and blocks, from memory it can read
        mips = [bu.decode(bu.BC3, 0, blocks, 64, 64)]
        _made_and_checked(product, b, bu.make_desc(bu.BC3, 0, [good.mip(64, 64)], CUTOFF, True), True, mips, CUTOFF, True, tu.host_blobs(product, b, mips, CUTOFF, True), "after refusals")
    finally:
        good.free()
        product.destroy_baker(b)
