"""ommxCreateTextureBC7 / ommxCreateTextureBC7Device on the GPU: a texture made from BC7 blocks (bc7_kernels.hip) is the UNORM8 texture
ommCpuCreateTexture makes from the bytes the reference decoder of tests/bc7_util.py gives for those blocks -- equal serialized blobs with both compress
flags, no tolerance -- and its tables equal the numpy reference of tests/sat_util.py.  Blocks are random in every bit but the mode, which is forced: at
least half of the blocks of an image have one of the modes 4..7 that carry an alpha.  Shapes sit where the decode changes path: widths that are and are
not multiples of 4 (one aligned store per block row against per-texel stores), partial last block columns and rows, the 64 blocks of a wave and the 4
block rows of a workgroup."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import sat_util as su
import texture_device_util as tu
import block_texture_util as bu
import bc7_util as b7
import lookup_util as lu

pytestmark = pytest.mark.gpu

CUTOFF = 0.5
FATAL = 3


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def _made_and_checked(product, baker, desc, device, mips, cutoff, disable_zorder, want, what):
    tex = b7.create(product, baker, desc, device)
    try:
        tu.check_texture(product, baker, tex, mips, cutoff, disable_zorder, want, what)
    finally:
        product.destroy_texture(baker, tex)


def _is_unorm8(product, tex):
    d = ot.TextureDesc()
    d.mips = None
    assert product.fn("ommCpuGetTextureDesc")(tex, C.byref(d)) == ot.SUCCESS
    return d.format == ot.TEX_UNORM8 and d.mipCount == 1


def test_every_shape(product, baker, hip):
    """tight pitch and one padded by 16 bytes of 0xFF, both tilings; device entry from hipMalloc memory at its base and 16 bytes behind it, one shape from
    pinned host memory; host entry from a numpy array 1 byte behind its start"""
    for n, (w, h) in enumerate(bu.shapes()):
        blocks = b7.random_blocks(w, h, seed=1000 * w + h)
        mips = [b7.decode(blocks, w, h)]
        for disable_zorder in su.tilings(w, h):
            want = tu.host_blobs(product, baker, mips, CUTOFF, disable_zorder)
            for pad in (0, 16):
                what = "bc7 %dx%d zorder-off %d pad %d" % (w, h, disable_zorder, pad)
                for lead in (0, 16):
                    src = bu.DeviceBlocks(hip, blocks, pad, lead)
                    try:
                        _made_and_checked(product, baker, b7.make_desc([src.mip(w, h)], CUTOFF, disable_zorder), True, mips, CUTOFF, disable_zorder, want, what + " device lead %d" % lead)
                    finally:
                        src.free()
                host = bu.HostBlocks(blocks, pad, lead=1)
                _made_and_checked(product, baker, b7.make_desc([host.mip(w, h)], CUTOFF, disable_zorder), False, mips, CUTOFF, disable_zorder, want, what + " host")
                if n == 20 and disable_zorder:
                    pinned = bu.PinnedBlocks(hip, blocks, pad)
                    try:
                        _made_and_checked(product, baker, b7.make_desc([pinned.mip(w, h)], CUTOFF, True), True, mips, CUTOFF, True, want, what + " pinned")
                    finally:
                        pinned.free()


# ---- completeness per mode ----
def _shifted(b, n, anchors=(0,)):
    """sixteen n-bit codes, texel i holding (i + b) mod 2^n -- over b = 0 .. 2^n - 1 every code at every texel --, an anchor holding it mod 2^(n-1)"""
    return [(i + b) % (1 << (n - 1) if i in anchors else 1 << n) for i in range(16)]


def _mode7_complete():
    """all 64 partitions x the 4 shifts of the 2-bit codes (both 1-bit codes at both anchors) x 4 draws of endpoints and P bits: 1024 blocks"""
    rng = np.random.RandomState(71)
    out = []
    for part in range(64):
        for b in range(4):
            for _ in range(4):
                e = rng.randint(0, 32, size=(4, 4))
                out.append(b7.build_mode7(part, *[tuple(int(v) for v in c) for c in e], tuple(int(v) for v in rng.randint(0, 2, size=4)), _shifted(b, 2, (0, b7.ANCHOR[part]))))
    return out


def _mode6_complete():
    """the 16 shifts of the 4-bit codes x the four P-bit pairs x 4 draws of endpoints: 256 blocks"""
    rng = np.random.RandomState(61)
    out = []
    for b in range(16):
        for p in ((0, 0), (1, 0), (0, 1), (1, 1)):
            for _ in range(4):
                e = rng.randint(0, 128, size=(4, 2))
                out.append(b7.build_mode6(*[tuple(int(v) for v in c) for c in e], p, _shifted(b, 4)))
    return out


def _mode4_complete():
    """4 rotations x 2 index modes x 8 shifts (every 3-bit code, every 2-bit code twice) x 4 draws of endpoints: 256 blocks"""
    rng = np.random.RandomState(41)
    out = []
    for rot in range(4):
        for idx_mode in range(2):
            for b in range(8):
                for _ in range(4):
                    e = rng.randint(0, 32, size=(3, 2))
                    out.append(b7.build_mode4(rot, idx_mode, *[tuple(int(v) for v in c) for c in e], tuple(int(v) for v in rng.randint(0, 64, size=2)), _shifted(b, 2), _shifted(b, 3)))
    return out


def _mode5_complete():
    """4 rotations x 4 shifts of each index set (the two sets out of step) x 16 draws of endpoints: 256 blocks"""
    rng = np.random.RandomState(51)
    out = []
    for rot in range(4):
        for b in range(4):
            for _ in range(16):
                e = rng.randint(0, 128, size=(3, 2))
                out.append(b7.build_mode5(rot, *[tuple(int(v) for v in c) for c in e], tuple(int(v) for v in rng.randint(0, 256, size=2)), _shifted(b, 2), _shifted(b + 1, 2)))
    return out


def _constant_modes():
    """modes 0..3 and the reserved byte, 64 random payloads each; modes 0..3 also with every higher bit of byte 0 set and clear: 320 blocks"""
    return [bytes(b) for m in (0, 1, 2, 3, 8) for b in b7.blocks_of_mode(m, 64, 90 + m)]


COMPLETE = {"mode7": _mode7_complete, "mode6": _mode6_complete, "mode4": _mode4_complete, "mode5": _mode5_complete, "modes0-3+reserved": _constant_modes}


@pytest.mark.parametrize("name", list(COMPLETE))
def test_complete_per_mode(product, baker, hip, name):
    """the blocks 16 to a row (64 texels wide), device and host entry"""
    raw = COMPLETE[name]()
    assert len(raw) % 16 == 0
    blocks = np.frombuffer(b"".join(raw), np.uint8).reshape(len(raw) // 16, 16, 16)
    w, h = 64, 4 * blocks.shape[0]
    mips = [b7.decode(blocks, w, h)]
    if name == "modes0-3+reserved":
        assert (mips[0][:-16] == 255).all() and (mips[0][-16:] == 0).all()
    else:
        assert (mips[0] != 255).mean() > 0.9 and len(np.unique(mips[0])) > 200
    want = tu.host_blobs(product, baker, mips, CUTOFF, True)
    for device in (True, False):
        src = bu.DeviceBlocks(hip, blocks, lead=16) if device else bu.HostBlocks(blocks, lead=1)
        try:
            _made_and_checked(product, baker, b7.make_desc([src.mip(w, h)], CUTOFF, True), device, mips, CUTOFF, True, want, name + (" device" if device else " host"))
        finally:
            if device:
                src.free()


def test_every_alpha_endpoint_pair_of_mode_5(product, baker, hip):
    """one 1024 x 1024 texture of 65 536 mode-5 blocks, block (a0, a1) at block column a0, block row a1, rotation 0, its alpha indices going through the four
    codes (texel 0: code 0), random colour fields and colour indices.  The expected texels are written down directly from the definition -- every block's
    16 texels are 4 values -- and the reference decoder must give the same before the library is asked."""
    rng = np.random.RandomState(55)
    a0, a1 = np.meshgrid(np.arange(256, dtype=np.uint64), np.arange(256, dtype=np.uint64))        # [row a1, column a0]
    idx = [0, 1, 2, 3] * 4
    alpha_bits = sum(k << (0 if i == 0 else 2 * i - 1) for i, k in enumerate(idx))              # 31 bits from bit 97
    lo = (rng.randint(0, 1 << 32, size=(256, 256)).astype(np.uint64) << np.uint64(32)) | rng.randint(0, 1 << 32, size=(256, 256)).astype(np.uint64)
    hi = (rng.randint(0, 1 << 32, size=(256, 256)).astype(np.uint64) << np.uint64(32)) | rng.randint(0, 1 << 32, size=(256, 256)).astype(np.uint64)
    lo = (lo & ~np.uint64(0xFF)) | np.uint64(0x20)                                                 # mode 5, rot 0
    lo = (lo & np.uint64((1 << 50) - 1)) | (a0 << np.uint64(50)) | ((a1 & np.uint64(63)) << np.uint64(58))
    hi = (hi & np.uint64(((1 << 33) - 1) & ~3)) | (a1 >> np.uint64(6)) | (np.uint64(alpha_bits) << np.uint64(33))   # A1's top 2 bits at 64..65, indices from 97
    blocks = np.ascontiguousarray(np.stack([lo, hi], axis=-1)).view(np.uint8).reshape(256, 256, 16)
    weights = np.array([0, 21, 43, 64], np.int64)[idx].reshape(1, 4, 1, 4)
    e0, e1 = a0.astype(np.int64).reshape(256, 1, 256, 1), a1.astype(np.int64).reshape(256, 1, 256, 1)
    want = (((64 - weights) * e0 + weights * e1 + 32) >> 6).astype(np.uint8).reshape(1024, 1024)
    assert want[4 * 100, 4 * 200] == 200 and want[4 * 100, 4 * 200 + 3] == 100
    assert np.array_equal(b7.decode(blocks, 1024, 1024), want)
    blobs = tu.host_blobs(product, baker, [want], CUTOFF, True)
    for device in (True, False):
        src = bu.DeviceBlocks(hip, blocks) if device else bu.HostBlocks(blocks)
        tex = b7.create(product, baker, b7.make_desc([src.mip(1024, 1024)], CUTOFF, True), device)
        if device:
            src.free()
        try:
            assert _is_unorm8(product, tex)
            tu.check_texture(product, baker, tex, [want], CUTOFF, True, blobs, "mode 5 endpoint pairs")
        finally:
            product.destroy_texture(baker, tex)


MIP_SHAPES = [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("disable_zorder", [True, False])
def test_a_mip_chain_from_independent_allocations(product, baker, hip, device, disable_zorder):
    """64 x 64 down to 1 x 1, every mip its own allocation, pitch (tight, as 0 and spelled out; padded by 16 or 32) and lead"""
    blocks = [b7.random_blocks(w, h, seed=31 + w) for (w, h) in MIP_SHAPES]
    mips = [b7.decode(b, w, h) for b, (w, h) in zip(blocks, MIP_SHAPES)]
    want = tu.host_blobs(product, baker, mips, CUTOFF, disable_zorder)
    if device:
        srcs = [bu.DeviceBlocks(hip, b, pad=16 * (k % 3), lead=16 * (k & 1), tight_pitch_as_zero=(k & 2) == 0) for k, b in enumerate(blocks)]
    else:
        srcs = [bu.HostBlocks(b, pad=(0, 16, 5)[k % 3], lead=k) for k, b in enumerate(blocks)]
    try:
        desc = b7.make_desc([s.mip(w, h) for s, (w, h) in zip(srcs, MIP_SHAPES)], CUTOFF, disable_zorder)
        _made_and_checked(product, baker, desc, device, mips, CUTOFF, disable_zorder, want, "mip chain")
    finally:
        if device:
            for s in srcs:
                s.free()


def test_blocks_produced_on_the_callers_stream_and_overwritten_after_the_call(product, baker, hip):
    """the blocks reach device memory through hipMemcpyAsync from pinned memory on a non-blocking stream, behind copies that keep the stream busy; the call is
    made on that stream with nothing waiting in between, and the source is overwritten as soon as it returns"""
    hip.rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    w, h = 512, 260
    blocks = b7.random_blocks(w, h, seed=77)
    mips = [b7.decode(blocks, w, h)]
    want = tu.host_blobs(product, baker, mips, CUTOFF, True)
    pinned = bu.PinnedBlocks(hip, blocks)
    target = hip.upload(np.full(pinned.nbytes, 0x80, np.uint8))       # holds other bytes (mode 7 blocks) until the copy lands
    busy = [hip.alloc(32 << 20), hip.alloc(32 << 20)]
    assert hip.rt.hipDeviceSynchronize() == 0
    stream = hip.stream_create(non_blocking=True)
    for k in range(8):
        assert hip.rt.hipMemcpyAsync(busy[k & 1], busy[1 - (k & 1)], 32 << 20, 3, stream) == 0
    assert hip.rt.hipMemcpyAsync(target, pinned.base, pinned.nbytes, 1, stream) == 0
    tex = b7.create(product, baker, b7.make_desc([(w, h, 0, target.value)], CUTOFF, True), True, stream=stream)
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


def _alpha_image_blocks():
    """64 x 64 of mode-6 blocks whose alpha endpoints follow a smooth noise, random indices: about half of the texels above the cut-off"""
    rng = np.random.RandomState(12)
    noise = ot.value_noise(5, 16, 16, octaves=2, base_cell=4) * 127
    out = []
    for by in range(16):
        for bx in range(16):
            a = (int(np.clip(noise[by, bx] + 25, 0, 127)), int(np.clip(noise[by, bx] - 25, 0, 127)))
            c = [tuple(int(v) for v in rng.randint(0, 128, size=2)) for _ in range(3)]
            out.append(b7.build_mode6(c[0], c[1], c[2], a, tuple(int(v) for v in rng.randint(0, 2, size=2)), [int(rng.randint(0, 8))] + [int(v) for v in rng.randint(0, 16, size=15)]))
    return np.frombuffer(b"".join(out), np.uint8).reshape(16, 16, 16)


def test_bake_and_resolve_with_a_bc7_made_texture(product, baker, hip):
    """64 x 64, 300 triangles, level 4, 4-state, cut-off 0.5: ommCpuBake and ommxBakeDevice give, byte for byte, what they give with the host-made UNORM8
    texture of the decoded bytes; ommxResolveHits accepts the texture and answers 4000 hits the same way, with and without the micromap"""
    lu.bind(product.dll)
    blocks = _alpha_image_blocks()
    texels = b7.decode(blocks, 64, 64)
    assert texels.dtype == np.uint8 and 0.2 < (texels > 127).mean() < 0.8
    uv, ix = ot.random_triangles(6, 300, 6.0 / 64)
    rng = np.random.default_rng(8)
    hits = np.zeros(4000, lu.HIT)
    hits["prim"] = rng.integers(0, 300, 4000)
    u, v = rng.random(4000, dtype=np.float32), rng.random(4000, dtype=np.float32)
    fold = u + v > 1
    hits["u"], hits["v"] = np.where(fold, 1 - u, u) * np.float32(0.98), np.where(fold, 1 - v, v) * np.float32(0.98)
    src = bu.DeviceBlocks(hip, blocks)
    made = {"blocks": b7.create(product, baker, b7.make_desc([src.mip(64, 64)], CUTOFF), True),
            "bytes": product.create_texture(baker, [texels], alpha_cutoff=CUTOFF)}
    src.free()
    got = {}
    try:
        for name, tex in made.items():
            d = ot.make_desc(tex, uv, ix, 4, addr=ot.WRAP, promo=ot.PROMO_FORCE_OPAQUE)
            host_bake = product.bake(baker, d)
            dev = lu.DeviceBake(product, hip, baker, d, uv, ix)
            try:
                resolved = [lu.resolve_device(product.dll, hip, baker, dev.ddesc, dev.rdesc, hits, flags) for flags in (0, lu.IGNORE_MICROMAP)]
                got[name] = (host_bake, dev.host, resolved)
            finally:
                dev.close()
    finally:
        for tex in made.values():
            product.destroy_texture(baker, tex)
    for x, y in zip(got["blocks"][:2], got["bytes"][:2]):
        assert x.same_as(y), x.diff(y)
        assert x.array_data.size > 0
    for x, y in zip(got["blocks"][2], got["bytes"][2]):
        assert np.array_equal(x, y)
    plain = got["blocks"][2][1]
    assert ((plain & 8) != 0).all() and 0.1 < (plain & 1).mean() < 0.9   # every hit was answered from the texture, and both ways


def test_memory_the_device_cannot_read_is_refused(product, hip):
    """on the device entry, a mip whose LAST byte lies outside its allocation (two rows of blocks with a pitch of 4 GiB less 16 bytes: the first row
    is the allocation's own, the second lies 4 GiB behind it), pageable host memory and a pointer the runtime does not know: INVALID_ARGUMENT with the line, the handle not written, nothing launched, and the
    device still healthy afterwards"""
    msgs = []
    b = product.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    b7.bind(product.dll)
    blocks = b7.random_blocks(64, 64, seed=3)
    pageable = np.zeros(blocks.size + 16, np.uint8)
    off = (-pageable.ctypes.data) % 16
    pageable[off:off + blocks.size] = blocks.reshape(-1)
    good = bu.DeviceBlocks(hip, blocks)
    try:
        for name, mips in (("last byte outside the allocation", [(64, 8, 0xFFFFFFF0, good.ptr)]),
                           ("pageable", [(64, 64, 0, pageable.ctypes.data + off)]), ("unknown", [(64, 64, 0, 0x10000)]),
                           ("pageable mip behind a good one", [good.mip(64, 64), (32, 32, 0, pageable.ctypes.data + off)])):
            del msgs[:]
            out = C.c_void_p(0x1234)
            r = product.dll.ommxCreateTextureBC7Device(b, C.byref(b7.make_desc(mips, CUTOFF)), None, C.byref(out))
            assert r == ot.INVALID_ARGUMENT and out.value == 0x1234, name
            assert len(msgs) == 1 and msgs[0][0] == FATAL and "is not memory the baker's device can read" in msgs[0][1], (name, msgs)
        assert hip.rt.hipDeviceSynchronize() == 0
        # the same baker and blocks, from memory it can read
        mips = [b7.decode(blocks, 64, 64)]
        _made_and_checked(product, b, b7.make_desc([good.mip(64, 64)], CUTOFF, True), True, mips, CUTOFF, True, tu.host_blobs(product, b, mips, CUTOFF, True), "after refusals")
    finally:
        good.free()
        product.destroy_baker(b)
