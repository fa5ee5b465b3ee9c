"""ommxCreateTextureDevice (include/omm_mi355x_ext.h): ctypes mirrors of its two structs, interleaved source images built in numpy with hostile
neighbours, and the comparison every GPU test of it makes -- the serialized blob of the device-made texture equals the blob of the texture
ommCpuCreateTexture makes from the numpy-extracted channel, and its tables equal the numpy reference of tests/sat_util.py."""
import ctypes as C
import numpy as np
import blobfmt
import ommtest as ot
import sat_util as su

UNORM8, FP32, FP16 = 0, 1, 2                       # ommxTexelFormat
CHANNEL_BYTES = {UNORM8: 1, FP32: 4, FP16: 2}
SOURCE_DTYPE = {UNORM8: np.uint8, FP32: np.uint32, FP16: np.uint16}   # sources are assembled as bit patterns


class DeviceTextureMipDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rowPitchInBytes", C.c_uint32), ("deviceData", C.c_void_p)]


class DeviceTextureDesc(C.Structure):
    _fields_ = [("channelFormat", C.c_int), ("pixelStrideInBytes", C.c_uint32), ("channelOffsetInBytes", C.c_uint32), ("flags", C.c_int),
                ("mips", C.POINTER(DeviceTextureMipDesc)), ("mipCount", C.c_uint32), ("alphaCutoff", C.c_float)]


def bind(dll):
    dll.ommxCreateTextureDevice.argtypes = [C.c_void_p, C.POINTER(DeviceTextureDesc), C.c_void_p, C.POINTER(C.c_void_p)]
    dll.ommxCreateTextureDevice.restype = C.c_int
    return dll


def make_desc(fmt, stride, offset, mips, alpha_cutoff=-1.0, disable_zorder=False):
    """mips: [(width, height, rowPitchInBytes, pointer)].  The desc keeps its mip array alive."""
    md = (DeviceTextureMipDesc * max(len(mips), 1))()
    for i, (w, h, pitch, ptr) in enumerate(mips):
        md[i].width, md[i].height, md[i].rowPitchInBytes, md[i].deviceData = w, h, pitch, ptr
    d = DeviceTextureDesc()
    d.channelFormat, d.pixelStrideInBytes, d.channelOffsetInBytes = fmt, stride, offset
    d.flags, d.mips, d.mipCount, d.alphaCutoff = (ot.TEXFLAG_DISABLE_ZORDER if disable_zorder else 0), md, len(mips), alpha_cutoff
    d._mips = md
    return d


# ---- cases ----
WIDTHS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513]     # around the 4 / 8 / 16-texel groups, the 64-lane rows of a workgroup and its 256 lanes
HEIGHTS = [1, 3, 4, 5, 64, 65]                                       # around the 4 rows of a workgroup and the 64-row blocks of the table's column pass


def shapes():
    """(w, h): every width with two heights and every height with two widths, paired arithmetically"""
    out = []
    for i, w in enumerate(WIDTHS):
        for h in (HEIGHTS[i % 6], HEIGHTS[(5 * i + 3) % 6]):
            if (w, h) not in out:
                out.append((w, h))
    for j, h in enumerate(HEIGHTS):
        for w in (WIDTHS[(5 * j + 1) % 14], WIDTHS[(3 * j + 6) % 14]):
            if (w, h) not in out:
                out.append((w, h))
    return out


# (format, pixel stride, channel offset): UNORM8 with every stride up to RGBA8 and every offset; FP16 / FP32 packed and as the first / last channel of RGBA
LAYOUTS = ([(UNORM8, s, o) for s in (1, 2, 3, 4) for o in range(s)] +
           [(FP16, 2, 0), (FP16, 8, 0), (FP16, 8, 6)] + [(FP32, 4, 0), (FP32, 16, 0), (FP32, 16, 12)])


def layout_id(layout):
    return "%s_s%d_o%d" % ({UNORM8: "unorm8", FP32: "fp32", FP16: "fp16"}[layout[0]], layout[1], layout[2])


def channel_bits(fmt, w, h, seed):
    """(h, w) bit patterns of a channel whose values straddle the cut-off 0.5: every byte value (UNORM8), floats of [0, 1) (FP32), every finite half
    bit pattern -- both signs, subnormals, zeros (FP16; NaN and inf have tests of their own)"""
    rng = np.random.RandomState(seed)
    if fmt == UNORM8:
        return rng.randint(0, 256, size=(h, w)).astype(np.uint8)
    if fmt == FP32:
        return rng.rand(h, w).astype(np.float32).view(np.uint32)
    bits = rng.randint(0, 1 << 16, size=(h, w)).astype(np.uint16)
    return np.where((bits & 0x7C00) == 0x7C00, bits & 0x83FF | 0x3800, bits).astype(np.uint16)   # exponent 31 -> 14: [0.5, 1)


def texels_of(fmt, bits):
    """what the texture must hold for a channel of these bit patterns: the bytes, the fp32 bit patterns, numpy's float16 -> float32"""
    if fmt == UNORM8:
        return bits
    if fmt == FP32:
        return bits.view(np.float32)
    return bits.view(np.float16).astype(np.float32)


def interleave(fmt, stride, offset, bits, pad_elems=0, lead_pixels=0):
    """-> (flat array of SOURCE_DTYPE[fmt], byte offset of the first pixel, row pitch in bytes).  The channel's bits sit at `offset` of every `stride`-byte
    pixel; everything else -- the other channels, `pad_elems` channel-sized elements behind each row, `lead_pixels` pixels in front of the image -- is hostile:
    the complement of the pixel's alpha for UNORM8 (a misread byte flips the indicator), NaN bit patterns for the float formats."""
    cb = CHANNEL_BYTES[fmt]
    h, w = bits.shape
    per_pixel, ch = stride // cb, offset // cb
    row_elems = w * per_pixel + pad_elems
    if fmt == UNORM8:
        img = np.repeat((255 - bits)[:, :, None], per_pixel, axis=2)
        pad = np.repeat((255 - bits[:, -1:]), pad_elems, axis=1)
        hostile_lead = np.full(lead_pixels * per_pixel, 255 - bits[0, 0], np.uint8)
    else:
        nan = np.uint32(0x7FC00001) if fmt == FP32 else np.uint16(0x7E01)
        k = np.arange(h * w * per_pixel).reshape(h, w, per_pixel)
        img = (nan | (k % 251).astype(SOURCE_DTYPE[fmt]) | ((k & 1) << (8 * cb - 1)).astype(SOURCE_DTYPE[fmt])).astype(SOURCE_DTYPE[fmt])   # NaNs of both signs
        pad = np.full((h, pad_elems), nan, SOURCE_DTYPE[fmt])
        hostile_lead = np.full(lead_pixels * per_pixel, nan, SOURCE_DTYPE[fmt])
    img = img.astype(SOURCE_DTYPE[fmt])
    img[:, :, ch] = bits
    rows = np.concatenate([img.reshape(h, w * per_pixel), pad.astype(SOURCE_DTYPE[fmt])], axis=1)
    assert rows.shape == (h, row_elems)
    flat = np.concatenate([hostile_lead.astype(SOURCE_DTYPE[fmt]), rows.reshape(-1)])
    return np.ascontiguousarray(flat), lead_pixels * stride, row_elems * cb


def extract(fmt, stride, offset, flat, first, pitch, w, h):
    """the channel back out of an interleaved source, by plain indexing (checks interleave itself)"""
    raw = flat.view(np.uint8)
    cb = CHANNEL_BYTES[fmt]
    idx = first + np.arange(h)[:, None, None] * pitch + np.arange(w)[None, :, None] * stride + offset + np.arange(cb)[None, None, :]
    return np.ascontiguousarray(raw[idx]).view(SOURCE_DTYPE[fmt]).reshape(h, w)


class Source:
    """an interleaved image in device memory; .mip is its (width, height, rowPitchInBytes, pointer)"""

    def __init__(self, hip, fmt, stride, offset, bits, pad_elems=0, lead_pixels=0, tight_pitch_as_zero=True):
        flat, first, pitch = interleave(fmt, stride, offset, bits, pad_elems, lead_pixels)
        h, w = bits.shape
        assert np.array_equal(extract(fmt, stride, offset, flat, first, pitch, w, h), bits)
        self.hip, self.nbytes = hip, flat.nbytes
        self.base = hip.upload(flat)
        self.mip = (w, h, 0 if (pad_elems == 0 and tight_pitch_as_zero) else pitch, self.base.value + first)

    def free(self):
        if self.base is not None:
            self.hip.free(self.base)
            self.base = None


def create(lib, baker, desc, stream=None, expect=ot.SUCCESS):
    bind(lib.dll)
    out = C.c_void_p()
    r = lib.dll.ommxCreateTextureDevice(baker, C.byref(desc), stream, C.byref(out))
    assert r == expect, (r, expect)
    return out if r == ot.SUCCESS else None


def host_blobs(lib, baker, mips, cutoff, disable_zorder, cache=None, key=None):
    """{compress: blob} of the texture ommCpuCreateTexture makes from `mips` (host arrays); its tables are checked against the numpy reference once"""
    if cache is not None and key in cache:
        return cache[key]
    tex = lib.create_texture(baker, mips, alpha_cutoff=float(np.float32(cutoff)), disable_zorder=disable_zorder)
    try:
        blobs = {c: su.serialize_texture(lib, baker, tex, c) for c in (0, 1)}
    finally:
        lib.destroy_texture(baker, tex)
    su.check_tables(blobfmt.parse_blob(blobs[0])["inputs"][0]["texture"], mips, cutoff, disable_zorder)
    if cache is not None:
        cache[key] = blobs
    return blobs


def check_texture(lib, baker, tex, mips, cutoff, disable_zorder, want_blobs, what=""):
    """the device-made texture `tex`: both blobs equal the host-made texture's, and its tables equal the numpy reference"""
    for compress in (0, 1):
        blob = su.serialize_texture(lib, baker, tex, compress)
        if compress == 0:
            su.check_tables(blobfmt.parse_blob(blob)["inputs"][0]["texture"], mips, cutoff, disable_zorder)
        assert blob == want_blobs[compress], "%s: blob (compress %d) differs from the host-made texture's" % (what, compress)
