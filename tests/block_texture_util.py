"""ommxCreateTextureBC / ommxCreateTextureBCDevice (include/omm_mi355x_ext.h): ctypes mirrors of the two structs, the numpy reference decoder of the
alpha of BC1..BC5 blocks -- written from the header's definition, sharing nothing with omm_amd/csrc/block_decode.h, and pinned by
tests/test_block_decode_reference.py --, block images with hostile padding, and the two ways a test hands them to the library."""
import ctypes as C
import struct
import numpy as np
import ommtest as ot

BC1, BC2, BC3, BC4, BC5 = range(5)                  # ommxBlockFormat
FORMATS = [(BC1, 0), (BC2, 0), (BC3, 0), (BC4, 0), (BC5, 0), (BC5, 1)]   # (format, channel)
BLOCK_BYTES = {BC1: 8, BC2: 16, BC3: 16, BC4: 8, BC5: 16}
NAMES = {BC1: "bc1", BC2: "bc2", BC3: "bc3", BC4: "bc4", BC5: "bc5"}


def format_id(fc):
    return NAMES[fc[0]] + (".%d" % fc[1] if fc[0] == BC5 else "")


class BlockTextureMipDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rowPitchInBytes", C.c_uint32), ("data", C.c_void_p)]


class BlockTextureDesc(C.Structure):
    _fields_ = [("format", C.c_int), ("channel", C.c_uint32), ("flags", C.c_int), ("mips", C.POINTER(BlockTextureMipDesc)), ("mipCount", C.c_uint32),
                ("alphaCutoff", C.c_float)]


def bind(dll):
    dll.ommxCreateTextureBC.argtypes = [C.c_void_p, C.POINTER(BlockTextureDesc), C.POINTER(C.c_void_p)]
    dll.ommxCreateTextureBC.restype = C.c_int
    dll.ommxCreateTextureBCDevice.argtypes = [C.c_void_p, C.POINTER(BlockTextureDesc), C.c_void_p, C.POINTER(C.c_void_p)]
    dll.ommxCreateTextureBCDevice.restype = C.c_int
    return dll


def make_desc(fmt, channel, mips, alpha_cutoff=-1.0, disable_zorder=False):
    """mips: [(width, height, rowPitchInBytes, pointer)].  The desc keeps its mip array alive."""
    md = (BlockTextureMipDesc * max(len(mips), 1))()
    for i, (w, h, pitch, ptr) in enumerate(mips):
        md[i].width, md[i].height, md[i].rowPitchInBytes, md[i].data = w, h, pitch, ptr
    d = BlockTextureDesc()
    d.format, d.channel, d.flags, d.mips, d.mipCount, d.alphaCutoff = fmt, channel, (ot.TEXFLAG_DISABLE_ZORDER if disable_zorder else 0), md, len(mips), alpha_cutoff
    d._mips = md
    return d


def create(lib, baker, desc, device, stream=None, expect=ot.SUCCESS):
    bind(lib.dll)
    out = C.c_void_p()
    r = lib.dll.ommxCreateTextureBCDevice(baker, C.byref(desc), stream, C.byref(out)) if device else lib.dll.ommxCreateTextureBC(baker, C.byref(desc), C.byref(out))
    assert r == expect, (r, expect)
    return out if r == ot.SUCCESS else None


# ---- the reference decoder: blocks (..., 8 relevant bytes) -> 16 texels each, texel i = 4 * y + x ----
def _u64(b8):
    b8 = b8.astype(np.uint64)
    return sum(b8[..., k] << np.uint64(8 * k) for k in range(8))


def relevant_bytes(fmt, channel, blocks):
    """(..., block bytes) -> the (..., 8) bytes that hold the alpha"""
    assert blocks.shape[-1] == BLOCK_BYTES[fmt] and (channel == 0 or fmt == BC5)
    return blocks[..., 8 * channel:8 * channel + 8]


def bc1_texels(b8):
    q = _u64(b8)
    c0, c1 = q & np.uint64(0xFFFF), (q >> np.uint64(16)) & np.uint64(0xFFFF)
    code = np.stack([(q >> np.uint64(32 + 2 * i)) & np.uint64(3) for i in range(16)], axis=-1)
    return np.where((c0 <= c1)[..., None] & (code == 3), 0, 255).astype(np.uint8)


def bc2_texels(b8):
    q = _u64(b8)
    return np.stack([(q >> np.uint64(4 * i)) & np.uint64(15) for i in range(16)], axis=-1).astype(np.uint8) * np.uint8(17)


def bc4_fraction(b8):
    """-> (n (..., 16) int64, D (..., 1) int64): the texel is n / D of 255"""
    q = _u64(b8)
    a0, a1 = (q & np.uint64(255)).astype(np.int64)[..., None], ((q >> np.uint64(8)) & np.uint64(255)).astype(np.int64)[..., None]
    k = np.stack([(q >> np.uint64(16 + 3 * i)) & np.uint64(7) for i in range(16)], axis=-1).astype(np.int64)
    six = a0 > a1
    n6 = np.where(k == 0, 7 * a0, np.where(k == 1, 7 * a1, (8 - k) * a0 + (k - 1) * a1))
    n4 = np.where(k == 0, 5 * a0, np.where(k == 1, 5 * a1, np.where(k == 6, 0, np.where(k == 7, 5 * 255, (6 - k) * a0 + (k - 1) * a1))))
    return np.where(six, n6, n4), np.where(six, 7, 5)


def bc4_texels(b8):
    n, d = bc4_fraction(b8)
    return (n.astype(np.float32) / d.astype(np.float32)) * (np.float32(1.0) / np.float32(255.0))   # one fp32 division, one fp32 multiplication


def block_texels(fmt, channel, blocks):
    b8 = relevant_bytes(fmt, channel, blocks)
    return bc1_texels(b8) if fmt == BC1 else bc2_texels(b8) if fmt == BC2 else bc4_texels(b8)


def decode(fmt, channel, blocks, w, h):
    """blocks (ceil(h / 4), ceil(w / 4), block bytes) uint8 -> the (h, w) texels of the texture: uint8 (BC1, BC2) or float32"""
    bh, bw = blocks.shape[:2]
    assert (bh, bw) == ((h + 3) // 4, (w + 3) // 4)
    t = block_texels(fmt, channel, blocks).reshape(bh, bw, 4, 4).transpose(0, 2, 1, 3).reshape(4 * bh, 4 * bw)
    return np.ascontiguousarray(t[:h, :w])


# ---- block images ----
WIDTHS = [1, 3, 4, 5, 8, 13, 16, 17, 63, 64, 65, 252, 255, 256, 257, 260]   # around a block, the aligned / per-texel store paths, the 64 blocks of a wave
HEIGHTS = [1, 3, 4, 5, 7, 8, 64, 65]                                        # around a block, the 4 block rows of a workgroup, the table's 64-row blocks


def shapes():
    """(w, h): every width with two heights and every height with two widths, paired arithmetically"""
    out = []
    for i, w in enumerate(WIDTHS):
        for h in (HEIGHTS[i % 8], HEIGHTS[(5 * i + 3) % 8]):
            if (w, h) not in out:
                out.append((w, h))
    for j, h in enumerate(HEIGHTS):
        for w in (WIDTHS[(5 * j + 1) % 16], WIDTHS[(3 * j + 6) % 16]):
            if (w, h) not in out:
                out.append((w, h))
    return out


def random_blocks(fmt, w, h, seed):
    """every byte random: the colour halves, the other BC5 channel and the codes of texels beyond w / h included"""
    return np.random.RandomState(seed).randint(0, 256, size=((h + 3) // 4, (w + 3) // 4, BLOCK_BYTES[fmt])).astype(np.uint8)


def rows_of(blocks, pad=0):
    """-> (flat uint8 array, row pitch in bytes): the rows of blocks one after the other, `pad` bytes of 0xFF behind each but the last"""
    bh, bw, bb = blocks.shape
    rows = np.full((bh, bw * bb + pad), 0xFF, np.uint8)
    rows[:, :bw * bb] = blocks.reshape(bh, bw * bb)
    flat = rows.reshape(-1)
    return np.ascontiguousarray(flat[:flat.size - pad] if pad else flat), bw * bb + pad


class DeviceBlocks:
    """rows of blocks in device memory, `lead` bytes (a multiple of 8) behind the 256-byte aligned base; .mip(w, h) is the desc's tuple"""

    def __init__(self, hip, blocks, pad=0, lead=0, tight_pitch_as_zero=True):
        flat, pitch = rows_of(blocks, pad)
        self.hip, self.lead, self.nbytes = hip, lead, flat.size
        self.base = hip.upload(np.concatenate([np.full(lead, 0xFF, np.uint8), flat]))
        self.ptr = self.base.value + lead
        self.pitch = 0 if (pad == 0 and tight_pitch_as_zero) else pitch

    def mip(self, w, h):
        return (w, h, self.pitch, self.ptr)

    def free(self):
        if self.base is not None:
            self.hip.free(self.base)
            self.base = None


class HostBlocks:
    """rows of blocks in a numpy array, `lead` bytes behind its start (1: no alignment at all)"""

    def __init__(self, blocks, pad=0, lead=0):
        flat, pitch = rows_of(blocks, pad)
        self.buf = np.empty(flat.size + lead, np.uint8)
        self.buf[:lead] = 0xFF
        self.buf[lead:] = flat
        self.ptr = self.buf.ctypes.data + lead
        self.pitch = 0 if pad == 0 else pitch

    def mip(self, w, h):
        return (w, h, self.pitch, self.ptr)


class PinnedBlocks:
    """rows of blocks in pinned host memory (hipHostMalloc)"""

    def __init__(self, hip, blocks, pad=0):
        flat, pitch = rows_of(blocks, pad)
        hip.rt.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        hip.rt.hipHostFree.argtypes = [C.c_void_p]
        self.hip, self.nbytes = hip, flat.size
        self.base = C.c_void_p()
        assert hip.rt.hipHostMalloc(C.byref(self.base), max(flat.size, 16), 0) == 0
        self.view = np.ctypeslib.as_array(C.cast(self.base, C.POINTER(C.c_uint8)), shape=(flat.size,))
        self.view[:] = flat
        self.ptr = self.base.value
        self.pitch = 0 if pad == 0 else pitch

    def mip(self, w, h):
        return (w, h, self.pitch, self.ptr)

    def free(self):
        if self.base is not None:
            self.view = None
            assert self.hip.rt.hipHostFree(self.base) == 0
            self.base = None


# ---- a DDS file around one mip of blocks (for decoders that read files) ----
FOURCC = {BC1: b"DXT1", BC2: b"DXT3", BC3: b"DXT5", BC4: b"ATI1", BC5: b"ATI2"}


def dds_bytes(fmt, blocks, w, h):
    payload = np.ascontiguousarray(blocks).tobytes()
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000            # caps, height, width, pixel format, linear size
    header = struct.pack("<4s7I44x", b"DDS ", 124, flags, h, w, len(payload), 0, 1)
    header += struct.pack("<2I4s5I", 32, 0x4, FOURCC[fmt], 0, 0, 0, 0, 0)   # pixel format: a FourCC
    header += struct.pack("<5I", 0x1000, 0, 0, 0, 0)      # caps (texture), caps2..4, reserved
    assert len(header) == 128
    return header + payload
