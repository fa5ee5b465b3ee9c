"""ommxCreateTextureBC7 / ommxCreateTextureBC7Device (include/omm_mi355x_ext.h): the ctypes mirror of the desc, a reference decoder of the alpha of BC7
blocks -- written from the header's definition in plain Python integers and numpy, sharing nothing with omm_amd/csrc/bc7_decode.h, and pinned by
tests/test_bc7_decode_reference.py --, a builder that packs a block from named fields, and block images whose modes are FORCED: a block of random
bytes has one of the modes 4..7, the only ones with an alpha, 6 % of the time, and 97.7 % of random texels decode to 255.  The mips of a desc are
ommxBlockTextureMipDesc (tests/block_texture_util.py), as are the ways a test hands blocks to the library."""
import ctypes as C
import struct
import numpy as np
import ommtest as ot
import block_texture_util as bu


class BC7TextureDesc(C.Structure):
    _fields_ = [("flags", C.c_int), ("mips", C.POINTER(bu.BlockTextureMipDesc)), ("mipCount", C.c_uint32), ("alphaCutoff", C.c_float)]


def bind(dll):
    dll.ommxCreateTextureBC7.argtypes = [C.c_void_p, C.POINTER(BC7TextureDesc), C.POINTER(C.c_void_p)]
    dll.ommxCreateTextureBC7.restype = C.c_int
    dll.ommxCreateTextureBC7Device.argtypes = [C.c_void_p, C.POINTER(BC7TextureDesc), C.c_void_p, C.POINTER(C.c_void_p)]
    dll.ommxCreateTextureBC7Device.restype = C.c_int
    return dll


def make_desc(mips, alpha_cutoff=-1.0, disable_zorder=False):
    """mips: [(width, height, rowPitchInBytes, pointer)].  The desc keeps its mip array alive."""
    md = (bu.BlockTextureMipDesc * max(len(mips), 1))()
    for i, (w, h, pitch, ptr) in enumerate(mips):
        md[i].width, md[i].height, md[i].rowPitchInBytes, md[i].data = w, h, pitch, ptr
    d = BC7TextureDesc()
    d.flags, d.mips, d.mipCount, d.alphaCutoff = (ot.TEXFLAG_DISABLE_ZORDER if disable_zorder else 0), md, len(mips), alpha_cutoff
    d._mips = md
    return d


def create(lib, baker, desc, device, stream=None, expect=ot.SUCCESS):
    bind(lib.dll)
    out = C.c_void_p()
    r = lib.dll.ommxCreateTextureBC7Device(baker, C.byref(desc), stream, C.byref(out)) if device else lib.dll.ommxCreateTextureBC7(baker, C.byref(desc), C.byref(out))
    assert r == expect, (r, expect)
    return out if r == ot.SUCCESS else None


# ---- the two tables of the format (the header's text) ----
MASK = [int(s, 16) for s in """
CCCC 8888 EEEE ECC8 C880 FEEC FEC8 EC80 C800 FFEC FE80 E800 FFE8 FF00 FFF0 F000
F710 008E 7100 08CE 008C 7310 3100 8CCE 088C 3110 6666 366C 17E8 0FF0 718E 399C
AAAA F0F0 5A5A 33CC 3C3C 55AA 9696 A55A 73CE 13C8 324C 3BDC 6996 C33C 9966 0660
0272 04E4 4E40 2720 C936 936C 39C6 639C 9336 9CC6 817E E718 CCF0 0FCC 7744 EE22""".split()]
ANCHOR = [int(s) for s in """
15 15 15 15 15 15 15 15  15 15 15 15 15 15 15 15  15  2  8  2  2  8  8 15   2  8  2  2  8  8  2  2
15 15  6  8  2  8 15 15   2  8  2  2  2 15 15  6   6  2  6  8 15 15  2  2  15 15 15 15 15  2  2 15""".split()]
WEIGHTS = {2: [0, 21, 43, 64], 3: [0, 9, 18, 27, 37, 46, 55, 64], 4: [0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64]}


# ---- the reference decoder: one block at a time, Python integers ----
def _bits(q, pos, n):
    return (q >> pos) & ((1 << n) - 1)


def _widen(v, n):
    return v if n == 8 else ((v << (8 - n)) | (v >> (2 * n - 8)))


def _indices(q, pos, n, anchors):
    """sixteen n-bit indices from bit `pos`; the texels in `anchors` have n - 1 bits"""
    out = []
    for i in range(16):
        k = n - 1 if i in anchors else n
        out.append(_bits(q, pos, k))
        pos += k
    return out, pos


def _lerp(e0, e1, w):
    return ((64 - w) * e0 + w * e1 + 32) >> 6


def mode_of(byte0):
    """0..7, or 8 for the reserved byte 0"""
    byte0 = int(byte0)
    return 8 if byte0 == 0 else (byte0 & -byte0).bit_length() - 1


def block_alpha(block):
    """16 bytes -> the 16 alpha bytes of the block, texel i = 4 * y + x"""
    raw = bytes(bytearray(block))
    assert len(raw) == 16
    q = int.from_bytes(raw, "little")
    m = mode_of(raw[0])
    if m == 8:
        return [0] * 16
    if m < 4:
        return [255] * 16
    if m == 4:
        rot, idx_mode = _bits(q, 5, 2), _bits(q, 7, 1)
        i2, end2 = _indices(q, 50, 2, (0,))
        i3, end3 = _indices(q, 81, 3, (0,))
        assert (end2, end3) == (81, 128)
        colour_idx, colour_n, alpha_idx, alpha_n = (i2, 2, i3, 3) if idx_mode == 0 else (i3, 3, i2, 2)
        if rot == 0:
            e0, e1, idx, n = _widen(_bits(q, 38, 6), 6), _widen(_bits(q, 44, 6), 6), alpha_idx, alpha_n
        else:
            p = 8 + 10 * (rot - 1)
            e0, e1, idx, n = _widen(_bits(q, p, 5), 5), _widen(_bits(q, p + 5, 5), 5), colour_idx, colour_n
        return [_lerp(e0, e1, WEIGHTS[n][k]) for k in idx]
    if m == 5:
        rot = _bits(q, 6, 2)
        ci, endc = _indices(q, 66, 2, (0,))
        ai, enda = _indices(q, 97, 2, (0,))
        assert (endc, enda) == (97, 128)
        if rot == 0:
            e0, e1, idx = _bits(q, 50, 8), _bits(q, 58, 8), ai
        else:
            p = 8 + 14 * (rot - 1)
            e0, e1, idx = _widen(_bits(q, p, 7), 7), _widen(_bits(q, p + 7, 7), 7), ci
        return [_lerp(e0, e1, WEIGHTS[2][k]) for k in idx]
    if m == 6:
        e0, e1 = (_bits(q, 49, 7) << 1) | _bits(q, 63, 1), (_bits(q, 56, 7) << 1) | _bits(q, 64, 1)
        idx, end = _indices(q, 65, 4, (0,))
        assert end == 128
        return [_lerp(e0, e1, WEIGHTS[4][k]) for k in idx]
    part = _bits(q, 8, 6)
    e = [_widen((_bits(q, 74 + 5 * k, 5) << 1) | _bits(q, 94 + k, 1), 6) for k in range(4)]   # subset 0 endpoint 0, 1; subset 1 endpoint 0, 1
    idx, end = _indices(q, 98, 2, (0, ANCHOR[part]))
    assert end == 128
    out = []
    for i in range(16):
        s = (MASK[part] >> i) & 1
        out.append(_lerp(e[2 * s], e[2 * s + 1], WEIGHTS[2][idx[i]]))
    return out


def block_texels(blocks):
    """(..., 16) uint8 -> (..., 16) uint8"""
    flat = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
    out = np.array([block_alpha(b.tobytes()) for b in flat], np.uint8).reshape(-1, 16)
    return out.reshape(blocks.shape[:-1] + (16,))


def decode(blocks, w, h):
    """blocks (ceil(h / 4), ceil(w / 4), 16) uint8 -> the (h, w) uint8 texels of the texture"""
    bh, bw = blocks.shape[:2]
    assert (bh, bw) == ((h + 3) // 4, (w + 3) // 4)
    t = block_texels(blocks).reshape(bh, bw, 4, 4).transpose(0, 2, 1, 3).reshape(4 * bh, 4 * bw)
    return np.ascontiguousarray(t[:h, :w])


# ---- a block from named fields ----
def _pack(fields):
    q, pos = 0, 0
    for value, n in fields:
        assert 0 <= value < (1 << n), (value, n)
        q |= value << pos
        pos += n
    assert pos == 128, pos
    return q.to_bytes(16, "little")


def _index_fields(idx, n, anchors):
    assert len(idx) == 16
    return [(v, n - 1 if i in anchors else n) for i, v in enumerate(idx)]


def build_mode4(rot, idx_mode, r, g, b, a, idx2, idx3):
    """r, g, b: pairs of 5-bit endpoints; a: a pair of 6-bit ones; idx2 / idx3: the sixteen 2-bit / 3-bit indices (texel 0: one bit less)"""
    f = [(1 << 4, 5), (rot, 2), (idx_mode, 1)] + [(v, 5) for c in (r, g, b) for v in c] + [(a[0], 6), (a[1], 6)]
    return _pack(f + _index_fields(idx2, 2, (0,)) + _index_fields(idx3, 3, (0,)))


def build_mode5(rot, r, g, b, a, colour_idx, alpha_idx):
    """r, g, b: pairs of 7-bit endpoints; a: a pair of 8-bit ones; the two sets of sixteen 2-bit indices (texel 0: 1 bit)"""
    f = [(1 << 5, 6), (rot, 2)] + [(v, 7) for c in (r, g, b) for v in c] + [(a[0], 8), (a[1], 8)]
    return _pack(f + _index_fields(colour_idx, 2, (0,)) + _index_fields(alpha_idx, 2, (0,)))


def build_mode6(r, g, b, a, p, idx):
    """r, g, b, a: pairs of 7-bit endpoints; p: the two P bits; sixteen 4-bit indices (texel 0: 3 bits)"""
    f = [(1 << 6, 7)] + [(v, 7) for c in (r, g, b, a) for v in c] + [(p[0], 1), (p[1], 1)]
    return _pack(f + _index_fields(idx, 4, (0,)))


def build_mode7(part, r, g, b, a, p, idx):
    """r, g, b, a: four 5-bit endpoints each (subset 0 endpoint 0, 1, subset 1 endpoint 0, 1); p: the four P bits in that order; sixteen 2-bit
    indices (texel 0 and texel ANCHOR[part]: 1 bit)"""
    f = [(1 << 7, 8), (part, 6)] + [(v, 5) for c in (r, g, b, a) for v in c] + [(v, 1) for v in p]
    return _pack(f + _index_fields(idx, 2, (0, ANCHOR[part])))


# ---- block images with forced modes ----
def force_mode(blocks, modes):
    """blocks (..., 16) uint8, modes (...) in 0..8 (8: the reserved byte 0) -> the blocks with byte 0 rewritten; every other bit stays"""
    out = np.array(blocks, np.uint8)
    m = np.asarray(modes).astype(np.int64)
    low = (np.int64(1) << np.minimum(m + 1, 8)) - 1
    b0 = (out[..., 0].astype(np.int64) & (0xFF ^ low)) | (np.int64(1) << np.minimum(m, 7))
    out[..., 0] = np.where(m == 8, 0, b0).astype(np.uint8)
    return out


def forced_modes(count, seed):
    """the modes of `count` blocks: 8 or more -> at least half in modes 4..7, all four present, the rest modes 0..3 with exactly one reserved block,
    shuffled; fewer -> modes 4..7 in turn, starting by seed"""
    if count < 8:
        return np.array([4 + (seed + k) % 4 for k in range(count)])
    rng = np.random.RandomState(seed ^ 0x5EED)
    alpha = (count + 1) // 2 + count // 8
    modes = np.concatenate([4 + (np.arange(alpha) + seed) % 4, rng.randint(0, 4, size=count - alpha - 1), [8]])
    rng.shuffle(modes)
    return modes


def random_blocks(w, h, seed):
    """every byte random but for the mode bits of byte 0: the colour fields and the index bits of texels beyond w / h included"""
    bh, bw = (h + 3) // 4, (w + 3) // 4
    raw = np.random.RandomState(seed).randint(0, 256, size=(bh, bw, 16)).astype(np.uint8)
    return force_mode(raw, forced_modes(bh * bw, seed).reshape(bh, bw))


def blocks_of_mode(mode, count, seed):
    """(count, 16): random blocks, all of one mode (8: reserved)"""
    raw = np.random.RandomState(seed).randint(0, 256, size=(count, 16)).astype(np.uint8)
    return force_mode(raw, np.full(count, mode))


# ---- a DDS file (DX10 header, DXGI_FORMAT_BC7_UNORM) around one mip of blocks, for decoders that read files ----
def dds_bytes(blocks, w, h):
    payload = np.ascontiguousarray(blocks).tobytes()
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000            # caps, height, width, pixel format, linear size
    header = struct.pack("<4s7I44x", b"DDS ", 124, flags, h, w, len(payload), 0, 1)
    header += struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)
    header += struct.pack("<5I", 0x1000, 0, 0, 0, 0)
    assert len(header) == 128
    return header + struct.pack("<5I", 98, 3, 0, 1, 0) + payload   # DXGI_FORMAT_BC7_UNORM, TEXTURE2D, misc, array size, misc2
