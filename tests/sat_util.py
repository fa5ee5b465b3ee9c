"""The summed-area table (SAT) of `alpha > cutoff`, pinned directly.

A plain numpy restatement of the table the reference builds per mip (texture_impl.cpp:191-220), the case lists of
test_sat_gpu.py, and the ctypes plumbing that gets a texture's table out of the library: ommCpuSerialize copies every mip's table
off the device into the blob, tests/blobfmt.py reads it back.  test_sat_reference.py checks this module without a GPU.
"""
import ctypes as C
import numpy as np
import blobfmt
import ommtest as ot


# ---- the reference ----
def indicator(tex, cutoff):
    """what the reference's texture load feeds to `>`, in float32: the texel itself (FP32) or byte * (1 / 255) (UNORM8)"""
    c = np.float32(cutoff)
    with np.errstate(invalid="ignore"):   # NaN texels compare false
        if tex.dtype == np.float32:
            return tex > c
        assert tex.dtype == np.uint8
        return tex.astype(np.float32) * (np.float32(1) / np.float32(255)) > c


def sat_reference(tex, cutoff):
    """(h, w) uint32: inclusive sums of the indicator over [0..y] x [0..x]"""
    s = indicator(tex, cutoff).astype(np.uint64).cumsum(axis=0, dtype=np.uint64).cumsum(axis=1, dtype=np.uint64)
    assert int(s[-1, -1]) < 2 ** 32
    return s.astype(np.uint32)


def sat_layout(shapes, tiling):
    """[(dataOffsetSAT, slot bytes)] per mip and the section's size (texture_impl.cpp:105,127-130): 4 bytes per element of the
    mip's storage (Morton-Z: the padded power-of-two square), every slot starting on a 64-byte boundary"""
    out, size = [], 0
    for (h, w) in shapes:
        start = size
        size = (size + 4 * blobfmt.mip_num_elements(w, h, tiling) + 63) & ~63
        out.append((start, size - start))
    return out, size


def ulp_up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf), dtype=np.float32)


def ulp_down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf), dtype=np.float32)


# ---- cases ----
WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513]
HEIGHTS = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200, 257]
BLOCK_EDGES = [63, 64, 65, 127, 128, 129]    # around the 64-texel chunks of the row pass and the 64-row blocks of the column pass
BIG_SHAPES = [(1, 4097), (4097, 1), (1025, 1030)]   # (w, h); DisableZOrder only
ZORDER_MAX = 300                                # Morton-Z pads to next_pow2(max(w, h))^2 elements per slot


def shapes():
    """(w, h): every width with h = 1, an edge of the 64-row block and one more height; every height with w = 1, an edge of the
    64-texel chunk and one more width (the pairing is arithmetic, not tuned); then the three big ones"""
    out = []
    for i, w in enumerate(WIDTHS):
        for h in (1, BLOCK_EDGES[i % 6], HEIGHTS[(5 * i + 3) % len(HEIGHTS)], HEIGHTS[(7 * i + 8) % len(HEIGHTS)]):
            if (w, h) not in out:
                out.append((w, h))
    for j, h in enumerate(HEIGHTS):
        for w in (1, BLOCK_EDGES[(j + 3) % 6], WIDTHS[(5 * j + 1) % len(WIDTHS)], WIDTHS[(7 * j + 6) % len(WIDTHS)]):
            if (w, h) not in out:
                out.append((w, h))
    return out


def tilings(w, h):
    """DisableZOrder values a shape runs with"""
    return [True, False] if max(w, h) <= ZORDER_MAX else [True]


CUTOFF = 0.5


def contents(w, h, fp32, seed):
    """[(name, texture)] for cut-off 0.5: random at density 0.5, all above, all below, a single texel above at the corners and on
    both sides of the 64 / 256 boundaries where the shape has them"""
    rng = np.random.RandomState(seed)
    lo, hi = (np.float32(0.25), np.float32(0.75)) if fp32 else (np.uint8(127), np.uint8(128))   # 127/255 < 0.5 < 128/255
    dt = np.float32 if fp32 else np.uint8
    out = [("random", np.where(rng.rand(h, w) < 0.5, hi, lo).astype(dt)),
           ("all_above", np.full((h, w), hi, dt)), ("all_below", np.full((h, w), lo, dt))]
    spots = [(0, 0), (w - 1, h - 1), (63, 63), (64, 64), (255, h // 2), (256, h // 2), (255, h - 1), (256, 0)]
    for (x, y) in dict.fromkeys(spots):
        if x < w and y < h:
            t = np.full((h, w), lo, dt)
            t[y, x] = hi
            out.append(("single_%d_%d" % (x, y), t))
    return out


UNORM8_KS = [0, 1, 127, 128, 254, 255]


def unorm8_cutoffs():
    """float32 cut-offs: k * (1 / 255) for the k above, one ulp to either side of each, 0.0 and 1.0.  (One ulp below k = 0 is
    negative: a texture created with it has no table.)"""
    out = []
    for k in UNORM8_KS:
        c = np.float32(k) * (np.float32(1) / np.float32(255))
        out += [ulp_down(c), c, ulp_up(c)]
    out += [np.float32(0.0), np.float32(1.0)]
    return out


def fp32_special_cases():
    """[(cutoff, texture)]: NaN, +-inf, -0.0 / +0.0, texels equal to the cut-off and one ulp to either side, among ordinary values"""
    out = []
    for n, c in enumerate([np.float32(0.0), np.float32(0.5), np.float32(0.3), np.float32(1.0)]):
        vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, c, ulp_up(c), ulp_down(c), 0.1, 0.9, -1.0, 2.0,
                         np.float32(1e-45), -np.float32(1e-45)], np.float32)
        rng = np.random.RandomState(100 + n)
        out.append((c, vals[rng.randint(0, vals.size, size=(67, 131))]))
    return out


# ---- product side: texture -> blob -> tables ----
class BlobDesc(C.Structure):
    _fields_ = [("data", C.c_void_p), ("size", C.c_uint64)]


class DeserializedDesc(C.Structure):
    _fields_ = [("flags", C.c_int), ("numInputDescs", C.c_int), ("inputDescs", C.POINTER(ot.BakeInputDesc)),
                ("numResultDescs", C.c_int), ("resultDescs", C.POINTER(ot.BakeResultDesc))]


def bind(dll):
    dll.ommCpuSerialize.argtypes = [C.c_void_p, C.POINTER(DeserializedDesc), C.POINTER(C.c_void_p)]
    dll.ommCpuGetSerializedResultDesc.argtypes = [C.c_void_p, C.POINTER(C.POINTER(BlobDesc))]
    dll.ommCpuDestroySerializedResult.argtypes = [C.c_void_p]
    dll.ommCpuDeserialize.argtypes = [C.c_void_p, C.POINTER(BlobDesc), C.POINTER(C.c_void_p)]
    dll.ommCpuGetDeserializedDesc.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DeserializedDesc))]
    dll.ommCpuDestroyDeserializedResult.argtypes = [C.c_void_p]


_TRI_UV = np.array([[0.1, 0.1], [0.9, 0.1], [0.1, 0.9]], np.float32)
_TRI_IX = np.arange(3, dtype=np.uint32)


def serialize_inputs(lib, baker, descs, compress):
    """ommCpuSerialize of input descs alone (no result descs) -> blob bytes"""
    bind(lib.dll)
    arr = (ot.BakeInputDesc * len(descs))(*descs)
    dd = DeserializedDesc(compress, len(descs), arr, 0, None)
    sh = C.c_void_p()
    assert lib.dll.ommCpuSerialize(baker, C.byref(dd), C.byref(sh)) == ot.SUCCESS
    pb = C.POINTER(BlobDesc)()
    assert lib.dll.ommCpuGetSerializedResultDesc(sh, C.byref(pb)) == ot.SUCCESS
    blob = C.string_at(pb.contents.data, pb.contents.size)
    assert lib.dll.ommCpuDestroySerializedResult(sh) == ot.SUCCESS
    return blob


def serialize_texture(lib, baker, tex, compress):
    """blob of one level-0 input over one triangle that uses the texture"""
    return serialize_inputs(lib, baker, [ot.make_desc(tex, _TRI_UV, _TRI_IX, 0)], compress)


def check_tables(parsed_texture, mips, cutoff, disable_zorder):
    """every assertion on the SAT section of one parsed texture against the numpy reference"""
    t = parsed_texture
    assert t["tiling"] == (0 if disable_zorder else 1)
    assert np.float32(t["alphaCutoff"]) == np.float32(cutoff)
    if np.float32(cutoff) < 0:
        assert not t["has_sat"] and t["sat_size"] == 0 and t["sat"] == []
        return
    layout, size = sat_layout([m.shape for m in mips], t["tiling"])
    assert t["has_sat"] and t["sat_size"] == size, (t["sat_size"], size)
    assert len(t["sat"]) == len(mips)
    for m, tex in enumerate(mips):
        h, w = tex.shape
        assert np.array_equal(t["mips"][m], tex, equal_nan=tex.dtype == np.float32), "texels of mip %d" % m
        assert t["mip_descs"][m][3] == blobfmt.mip_num_elements(w, h, t["tiling"])
        assert t["mip_descs"][m][4] == layout[m][0] and layout[m][0] % 64 == 0, (m, t["mip_descs"][m], layout[m])
        want, got = sat_reference(tex, cutoff), t["sat"][m]
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            y, x = bad[0]
            raise AssertionError("SAT of mip %d (%dx%d): %d entries differ, first at (x=%d, y=%d): %d, reference %d"
                                 % (m, w, h, len(bad), x, y, got[y, x], want[y, x]))
        rest = t["sat_rest"][m]
        assert len(rest) == layout[m][1] - 4 * w * h
        assert rest.count(0) == len(rest), "non-zero bytes behind the table in the slot of mip %d" % m


def tables_of(lib, baker, mips, cutoff, disable_zorder, compress_modes=(0, 1), xxh64=None):
    """create the texture, serialize with each compress flag, check every table; returns the last blob"""
    tex = lib.create_texture(baker, mips, alpha_cutoff=float(np.float32(cutoff)), disable_zorder=disable_zorder)
    blob = None
    try:
        for compress in compress_modes:
            blob = serialize_texture(lib, baker, tex, compress)
            parsed = blobfmt.parse_blob(blob, xxh64=xxh64)
            assert len(parsed["inputs"]) == 1 and parsed["flags"] == compress
            check_tables(parsed["inputs"][0]["texture"], mips, cutoff, disable_zorder)
    finally:
        lib.destroy_texture(baker, tex)
    return blob
