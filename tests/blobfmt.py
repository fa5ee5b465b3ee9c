"""Reader for the reference's serialized bake blobs (test-side only).

Layout restated from /root/reference/libraries/omm-lib/src/serialize_impl.cpp:81-276,351-582 and
texture_impl.h:232-336.  Used to turn the golden blobs embedded in the reference's
test-suite (tests/golden/blobs.json) into bake inputs / expected outputs.
"""
import struct
import numpy as np


def lz4_block_decompress(src, out_size):
    """Plain LZ4 block format (lz4.org block spec)."""
    out = bytearray()
    i, n = 0, len(src)
    while i < n:
        tok = src[i]; i += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = src[i]; i += 1; ll += b
                if b != 255:
                    break
        out += src[i:i + ll]; i += ll
        if i >= n:
            break
        off = src[i] | (src[i + 1] << 8); i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = src[i]; i += 1; ml += b
                if b != 255:
                    break
        ml += 4
        start = len(out) - off
        assert 0 < off <= len(out), "LZ4 match offset outside the output"
        if off >= ml:
            out += out[start:start + ml]
        else:   # overlapping match: the last `off` bytes repeat
            out += (bytes(out[start:]) * (ml // off + 1))[:ml]
    assert len(out) == out_size, (len(out), out_size)
    return bytes(out)


class Reader:
    def __init__(self, data):
        self.d, self.o = data, 0

    def take(self, n):
        b = self.d[self.o:self.o + n]
        assert len(b) == n, "blob truncated"
        self.o += n
        return b

    def fmt(self, f):
        v = struct.unpack_from("<" + f, self.d, self.o)
        self.o += struct.calcsize("<" + f)
        return v[0] if len(v) == 1 else v


def morton_to_xy(i):
    def compact(x):
        x &= 0x55555555
        x = (x | (x >> 1)) & 0x33333333
        x = (x | (x >> 2)) & 0x0F0F0F0F
        x = (x | (x >> 4)) & 0x00FF00FF
        x = (x | (x >> 8)) & 0x0000FFFF
        return x
    return compact(i), compact(i >> 1)


def xy_to_morton(x, y):
    def spread(v):
        v = (v | (v << 8)) & 0x00FF00FF
        v = (v | (v << 4)) & 0x0F0F0F0F
        v = (v | (v << 2)) & 0x33333333
        v = (v | (v << 1)) & 0x55555555
        return v
    return spread(x) | (spread(y) << 1)


def morton_index(w, h):
    """(h, w) array of the Morton-Z index of every texel (xy_to_morton for whole arrays)"""
    def spread(v):
        v = v.astype(np.uint64)
        for s, m in ((8, 0x00FF00FF), (4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555)):
            v = (v | (v << np.uint64(s))) & np.uint64(m)
        return v
    return (spread(np.arange(w))[None, :] | (spread(np.arange(h))[:, None] << np.uint64(1))).astype(np.int64)


def next_pow2(v):
    return 1 << max(0, int(v) - 1).bit_length()


def mip_num_elements(w, h, tiling):
    """texels of a mip's storage slot (texture_impl.cpp:107-117): Morton-Z pads to a power-of-two square"""
    return next_pow2(max(w, h)) ** 2 if tiling == 1 else w * h


def parse_blob(blob, xxh64=None):
    """Returns dict(version=..., inputs=[...], results=[...]).  xxh64(data, seed)->int optionally verifies the digest.
    texture: `mips` are the texels; when the blob carries a summed-area-table section (`has_sat`), `sat[m]` is mip m's table as an
    (h, w) uint32 array -- row-major with stride w in BOTH tilings (texture_impl.cpp:191-220), read at the mip's dataOffsetSAT --
    and `sat_rest[m]` the raw bytes of the remainder of that mip's slot (up to the next mip's offset, or the end of the section);
    `mip_descs[m]` = (w, h, dataOffset, numElements, dataOffsetSAT) and `sat_size` the section's size as stored."""
    r = Reader(blob)
    digest = r.fmt("Q")
    if xxh64 is not None:
        assert xxh64(blob[8:], 42) == digest, "blob digest mismatch"
    major, minor, patch, ver, flags = r.fmt("iiiii")
    decomp = r.fmt("i") if ver >= 2 else 0
    body = blob[r.o:]
    if decomp:
        body = lz4_block_decompress(body, decomp)
    r = Reader(body)
    out = dict(version=(major, minor, patch, ver), flags=flags, inputs=[], results=[])
    for _ in range(r.fmt("i")):
        d = {}
        d["bakeFlags"] = r.fmt("I")
        nm = r.fmt("i")
        mips = [r.fmt("iiffQQQ") for _ in range(nm)]
        tiling = r.fmt("i")
        if ver >= 3:
            texflags, tex_cutoff = r.fmt("I"), r.fmt("f")
        else:
            texflags, tex_cutoff = (0 if tiling == 1 else 1), -1.0
        texfmt = r.fmt("i")
        data = r.take(r.fmt("Q"))
        sat = r.take(r.fmt("Q"))
        px = 4 if texfmt == 1 else 1
        arrays = []
        for (w, h, rw, rh, off, ne, offsat) in mips:
            raw = np.frombuffer(data, np.float32 if texfmt == 1 else np.uint8, count=ne, offset=off)
            a = np.empty((h, w), raw.dtype)
            if tiling == 1:  # Morton-Z internal order
                a[:] = raw[morton_index(w, h)]
            else:
                a[:] = raw.reshape(h, w)
            arrays.append(a)
        sats, rests = [], []
        if len(sat):
            for m, (w, h, rw, rh, off, ne, offsat) in enumerate(mips):
                end = mips[m + 1][6] if m + 1 < nm else len(sat)
                assert offsat + 4 * w * h <= end <= len(sat), "SAT slot of mip %d does not fit its section" % m
                sats.append(np.frombuffer(sat, "<u4", count=w * h, offset=offsat).reshape(h, w))
                rests.append(sat[offsat + 4 * w * h:end])
        d["texture"] = dict(mips=arrays, tiling=tiling, flags=texflags, alphaCutoff=tex_cutoff, format=texfmt, has_sat=len(sat) != 0,
                            sat=sats, sat_rest=rests, sat_size=len(sat), mip_descs=[(m[0], m[1], m[4], m[5], m[6]) for m in mips])
        d["addressingMode"], d["filter"], d["borderAlpha"], d["alphaMode"] = r.fmt("iifi")
        d["texCoordFormat"] = r.fmt("i")
        d["texCoords"] = r.take(r.fmt("Q"))
        d["texCoordStrideInBytes"] = r.fmt("I")
        d["indexFormat"], d["indexCount"] = r.fmt("iI")
        isz = {2: 1, 0: 2, 1: 4}[d["indexFormat"]]
        d["indexBuffer"] = r.take(isz * d["indexCount"])
        d["dynamicSubdivisionScale"], d["rejectionThreshold"], d["alphaCutoff"] = r.fmt("fff")
        d["alphaCutoffLessEqual"], d["alphaCutoffGreater"], d["format"] = r.fmt("iii")
        nf = r.fmt("Q")
        d["formats"] = r.take(4 * nf)
        d["unknownStatePromotion"] = r.fmt("i")
        d["unresolvedTriState"] = r.fmt("i") if ver >= 2 else -4
        d["maxSubdivisionLevel"] = r.fmt("B")
        d["maxArrayDataSize"] = r.fmt("I") if ver >= 4 else 0xFFFFFFFF
        ns = r.fmt("Q")
        d["subdivisionLevels"] = r.take(ns)
        d["maxWorkloadSize"] = r.fmt("Q")
        if d["texture"]["has_sat"] and ver < 3:
            d["texture"]["alphaCutoff"] = d["alphaCutoff"]
        out["inputs"].append(d)
    for _ in range(r.fmt("i")):
        res = {}
        res["arrayData"] = r.take(r.fmt("I"))
        n = r.fmt("I"); res["descArray"] = r.take(8 * n)
        n = r.fmt("I"); res["descArrayHistogram"] = r.take(8 * n)
        res["indexFormat"] = r.fmt("i")
        n = r.fmt("I"); res["indexBuffer"] = r.take({2: 1, 0: 2, 1: 4}[res["indexFormat"]] * n)
        res["indexCount"] = n
        n = r.fmt("I"); res["indexHistogram"] = r.take(8 * n)
        out["results"].append(res)
    assert r.o == len(body), "trailing bytes in blob: %d" % (len(body) - r.o)
    return out
