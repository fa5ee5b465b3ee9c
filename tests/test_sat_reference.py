"""No GPU: the numpy reference of the summed-area table (tests/sat_util.py), the case lists of test_sat_gpu.py and the SAT fields
of the blob parser (tests/blobfmt.py), each held to something that is not itself."""
import os
import struct
import subprocess
import numpy as np
import pytest
import blobfmt
import sat_util as su
import ommtest as ot
from test_golden_blob import BLOBS

ROOT = ot.ROOT


def loops_sat(tex, cutoff):
    """texture_impl.cpp:191-220 as written there: indicator, running sum along x, then along y, in uint32"""
    h, w = tex.shape
    c = np.float32(cutoff)
    s = np.zeros((h, w), np.uint32)
    for j in range(h):
        for i in range(w):
            a = tex[j, i] if tex.dtype == np.float32 else np.float32(tex[j, i]) * (np.float32(1) / np.float32(255))
            s[j, i] = 1 if a > c else 0
    for j in range(h):
        for i in range(1, w):
            s[j, i] += s[j, i - 1]
    for j in range(1, h):
        for i in range(w):
            s[j, i] += s[j - 1, i]
    return s


def test_numpy_reference_is_the_three_loops():
    rng = np.random.RandomState(1)
    for (w, h) in [(1, 1), (1, 9), (9, 1), (5, 3), (17, 13)]:
        u8 = rng.randint(0, 256, size=(h, w)).astype(np.uint8)
        for c in (0.0, 0.5, 127 / 255.0, 1.0):
            assert np.array_equal(su.sat_reference(u8, c), loops_sat(u8, c))
    for c, tex in su.fp32_special_cases():
        t = np.ascontiguousarray(tex[:9, :14])
        assert np.array_equal(su.sat_reference(t, c), loops_sat(t, c))
    # the properties the special values are there for
    one = lambda v, c: bool(su.indicator(np.array([[v]], np.float32), c)[0, 0])
    assert not one(np.nan, 0.5) and one(np.inf, 0.5) and not one(-np.inf, 0.5)
    assert not one(-0.0, 0.0) and not one(0.0, 0.0) and one(1e-45, 0.0)
    assert not one(0.5, 0.5) and one(su.ulp_up(0.5), 0.5) and not one(su.ulp_down(0.5), 0.5)


def test_golden_blobs_that_carry_a_table_are_reproduced():
    """Every committed blob with a SAT section: the numpy reference rebuilds it from the blob's own texels and cut-off.  (None of the blobs
    of golden/blobs.json carries one -- tests/README.md says so; the loop is here for the day one does.)"""
    for name, blob in BLOBS.items():
        for inp in blobfmt.parse_blob(blob)["inputs"]:
            t = inp["texture"]
            if t["has_sat"]:
                for m, tex in enumerate(t["mips"]):
                    assert np.array_equal(t["sat"][m], su.sat_reference(tex, t["alphaCutoff"])), (name, m)
            else:
                assert t["sat"] == [] and t["sat_rest"] == [] and t["sat_size"] == 0


def test_unorm8_indicator_is_the_compilers(tmp_path):
    """byte * (1 / 255) > cutoff in numpy == the same expression compiled by g++ (tests/native/unorm8_indicator.cpp): all 256 bytes, every cut-off
    of the GPU tests"""
    exe = str(tmp_path / "unorm8_indicator")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "unorm8_indicator.cpp"), "-o", exe], check=True)
    cuts = su.unorm8_cutoffs() + [np.float32(su.CUTOFF), np.float32(0.3), np.float32(0.7)]
    r = subprocess.run([exe] + ["%08x" % int(np.float32(c).view(np.uint32)) for c in cuts], stdout=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0
    lines = r.stdout.split()
    assert len(lines) == len(cuts) == 23
    allbytes = np.arange(256, dtype=np.uint8).reshape(1, 256)
    for c, line in zip(cuts, lines):
        mine = "".join("1" if v else "0" for v in su.indicator(allbytes, c)[0])
        assert mine == line, (float(c), mine, line)
    # the cut-offs sit where they are meant to: k/255 itself is not above the cut-off k * (1/255), one ulp below it is
    for n, k in enumerate(su.UNORM8_KS):
        below, at, above = cuts[3 * n:3 * n + 3]
        assert below < at < above
        assert su.indicator(allbytes, at)[0].sum() == 255 - k
        assert su.indicator(allbytes, below)[0].sum() == 256 - k
        assert su.indicator(allbytes, above)[0].sum() == 255 - k
    assert cuts[0] < 0    # one ulp below zero: such a texture has no table


def test_case_list_covers_the_edges_it_claims():
    shp = su.shapes()
    assert len(set(shp)) == len(shp)
    for w in su.WIDTHS:
        hs = [h for (ww, h) in shp if ww == w]
        assert len(hs) >= 3 and 1 in hs and set(hs) & set(su.BLOCK_EDGES), (w, hs)
    for h in su.HEIGHTS:
        ws = [w for (w, hh) in shp if hh == h]
        assert len(ws) >= 3 and 1 in ws and set(ws) & set(su.BLOCK_EDGES), (h, ws)
    assert all(w in su.WIDTHS and h in su.HEIGHTS for (w, h) in shp)
    z = [(w, h) for (w, h) in shp if False in su.tilings(w, h)]
    assert len([1 for (w, h) in z if w != h and (w & (w - 1) or h & (h - 1))]) >= 5   # Morton-Z with a table, neither square nor a power of two
    assert all(su.tilings(w, h) == [True] for (w, h) in su.BIG_SHAPES)
    for fp32 in (False, True):
        cs = dict(su.contents(300, 200, fp32, 3))
        assert {"random", "all_above", "all_below", "single_0_0", "single_299_199", "single_63_63", "single_64_64", "single_255_100", "single_256_100"} <= set(cs)
        assert su.sat_reference(cs["all_above"], su.CUTOFF)[-1, -1] == 300 * 200 and su.sat_reference(cs["all_below"], su.CUTOFF)[-1, -1] == 0
        assert su.sat_reference(cs["single_64_64"], su.CUTOFF).sum() == (300 - 64) * (200 - 64)
        assert abs(int(su.sat_reference(cs["random"], su.CUTOFF)[-1, -1]) - 30000) < 1000
        assert [n for n, _ in su.contents(1, 1, fp32, 3)] == ["random", "all_above", "all_below", "single_0_0"]
    assert su.sat_layout([(129, 257), (65, 64), (1, 1)], 0) == ([(0, 132672), (132672, 16640), (149312, 64)], 149376)
    assert su.sat_layout([(129, 257), (65, 64), (1, 1)], 1) == ([(0, 4 * 512 * 512), (4 * 512 * 512, 4 * 128 * 128), (4 * 512 * 512 + 4 * 128 * 128, 64)], 4 * 512 * 512 + 4 * 128 * 128 + 64)


# ---- the parser's SAT fields against a blob written here ----
def _align(n):
    return (n + 63) & ~63


def _write_blob(mips, tiling, sats, garbage=b"\x00", compress=False):
    """a version-5 blob with one input (texture_impl.h:232-267, serialize_impl.cpp:81-157), written independently of the parser"""
    fp32 = mips[0].dtype == np.float32
    data, sat, descs = bytearray(), bytearray(), []
    for m, tex in enumerate(mips):
        h, w = tex.shape
        n = max(w, h)
        side = 1
        while side < n:
            side *= 2
        ne = side * side if tiling == 1 else w * h
        slot = np.zeros(ne, tex.dtype)
        if tiling == 1:
            for j in range(h):
                for i in range(w):
                    slot[blobfmt.xy_to_morton(i, j)] = tex[j, i]
        else:
            slot[:] = tex.reshape(-1)
        descs.append(struct.pack("<iiffQQQ", w, h, 1.0 / w, 1.0 / h, len(data), ne, len(sat)))
        data += slot.tobytes()
        data += bytes(_align(len(data)) - len(data))
        if sats is not None:
            s = sats[m].astype("<u4").tobytes()
            tail = _align(len(sat) + 4 * ne) - len(sat) - len(s)
            sat += s + (garbage * (tail // len(garbage) + 1))[:tail]
    body = struct.pack("<i", 1) + struct.pack("<Ii", 0, len(mips)) + b"".join(descs)
    body += struct.pack("<iIfi", tiling, 0 if tiling == 1 else 1, 0.5 if sats is not None else -1.0, 1 if fp32 else 0)
    body += struct.pack("<Q", len(data)) + bytes(data) + struct.pack("<Q", len(sat)) + bytes(sat)
    uv, ix = np.zeros(6, np.float32).tobytes(), np.arange(3, dtype=np.uint32).tobytes()
    body += struct.pack("<iifi", ot.CLAMP, ot.LINEAR, 0.0, 0) + struct.pack("<iQ", ot.UV32_FLOAT, len(uv)) + uv + struct.pack("<I", 0)
    body += struct.pack("<iI", ot.IDX_U32, 3) + ix + struct.pack("<fff", 0.0, 0.0, 0.5) + struct.pack("<iii", ot.T, ot.O, ot.FMT_4STATE)
    body += struct.pack("<Q", 0) + struct.pack("<ii", 0, -4) + struct.pack("<B", 0) + struct.pack("<I", 0xFFFFFFFF) + struct.pack("<Q", 0) + struct.pack("<Q", 2 ** 64 - 1)
    body += struct.pack("<i", 0)
    raw_size = 0
    if compress:   # one sequence of literals only, then a run: [token][literals][offset][token of the end]
        raw_size = len(body)
        n = len(body)
        lit = bytes([0xF0]) + b"".join(b"\xff" for _ in range((n - 15) // 255)) + bytes([(n - 15) % 255]) + body
        body = lit
    return struct.pack("<Qiiiiii", 0, 1, 9, 0, 5, 1 if compress else 0, raw_size) + body


@pytest.mark.parametrize("tiling", [0, 1])
@pytest.mark.parametrize("compress", [False, True])
def test_parser_returns_each_mips_table_and_the_rest_of_its_slot(tiling, compress):
    rng = np.random.RandomState(5)
    mips = [rng.rand(5, 7).astype(np.float32), rng.rand(3, 2).astype(np.float32), rng.rand(1, 1).astype(np.float32)]
    sats = [rng.randint(0, 2 ** 32, size=m.shape, dtype=np.uint64).astype(np.uint32) for m in mips]
    p = blobfmt.parse_blob(_write_blob(mips, tiling, sats, garbage=b"\x5a\x00\xa5", compress=compress))
    t = p["inputs"][0]["texture"]
    assert t["has_sat"] and t["tiling"] == tiling
    layout, size = su.sat_layout([m.shape for m in mips], tiling)
    assert t["sat_size"] == size
    assert layout == ([(0, 192), (192, 64), (256, 64)] if tiling == 0 else [(0, 256), (256, 64), (320, 64)])
    for m in range(3):
        assert np.array_equal(t["mips"][m], mips[m])
        assert t["sat"][m].dtype == np.uint32 and t["sat"][m].shape == mips[m].shape and np.array_equal(t["sat"][m], sats[m])
        rest = t["sat_rest"][m]
        assert len(rest) == layout[m][1] - 4 * mips[m].size and rest == (b"\x5a\x00\xa5" * 100)[:len(rest)]
        assert t["mip_descs"][m][4] == layout[m][0]
    # check_tables goes red on: a wrong entry, a dirty slot
    good = [su.sat_reference(m, 0.5) for m in mips]
    su.check_tables(blobfmt.parse_blob(_write_blob(mips, tiling, good))["inputs"][0]["texture"], mips, 0.5, tiling == 0)
    with pytest.raises(AssertionError, match="non-zero bytes behind the table"):
        su.check_tables(blobfmt.parse_blob(_write_blob(mips, tiling, good, garbage=b"\x00\x00\x00\x01"))["inputs"][0]["texture"], mips, 0.5, tiling == 0)
    bad = [g.copy() for g in good]
    bad[1][2, 1] += 1
    with pytest.raises(AssertionError, match=r"SAT of mip 1 \(2x3\): 1 entries differ, first at \(x=1, y=2\)"):
        su.check_tables(blobfmt.parse_blob(_write_blob(mips, tiling, bad))["inputs"][0]["texture"], mips, 0.5, tiling == 0)
    # no table
    t = blobfmt.parse_blob(_write_blob(mips, tiling, None))["inputs"][0]["texture"]
    assert not t["has_sat"] and t["sat"] == [] and t["sat_rest"] == [] and t["sat_size"] == 0
    su.check_tables(t, mips, -1.0, tiling == 0)


def test_morton_index_and_lz4_matches():
    idx = blobfmt.morton_index(37, 21)
    assert idx.shape == (21, 37)
    assert all(idx[j, i] == blobfmt.xy_to_morton(i, j) for j in range(21) for i in range(37))
    assert blobfmt.morton_index(65536, 1)[0, 65535] == blobfmt.xy_to_morton(65535, 0)
    assert [blobfmt.next_pow2(v) for v in (1, 2, 3, 4, 5, 300, 512, 513)] == [1, 2, 4, 4, 8, 512, 512, 1024]
    # literals "abcd", match offset 4 length 11 (overlapping: the run repeats), literals "xyz12"; then offset 1 (one byte repeated) and a far match
    seq = bytes([0x47]) + b"abcd" + bytes([4, 0]) + bytes([0x50]) + b"xyz12"
    assert blobfmt.lz4_block_decompress(seq, 20) == b"abcd" + b"abcdabcdabc" + b"xyz12"
    seq = bytes([0x1F]) + b"q" + bytes([1, 0]) + bytes([6]) + bytes([0x30]) + b"end"
    assert blobfmt.lz4_block_decompress(seq, 1 + 25 + 3) == b"q" * 26 + b"end"
    seq = bytes([0x80]) + b"01234567" + bytes([8, 0]) + bytes([0x10]) + b"!"
    assert blobfmt.lz4_block_decompress(seq, 13) == b"01234567" + b"0123" + b"!"
