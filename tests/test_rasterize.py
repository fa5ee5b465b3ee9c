"""ommxRasterizeMicromap and ommxDebugSaveImagePNG without a GPU: the arithmetic of omm_amd/csrc/raster_cover.h and the PNG writer as plain C++ under
the sanitizers (tests/native/raster_check.cpp), the PNG entry read back with the standard library, the symbols and the struct layouts, every argument
check of include/omm_mi355x_ext.h that is made before the device is touched, and the numpy model of tests/rasterize_util.py held to its second
statement with loops."""
import ctypes as C
import os
import struct
import subprocess
import zlib
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import rasterize_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3


def test_cover_colours_and_png_as_host_code(tmp_path):
    """raster_cover.h against 128-bit integers on dyadic inputs (coverage, the three areas, barycentrics, every covered pixel inside the box), the colour
    arithmetic for 5 x 256 x 8 combinations, and png_store.h read back by a reader of its own.  A stand-alone program under AddressSanitizer and
    UBSan, run directly."""
    exe = str(tmp_path / "raster_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "raster_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path / "check.png")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert " 0 failures" in r.stdout and int(r.stdout.split("raster_check:")[1].split()[0]) > 1000000, r.stdout


# ---- the PNG entry ----
@pytest.fixture(scope="module")
def dll():
    return ru.bind(lu.bind(C.CDLL(ot.product_path())))


def parse_png(data):
    """(width, height, rows) of an 8-bit RGBA PNG of stored blocks, with the standard library only; every chunk's CRC and the file's structure are checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        at += 12 + n
    assert at == len(data) and [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 6, 0, 0, 0)
    z = chunks[1][1]
    raw = zlib.decompress(z)                                   # (checks the Adler-32)
    assert len(raw) == h * (1 + 4 * w)
    # stored blocks only, none above 65 535 bytes, all but the last full
    p, sizes = 2, []
    while True:
        final, n, nn = z[p], *struct.unpack("<HH", z[p + 1:p + 5])
        assert final in (0, 1) and n ^ nn == 0xFFFF
        sizes.append(n)
        p += 5 + n
        if final:
            break
    assert p + 4 == len(z) and all(s == 65535 for s in sizes[:-1]) and sum(sizes) == len(raw)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 4 * w)
    assert not rows[:, 0].any()                                # filter byte 0
    return w, h, rows[:, 1:].reshape(h, w, 4)


@pytest.mark.parametrize("w,h,pitch", [(1, 1, 0), (3, 2, 0), (3, 2, 17), (16384, 1, 0), (16383, 3, 0)], ids=["1x1", "3x2", "3x2_pitch17", "row_65537_bytes", "rows_65533_bytes"])
def test_png_read_back_with_the_standard_library(dll, tmp_path, w, h, pitch):
    rng = np.random.default_rng(w * 7 + h)
    step = pitch or 4 * w
    img = rng.integers(0, 256, step * h, dtype=np.uint8)
    path = str(tmp_path / "out.png")
    assert dll.ommxDebugSaveImagePNG(path.encode(), img.ctypes.data, w, h, pitch) == ot.SUCCESS
    gw, gh, got = parse_png(open(path, "rb").read())
    want = np.lib.stride_tricks.as_strided(img, (h, 4 * w), (step, 1)).reshape(h, w, 4)
    assert (gw, gh) == (w, h) and np.array_equal(got, want)


def test_png_opens_in_pillow(dll, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (65, 257, 4), dtype=np.uint8)
    path = str(tmp_path / "out.png")
    assert dll.ommxDebugSaveImagePNG(path.encode(), img.ctypes.data, 257, 65, 0) == ot.SUCCESS
    with Image.open(path) as im:
        assert im.mode == "RGBA" and im.size == (257, 65) and np.array_equal(np.asarray(im), img)


def test_png_refusals(dll, tmp_path):
    img = np.zeros(64, np.uint8)
    path = str(tmp_path / "never.png").encode()
    call = dll.ommxDebugSaveImagePNG
    assert call(None, img.ctypes.data, 2, 2, 0) == ot.INVALID_ARGUMENT
    assert call(path, None, 2, 2, 0) == ot.INVALID_ARGUMENT
    assert call(path, img.ctypes.data, 0, 2, 0) == ot.INVALID_ARGUMENT
    assert call(path, img.ctypes.data, 2, 0, 0) == ot.INVALID_ARGUMENT
    assert call(path, img.ctypes.data, 2, 2, 7) == ot.INVALID_ARGUMENT and call(path, img.ctypes.data, 2, 2, 8) == ot.SUCCESS
    os.remove(path)
    assert call(str(tmp_path / "no_such_directory" / "x.png").encode(), img.ctypes.data, 2, 2, 0) == ot.FAILURE
    assert not os.path.exists(path)


# ---- the ABI ----
def test_symbols_are_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    for name in ("ommxRasterizeMicromap", "ommxDebugSaveImagePNG"):
        assert any(line.split()[-1] == name and line.split()[-2] == "T" for line in out.splitlines() if line.strip()), name


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxRasterDesc), offsetof(ommxRasterDesc, uvMin), offsetof(ommxRasterDesc, uvMax),
           offsetof(ommxRasterDesc, width), offsetof(ommxRasterDesc, height), offsetof(ommxRasterDesc, firstPrimitive), offsetof(ommxRasterDesc, primitiveCount),
           offsetof(ommxRasterDesc, flags), offsetof(ommxRasterDesc, reserved));
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(ommxRasterOutputs), offsetof(ommxRasterOutputs, primitiveIds), offsetof(ommxRasterOutputs, microTriangles),
           offsetof(ommxRasterOutputs, states), offsetof(ommxRasterOutputs, alphaTest), offsetof(ommxRasterOutputs, rgba));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxRasterInfo), offsetof(ommxRasterInfo, coveredPixels), offsetof(ommxRasterInfo, pixelsPerState),
           offsetof(ommxRasterInfo, invalidPixels), offsetof(ommxRasterInfo, alphaAbovePixels), offsetof(ommxRasterInfo, contradictions),
           offsetof(ommxRasterInfo, drawnPrimitives), offsetof(ommxRasterInfo, degeneratePrimitives));
    printf("%d %d %d %d %u\n", (int)ommxRasterFlags_None, (int)ommxRasterFlags_NoContour, (int)ommxRasterFlags_MonochromeUnknowns,
           (int)ommxRasterFlags_HighlightReuse, OMMX_RASTER_MAX_SIZE);
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    a, b, c, d = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    D, O, I = ru.RasterDesc, ru.RasterOutputs, ru.RasterInfo
    assert a == [C.sizeof(D)] + [getattr(D, f).offset for f, _ in D._fields_] == [40, 0, 8, 16, 20, 24, 28, 32, 36]
    assert b == [C.sizeof(O)] + [getattr(O, f).offset for f in ru.OUTPUTS] == [40, 0, 8, 16, 24, 32]
    assert c == [C.sizeof(I)] + [getattr(I, f).offset for f in ru.INFO_FIELDS] == [72, 0, 8, 40, 48, 56, 64, 68]
    assert d == [0, ru.NO_CONTOUR, ru.MONOCHROME_UNKNOWNS, ru.HIGHLIGHT_REUSE, ru.MAX_SIZE] == [0, 1, 2, 4, 16384]


# ---- the argument checks: refused before the device is touched, each with its log line ----
@pytest.fixture()
def session():
    lib = ot.Lib("product")
    ru.bind(lib.dll)
    msgs = []
    baker = lib.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    yield lib, baker, msgs
    assert lib.destroy_baker(baker) == ot.SUCCESS


PTR = 0x10000   # never dereferenced


def result_desc(index_format=ot.IDX_U32, index_count=5):
    r = ot.BakeResultDesc()
    r.arrayData, r.arrayDataSize = PTR, 64
    r.descArray, r.descArrayCount = C.cast(PTR, C.POINTER(ot.MicromapDesc)), 2
    r.indexBuffer, r.indexCount, r.indexFormat = PTR, index_count, index_format
    return r


def null_field(name):
    r = result_desc()
    setattr(r, name, None)
    return r


def outputs(ids=PTR, micro=PTR):
    return ru.RasterOutputs(ids, micro, PTR, PTR, PTR + 1)   # (rgba needs no alignment)


def input_desc():
    """a desc without a texture: what is left to refuse once everything else is right, as ommxResolveHits refuses it"""
    d = ot.default_bake_desc()
    d.texCoords, d.indexBuffer, d.indexCount = PTR, PTR, 6
    return d


NAN, INF = float("nan"), float("inf")
# (name, result, desc, outputs, the words of its line): in the documented order
REFUSED = [
    ("flags 8", result_desc, lambda: ru.c_desc(flags=8), outputs, "flags"),
    ("flag bit 31", result_desc, lambda: ru.c_desc(flags=0x80000001), outputs, "flags"),
    ("reserved[0]", result_desc, lambda: ru.c_desc(reserved=(1, 0, 0, 0)), outputs, "reserved"),
    ("reserved[3]", result_desc, lambda: ru.c_desc(reserved=(0, 0, 0, 9)), outputs, "reserved"),
    ("width 0", result_desc, lambda: ru.c_desc(width=0), outputs, "width and height"),
    ("height 0", result_desc, lambda: ru.c_desc(height=0), outputs, "width and height"),
    ("width 16385", result_desc, lambda: ru.c_desc(width=16385), outputs, "width and height"),
    ("height 2^31", result_desc, lambda: ru.c_desc(height=1 << 31), outputs, "width and height"),
    ("uvMin NaN", result_desc, lambda: ru.c_desc(view=(NAN, 0, 1, 1)), outputs, "viewport"),
    ("uvMax Inf", result_desc, lambda: ru.c_desc(view=(0, 0, 1, INF)), outputs, "viewport"),
    ("uvMin -Inf", result_desc, lambda: ru.c_desc(view=(0, -INF, 1, 1)), outputs, "viewport"),
    ("uvMax == uvMin on u", result_desc, lambda: ru.c_desc(view=(0.5, 0, 0.5, 1)), outputs, "viewport"),
    ("uvMax < uvMin on v", result_desc, lambda: ru.c_desc(view=(0, 1, 1, 0)), outputs, "viewport"),
    ("unknown indexFormat", lambda: result_desc(index_format=3), ru.c_desc, outputs, "indexFormat"),
    ("null indexBuffer", lambda: null_field("indexBuffer"), ru.c_desc, outputs, "null array"),
    ("null descArray", lambda: null_field("descArray"), ru.c_desc, outputs, "null array"),
    ("null arrayData", lambda: null_field("arrayData"), ru.c_desc, outputs, "null array"),
    ("primitiveIds at 2 modulo 4", result_desc, ru.c_desc, lambda: outputs(ids=PTR + 2), "4-byte aligned"),
    ("microTriangles at 1 modulo 4", result_desc, ru.c_desc, lambda: outputs(micro=PTR + 1), "4-byte aligned"),
    ("no texture", result_desc, ru.c_desc, outputs, "no texture"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    _, make_result, make_desc, make_outputs, words = case
    for want_info in (True, False):
        info = ru.RasterInfo()
        info.contradictions = 77
        r, o, d = make_result(), make_outputs(), input_desc()
        got = lib.dll.ommxRasterizeMicromap(baker, C.byref(d), C.byref(r), C.byref(make_desc()), C.byref(o), C.byref(info) if want_info else None, None)
        assert got == ot.INVALID_ARGUMENT and info.contradictions == 77
        assert len(msgs) == 1 + (not want_info) and msgs[-1][0] == FATAL and words in msgs[-1][1], msgs
    assert len({m[1] for m in msgs}) == 1


def test_every_refusal_has_a_log_line_of_its_own_and_the_order_is_the_documented_one(session):
    lib, baker, msgs = session
    call = lib.dll.ommxRasterizeMicromap
    lines = []
    for _, make_result, make_desc, make_outputs, words in REFUSED:
        r, o, d = make_result(), make_outputs(), input_desc()
        assert call(baker, C.byref(d), C.byref(r), C.byref(make_desc()), C.byref(o), None, None) == ot.INVALID_ARGUMENT
        if msgs[-1][1] not in lines:
            lines.append(msgs[-1][1])
    assert len(lines) == len({c[4] for c in REFUSED}) == 8
    # a call that is wrong in every way at once is refused for the first reason of the documented order; mending that reason shows the next
    def bad_result():
        r = null_field("indexBuffer")
        r.indexFormat = 3
        return r
    wrong = dict(result=bad_result,
                 desc=lambda: ru.c_desc(view=(0, 0, NAN, 1), width=0, flags=8, reserved=(0, 1, 0, 0)), outputs=lambda: outputs(ids=PTR + 2))
    mends = [("desc", lambda: ru.c_desc(view=(0, 0, NAN, 1), width=0, reserved=(0, 1, 0, 0))), ("desc", lambda: ru.c_desc(view=(0, 0, NAN, 1), width=0)),
             ("desc", lambda: ru.c_desc(view=(0, 0, NAN, 1))), ("desc", ru.c_desc), ("result", lambda: null_field("indexBuffer")), ("result", result_desc),
             ("outputs", outputs)]
    seen = []
    for what, mend in [(None, None)] + mends:
        if what:
            wrong[what] = mend
        r, o, d = wrong["result"](), wrong["outputs"](), input_desc()
        assert call(baker, C.byref(d), C.byref(r), C.byref(wrong["desc"]()), C.byref(o), None, None) == ot.INVALID_ARGUMENT
        seen.append(msgs[-1][1])
    assert seen == lines, (seen, lines)


def test_handles_and_null_arguments(session):
    lib, baker, msgs = session
    call = lib.dll.ommxRasterizeMicromap
    d, r, rd, o, info = input_desc(), result_desc(), ru.c_desc(), outputs(), ru.RasterInfo()
    assert call(None, C.byref(d), C.byref(r), C.byref(rd), C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and not msgs
    assert call(baker, None, C.byref(r), C.byref(rd), C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and "deviceDesc" in msgs[-1][1]
    assert call(baker, C.byref(d), None, C.byref(rd), C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and "deviceResult" in msgs[-1][1]
    assert call(baker, C.byref(d), C.byref(r), None, C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and "ommxRasterDesc" in msgs[-1][1]
    assert call(baker, C.byref(d), C.byref(r), C.byref(rd), None, None, None) == ot.INVALID_ARGUMENT and "outputs" in msgs[-1][1] and "outInfo" in msgs[-1][1]
    # the first four in the documented order: every argument null at once names the input desc
    assert call(baker, None, None, None, None, None, None) == ot.INVALID_ARGUMENT and msgs[-1][1] == msgs[0][1]
    assert len(msgs) == 5 and len({m[1] for m in msgs}) == 4 and all(m[0] == FATAL for m in msgs)
    # a handle that is no baker: the type is the handle's low three bits (4 is a texture's), judged before the handle is followed
    other = C.c_void_p((baker.value & ~7) | 4)
    assert call(other, C.byref(d), C.byref(r), C.byref(rd), C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and len(msgs) == 5
    # the input desc is judged as ommxResolveHits judges it: the same code and the same line for a desc without a texture
    lu.bind(lib.dll)
    assert lib.dll.ommxResolveHits(baker, C.byref(d), C.byref(r), None, 0, None, 0, None) == ot.INVALID_ARGUMENT
    assert call(baker, C.byref(d), C.byref(r), C.byref(rd), C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and msgs[-1][1] == msgs[-2][1]


# ---- the models ----
def tiny_scene(rng, triangles, index_dtype=np.uint32, filt=ot.NEAREST, grid=8):
    """random triangles on a 1/grid lattice (pixel centres of the views below fall on edges and vertices), a few of them degenerate, over a 4 x 4 texture;
    the result: level-2 and level-3 blocks in both formats, special indices, an entry beyond the descriptors, and fewer entries than triangles"""
    pts = rng.integers(-2, grid + 3, (3 * triangles, 2)).astype(np.float64) / grid
    pts[3:6] = pts[3]                                       # a repeated vertex
    pts[8] = 2 * pts[7] - pts[6]                            # collinear
    ix = np.arange(3 * triangles).astype(index_dtype)
    tex = rng.integers(0, 2, (4, 4)).astype(np.uint8) * 255 if filt == ot.NEAREST else rng.integers(0, 256, (4, 4)).astype(np.uint8)
    blocks = [lu.pack(rng.integers(0, 4, 16), 2), lu.pack(rng.integers(0, 2, 64), 1), lu.pack(rng.integers(0, 4, 64), 2)]
    offsets = np.cumsum([1] + [len(b) + 1 for b in blocks])
    array = np.zeros(offsets[-1], np.uint8)
    for o, b in zip(offsets, blocks):
        array[o:o + len(b)] = b
    descs = [(offsets[0], 2, 2), (offsets[1], 3, 1), (offsets[2], 3, 2)]
    index = rng.integers(-4, 4, triangles - 2)              # (3 is beyond the descriptors)
    res = lu.Result(array, descs, index, ot.IDX_U16)
    return ru.Scene(tex, pts, ix, ru.HostResult.of(res), filt=filt, addr=ot.WRAP, le=ot.T, gt=ot.O)


@pytest.mark.parametrize("trial", range(6))
def test_the_loops_equal_the_vectorised_model(dll, trial):
    """brute() == model() on tiny scenes: every output and the info, for whole and partial primitive ranges and every flag"""
    rng = np.random.default_rng(100 + trial)
    sc = tiny_scene(rng, 12, [np.uint32, np.uint16, np.uint8][trial % 3], filt=ot.LINEAR if trial % 2 else ot.NEAREST)
    view = [(0, 0, 1, 1), (-0.25, -0.25, 1.25, 1.25), (0.25, 0.125, 0.75, 0.5)][trial % 3]
    w, h = [(8, 8), (12, 7), (16, 5)][trial % 3]
    k = np.rint(sc.uv_read.astype(np.float64) * 8).astype(np.int64).reshape(-1, 3, 2)          # the lattice: exact integers
    flat = set(np.nonzero((k[:, 1, 0] - k[:, 0, 0]) * (k[:, 2, 1] - k[:, 0, 1]) == (k[:, 1, 1] - k[:, 0, 1]) * (k[:, 2, 0] - k[:, 0, 0]))[0].tolist())
    assert {1, 2} <= flat
    seen = set()
    for first, count, flags in ((0, ru.ALL, 0), (2, 7, ru.HIGHLIGHT_REUSE), (5, 0, ru.NO_CONTOUR), (1, 50, ru.MONOCHROME_UNKNOWNS | ru.NO_CONTOUR | ru.HIGHLIGHT_REUSE)):
        a, b = ru.model(dll, sc, view, w, h, first, count, flags), ru.brute(dll, sc, view, w, h, first, count, flags)
        assert ru.same(b, a)
        i = a["info"]
        assert i["coveredPixels"] == sum(i["pixelsPerState"]) + i["invalidPixels"] == int((a["primitiveIds"] != ru.NONE).sum())
        assert i["degeneratePrimitives"] == len([p for p in ru.primitive_range(sc, first, count) if p in flat]) >= (1 if count else 0)
        seen |= set(np.unique(a["states"]).tolist())
        if count == 0:
            assert i["coveredPixels"] == 0 and (a["states"] == ru.STATE_NONE).all() and (a["rgba"][..., 0] == a["rgba"][..., 2]).all()
    assert ru.STATE_NONE in seen and len(seen) >= 3


def test_micro_index_restated(dll):
    """rasterize_util.micro_index == the index ommxLookupOpacityHost reads (lookup_util.digit_result spells it out) at random points, on edges and beyond
    the triangle; the micro-triangle holds the point (lookup_util.micro_vertices)"""
    rng = np.random.default_rng(5)
    for level in (0, 1, 2, 5, 9):
        n = 1 << level
        u = np.concatenate([rng.random(400), rng.integers(0, n + 1, 200) / n, [0, 1, 0, np.nan, -1, 2, 0.5]]).astype(np.float32)
        v = np.concatenate([rng.random(400) * (1 - u[:400]), rng.integers(0, n + 1, 200) / n, [0, 0, 1, 0.5, 0.5, 0.5, 0.5]]).astype(np.float32)
        res = lu.digit_result(level)
        got = lu.digits_to_index(level, lu.lookup_host(dll, res.desc, lu.digit_hits(level, u, v)), len(u)) if level else np.zeros(len(u), np.uint32)
        assert np.array_equal(ru.micro_index(u, v, np.full(len(u), level)), got.astype(np.int64)), level
        if level:
            lu.check_index_is_a_holder(level, u[:600], v[:600], got[:600])


def test_linear_blend_in_fp32_agrees_with_the_float64_sampler():
    """rasterize_util.sample_alpha32 (the kernel's fp32 blend) against lookup_util.sample_alpha (float64 blend): the same texels and weights, values within
    fp32 rounding of each other; Nearest is the same function"""
    rng = np.random.default_rng(9)
    for tex in (rng.integers(0, 256, (5, 7)).astype(np.uint8), rng.random((8, 8)).astype(np.float32)):
        for addr in (ot.WRAP, ot.MIRROR, ot.CLAMP, ot.BORDER, ot.MIRROR_ONCE):
            tu, tv = (rng.random(500) * 3 - 1).astype(np.float32), (rng.random(500) * 3 - 1).astype(np.float32)
            sc = ru.Scene(tex, np.zeros((3, 2)), np.arange(3, dtype=np.uint32), None, addr=addr, filt=ot.LINEAR, border=0.25)
            a32, a64 = ru.sample_alpha32(sc, tu, tv), lu.sample_alpha(tex, tu, tv, addr, ot.LINEAR, 0.25)
            assert np.abs(a32.astype(np.float64) - a64).max() <= 8 * 2.0 ** -24     # twelve roundings of half an ulp of values in [0, 1]: 12 * 2^-25
            sc.filt = ot.NEAREST
            assert np.array_equal(ru.sample_alpha32(sc, tu, tv).astype(np.float64), lu.sample_alpha(tex, tu, tv, addr, ot.NEAREST, 0.25))
