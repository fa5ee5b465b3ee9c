"""ommxReorientMicromap without a GPU: the rule as include/omm_mi355x_lookup.h states it (ommx_reorient_index compiled as host code) held to the numpy
map from discrete barycentrics and to hits through ommx_micro_vertices / ommx_micro_index; the transducer constants of omm_amd/csrc/reorient_map.h
rebuilt from the forward decode; the walk, the tile tables and the source-address arithmetic as plain C++ under the sanitizers
(tests/native/reorient_check.cpp); the numpy restatement of the definition held to a second statement with loops and to the restatement of
ommxCoarsenMicromap; the symbol and the struct layouts; and every argument check of include/omm_mi355x_ext.h -- all made before the device is touched."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
import ommtest as ot
import coarsen_util as cu
import reorient_util as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3
SENTINEL = 0x5EED5EED
LEVEL1 = {0: [0, 1, 2, 3], 1: [2, 1, 3, 0], 2: [3, 1, 0, 2], 3: [0, 1, 3, 2], 4: [3, 1, 2, 0], 5: [2, 1, 0, 3]}
LEVEL2_O1 = [10, 9, 11, 8, 7, 5, 4, 6, 12, 13, 15, 14, 3, 1, 2, 0]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return rt.host_header(tmp_path_factory.mktemp("reorient_shim"))


# ---- the rule ----
def test_check_values_of_the_definition(shim):
    """the level-1 table and the level-2 row of the header's comment, from the header's function and from the numpy map"""
    for o, want in LEVEL1.items():
        assert rt.header_map(shim, 1, o).tolist() == want == rt.source_map(1, o).tolist()
    assert rt.header_map(shim, 2, 1).tolist() == LEVEL2_O1 == rt.source_map(2, 1).tolist()
    src = open(os.path.join(ROOT, "include", "omm_mi355x_lookup.h")).read()
    perms = int(re.search(r"#define OMMX_REORIENT_PERMS (0x[0-9a-f]+)ull", src).group(1), 16)
    assert perms == sum(p[k] << (6 * o + 2 * k) for o, p in enumerate(rt.PERMS) for k in range(3))


def test_reorient_index_is_a_hierarchical_bijection(shim):
    """ommx_reorient_index as host code, levels 0..8 under all six orientations: equal to the numpy map from discrete barycentrics; a bijection;
    map_{l+1}(4j + c) >> 2 == map_l(j); o followed by its inverse is the identity; orientation 0 is the identity"""
    previous = {}
    for level in range(9):
        identity = np.arange(4 ** level)
        for o in range(6):
            m = rt.header_map(shim, level, o)
            assert np.array_equal(m, rt.source_map(level, o)), (level, o)
            assert np.array_equal(np.sort(m), identity)
            if level:
                assert np.array_equal(m >> 2, np.repeat(previous[o], 4)), (level, o)
            previous[o] = m
            # out = src[m_o]; then under o' = inverse: back[j] = out[m_o'[j]] = src[m_o[m_o'[j]]]
            assert np.array_equal(m[rt.header_map(shim, level, rt.INVERSE[o])], identity), (level, o)
        assert np.array_equal(previous[0], identity)


def test_reorient_index_at_its_edges(shim):
    """a level above 12 is 12, an index beyond 4^level is reduced modulo 4^level, an orientation above 5 returns the index as it came"""
    f = shim.shim_reorient_index
    rng = np.random.default_rng(3)
    for j in rng.integers(0, 4 ** 12, 200).tolist():
        for o in range(6):
            assert f(j, 13, o) == f(j, 12, o) == f(j, 0xFFFFFFFF, o) == f(j | 0xFF000000, 12, o)
            assert f(j, 5, o) == f(j & 1023, 5, o) < 1024 and f(j, 0, o) == 0
        assert f(j, 12, 6) == j and f(j | 0xFF000000, 3, 255) == j | 0xFF000000 and f(j, 0, 0xFFFFFFFF) == j


def test_reorient_index_through_hits(shim):
    """the hit statement of the definition, levels 0..4: the centroid of output micro-triangle j' with its barycentrics handed to the old vertices
    lies in source micro-triangle ommx_reorient_index(j')"""
    for level in range(5):
        for o in range(6):
            assert rt.brute_map(shim, level, o) == rt.header_map(shim, level, o).tolist(), (level, o)


def test_transducer_constants_are_rebuilt_from_the_forward_decode():
    """kReorientCodes012 / kReorientCodes345 of reorient_map.h: the digit emitted and the next state for each (state, digit), derived from the numpy
    map of levels 1 and 2 (which comes from the forward decode alone); the sub-maps below every node of levels 3..6 are again among the six"""
    level1 = {tuple(rt.source_map(1, o).tolist()): o for o in range(6)}
    assert len(level1) == 6
    emit, nxt = np.zeros((6, 4), np.int64), np.zeros((6, 4), np.int64)
    for o in range(6):
        m1, m2 = rt.source_map(1, o), rt.source_map(2, o)
        for c in range(4):
            emit[o, c] = m1[c]
            nxt[o, c] = level1[tuple((m2[4 * c:4 * c + 4] & 3).tolist())]
    code = [sum(int(emit[s, c] | nxt[s, c] << 2) << (5 * (4 * (s % 3) + c)) for s in states for c in range(4)) for states in ((0, 1, 2), (3, 4, 5))]
    src = open(os.path.join(ROOT, "omm_amd", "csrc", "reorient_map.h")).read()
    got = [int(re.search(r"kReorientCodes%s = (0x[0-9a-f]+)ull" % name, src).group(1), 16) for name in ("012", "345")]
    assert got == code
    for level in range(3, 7):
        idx = np.arange(4 ** level)
        for o in range(6):
            s, source = np.full(len(idx), o), np.zeros(len(idx), np.int64)
            for i in range(level - 1, -1, -1):
                c = (idx >> (2 * i)) & 3
                source, s = (source << 2) | emit[s, c], nxt[s, c]
            assert np.array_equal(source, rt.source_map(level, o)), (level, o)


def test_map_tiles_and_addresses_as_host_code(tmp_path):
    """reorient_map.h == ommx_reorient_index: the walk and the tile tables on every index of levels 0..9 (strided above, with every tile's first and
    last field), the tiles on bytes at every source misalignment 0..15 with the block at the end of an exact-size allocation and every read
    witnessed.  A stand-alone program under AddressSanitizer and UBSan, run directly."""
    exe = str(tmp_path / "reorient_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "reorient_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert " 0 failures" in r.stdout and int(r.stdout.split("reorient_check:")[1].split()[0]) > 8000000, r.stdout


# ---- the restatement ----
def _random_source(rng, trial):
    blocks = []
    for j in range(int(rng.integers(1, 5))):
        level, bits = int(rng.integers(0, 5)), int(rng.integers(1, 3))
        if blocks and rng.random() < 0.2:
            blocks.append(blocks[int(rng.integers(0, len(blocks)))])
        elif rng.random() < 0.15:
            blocks.append((np.full(4 ** level, int(rng.integers(0, 2 * bits)), np.uint8), level, bits))
        elif rng.random() < 0.2:                                       # symmetric under every orientation at level 1: the middle child differs
            blocks.append((np.array([1, 0, 1, 1], np.uint8), 1, bits))
        else:
            blocks.append((cu.planted_states(level, bits, trial * 10 + j), level, bits))
    T = int(rng.integers(0, 14))
    return blocks, rng.integers(-5, len(blocks) + 1, T).tolist(), rng.integers(0, 8, T).tolist()


def test_restatement_equals_the_loops(shim):
    """restate_reorient == brute_reorient on random hand-built sources under all four flag combinations: blocks in output order state for state,
    every index entry, the info's counts"""
    rng = np.random.default_rng(11)
    n = 0
    for trial in range(80):
        blocks, index, orient = _random_source(rng, trial)
        host = cu.table_of_blocks(blocks, first_offset=trial % 3, gap=trial % 2) + (np.array(index, np.int64), None)
        for flags in (0, 1, 2, 3):
            ref = rt.restate_reorient(host, np.array(orient, np.uint8), flags)
            outs, entries, counts = rt.brute_reorient(shim, blocks, index, orient, flags)
            assert entries == ref["index"].tolist(), (trial, flags)
            assert [(o[1], o[2]) for o in outs] == [(int(l), int(f)) for _, l, f in ref["descs"]]
            for o, (off, l, f) in zip(outs, ref["descs"]):
                assert o[0] == cu.block_states(ref["array"], int(off), int(l), int(f)).tolist()
            i = ref["info"]
            assert counts == (i["referencedBlocks"], i["reorientedBlocks"], i["uniformBlocks"], i["duplicateBlocks"], i["skippedPrimitives"])
            if not flags:
                assert i["referencedBlocks"] == i["descArrayCount"] + i["uniformBlocks"] + i["duplicateBlocks"]
            n += 1
    assert n == 320


def test_properties_of_the_restatement():
    """orientation 0 is restate_coarsen at cap 12 under all four flag combinations, through the desc and per primitive; o then its inverse decodes to
    the source's states per primitive; a block symmetric under a reflection merges with its orientation-0 item; garbage in the unused bits of
    one-byte blocks changes nothing"""
    rng = np.random.default_rng(12)
    blocks = [(cu.planted_states(level, 1 + level % 2, 50 + level), level, 1 + level % 2) for level in range(7)]
    blocks += [(np.full(16, 1, np.uint8), 2, 2), blocks[3]]
    a, d = cu.table_of_blocks(blocks, first_offset=1, gap=1)
    index = rng.integers(-4, len(blocks), 200)
    bad = index.copy()
    bad[[0, 7]] = [-5, len(blocks)]
    for flags in (0, 1, 2, 3):
        for src in ((a, d, index, None), (a, d, bad, len(a) - 1)):
            coarse = cu.restate_coarsen(src[0], src[1], src[2], ot.IDX_U32, 12, 3, flags, src[3])
            for orientations in (0, np.zeros(200, np.uint8)):
                one = rt.restate_reorient(src, orientations, flags)
                cu.assert_same(dict(one, index=one["index"].astype(coarse["index"].dtype)), coarse)
                for field in ("arrayDataSize", "descArrayCount", "referencedBlocks", "uniformBlocks", "duplicateBlocks", "skippedPrimitives"):
                    assert one["info"][field] == coarse["info"][field], (field, flags)
                assert one["info"]["reorientedBlocks"] == 0

    def states_per_primitive(r):
        return [int(e) if e < 0 else cu.block_states(r["array"], *(int(x) for x in r["descs"][int(e)])).tolist() for e in r["index"]]
    orient = rng.integers(0, 6, 200).astype(np.uint8)
    there = rt.restate_reorient((a, d, index, None), orient)
    back = rt.restate_reorient((there["array"], there["descs"], there["index"], None), np.array(rt.INVERSE, np.uint8)[orient])
    assert states_per_primitive(back) == states_per_primitive(rt.restate_reorient((a, d, index, None), 0))
    # reflection 3 swaps vertices 1 and 2: a level-2 block built as s | s[map_3] is symmetric under it
    s = cu.planted_states(2, 2, 9)
    sym = np.maximum(s, s[rt.source_map(2, 3)])
    assert np.array_equal(sym, sym[rt.source_map(2, 3)]) and not np.array_equal(sym, sym[rt.source_map(2, 1)])
    sa, sd = cu.table_of_blocks([(sym, 2, 2)])
    merged = rt.restate_reorient((sa, sd, np.zeros(3, np.int64), None), np.array([0, 3, 1], np.uint8))
    assert merged["info"]["referencedBlocks"] == 3 and merged["info"]["duplicateBlocks"] == 1 and merged["index"].tolist() == [0, 0, 1]
    dirty = a.copy()
    for o, l, f in d.tolist():
        if f * 4 ** l < 8:
            dirty[o] |= (0xFF << (f * 4 ** l)) & 0xFF
    assert not np.array_equal(dirty, a)
    cu.assert_same(rt.restate_reorient((dirty, d, index, None), orient), there)


# ---- the ABI ----
def test_symbol_is_exported():
    dll = C.CDLL(ot.product_path())
    assert hasattr(dll, "ommxReorientMicromap")
    out = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    assert any(line.split()[-1] == "ommxReorientMicromap" and line.split()[-2] == "T" for line in out.splitlines() if line.strip())


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxReorientDesc), offsetof(ommxReorientDesc, deviceOrientations), offsetof(ommxReorientDesc, orientation),
           offsetof(ommxReorientDesc, reserved), offsetof(ommxReorientDesc, flags));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxReorientInfo), offsetof(ommxReorientInfo, arrayDataSize), offsetof(ommxReorientInfo, descArrayCount),
           offsetof(ommxReorientInfo, referencedBlocks), offsetof(ommxReorientInfo, reorientedBlocks), offsetof(ommxReorientInfo, uniformBlocks),
           offsetof(ommxReorientInfo, duplicateBlocks), offsetof(ommxReorientInfo, skippedPrimitives));
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    a, b = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    D, I = rt.ReorientDesc, rt.ReorientInfo
    assert a == [C.sizeof(D), D.deviceOrientations.offset, D.orientation.offset, D.reserved.offset, D.flags.offset] == [16, 0, 8, 9, 12]
    assert b == [C.sizeof(I)] + [getattr(I, f).offset for f in rt.INFO_FIELDS] == [32, 0, 8, 12, 16, 20, 24, 28]


# ---- the argument checks: refused before the device is touched, each with its log line ----
@pytest.fixture()
def session():
    lib = ot.Lib("product")
    rt.bind(lib.dll)
    msgs = []
    baker = lib.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    yield lib, baker, msgs
    assert lib.destroy_baker(baker) == ot.SUCCESS


PTR = 0x10000   # never dereferenced


def result_desc(index_format=ot.IDX_U32, index_count=5, desc_count=2):
    r = ot.BakeResultDesc()
    r.arrayData, r.arrayDataSize = PTR, 64
    r.descArray, r.descArrayCount = C.cast(PTR, C.POINTER(ot.MicromapDesc)), desc_count
    r.indexBuffer, r.indexCount, r.indexFormat = PTR, index_count, index_format
    return r


def null_field(name):
    r = result_desc()
    setattr(r, name, None)
    return r


REFUSED = [
    ("flags 4", result_desc, lambda: rt.c_desc(flags=4), "flags"),
    ("flag bit 31", result_desc, lambda: rt.c_desc(PTR, flags=0x80000001), "flags"),
    ("reserved[0]", result_desc, lambda: rt.c_desc(reserved=(1, 0, 0)), "reserved"),
    ("reserved[2]", result_desc, lambda: rt.c_desc(PTR, reserved=(0, 0, 0x80)), "reserved"),
    ("orientation 6", result_desc, lambda: rt.c_desc(orientation=6), "orientation"),
    ("orientation 255", result_desc, lambda: rt.c_desc(orientation=255, flags=3), "orientation"),
    ("unknown indexFormat", lambda: result_desc(index_format=3), rt.c_desc, "indexFormat"),
    ("unknown indexFormat of an empty source", lambda: result_desc(index_format=7, index_count=0), lambda: rt.c_desc(PTR), "indexFormat"),
    ("null indexBuffer", lambda: null_field("indexBuffer"), rt.c_desc, "null array"),
    ("null descArray", lambda: null_field("descArray"), lambda: rt.c_desc(PTR), "null array"),
    ("null arrayData", lambda: null_field("arrayData"), lambda: rt.c_desc(orientation=5), "null array"),
    ("six items per descriptor", lambda: result_desc(desc_count=0xFFFFFFFF // 6 + 1), lambda: rt.c_desc(PTR), "descArrayCount"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    _, make_result, make_desc, words = case
    for want_result in (True, False):
        out, info = C.c_void_p(SENTINEL), rt.ReorientInfo()
        info.skippedPrimitives = 77
        r = lib.dll.ommxReorientMicromap(baker, C.byref(make_result()), C.byref(make_desc()), C.byref(out) if want_result else None, C.byref(info), None)
        assert r == ot.INVALID_ARGUMENT and out.value == SENTINEL and info.skippedPrimitives == 77
        assert len(msgs) == 1 + (not want_result) and msgs[-1][0] == FATAL and words in msgs[-1][1], msgs
    assert len({m[1] for m in msgs}) == 1


def test_every_refusal_has_a_log_line_of_its_own(session):
    lib, baker, msgs = session
    lines = set()
    for _, make_result, make_desc, words in REFUSED:
        info = rt.ReorientInfo()
        assert lib.dll.ommxReorientMicromap(baker, C.byref(make_result()), C.byref(make_desc()), None, C.byref(info), None) == ot.INVALID_ARGUMENT
        lines.add(msgs[-1][1])
    assert len(lines) == len({c[3] for c in REFUSED}) == 6


def test_the_checks_come_in_the_documented_order(session):
    """an input that fails several checks is refused for the first of them in the header's order"""
    lib, baker, msgs = session
    call = lib.dll.ommxReorientMicromap
    info = rt.ReorientInfo()
    everything = null_field("indexBuffer")
    everything.indexFormat, everything.descArrayCount = 3, 0xFFFFFFFF
    steps = [(rt.c_desc(None, 6, flags=8, reserved=(0, 1, 0)), "flags"), (rt.c_desc(None, 6, reserved=(0, 1, 0)), "reserved"), (rt.c_desc(None, 6), "orientation"),
             (rt.c_desc(PTR, 6), "indexFormat")]
    for desc, words in steps:
        assert call(baker, C.byref(everything), C.byref(desc), None, C.byref(info), None) == ot.INVALID_ARGUMENT and words in msgs[-1][1], msgs[-1]
    everything.indexFormat = ot.IDX_U16
    assert call(baker, C.byref(everything), C.byref(rt.c_desc(PTR)), None, C.byref(info), None) == ot.INVALID_ARGUMENT and "null array" in msgs[-1][1]
    everything.indexBuffer = PTR
    assert call(baker, C.byref(everything), C.byref(rt.c_desc(PTR)), None, C.byref(info), None) == ot.INVALID_ARGUMENT and "descArrayCount" in msgs[-1][1]
    assert call(baker, C.byref(everything), C.byref(rt.c_desc(PTR, flags=4)), None, None, None) == ot.INVALID_ARGUMENT and "outResult" in msgs[-1][1]
    assert call(baker, C.byref(everything), None, None, None, None) == ot.INVALID_ARGUMENT and "ommxReorientDesc" in msgs[-1][1]
    assert call(baker, None, None, None, None, None) == ot.INVALID_ARGUMENT and "deviceResult" in msgs[-1][1]
    assert all(m[0] == FATAL for m in msgs)


def test_handles_and_the_empty_result(session):
    lib, baker, msgs = session
    rd, gd, out, info = result_desc(), rt.c_desc(), C.c_void_p(SENTINEL), rt.ReorientInfo()
    call = lib.dll.ommxReorientMicromap
    assert call(None, C.byref(rd), C.byref(gd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and not msgs
    assert call(baker, None, C.byref(gd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "deviceResult" in msgs[-1][1]
    assert call(baker, C.byref(rd), None, C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "ommxReorientDesc" in msgs[-1][1]
    assert call(baker, C.byref(rd), C.byref(gd), None, None, None) == ot.INVALID_ARGUMENT and "outResult" in msgs[-1][1] and "outInfo" in msgs[-1][1]
    assert len(msgs) == 3 and len({m[1] for m in msgs}) == 3 and all(m[0] == FATAL for m in msgs) and out.value == SENTINEL
    # a handle that is no baker: the type is the handle's low three bits (4 is a texture's), judged before the handle is followed
    other = C.c_void_p((baker.value & ~7) | 4)
    assert call(other, C.byref(rd), C.byref(gd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and out.value == SENTINEL and len(msgs) == 3
    # indexCount == 0: SUCCESS without a launch, whatever the pointers are; the info is zero and the result is empty and can be destroyed
    for source, desc in ((result_desc(index_count=0), rt.c_desc()), (result_desc(ot.IDX_U8, index_count=0), rt.c_desc(PTR, flags=3)),
                         (result_desc(ot.IDX_U16, index_count=0, desc_count=0), rt.c_desc(orientation=4))):
        out = C.c_void_p(SENTINEL)
        info.descArrayCount = info.skippedPrimitives = info.reorientedBlocks = 9
        info.arrayDataSize = 9
        assert call(baker, C.byref(source), C.byref(desc), C.byref(out), C.byref(info), None) == ot.SUCCESS
        assert rt.info_dict(info) == dict.fromkeys(rt.INFO_FIELDS, 0) and out.value not in (None, SENTINEL)
        pd = C.POINTER(ot.BakeResultDesc)()
        assert lib.dll.ommxGetDeviceBakeResultDesc(out, C.byref(pd)) == ot.SUCCESS
        e = pd.contents
        assert (e.arrayDataSize, e.descArrayCount, e.indexCount, e.descArrayHistogramCount, e.indexHistogramCount) == (0, 0, 0, 0, 0) and not e.arrayData
        assert e.indexFormat == ot.IDX_U32
        assert lib.dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
        info.skippedPrimitives = 9
        assert call(baker, C.byref(source), C.byref(desc), None, C.byref(info), None) == ot.SUCCESS and info.skippedPrimitives == 0
    assert len(msgs) == 3
