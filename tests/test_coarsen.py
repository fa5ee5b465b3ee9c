"""ommxCoarsenMicromap without a GPU: the word arithmetic of omm_amd/csrc/coarsen_reduce.h as plain C++ under the sanitizers
(tests/native/coarsen_check.cpp), the numpy restatement of the definition held to a second statement with loops over single states, the symbol and the
struct layouts, and every argument check of include/omm_mi355x_ext.h -- all of them are made before the device is touched."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3
SENTINEL = 0x5EED5EED


def test_word_arithmetic_as_host_code(tmp_path):
    """coarsen_reduce.h == a loop over single states: one-level reductions of 8-field groups exhaustively, two and three levels on random words, both
    formats and both mixedState values, the uniformity test.  A stand-alone program under AddressSanitizer and UBSan, run directly."""
    exe = str(tmp_path / "coarsen_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "coarsen_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert " 0 failures" in r.stdout and int(r.stdout.split("coarsen_check:")[1].split()[0]) > 1000000, r.stdout


def test_restatement_equals_the_loops():
    """restate_coarsen == brute_coarsen: every 2-state block of levels 0..2 to every level (exhaustive on the states), then seeded tables of blocks of
    levels 0..4 in both formats with shared, repeated and unreferenced blocks, under every flag combination and both mixedState values"""
    n = 0
    for level in (0, 1, 2):
        for word in range(1 << (4 ** level)):
            states = [(word >> i) & 1 for i in range(4 ** level)]
            for target in range(level + 1):
                for mixed in ((2, 3) if level < 2 else (2 + word % 2,)):      # (level 2: 65536 words, the two values in turn)
                    assert cu.coarsen_states(states, level, target, 1, mixed).tolist() == cu.brute_states(states, level, target, 1, mixed)
                    n += 1
    rng = np.random.default_rng(1)
    for trial in range(100):
        blocks = []
        for k in range(int(rng.integers(1, 7))):
            level, bits = int(rng.integers(0, 5)), int(rng.integers(1, 3))
            blocks.append((cu.planted_states(level, bits, trial * 10 + k), level, bits))
        if trial % 3 == 0:
            blocks.append(blocks[0])
        index = rng.integers(-4, len(blocks), 12).tolist()
        array_data, descs = cu.table_of_blocks(blocks, first_offset=trial % 3, gap=trial % 2)
        for cap in range(5):
            for flags in range(4):
                mixed = 2 + trial % 2
                ref = cu.restate_coarsen(array_data, descs, index, ot.IDX_U8, cap, mixed, flags)
                outs, entries = cu.brute_coarsen(blocks, index, cap, mixed, flags)
                assert entries == ref["index"].tolist(), (trial, cap, flags)
                assert [(o[1], o[2]) for o in outs] == [(int(l), int(f)) for _, l, f in ref["descs"]]
                for o, (off, l, f) in zip(outs, ref["descs"]):
                    assert o[0] == cu.block_states(ref["array"], int(off), int(l), int(f)).tolist()
                n += 1
    assert n > 190000


def test_properties_of_the_restatement():
    """on the statistics table: the rule is associative (a then b == min(a, b) state for state), a cap at or above every level changes no state, offsets
    are packed and naturally aligned, sizes descend, the histograms add up, the invariant of the info holds"""
    array_data, descs, index, _ = su.table_arrays()
    full = cu.restate_coarsen(array_data, descs, index, ot.IDX_U16, 12, 3, cu.NO_SPECIAL | cu.NO_DEDUP)
    view = lambda r: [cu.block_states(r["array"], int(o), int(l), int(f)).tolist() for o, l, f in r["descs"]]
    for d, (o, l, f) in enumerate(descs[:su.TABLE_WELL_FORMED]):
        if d != 7:      # (block 7 is never selected)
            assert cu.block_states(array_data, int(o), int(l), int(f)).tolist() in view(full)
    for a in range(0, 10):
        first = cu.restate_coarsen(array_data, descs, index, ot.IDX_U16, a, 3, cu.NO_SPECIAL | cu.NO_DEDUP)
        for b in (0, 1, 3, 6, 12):
            second = cu.restate_coarsen(first["array"], first["descs"], first["index"], ot.IDX_U16, b, 3, cu.NO_SPECIAL | cu.NO_DEDUP)
            once = cu.restate_coarsen(array_data, descs, index, ot.IDX_U16, min(a, b), 3, cu.NO_SPECIAL | cu.NO_DEDUP)
            assert sorted(view(second)) == sorted(view(once)) and second["info"]["arrayDataSize"] == once["info"]["arrayDataSize"]
        ref = cu.restate_coarsen(array_data, descs, index, ot.IDX_U16, a, 2)
        sizes = [su.block_bytes(int(l), int(f)) for _, l, f in ref["descs"]]
        assert sizes == sorted(sizes, reverse=True) and ref["descs"][:, 0].tolist() == np.cumsum([0] + sizes)[:-1].tolist()
        assert all(int(o) % s == 0 for (o, _, _), s in zip(ref["descs"], sizes)) and sum(sizes) == len(ref["array"]) == ref["info"]["arrayDataSize"]
        assert sum(ref["array_hist"].values()) == len(ref["descs"]) and sum(ref["index_hist"].values()) == int((ref["index"] >= 0).sum())
        i = ref["info"]
        assert i["referencedBlocks"] == i["descArrayCount"] + i["uniformBlocks"] + i["duplicateBlocks"] and i["skippedPrimitives"] == 8


# ---- the ABI ----
def test_symbol_is_exported():
    dll = C.CDLL(ot.product_path())
    assert hasattr(dll, "ommxCoarsenMicromap")
    out = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    assert any(line.split()[-1] == "ommxCoarsenMicromap" and line.split()[-2] == "T" for line in out.splitlines() if line.strip())


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxCoarsenDesc), offsetof(ommxCoarsenDesc, maxSubdivisionLevel), offsetof(ommxCoarsenDesc, mixedState),
           offsetof(ommxCoarsenDesc, reserved), offsetof(ommxCoarsenDesc, flags));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxCoarsenInfo), offsetof(ommxCoarsenInfo, arrayDataSize), offsetof(ommxCoarsenInfo, descArrayCount),
           offsetof(ommxCoarsenInfo, referencedBlocks), offsetof(ommxCoarsenInfo, coarsenedBlocks), offsetof(ommxCoarsenInfo, uniformBlocks),
           offsetof(ommxCoarsenInfo, duplicateBlocks), offsetof(ommxCoarsenInfo, skippedPrimitives));
    printf("%d %d %d\n", (int)ommxCoarsenFlags_None, (int)ommxCoarsenFlags_DisableSpecialIndices, (int)ommxCoarsenFlags_DisableDuplicateDetection);
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    a, b, c = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    D, I = cu.CoarsenDesc, cu.CoarsenInfo
    assert a == [C.sizeof(D), D.maxSubdivisionLevel.offset, D.mixedState.offset, D.reserved.offset, D.flags.offset] == [12, 0, 4, 5, 8]
    assert b == [C.sizeof(I)] + [getattr(I, f).offset for f in cu.INFO_FIELDS] == [32, 0, 8, 12, 16, 20, 24, 28]
    assert c == [cu.NONE, cu.NO_SPECIAL, cu.NO_DEDUP] == [0, 1, 2]


# ---- the argument checks: refused before the device is touched, each with its log line ----
@pytest.fixture()
def session():
    lib = ot.Lib("product")
    cu.bind(lib.dll)
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


REFUSED = [
    ("unknown indexFormat", lambda: result_desc(index_format=3), lambda: cu.c_desc(4), "indexFormat"),
    ("mixedState 0", lambda: result_desc(), lambda: cu.c_desc(4, mixed=0), "mixedState"),
    ("mixedState 1", lambda: result_desc(), lambda: cu.c_desc(4, mixed=1), "mixedState"),
    ("mixedState 4", lambda: result_desc(), lambda: cu.c_desc(4, mixed=4), "mixedState"),
    ("flag bit 2", lambda: result_desc(), lambda: cu.c_desc(4, flags=4), "flags"),
    ("flag bit 31", lambda: result_desc(), lambda: cu.c_desc(4, flags=0x80000001), "flags"),
    ("reserved[0]", lambda: result_desc(), lambda: cu.c_desc(4, reserved=(1, 0, 0)), "reserved"),
    ("reserved[2]", lambda: result_desc(), lambda: cu.c_desc(4, reserved=(0, 0, 0x80)), "reserved"),
    ("null indexBuffer", lambda: null_field("indexBuffer"), lambda: cu.c_desc(4), "null array"),
    ("null descArray", lambda: null_field("descArray"), lambda: cu.c_desc(4), "null array"),
    ("null arrayData", lambda: null_field("arrayData"), lambda: cu.c_desc(4), "null array"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    _, make_result, make_desc, words = case
    for want_result in (True, False):
        out, info = C.c_void_p(SENTINEL), cu.CoarsenInfo()
        info.skippedPrimitives = 77
        r = lib.dll.ommxCoarsenMicromap(baker, C.byref(make_result()), C.byref(make_desc()), C.byref(out) if want_result else None, C.byref(info), None)
        assert r == ot.INVALID_ARGUMENT and out.value == SENTINEL and info.skippedPrimitives == 77
        assert len(msgs) == 1 + (not want_result) and msgs[-1][0] == FATAL and words in msgs[-1][1], msgs


def test_handles_and_the_empty_result(session):
    lib, baker, msgs = session
    rd, cd, out, info = result_desc(), cu.c_desc(4), C.c_void_p(SENTINEL), cu.CoarsenInfo()
    call = lib.dll.ommxCoarsenMicromap
    assert call(None, C.byref(rd), C.byref(cd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and not msgs
    assert call(baker, None, C.byref(cd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "deviceResult" in msgs[-1][1]
    assert call(baker, C.byref(rd), None, C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "ommxCoarsenDesc" in msgs[-1][1]
    assert call(baker, C.byref(rd), C.byref(cd), None, None, None) == ot.INVALID_ARGUMENT and "outResult" in msgs[-1][1] and "outInfo" in msgs[-1][1]
    assert len(msgs) == 3 and all(m[0] == FATAL for m in msgs) and out.value == SENTINEL
    # a handle that is no baker: the type is the handle's low three bits (4 is a texture's), judged before the handle is followed
    other = C.c_void_p((baker.value & ~7) | 4)
    assert call(other, C.byref(rd), C.byref(cd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and out.value == SENTINEL and len(msgs) == 3
    # indexCount == 0: SUCCESS without a launch, whatever the pointers are; the info is zero and the result is empty and can be destroyed
    empty = result_desc(index_count=0)
    info.descArrayCount = info.skippedPrimitives = 9
    info.arrayDataSize = 9
    assert call(baker, C.byref(empty), C.byref(cd), C.byref(out), C.byref(info), None) == ot.SUCCESS
    assert cu.info_dict(info) == dict.fromkeys(cu.INFO_FIELDS, 0) and out.value not in (None, SENTINEL)
    pd = C.POINTER(ot.BakeResultDesc)()
    assert lib.dll.ommxGetDeviceBakeResultDesc(out, C.byref(pd)) == ot.SUCCESS
    e = pd.contents
    assert (e.arrayDataSize, e.descArrayCount, e.indexCount, e.descArrayHistogramCount, e.indexHistogramCount) == (0, 0, 0, 0, 0) and not e.arrayData
    assert e.indexFormat == ot.IDX_U32
    assert lib.dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
    info.skippedPrimitives = 9
    assert call(baker, C.byref(empty), C.byref(cd), None, C.byref(info), None) == ot.SUCCESS and info.skippedPrimitives == 0
