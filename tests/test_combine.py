"""ommxCombineMicromaps without a GPU: the word arithmetic of omm_amd/csrc/combine_expand.h as plain C++ under the sanitizers
(tests/native/combine_check.cpp), the numpy restatement of the definition held to a second statement with loops over single states, the symbol and the
struct layouts, and every argument check of include/omm_mi355x_ext.h -- all of them are made before the device is touched."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import ommtest as ot
import coarsen_util as cu
import combine_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3
SENTINEL = 0x5EED5EED


def test_word_arithmetic_as_host_code(tmp_path):
    """combine_expand.h == loops over single fields: the repetition by 1, 2 and 3 levels on every 8-field group and on random words, the broadcast, the
    K-way join for K = 1..16 in both formats with both mixedState values.  A stand-alone program under AddressSanitizer and UBSan, run directly."""
    exe = str(tmp_path / "combine_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "combine_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert " 0 failures" in r.stdout and int(r.stdout.split("combine_check:")[1].split()[0]) > 1000000, r.stdout


def _random_sources(rng, K, trial):
    """K hand-built sources over 14 primitives: blocks of levels 0..4 in both formats from planted states, specials mixed in, some sources given twice"""
    T, sources = 14, []
    for k in range(K):
        if k and rng.random() < 0.2:
            sources.append(sources[int(rng.integers(0, k))])
            continue
        blocks = []
        for j in range(int(rng.integers(1, 5))):
            level, bits = int(rng.integers(0, 5)), int(rng.integers(1, 3))
            blocks.append((cu.planted_states(level, bits, trial * 100 + k * 10 + j), level, bits))
        if trial % 4 == 0:
            blocks.append((np.full(4 ** 2, k % 4 if blocks[0][2] == 2 else k % 2, np.uint8), 2, blocks[0][2]))      # a uniform block
        index = rng.integers(-4, len(blocks), T)
        index[:3] = index[3:6] if trial % 2 else index[:3]                                                          # repeated tuples
        sources.append((blocks, index.tolist()))
    return sources


def test_restatement_equals_the_loops():
    """restate_combine == brute_combine on random tuples: K in {1, 2, 3, 16}, both output formats, both mixedState values, specials mixed in; blocks in
    output order state for state, every index entry, the info's counts"""
    rng = np.random.default_rng(2)
    n = 0
    for trial in range(60):
        for K in (1, 2, 3, 16):
            sources = _random_sources(rng, K, trial)
            tables = {}
            for blocks, _ in sources:
                if id(blocks) not in tables:
                    tables[id(blocks)] = cu.table_of_blocks(blocks, first_offset=trial % 3, gap=trial % 2)
            host = [tables[id(blocks)] + (np.array(index), None) for blocks, index in sources]
            for fmt in (1, 2):
                mixed = 2 + (trial + fmt) % 2
                ref = mu.restate_combine(host, fmt, mixed)
                outs, entries, counts = mu.brute_combine(sources, fmt, mixed)
                assert entries == ref["index"].tolist(), (trial, K, fmt)
                assert [o[1] for o in outs] == ref["descs"][:, 1].tolist() and (ref["descs"][:, 2] == fmt).all()
                for o, (off, l, f) in zip(outs, ref["descs"]):
                    assert o[0] == cu.block_states(ref["array"], int(off), int(l), int(f)).tolist()
                i = ref["info"]
                assert counts == (i["combinedTuples"], i["refinedTuples"], i["uniformBlocks"], i["duplicateBlocks"]) and i["skippedPrimitives"] == 0
                assert i["combinedTuples"] == i["descArrayCount"] + i["uniformBlocks"] + i["duplicateBlocks"]
                n += 1
    assert n == 480


def test_properties_of_the_restatement():
    """on two sources of planted blocks: the order of the sources changes no byte; a source joined with itself in its own format is itself, state for
    state; the format-1 output is & 1 of the format-2 output; offsets are packed, sizes descend, the histograms add up; bad entries skip once"""
    rng = np.random.default_rng(3)
    blocks_a = [(cu.planted_states(level, 2, 40 + level), level, 2) for level in range(6)]
    blocks_b = [(cu.planted_states(level, 1 + level % 2, 50 + level), level, 1 + level % 2) for level in range(6)]
    a, b = cu.table_of_blocks(blocks_a, first_offset=1), cu.table_of_blocks(blocks_b, gap=2)
    ia, ib = rng.integers(-4, 6, 200), rng.integers(-4, 6, 200)
    sa, sb = a + (ia, None), b + (ib, None)
    view = lambda r: [cu.block_states(r["array"], int(o), int(l), int(f)) for o, l, f in r["descs"]]
    for mixed in (2, 3):
        ab, ba = mu.restate_combine([sa, sb], 2, mixed), mu.restate_combine([sb, sa], 2, mixed)
        cu.assert_same(ab, ba)
        assert ab["info"] == ba["info"] and ab["info"]["refinedTuples"] > 0
        two = mu.restate_combine([sa, sb], 1, mixed)
        special = ab["index"] < 0
        assert np.array_equal(two["index"][special], -(((-(ab["index"][special].astype(np.int64) + 1)) & 1) + 1))
        for i in np.nonzero(~special)[0].tolist():
            want = view(ab)[ab["index"][i]] & 1
            got = view(two)[two["index"][i]] if two["index"][i] >= 0 else np.full(len(want), -(two["index"][i] + 1))
            assert np.array_equal(got, want)
        sizes = [max(1, 4 ** int(l) * int(f) // 8) for _, l, f in ab["descs"]]
        assert sizes == sorted(sizes, reverse=True) and ab["descs"][:, 0].tolist() == np.cumsum([0] + sizes)[:-1].tolist()
        assert sum(sizes) == len(ab["array"]) == ab["info"]["arrayDataSize"]
        assert sum(ab["array_hist"].values()) == len(ab["descs"]) and sum(ab["index_hist"].values()) == int((ab["index"] >= 0).sum())
        aa = mu.restate_combine([sa, sa], 2, mixed)
        for i, e in enumerate(ia.tolist()):
            got = aa["index"][i]
            if e < 0:
                assert got == e
            elif got >= 0:
                assert np.array_equal(view(aa)[got], blocks_a[e][0])
            else:
                assert (blocks_a[e][0] == -(got + 1)).all()
    bad = ia.copy()
    bad[[0, 5]] = [-5, 6]
    r = mu.restate_combine([a + (bad, None), sb], 2, 3)
    assert r["info"]["skippedPrimitives"] == 2 and r["index"][0] == r["index"][5] == -4


# ---- the ABI ----
def test_symbol_is_exported():
    dll = C.CDLL(ot.product_path())
    assert hasattr(dll, "ommxCombineMicromaps")
    out = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    assert any(line.split()[-1] == "ommxCombineMicromaps" and line.split()[-2] == "T" for line in out.splitlines() if line.strip())


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxCombineDesc), offsetof(ommxCombineDesc, format), offsetof(ommxCombineDesc, mixedState),
           offsetof(ommxCombineDesc, reserved), offsetof(ommxCombineDesc, flags));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxCombineInfo), offsetof(ommxCombineInfo, arrayDataSize), offsetof(ommxCombineInfo, descArrayCount),
           offsetof(ommxCombineInfo, combinedTuples), offsetof(ommxCombineInfo, refinedTuples), offsetof(ommxCombineInfo, uniformBlocks),
           offsetof(ommxCombineInfo, duplicateBlocks), offsetof(ommxCombineInfo, skippedPrimitives));
    printf("%d\n", (int)OMMX_COMBINE_MAX_SOURCES);
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    a, b, c = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    D, I = mu.CombineDesc, mu.CombineInfo
    assert a == [C.sizeof(D), D.format.offset, D.mixedState.offset, D.reserved.offset, D.flags.offset] == [12, 0, 4, 5, 8]
    assert b == [C.sizeof(I)] + [getattr(I, f).offset for f in mu.INFO_FIELDS] == [32, 0, 8, 12, 16, 20, 24, 28]
    assert c == [mu.MAX_SOURCES] == [16]


# ---- the argument checks: refused before the device is touched, each with its log line ----
@pytest.fixture()
def session():
    lib = ot.Lib("product")
    mu.bind(lib.dll)
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


GOOD = lambda: mu.c_desc(2)
REFUSED = [
    ("resultCount 17", lambda: [result_desc()] * 17, GOOD, "resultCount"),
    ("null element", lambda: [result_desc(), None], GOOD, "element of deviceResults"),
    ("format 0", lambda: [result_desc()], lambda: mu.c_desc(0), "format"),
    ("format 3", lambda: [result_desc()], lambda: mu.c_desc(3), "format"),
    ("mixedState 0", lambda: [result_desc()], lambda: mu.c_desc(2, mixed=0), "mixedState"),
    ("mixedState 1", lambda: [result_desc()], lambda: mu.c_desc(1, mixed=1), "mixedState"),
    ("mixedState 4", lambda: [result_desc()], lambda: mu.c_desc(2, mixed=4), "mixedState"),
    ("flags 1", lambda: [result_desc()], lambda: mu.c_desc(2, flags=1), "flags"),
    ("flag bit 31", lambda: [result_desc()], lambda: mu.c_desc(2, flags=0x80000000), "flags"),
    ("reserved[0]", lambda: [result_desc()], lambda: mu.c_desc(2, reserved=(1, 0, 0)), "reserved"),
    ("reserved[2]", lambda: [result_desc()], lambda: mu.c_desc(2, reserved=(0, 0, 0x80)), "reserved"),
    ("unknown indexFormat", lambda: [result_desc(), result_desc(index_format=3)], GOOD, "indexFormat"),
    ("indexCount differs", lambda: [result_desc(), result_desc(ot.IDX_U8, index_count=6)], GOOD, "indexCount"),
    ("indexCount 0 and 5", lambda: [result_desc(index_count=0), result_desc()], GOOD, "indexCount"),
    ("null indexBuffer", lambda: [result_desc(), null_field("indexBuffer")], GOOD, "null array"),
    ("null descArray", lambda: [null_field("descArray"), result_desc()], GOOD, "null array"),
    ("null arrayData", lambda: [null_field("arrayData")], GOOD, "null array"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    _, make_results, make_desc, words = case
    for want_result in (True, False):
        out, info = C.c_void_p(SENTINEL), mu.CombineInfo()
        info.skippedPrimitives = 77
        rds = make_results()
        r = lib.dll.ommxCombineMicromaps(baker, mu.pointer_array(rds), len(rds), C.byref(make_desc()), C.byref(out) if want_result else None, C.byref(info), None)
        assert r == ot.INVALID_ARGUMENT and out.value == SENTINEL and info.skippedPrimitives == 77
        assert len(msgs) == 1 + (not want_result) and msgs[-1][0] == FATAL and words in msgs[-1][1], msgs
    assert len({m[1] for m in msgs}) == 1


def test_every_refusal_has_a_log_line_of_its_own(session):
    lib, baker, msgs = session
    lines = set()
    for _, make_results, make_desc, words in REFUSED:
        rds, info = make_results(), mu.CombineInfo()
        assert lib.dll.ommxCombineMicromaps(baker, mu.pointer_array(rds), len(rds), C.byref(make_desc()), None, C.byref(info), None) == ot.INVALID_ARGUMENT
        lines.add(msgs[-1][1])
    assert len(lines) == len({c[3] for c in REFUSED}) == 9


def test_handles_and_the_empty_result(session):
    lib, baker, msgs = session
    rds, cd, out, info = mu.pointer_array([result_desc()]), mu.c_desc(2), C.c_void_p(SENTINEL), mu.CombineInfo()
    call = lib.dll.ommxCombineMicromaps
    assert call(None, rds, 1, C.byref(cd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and not msgs
    assert call(baker, None, 1, C.byref(cd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "deviceResults" in msgs[-1][1]
    assert call(baker, rds, 1, None, C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "ommxCombineDesc" in msgs[-1][1]
    assert call(baker, rds, 0, C.byref(cd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "resultCount" in msgs[-1][1]
    assert call(baker, rds, 1, C.byref(cd), None, None, None) == ot.INVALID_ARGUMENT and "outResult" in msgs[-1][1] and "outInfo" in msgs[-1][1]
    assert len(msgs) == 4 and len({m[1] for m in msgs}) == 4 and all(m[0] == FATAL for m in msgs) and out.value == SENTINEL
    # a handle that is no baker: the type is the handle's low three bits (4 is a texture's), judged before the handle is followed
    other = C.c_void_p((baker.value & ~7) | 4)
    assert call(other, rds, 1, C.byref(cd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and out.value == SENTINEL and len(msgs) == 4
    # indexCount == 0 in every source: SUCCESS without a launch, whatever the pointers are; the info is zero and the result is empty and can be destroyed
    empty = mu.pointer_array([result_desc(index_count=0), result_desc(ot.IDX_U8, index_count=0)])
    info.descArrayCount = info.skippedPrimitives = 9
    info.arrayDataSize = 9
    assert call(baker, empty, 2, C.byref(cd), C.byref(out), C.byref(info), None) == ot.SUCCESS
    assert mu.info_dict(info) == dict.fromkeys(mu.INFO_FIELDS, 0) and out.value not in (None, SENTINEL)
    pd = C.POINTER(ot.BakeResultDesc)()
    assert lib.dll.ommxGetDeviceBakeResultDesc(out, C.byref(pd)) == ot.SUCCESS
    e = pd.contents
    assert (e.arrayDataSize, e.descArrayCount, e.indexCount, e.descArrayHistogramCount, e.indexHistogramCount) == (0, 0, 0, 0, 0) and not e.arrayData
    assert e.indexFormat == ot.IDX_U32
    assert lib.dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
    info.skippedPrimitives = 9
    assert call(baker, empty, 2, C.byref(cd), None, C.byref(info), None) == ot.SUCCESS and info.skippedPrimitives == 0
    assert len(msgs) == 4
