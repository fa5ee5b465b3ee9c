"""ommxGatherMicromaps without a GPU: the address and shift arithmetic of omm_amd/csrc/gather_copy.h as plain C++ under the sanitizers
(tests/native/gather_check.cpp), the numpy restatement of the definition held to a second statement with loops over single states and to the
restatement of ommxCoarsenMicromap, the symbol and the struct layouts, and every argument check of include/omm_mi355x_ext.h -- all of them are made
before the device is touched."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import ommtest as ot
import coarsen_util as cu
import combine_util as mu
import gather_util as gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3
SENTINEL = 0x5EED5EED


def test_copy_arithmetic_as_host_code(tmp_path):
    """gather_copy.h == a byte loop: every source misalignment 0..15 x every length 1..80, 256, 4096 and 4097 bytes, the blocks below 16 bytes, the
    128-bit byte shifts.  The block ends where its exact-size heap allocation ends and every read of the header is witnessed, so a read outside the
    block fails the run.  A stand-alone program under AddressSanitizer and UBSan, run directly."""
    exe = str(tmp_path / "gather_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "gather_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert " 0 failures" in r.stdout and int(r.stdout.split("gather_check:")[1].split()[0]) > 600000, r.stdout


def _random_sources(rng, K, trial):
    """K hand-built sources of 0..9 primitives: blocks of levels 0..4 in both formats from planted states, uniform blocks and copies of other sources'
    blocks mixed in, specials among the entries, some sources given twice"""
    sources, pool = [], []
    for k in range(K):
        if k and rng.random() < 0.2:
            sources.append(sources[int(rng.integers(0, k))])
            continue
        blocks = []
        for j in range(int(rng.integers(1, 5))):
            level, bits = int(rng.integers(0, 5)), int(rng.integers(1, 3))
            if pool and rng.random() < 0.3:
                blocks.append(pool[int(rng.integers(0, len(pool)))])                       # another source's block: a duplicate across sources
            elif rng.random() < 0.15:
                blocks.append((np.full(4 ** level, int(rng.integers(0, 2 * bits)), np.uint8), level, bits))   # uniform
            else:
                blocks.append((cu.planted_states(level, bits, trial * 100 + k * 10 + j), level, bits))
        pool += blocks
        T = int(rng.integers(0, 10)) if trial % 3 else 6
        sources.append((blocks, rng.integers(-4, len(blocks), T).tolist()))
    return sources


def _host(sources, trial):
    tables = {}
    for blocks, _ in sources:
        if id(blocks) not in tables:
            tables[id(blocks)] = cu.table_of_blocks(blocks, first_offset=trial % 3, gap=trial % 2)
    return [tables[id(blocks)] + (np.array(index, np.int64), None) for blocks, index in sources]


def test_restatement_equals_the_loops():
    """restate_gather == brute_gather on random hand-built sources: K in {1, 2, 3, 7}, the NULL selection and explicit selections with repeats and
    with references beyond the sources, all four flag combinations; blocks in output order state for state, every index entry, the info's counts"""
    rng = np.random.default_rng(5)
    n = 0
    for trial in range(60):
        for K in (1, 2, 3, 7):
            sources = _random_sources(rng, K, trial)
            host = _host(sources, trial)
            picks = [None]
            pairs = [(int(rng.integers(0, K + 1)), int(rng.integers(0, 11))) for _ in range(int(rng.integers(0, 30)))]
            picks.append(pairs + pairs[:5])
            for selection in picks:
                for flags in (0, 1, 2, 3):
                    ref = gt.restate_gather(host, None if selection is None else np.array(selection, np.int64).reshape(-1, 2), flags)
                    outs, entries, counts = gt.brute_gather(sources, selection, flags)
                    assert entries == ref["index"].tolist(), (trial, K, flags)
                    assert [(o[1], o[2]) for o in outs] == [(int(l), int(f)) for _, l, f in ref["descs"]]
                    for o, (off, l, f) in zip(outs, ref["descs"]):
                        assert o[0] == cu.block_states(ref["array"], int(off), int(l), int(f)).tolist()
                    i = ref["info"]
                    assert counts == (i["referencedBlocks"], i["uniformBlocks"], i["duplicateBlocks"], i["skippedPrimitives"])
                    assert i["primitiveCount"] == len(entries)
                    if not flags:
                        assert i["referencedBlocks"] == i["descArrayCount"] + i["uniformBlocks"] + i["duplicateBlocks"]
                    n += 1
    assert n == 60 * 4 * 2 * 4


def _planted_source(rng, seed, count, prims, offset=0, gap=0, garbage=False):
    blocks = [(cu.planted_states(level, 1 + (level + seed) % 2, seed + level), level, 1 + (level + seed) % 2) for level in range(count)]
    blocks.append((np.full(16, 1, np.uint8), 2, 2))                   # uniform
    blocks.append(blocks[3])                                          # a duplicate within the source
    a, d = cu.table_of_blocks(blocks, first_offset=offset, gap=gap)
    if garbage:                                                       # the unused bits of the one-byte blocks hold ones
        for o, l, f in d.tolist():
            if f * 4 ** l < 8:
                a[o] |= (0xFF << (f * 4 ** l)) & 0xFF
    return a, d, rng.integers(-4, len(blocks), prims), None


def _blocks(r):
    return [(int(l), int(f), r["array"][int(o):int(o) + max(1, 4 ** int(l) * int(f) // 8)].tobytes()) for o, l, f in r["descs"]]


def _per_primitive(r):
    """what each primitive reads: its special entry, or the level, format and bytes of its block"""
    blocks = _blocks(r)
    return [int(e) if e < 0 else blocks[int(e)] for e in r["index"]]


def test_properties_of_the_restatement():
    """K = 1 with the NULL selection is restate_coarsen at cap 12 under all four flag combinations (index values; the coarsening keeps the source's
    index format); gathering a gather's output changes nothing; the concatenation of two sources followed by a selection of its second half is a
    gather of the second source; garbage in the unused bits of one-byte blocks changes no output byte; offsets are packed and sizes descend"""
    rng = np.random.default_rng(6)
    a = _planted_source(rng, 40, 7, 150, offset=1, gap=1)
    b = _planted_source(rng, 41, 6, 90)
    bad = a[2].copy()
    bad[[0, 7]] = [-5, len(a[1])]
    for flags in (0, 1, 2, 3):
        for src in (a, b, (a[0], a[1], bad, len(a[0]) - 1)):
            one = gt.restate_gather([src], None, flags)
            coarse = cu.restate_coarsen(src[0], src[1], src[2], ot.IDX_U32, 12, 3, flags, src[3])
            cu.assert_same(dict(one, index=one["index"].astype(coarse["index"].dtype)), coarse)
            for field in ("arrayDataSize", "descArrayCount", "referencedBlocks", "uniformBlocks", "duplicateBlocks", "skippedPrimitives"):
                assert one["info"][field] == coarse["info"][field], (field, flags)
            again = gt.restate_gather([(one["array"], one["descs"], one["index"], None)], None, flags)
            cu.assert_same(again, one)
            assert again["info"] == dict(one["info"], referencedBlocks=one["info"]["descArrayCount"], skippedPrimitives=0,
                                         uniformBlocks=one["info"]["uniformBlocks"] if flags & 1 else 0, duplicateBlocks=0)
        both = gt.restate_gather([a, b], None, flags)
        assert both["info"]["primitiveCount"] == 240
        cat = (both["array"], both["descs"], both["index"], None)
        half = np.stack([np.zeros(90, np.int64), np.arange(150, 240)], 1)
        second = gt.restate_gather([cat], half, flags)
        alone = gt.restate_gather([b], None, flags)
        # what every primitive reads is the same, and so is the set of blocks; their order within a size class is by rank, and a block that the
        # concatenation merged into one of the first source ranks there -- with default flags the two sources share no block that stays a block
        assert _per_primitive(second) == _per_primitive(alone)
        assert all(second["info"][f] == alone["info"][f] for f in ("arrayDataSize", "descArrayCount", "primitiveCount", "skippedPrimitives"))
        assert sorted(_blocks(second)) == sorted(_blocks(alone))
        if not flags:
            cu.assert_same(second, alone)
        sizes = [max(1, 4 ** int(l) * int(f) // 8) for _, l, f in both["descs"]]
        assert sizes == sorted(sizes, reverse=True) and both["descs"][:, 0].tolist() == np.cumsum([0] + sizes)[:-1].tolist()
        assert sum(sizes) == len(both["array"]) == both["info"]["arrayDataSize"]
        assert sum(both["array_hist"].values()) == len(both["descs"]) and sum(both["index_hist"].values()) == int((both["index"] >= 0).sum())
    clean, dirty = _planted_source(np.random.default_rng(7), 40, 7, 150), _planted_source(np.random.default_rng(7), 40, 7, 150, garbage=True)
    assert not np.array_equal(clean[0], dirty[0])
    cu.assert_same(gt.restate_gather([dirty]), gt.restate_gather([clean]))
    merged = gt.restate_gather([clean, dirty])
    assert merged["info"]["descArrayCount"] == gt.restate_gather([clean])["info"]["descArrayCount"]


# ---- the ABI ----
def test_symbol_is_exported():
    dll = C.CDLL(ot.product_path())
    assert hasattr(dll, "ommxGatherMicromaps")
    out = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    assert any(line.split()[-1] == "ommxGatherMicromaps" and line.split()[-2] == "T" for line in out.splitlines() if line.strip())


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxGatherDesc), offsetof(ommxGatherDesc, selection), offsetof(ommxGatherDesc, selectionCount),
           offsetof(ommxGatherDesc, flags), offsetof(ommxGatherDesc, reserved));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxGatherInfo), offsetof(ommxGatherInfo, arrayDataSize), offsetof(ommxGatherInfo, descArrayCount),
           offsetof(ommxGatherInfo, primitiveCount), offsetof(ommxGatherInfo, referencedBlocks), offsetof(ommxGatherInfo, uniformBlocks),
           offsetof(ommxGatherInfo, duplicateBlocks), offsetof(ommxGatherInfo, skippedPrimitives));
    printf("%zu %zu %zu\n", sizeof(ommxPrimitiveRef), offsetof(ommxPrimitiveRef, source), offsetof(ommxPrimitiveRef, primitive));
    printf("%d %d %d %d\n", (int)OMMX_GATHER_MAX_SOURCES, (int)ommxGatherFlags_None, (int)ommxGatherFlags_DisableSpecialIndices,
           (int)ommxGatherFlags_DisableDuplicateDetection);
    printf("%d %d\n", (int)ommxCoarsenFlags_DisableSpecialIndices, (int)ommxCoarsenFlags_DisableDuplicateDetection);
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    a, b, c, d, e = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    D, I = gt.GatherDesc, gt.GatherInfo
    assert a == [C.sizeof(D), D.selection.offset, D.selectionCount.offset, D.flags.offset, D.reserved.offset] == [24, 0, 8, 12, 16]
    assert b == [C.sizeof(I)] + [getattr(I, f).offset for f in gt.INFO_FIELDS] == [32, 0, 8, 12, 16, 20, 24, 28]
    assert c == [gt.REF.itemsize, gt.REF.fields["source"][1], gt.REF.fields["primitive"][1]] == [8, 0, 4]
    assert d == [gt.MAX_SOURCES, gt.NONE, gt.NO_SPECIAL, gt.NO_DEDUP] == [4096, 0, 1, 2]
    assert e == d[2:]                                  # the same values as ommxCoarsenFlags


# ---- the argument checks: refused before the device is touched, each with its log line ----
@pytest.fixture()
def session():
    lib = ot.Lib("product")
    gt.bind(lib.dll)
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


GOOD = lambda: gt.c_desc()
SELECTED = lambda: gt.c_desc(PTR, 3)
REFUSED = [
    ("resultCount 4097", lambda: [result_desc()] * 4097, GOOD, "resultCount"),
    ("null element", lambda: [result_desc(), None], GOOD, "element of deviceResults"),
    ("null last element", lambda: [result_desc()] * 4095 + [None], SELECTED, "element of deviceResults"),
    ("flags 4", lambda: [result_desc()], lambda: gt.c_desc(flags=4), "flags"),
    ("flag bit 31", lambda: [result_desc()], lambda: gt.c_desc(PTR, 3, flags=0x80000001), "flags"),
    ("reserved 1", lambda: [result_desc()], lambda: gt.c_desc(reserved=1), "reserved"),
    ("reserved bit 31", lambda: [result_desc()], lambda: gt.c_desc(PTR, 3, reserved=0x80000000), "reserved"),
    ("null selection with a count", lambda: [result_desc()], lambda: gt.c_desc(None, 1), "selectionCount"),
    ("unknown indexFormat", lambda: [result_desc(), result_desc(index_format=3)], GOOD, "indexFormat"),
    ("unknown indexFormat of an empty source", lambda: [result_desc(index_format=7, index_count=0), result_desc()], SELECTED, "indexFormat"),
    ("null indexBuffer", lambda: [result_desc(), null_field("indexBuffer")], GOOD, "null array"),
    ("null descArray", lambda: [null_field("descArray"), result_desc()], SELECTED, "null array"),
    ("null arrayData", lambda: [null_field("arrayData")], GOOD, "null array"),
    ("2^32 primitives", lambda: [result_desc(index_count=0x80000000)] * 2, GOOD, "indexCount"),
    ("2^32 primitives over 4096", lambda: [result_desc(index_count=1 << 20)] * 4096, GOOD, "indexCount"),
    ("2^32 descriptors", lambda: [result_desc(desc_count=0xFFFFFFFF), result_desc(desc_count=1)], GOOD, "descArrayCount"),
    ("2^32 descriptors under a selection", lambda: [result_desc(index_count=0x80000000, desc_count=0x80000000)] * 2, SELECTED, "descArrayCount"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    _, make_results, make_desc, words = case
    for want_result in (True, False):
        out, info = C.c_void_p(SENTINEL), gt.GatherInfo()
        info.skippedPrimitives = 77
        rds = make_results()
        r = lib.dll.ommxGatherMicromaps(baker, mu.pointer_array(rds), len(rds), C.byref(make_desc()), C.byref(out) if want_result else None, C.byref(info), None)
        assert r == ot.INVALID_ARGUMENT and out.value == SENTINEL and info.skippedPrimitives == 77
        assert len(msgs) == 1 + (not want_result) and msgs[-1][0] == FATAL and words in msgs[-1][1], msgs
    assert len({m[1] for m in msgs}) == 1


def test_every_refusal_has_a_log_line_of_its_own(session):
    lib, baker, msgs = session
    lines = set()
    for _, make_results, make_desc, words in REFUSED:
        rds, info = make_results(), gt.GatherInfo()
        assert lib.dll.ommxGatherMicromaps(baker, mu.pointer_array(rds), len(rds), C.byref(make_desc()), None, C.byref(info), None) == ot.INVALID_ARGUMENT
        lines.add(msgs[-1][1])
    assert len(lines) == len({c[3] for c in REFUSED}) == 9


def test_the_checks_come_in_the_documented_order(session):
    """an input that fails several checks is refused for the first of them in the header's order"""
    lib, baker, msgs = session
    call = lib.dll.ommxGatherMicromaps
    info = gt.GatherInfo()
    everything = [null_field("indexBuffer"), result_desc(index_format=3), result_desc(index_count=0xFFFFFFFF, desc_count=0xFFFFFFFF)]
    steps = [(gt.c_desc(None, 2, flags=8, reserved=1), "flags"), (gt.c_desc(None, 2, reserved=1), "reserved"), (gt.c_desc(None, 2), "selectionCount"),
             (gt.c_desc(), "indexFormat")]
    for desc, words in steps:
        assert call(baker, mu.pointer_array(everything), 3, C.byref(desc), None, C.byref(info), None) == ot.INVALID_ARGUMENT and words in msgs[-1][1], msgs[-1]
    everything[1] = result_desc()
    assert call(baker, mu.pointer_array(everything), 3, C.byref(gt.c_desc()), None, C.byref(info), None) == ot.INVALID_ARGUMENT and "null array" in msgs[-1][1]
    everything[0] = result_desc()
    assert call(baker, mu.pointer_array(everything), 3, C.byref(gt.c_desc()), None, C.byref(info), None) == ot.INVALID_ARGUMENT and "indexCount" in msgs[-1][1]
    assert call(baker, mu.pointer_array(everything), 3, C.byref(gt.c_desc(PTR, 1)), None, C.byref(info), None) == ot.INVALID_ARGUMENT and "descArrayCount" in msgs[-1][1]
    assert call(baker, mu.pointer_array(everything), 3, C.byref(gt.c_desc(PTR, 1)), None, None, None) == ot.INVALID_ARGUMENT and "outResult" in msgs[-1][1]
    assert call(baker, mu.pointer_array(everything + [None]), 4, C.byref(gt.c_desc(PTR, 1)), None, None, None) == ot.INVALID_ARGUMENT and "element" in msgs[-1][1]
    assert call(baker, mu.pointer_array(everything + [None]), 4097, C.byref(gt.c_desc(PTR, 1)), None, None, None) == ot.INVALID_ARGUMENT and "resultCount" in msgs[-1][1]
    assert call(baker, mu.pointer_array(everything), 4097, None, None, None, None) == ot.INVALID_ARGUMENT and "ommxGatherDesc" in msgs[-1][1]
    assert call(baker, None, 4097, None, None, None, None) == ot.INVALID_ARGUMENT and "deviceResults" in msgs[-1][1]
    assert all(m[0] == FATAL for m in msgs)


def test_handles_and_the_empty_result(session):
    lib, baker, msgs = session
    rds, gd, out, info = mu.pointer_array([result_desc()]), gt.c_desc(), C.c_void_p(SENTINEL), gt.GatherInfo()
    call = lib.dll.ommxGatherMicromaps
    assert call(None, rds, 1, C.byref(gd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and not msgs
    assert call(baker, None, 1, C.byref(gd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "deviceResults" in msgs[-1][1]
    assert call(baker, rds, 1, None, C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "ommxGatherDesc" in msgs[-1][1]
    assert call(baker, rds, 0, C.byref(gd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "resultCount" in msgs[-1][1]
    assert call(baker, rds, 1, C.byref(gd), None, None, None) == ot.INVALID_ARGUMENT and "outResult" in msgs[-1][1] and "outInfo" in msgs[-1][1]
    assert len(msgs) == 4 and len({m[1] for m in msgs}) == 4 and all(m[0] == FATAL for m in msgs) and out.value == SENTINEL
    # a handle that is no baker: the type is the handle's low three bits (4 is a texture's), judged before the handle is followed
    other = C.c_void_p((baker.value & ~7) | 4)
    assert call(other, rds, 1, C.byref(gd), C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and out.value == SENTINEL and len(msgs) == 4
    # primitiveCount == 0 -- every source empty under the NULL selection, or an empty selection over sources that are not: SUCCESS without a launch,
    # whatever the pointers are; the info is zero and the result is empty and can be destroyed
    empty = mu.pointer_array([result_desc(index_count=0), result_desc(ot.IDX_U8, index_count=0)])
    full = mu.pointer_array([result_desc(), result_desc(ot.IDX_U16)])
    for sources, desc in ((empty, gt.c_desc()), (full, gt.c_desc(PTR, 0)), (empty, gt.c_desc(PTR, 0, flags=3))):
        out = C.c_void_p(SENTINEL)
        info.descArrayCount = info.skippedPrimitives = info.primitiveCount = 9
        info.arrayDataSize = 9
        assert call(baker, sources, 2, C.byref(desc), C.byref(out), C.byref(info), None) == ot.SUCCESS
        assert gt.info_dict(info) == dict.fromkeys(gt.INFO_FIELDS, 0) and out.value not in (None, SENTINEL)
        pd = C.POINTER(ot.BakeResultDesc)()
        assert lib.dll.ommxGetDeviceBakeResultDesc(out, C.byref(pd)) == ot.SUCCESS
        e = pd.contents
        assert (e.arrayDataSize, e.descArrayCount, e.indexCount, e.descArrayHistogramCount, e.indexHistogramCount) == (0, 0, 0, 0, 0) and not e.arrayData
        assert e.indexFormat == ot.IDX_U32
        assert lib.dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
        info.skippedPrimitives = 9
        assert call(baker, sources, 2, C.byref(desc), None, C.byref(info), None) == ot.SUCCESS and info.skippedPrimitives == 0
    assert len(msgs) == 4
