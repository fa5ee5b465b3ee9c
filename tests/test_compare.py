"""ommxCompareMicromaps without a GPU: the word arithmetic of omm_amd/csrc/compare_count.h as plain C++ under the sanitizers
(tests/native/compare_check.cpp), the numpy restatement of the definition held to a second statement with loops over single fields, properties of
the definition, the symbol and the struct layouts, and every argument check of include/omm_mi355x_ext.h -- all of them are made before the device
is touched."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import ommtest as ot
import coarsen_util as cu
import compare_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3
SENTINEL = 0x5EED5EED


def test_word_arithmetic_as_host_code(tmp_path):
    """compare_count.h == loops over single fields: the sixteen counts of random words for 1, 4, 16 and 64 valid fields, both field widths per side,
    with and without Force2State; the masks partition the valid fields; the relation byte of every 0/1 matrix.  A stand-alone program under
    AddressSanitizer and UBSan, run directly."""
    exe = str(tmp_path / "compare_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "compare_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert " 0 failures" in r.stdout and int(r.stdout.split("compare_check:")[1].split()[0]) > 1000000, r.stdout


def _random_source(rng, trial, k, T):
    """a hand-built source over T primitives: blocks of levels 0..4 in both formats from planted states at odd offsets (random bytes between them and
    in the unused bits of one-byte blocks), then descriptors that fail the rule in every way; specials and bad entries in the index"""
    blocks = []
    for j in range(int(rng.integers(2, 6))):
        level, bits = int(rng.integers(0, 5)), int(rng.integers(1, 3))
        blocks.append((cu.planted_states(level, bits, trial * 100 + k * 10 + j), level, bits))
    array, descs = cu.table_of_blocks(blocks, first_offset=trial % 3, gap=trial % 2)
    for o, l, f in descs.tolist():
        if l <= 1 and 4 ** l * f < 8:
            array[o] |= (int(rng.integers(0, 256)) << (4 ** l * f)) & 0xFF          # garbage in the unused bits
    good = len(descs)
    descs = np.concatenate([descs, [(0, 13, 2), (0, 2, 0), (0, 2, 3), (len(array) - 1, 2, 2), (len(array), 0, 1)]])   # level, formats, one byte past, at the end
    index = rng.integers(-4, good, T)
    bad = rng.random(T) < 0.2
    index[bad] = rng.choice([-5, -100, len(descs), len(descs) + 50] + list(range(good, len(descs))), int(bad.sum()))
    return array, descs, index, None


def test_restatement_equals_the_loops():
    """restate_compare == brute_compare on random hand-built pairs: levels 0..4, both formats per side, specials, bad entries of every kind on either
    side, the same pair under several primitives; with and without Force2State; relations, levels, matrices and the info"""
    rng = np.random.default_rng(7)
    kinds = set()
    for trial in range(60):
        T = 24
        a, b = _random_source(rng, trial, 0, T), _random_source(rng, trial, 1, T)
        b[2][:4] = b[2][4:8]
        a[2][:4] = a[2][4:8]                                     # the same pair under several primitives
        if trial % 5 == 0:
            b = a                                                # A == B
        for force2 in (False, True):
            ref = pu.restate_compare(a, b, force2)
            relations, levels, confusion, info = pu.brute_compare(a, b, force2)
            assert ref["relations"].tolist() == relations and ref["levels"].tolist() == levels, (trial, force2)
            assert ref["confusion"].tolist() == confusion and ref["info"] == info, (trial, force2)
            assert all(sum(sum(m, [])) == 4 ** l for m, l in zip(confusion, levels) if l != 0xFF)
            kinds |= set(relations)
            if force2:
                assert all(r in (0, pu.CONFLICT, pu.SKIPPED) for r in relations)
    assert {0, pu.SKIPPED, pu.CONFLICT, pu.A_WEAKER, pu.B_WEAKER, pu.HINT} <= kinds and len(kinds) > 10


def test_properties_of_the_restatement():
    """compare(X, X) is all-diagonal and identical; exchanging A and B transposes every matrix and the totals and swaps the weaker bits and counts; the
    totals add up to (indexCount - skipped) * 4^12; a skipped primitive adds to nothing else"""
    rng = np.random.default_rng(8)
    blocks_a = [(cu.planted_states(level, 2, 40 + level), level, 2) for level in range(6)]
    blocks_b = [(cu.planted_states(level, 1 + level % 2, 50 + level), level, 1 + level % 2) for level in range(6)]
    a, b = cu.table_of_blocks(blocks_a, first_offset=1), cu.table_of_blocks(blocks_b, gap=2)
    ia, ib = rng.integers(-4, 6, 200), rng.integers(-4, 6, 200)
    ia[[0, 5]], ib[[5, 9]] = [-5, 6], [7, -9]
    sa, sb = a + (ia, None), b + (ib, None)
    for force2 in (False, True):
        xx = pu.restate_compare(sa, sa, force2)
        kept = xx["relations"] != pu.SKIPPED
        assert (xx["relations"][kept] == 0).all() and xx["info"]["identicalPrimitives"] == int(kept.sum()) == 198
        off = xx["confusion"].copy()
        off[:, range(4), range(4)] = 0
        assert not off.any() and xx["info"]["firstConflictPrimitive"] == pu.NO_CONFLICT
        ab, ba = pu.restate_compare(sa, sb, force2), pu.restate_compare(sb, sa, force2)
        assert np.array_equal(ab["confusion"].transpose(0, 2, 1), ba["confusion"]) and np.array_equal(ab["levels"], ba["levels"])
        assert ab["info"]["totals"] == [list(row) for row in zip(*ba["info"]["totals"])]
        swap = lambda r: (r & ~np.uint8(pu.A_WEAKER | pu.B_WEAKER)) | ((r & pu.A_WEAKER) << 1) | ((r & pu.B_WEAKER) >> 1)
        assert np.array_equal(swap(ab["relations"]), ba["relations"])
        i, j = ab["info"], ba["info"]
        assert (i["aWeakerPrimitives"], i["bWeakerPrimitives"]) == (j["bWeakerPrimitives"], j["aWeakerPrimitives"])
        for f in ("identicalPrimitives", "conflictPrimitives", "hintPrimitives", "skippedPrimitives", "comparedPairs", "refinedPairs", "firstConflictPrimitive"):
            assert i[f] == j[f], f
        assert i["skippedPrimitives"] == 3 and sum(sum(i["totals"], [])) == (200 - 3) * pu.UNIT
        skipped = ab["relations"] == pu.SKIPPED
        assert (ab["levels"][skipped] == 0xFF).all() and not ab["confusion"][skipped].any()
        assert i["conflictPrimitives"] > 0 and i["firstConflictPrimitive"] == int(np.nonzero(ab["relations"] & pu.CONFLICT)[0][0])
        if not force2:
            assert i["aWeakerPrimitives"] > 0 and i["bWeakerPrimitives"] > 0 and i["hintPrimitives"] > 0 and i["refinedPairs"] > 0


# ---- the ABI ----
def test_symbol_is_exported():
    dll = C.CDLL(ot.product_path())
    assert hasattr(dll, "ommxCompareMicromaps")
    out = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    assert any(line.split()[-1] == "ommxCompareMicromaps" and line.split()[-2] == "T" for line in out.splitlines() if line.strip())


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(ommxCompareDesc), offsetof(ommxCompareDesc, flags), offsetof(ommxCompareDesc, reserved));
    printf("%zu %zu %zu %zu\n", sizeof(ommxCompareOutputs), offsetof(ommxCompareOutputs, relations), offsetof(ommxCompareOutputs, levels),
           offsetof(ommxCompareOutputs, confusion));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxCompareInfo), offsetof(ommxCompareInfo, totals),
           offsetof(ommxCompareInfo, identicalPrimitives), offsetof(ommxCompareInfo, conflictPrimitives), offsetof(ommxCompareInfo, aWeakerPrimitives),
           offsetof(ommxCompareInfo, bWeakerPrimitives), offsetof(ommxCompareInfo, hintPrimitives), offsetof(ommxCompareInfo, skippedPrimitives),
           offsetof(ommxCompareInfo, comparedPairs), offsetof(ommxCompareInfo, refinedPairs), offsetof(ommxCompareInfo, firstConflictPrimitive),
           offsetof(ommxCompareInfo, reserved));
    printf("%u %u %u %u %u %d %d\n", OMMX_RELATION_CONFLICT, OMMX_RELATION_A_WEAKER, OMMX_RELATION_B_WEAKER, OMMX_RELATION_HINT, OMMX_RELATION_SKIPPED,
           (int)ommxCompareFlags_None, (int)ommxCompareFlags_Force2State);
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    a, b, c, d = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    D, O, I = pu.CompareDesc, pu.CompareOutputs, pu.CompareInfo
    assert a == [C.sizeof(D), D.flags.offset, D.reserved.offset] == [8, 0, 4]
    assert b == [C.sizeof(O), O.relations.offset, O.levels.offset, O.confusion.offset] == [24, 0, 8, 16]
    assert c == [C.sizeof(I), I.totals.offset] + [getattr(I, f).offset for f in pu.COUNT_FIELDS] == [168, 0] + list(range(128, 168, 4))
    assert d == [pu.CONFLICT, pu.A_WEAKER, pu.B_WEAKER, pu.HINT, pu.SKIPPED, 0, pu.FORCE_2STATE] == [1, 2, 4, 8, 0x80, 0, 1]


# ---- the argument checks: refused before the device is touched, each with its log line ----
@pytest.fixture()
def session():
    lib = ot.Lib("product")
    pu.bind(lib.dll)
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


def outputs(confusion=PTR):
    return pu.CompareOutputs(PTR, PTR, confusion)


# (name, A, B, desc, outputs, the words of its line): in the documented order
REFUSED = [
    ("flags 2", result_desc, result_desc, lambda: pu.c_desc(2), outputs, "flags"),
    ("flag bit 31", result_desc, result_desc, lambda: pu.c_desc(0x80000001), outputs, "flags"),
    ("reserved", result_desc, result_desc, lambda: pu.c_desc(1, reserved=1), outputs, "reserved"),
    ("unknown indexFormat in A", lambda: result_desc(index_format=3), result_desc, pu.c_desc, outputs, "indexFormat"),
    ("unknown indexFormat in B", result_desc, lambda: result_desc(index_format=7), pu.c_desc, outputs, "indexFormat"),
    ("indexCount differs", result_desc, lambda: result_desc(ot.IDX_U8, index_count=6), pu.c_desc, outputs, "indexCount"),
    ("indexCount 0 and 5", lambda: result_desc(index_count=0), result_desc, pu.c_desc, outputs, "indexCount"),
    ("null indexBuffer", result_desc, lambda: null_field("indexBuffer"), pu.c_desc, outputs, "null array"),
    ("null descArray", lambda: null_field("descArray"), result_desc, pu.c_desc, outputs, "null array"),
    ("null arrayData", lambda: null_field("arrayData"), result_desc, pu.c_desc, outputs, "null array"),
    ("confusion at 8 modulo 16", result_desc, result_desc, pu.c_desc, lambda: outputs(PTR + 8), "16-byte aligned"),
    ("confusion at 4 modulo 16", result_desc, result_desc, pu.c_desc, lambda: outputs(PTR + 4), "16-byte aligned"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    _, make_a, make_b, make_desc, make_outputs, words = case
    for want_info in (True, False):
        info = pu.CompareInfo()
        info.skippedPrimitives = 77
        a, b, o = make_a(), make_b(), make_outputs()
        r = lib.dll.ommxCompareMicromaps(baker, C.byref(a), C.byref(b), C.byref(make_desc()), C.byref(o), C.byref(info) if want_info else None, None)
        assert r == ot.INVALID_ARGUMENT and info.skippedPrimitives == 77
        assert len(msgs) == 1 + (not want_info) and msgs[-1][0] == FATAL and words in msgs[-1][1], msgs
    assert len({m[1] for m in msgs}) == 1


def test_every_refusal_has_a_log_line_of_its_own_and_the_order_is_the_documented_one(session):
    lib, baker, msgs = session
    lines = []
    for _, make_a, make_b, make_desc, make_outputs, words in REFUSED:
        a, b, o = make_a(), make_b(), make_outputs()
        assert lib.dll.ommxCompareMicromaps(baker, C.byref(a), C.byref(b), C.byref(make_desc()), C.byref(o), None, None) == ot.INVALID_ARGUMENT
        if msgs[-1][1] not in lines:
            lines.append(msgs[-1][1])
    assert len(lines) == len({c[5] for c in REFUSED}) == 6
    # a call that is wrong in every way at once is refused for the first reason of the documented order; mending that reason shows the next
    wrong = dict(a=lambda: null_field("indexBuffer"), b=lambda: result_desc(index_format=3, index_count=6), desc=lambda: pu.c_desc(2, reserved=1),
                 outputs=lambda: outputs(PTR + 8))
    mends = [("desc", lambda: pu.c_desc(0, reserved=1)), ("desc", pu.c_desc), ("b", lambda: result_desc(index_count=6)), ("b", result_desc), ("a", result_desc),
             ("outputs", outputs)]
    seen = []
    for what, mend in [(None, None)] + mends[:-1]:
        if what:
            wrong[what] = mend
        a, b, o = wrong["a"](), wrong["b"](), wrong["outputs"]()
        assert lib.dll.ommxCompareMicromaps(baker, C.byref(a), C.byref(b), C.byref(wrong["desc"]()), C.byref(o), None, None) == ot.INVALID_ARGUMENT
        seen.append(msgs[-1][1])
    assert seen == lines, (seen, lines)


def test_handles_and_the_empty_call(session):
    lib, baker, msgs = session
    a, b, cd, o, info = result_desc(), result_desc(ot.IDX_U16), pu.c_desc(), outputs(), pu.CompareInfo()
    call = lib.dll.ommxCompareMicromaps
    assert call(None, C.byref(a), C.byref(b), C.byref(cd), C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and not msgs
    assert call(baker, None, C.byref(b), C.byref(cd), C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and "deviceResultA" in msgs[-1][1]
    assert call(baker, C.byref(a), None, C.byref(cd), C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and "deviceResultB" in msgs[-1][1]
    assert call(baker, C.byref(a), C.byref(b), None, C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and "ommxCompareDesc" in msgs[-1][1]
    assert call(baker, C.byref(a), C.byref(b), C.byref(cd), None, None, None) == ot.INVALID_ARGUMENT and "outputs" in msgs[-1][1] and "outInfo" in msgs[-1][1]
    # the first four in the documented order: every argument null at once names A
    assert call(baker, None, None, None, None, None, None) == ot.INVALID_ARGUMENT and msgs[-1][1] == msgs[0][1]
    assert len(msgs) == 5 and len({m[1] for m in msgs}) == 4 and all(m[0] == FATAL for m in msgs)
    # a handle that is no baker: the type is the handle's low three bits (4 is a texture's), judged before the handle is followed
    other = C.c_void_p((baker.value & ~7) | 4)
    assert call(other, C.byref(a), C.byref(b), C.byref(cd), C.byref(o), C.byref(info), None) == ot.INVALID_ARGUMENT and len(msgs) == 5
    # indexCount == 0 in both: SUCCESS without a launch, whatever the pointers are; the info is zeros but for firstConflictPrimitive; no output is written
    ea, eb = result_desc(index_count=0), result_desc(ot.IDX_U8, index_count=0)
    for f in pu.COUNT_FIELDS:
        setattr(info, f, 9)
    info.totals[2][1] = 9
    assert call(baker, C.byref(ea), C.byref(eb), C.byref(pu.c_desc(pu.FORCE_2STATE)), C.byref(o), C.byref(info), None) == ot.SUCCESS
    want = dict.fromkeys(pu.COUNT_FIELDS, 0)
    want.update(firstConflictPrimitive=pu.NO_CONFLICT, totals=[[0] * 4 for _ in range(4)])
    assert pu.info_dict(info) == want
    assert call(baker, C.byref(ea), C.byref(ea), C.byref(cd), C.byref(o), None, None) == ot.SUCCESS
    assert call(baker, C.byref(ea), C.byref(eb), C.byref(cd), None, C.byref(info), None) == ot.SUCCESS and len(msgs) == 5
