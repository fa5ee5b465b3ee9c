"""ommxMergeSimilarMicromaps without a GPU: the word arithmetic of omm_amd/csrc/merge_words.h as plain C++ under the sanitizers
(tests/native/merge_check.cpp), the numpy restatement of the definition held to a second statement with loops over single fields and single items,
properties of the definition, the symbol and the struct layouts, and every argument check of include/omm_mi355x_ext.h -- all of them are made before
the device is touched."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import ommtest as ot
import coarsen_util as cu
import merge_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3


def test_word_arithmetic_as_host_code(tmp_path):
    """merge_words.h == loops over single fields: distance and both joins on random words, pos against a table written out in the program, the key at
    1, 27 and 28 samples, the limit of every level.  A stand-alone program under AddressSanitizer and UBSan, run directly."""
    exe = str(tmp_path / "merge_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "merge_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert " 0 failures" in r.stdout and int(r.stdout.split("merge_check:")[1].split()[0]) > 500000, r.stdout


def _random_source(rng, trial, T):
    """a hand-built source over T primitives: families of near-copies at levels 0..4 in both formats at odd offsets (random bytes between them and in
    the unused bits of one-byte blocks), then descriptors that fail the rule in every way; specials and bad entries in the index"""
    blocks = []
    for j in range(int(rng.integers(2, 5))):
        level, bits = int(rng.integers(0, 5)), int(rng.integers(1, 3))
        if trial % 4 == 3:
            bits = 2
        blocks += gu.near_copies(level, int(rng.integers(1, 6)), 0.08, trial * 100 + j, bits)
    order = rng.permutation(len(blocks))
    blocks = [blocks[k] for k in order]
    array, descs = cu.table_of_blocks(blocks, first_offset=trial % 3, gap=trial % 2, filler=int(rng.integers(0, 256)))
    gaps = np.ones(len(array), bool)
    for o, l, f in descs.tolist():
        gaps[o:o + max(1, 4 ** l * f // 8)] = False
        if 4 ** l * f < 8:
            array[o] |= (int(rng.integers(0, 256)) << (4 ** l * f)) & 0xFF          # garbage in the unused bits
    array[gaps] = rng.integers(0, 256, int(gaps.sum()))                             # gaps of random bytes
    good = len(descs)
    descs = np.concatenate([descs, [(0, 13, 2), (0, 2, 0), (0, 2, 3), (len(array) - 1, 2, 2), (len(array), 0, 1), (len(array) - 3, 2, 2)]])
    index = rng.integers(-4, good, T)
    bad = rng.random(T) < 0.15
    index[bad] = rng.choice([-5, -100, len(descs), len(descs) + 50] + list(range(good, len(descs))), int(bad.sum()))
    return array, descs, index


def test_restatement_equals_the_loops():
    """restate_merge == brute_merge on random hand-built sources: levels 0..4, both formats, odd offsets, gaps of random bytes, garbage in the unused
    bits of one-byte blocks, descriptors that fail the bounds rule in every way, specials and bad entries; several limits, rounds, samples, seeds,
    both mixed states and DisableSpecialIndices; blocks, index, roots and the info"""
    rng = np.random.default_rng(11)
    absorbed = later = 0
    for trial in range(48):
        array, descs, index = _random_source(rng, trial, 40)
        for fmt in (ot.IDX_U8, ot.IDX_U32)[:1 + trial % 2]:
            kw = dict(rounds=(0, 1, 3, 32)[trial % 4], samples=(0, 1, 28, 2)[(trial // 4) % 4], seed=(0, 0xFFFFFFFF, 7)[trial % 3], mixed=2 + trial % 2,
                      flags=gu.NO_SPECIAL if trial % 5 == 0 else 0)
            limit = (0, gu.UNIT // 20, gu.UNIT // 4, gu.UNIT)[(trial // 2) % 4]
            ref = gu.restate_merge(array, descs, index, fmt, limit, **kw)
            brute = gu.brute_merge(array, descs, index, limit, **kw)
            assert gu.output_states(ref) == [(list(s), l, f) for s, l, f in brute["blocks"]], trial
            assert ref["index"].tolist() == brute["index"] and ref["roots"].tolist() == brute["roots"] and ref["info"] == brute["info"], trial
            i = ref["info"]
            if not kw["flags"]:
                assert i["referencedBlocks"] == i["descArrayCount"] + i["absorbedBlocks"] + i["uniformBlocks"] + i["duplicateBlocks"]   # the counting identity
            gu.lost_known_fields(ref, descs, index)                                 # the safety statement, field by field
            absorbed += i["absorbedBlocks"]
            later += sum(i["absorbedPerRound"][1:])
            assert i["skippedPrimitives"] > 0 or not (index < -4).any()
    assert absorbed > 100 and later > 0


def test_no_distance_is_the_coarsening_at_cap_12():
    """maxDistance == 0: arrayData, descArray, the index buffer and both histograms are those of restate_coarsen at cap 12 with the same flags, though
    equal blocks are absorbed on the way"""
    rng = np.random.default_rng(12)
    absorbed = 0
    for trial in range(12):
        array, descs, index = _random_source(rng, trial, 60)
        twice = np.concatenate([descs[:4], descs])                                   # equal blocks under several descriptors
        index = np.where(index >= 0, index + rng.integers(0, 2, len(index)) * 4 * (index < 4), index)
        for flags in (0, gu.NO_SPECIAL):
            ref = gu.restate_merge(array, twice, index, ot.IDX_U16, 0, mixed=2 + trial % 2, flags=flags)
            want = cu.restate_coarsen(array, twice, index, ot.IDX_U16, 12, 2 + trial % 2, flags)
            cu.assert_same(ref, want)
            for f in ("arrayDataSize", "descArrayCount", "referencedBlocks", "skippedPrimitives"):
                assert ref["info"][f] == want["info"][f], f
            if not flags:                                                            # (an absorbed copy of a uniform block is absorbed, not uniform)
                assert sum(ref["info"][f] for f in ("absorbedBlocks", "uniformBlocks", "duplicateBlocks")) == want["info"]["uniformBlocks"] + want["info"]["duplicateBlocks"]
            absorbed += ref["info"]["absorbedBlocks"]
    assert absorbed > 0


def _flipped(states, fields):
    s = states.copy()
    s[fields] ^= 1
    return s


def test_a_chain_is_compared_with_its_leader_only():
    """A - B - C at level 3 with one sample at a field all three share: A-B and B-C are within the limit and A-C is not.  C is compared with A only and
    survives the round; B is absorbed; the next round compares C with the joined leader and keeps it again"""
    A = np.zeros(64, np.uint8)
    at = gu.pos(0, 3, 0, 0)
    others = [f for f in range(64) if f != at and f != gu.pos(0, 3, 1, 0)]
    B, C = _flipped(A, others[:3]), _flipped(A, others[:6])
    array, descs = cu.table_of_blocks([(A, 3, 2), (B, 3, 2), (C, 3, 2)])
    limit = 3 * 4 ** 9                                                                # three fields of a level-3 block
    one = gu.restate_merge(array, descs, [0, 1, 2], ot.IDX_U8, limit, rounds=1, samples=1)
    assert one["roots"].tolist() == [0, 0, 2] and one["info"]["absorbedPerRound"][:2] == [1, 0]
    assert one["states"][2].tolist() == C.tolist() and (one["states"][0][others[:3]] == 3).all() and one["states"][0].sum() == 9
    two = gu.restate_merge(array, descs, [0, 1, 2], ot.IDX_U8, limit, rounds=2, samples=1)
    assert two["roots"].tolist() == [0, 0, 2] and two["info"]["absorbedBlocks"] == 1   # C against the joined A: six fields apart
    wide = gu.restate_merge(array, descs, [0, 1, 2], ot.IDX_U8, 2 * limit, rounds=1, samples=1)
    assert wide["roots"].tolist() == [0, 0, 0]
    brute = gu.brute_merge(array, descs, [0, 1, 2], limit, rounds=2, samples=1)
    assert brute["roots"] == [0, 0, 2] and brute["info"] == two["info"]


def test_a_leader_is_never_absorbed_in_its_own_round():
    """two keys in one round: the leader of the second key is within the limit of the first key's leader, and stays; in the round in which they share
    a key it is absorbed, with what it has absorbed itself: roots follow the chain"""
    base = np.zeros(16, np.uint8)
    p0, p1 = gu.pos(5, 2, 0, 0), gu.pos(5, 2, 1, 0)
    assert p0 != p1
    free = [f for f in range(16) if f not in (p0, p1)]
    X = base.copy()
    Y = base.copy()
    Y[p0] = 1                                                                          # another key in round 0, the same in round 1
    Y2 = _flipped(Y, free[:1])
    array, descs = cu.table_of_blocks([(X, 2, 2), (Y, 2, 2), (Y2, 2, 2)])
    limit = 2 * 4 ** 10
    one = gu.restate_merge(array, descs, [0, 1, 2, 2], ot.IDX_U8, limit, rounds=1, samples=1, seed=5)
    assert one["roots"].tolist() == [0, 1, 1] and one["info"]["absorbedPerRound"][0] == 1
    two = gu.restate_merge(array, descs, [0, 1, 2, 2], ot.IDX_U8, limit, rounds=2, samples=1, seed=5, mixed=2)
    assert two["roots"].tolist() == [0, 0, 0] and two["info"]["absorbedPerRound"][:3] == [1, 1, 0]
    final = two["states"][0]
    assert final[p0] == 2 and final[free[0]] == 2 and (np.delete(final, [p0, free[0]]) == 0).all()
    assert two["index"].tolist() == [0, 0, 0, 0] and two["info"]["descArrayCount"] == 1
    brute = gu.brute_merge(array, descs, [0, 1, 2, 2], limit, rounds=2, samples=1, seed=5, mixed=2)
    assert brute["roots"] == [0, 0, 0] and brute["info"] == two["info"] and brute["blocks"][0][0] == final.tolist()


def test_only_4_state_blocks_above_level_0_take_part():
    """equal 2-state blocks and equal level-0 blocks are no candidates: they pass through and the tail merges them"""
    blocks = [(cu.planted_states(3, 1, 1), 3, 1)] * 2 + [(np.array([2], np.uint8), 0, 2)] * 2 + [(np.array([1, 0, 1, 1], np.uint8), 1, 1)] * 2
    array, descs = cu.table_of_blocks(blocks, first_offset=1)
    ref = gu.restate_merge(array, descs, np.arange(6), ot.IDX_U8, gu.UNIT)
    i = ref["info"]
    assert (i["candidateBlocks"], i["absorbedBlocks"], i["referencedBlocks"], i["uniformBlocks"], i["duplicateBlocks"]) == (0, 0, 6, 2, 2)
    assert ref["roots"].tolist() == list(range(6))
    cu.assert_same(ref, cu.restate_coarsen(array, descs, np.arange(6), ot.IDX_U8, 12))


# ---- the ABI ----
def test_symbol_is_exported():
    dll = C.CDLL(ot.product_path())
    assert hasattr(dll, "ommxMergeSimilarMicromaps")
    out = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    assert any(line.split()[-1] == "ommxMergeSimilarMicromaps" and line.split()[-2] == "T" for line in out.splitlines() if line.strip())


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxMergeDesc), offsetof(ommxMergeDesc, maxDistance), offsetof(ommxMergeDesc, rounds),
           offsetof(ommxMergeDesc, samples), offsetof(ommxMergeDesc, seed), offsetof(ommxMergeDesc, mixedState), offsetof(ommxMergeDesc, reserved),
           offsetof(ommxMergeDesc, flags));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxMergeInfo), offsetof(ommxMergeInfo, arrayDataSize), offsetof(ommxMergeInfo, descArrayCount),
           offsetof(ommxMergeInfo, referencedBlocks), offsetof(ommxMergeInfo, candidateBlocks), offsetof(ommxMergeInfo, absorbedBlocks),
           offsetof(ommxMergeInfo, uniformBlocks), offsetof(ommxMergeInfo, duplicateBlocks), offsetof(ommxMergeInfo, skippedPrimitives),
           offsetof(ommxMergeInfo, absorbedPerRound));
    printf("%d %d %d\n", OMMX_MERGE_MAX_ROUNDS, OMMX_MERGE_MAX_SAMPLES, (int)ommxCoarsenFlags_DisableSpecialIndices);
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    """four 32-bit words, the mixed state with its three reserved bytes, the flags: 24 bytes; the info is 168 bytes"""
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    a, b, c = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    D, I = gu.MergeDesc, gu.MergeInfo
    assert a == [C.sizeof(D), D.maxDistance.offset, D.rounds.offset, D.samples.offset, D.seed.offset, D.mixedState.offset, D.reserved.offset, D.flags.offset]
    assert a == [24, 0, 4, 8, 12, 16, 17, 20]
    assert b == [C.sizeof(I)] + [getattr(I, f).offset for f in gu.COUNT_FIELDS] + [I.absorbedPerRound.offset] == [168, 0] + list(range(8, 40, 4))
    assert c == [gu.MAX_ROUNDS, gu.MAX_SAMPLES, gu.NO_SPECIAL] == [32, 28, 1]


# ---- the argument checks: refused before the device is touched, each with its log line ----
@pytest.fixture()
def session():
    lib = ot.Lib("product")
    gu.bind(lib.dll)
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


# (name, result, desc, the words of its line): in the documented order
REFUSED = [
    ("unknown indexFormat", lambda: result_desc(index_format=3), gu.c_desc, "indexFormat"),
    ("maxDistance 4^12 + 1", result_desc, lambda: gu.c_desc(gu.UNIT + 1), "maxDistance"),
    ("maxDistance all ones", result_desc, lambda: gu.c_desc(0xFFFFFFFF), "maxDistance"),
    ("rounds 33", result_desc, lambda: gu.c_desc(rounds=33), "rounds"),
    ("samples 29", result_desc, lambda: gu.c_desc(samples=29), "samples"),
    ("mixedState 0", result_desc, lambda: gu.c_desc(mixed=0), "mixedState"),
    ("mixedState 4", result_desc, lambda: gu.c_desc(mixed=4), "mixedState"),
    ("DisableDuplicateDetection", result_desc, lambda: gu.c_desc(flags=2), "flags"),
    ("flag bit 31", result_desc, lambda: gu.c_desc(flags=0x80000001), "flags"),
    ("reserved", result_desc, lambda: gu.c_desc(reserved=(0, 0, 1)), "reserved"),
    ("null indexBuffer", lambda: null_field("indexBuffer"), gu.c_desc, "null array"),
    ("null descArray", lambda: null_field("descArray"), gu.c_desc, "null array"),
    ("null arrayData", lambda: null_field("arrayData"), gu.c_desc, "null array"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    _, make_result, make_desc, words = case
    for want_info in (True, False):
        info, out = gu.MergeInfo(), C.c_void_p(0x77)
        info.skippedPrimitives = 77
        rd = make_result()
        r = lib.dll.ommxMergeSimilarMicromaps(baker, C.byref(rd), C.byref(make_desc()), PTR, C.byref(out), C.byref(info) if want_info else None, None)
        assert r == ot.INVALID_ARGUMENT and info.skippedPrimitives == 77 and out.value == 0x77
        assert len(msgs) == 1 + (not want_info) and msgs[-1][0] == FATAL and words in msgs[-1][1], msgs
    assert len({m[1] for m in msgs}) == 1


def test_every_refusal_has_a_log_line_of_its_own_and_the_order_is_the_documented_one(session):
    lib, baker, msgs = session
    lines = []
    for _, make_result, make_desc, words in REFUSED:
        rd = make_result()
        assert lib.dll.ommxMergeSimilarMicromaps(baker, C.byref(rd), C.byref(make_desc()), PTR, None, None, None) == ot.INVALID_ARGUMENT
        if msgs[-1][1] not in lines:
            lines.append(msgs[-1][1])
    assert len(lines) == len({c[3] for c in REFUSED}) == 8
    # a call that is wrong in every way at once is refused for the first reason of the documented order; mending that reason shows the next
    def all_wrong():
        r = null_field("indexBuffer")
        r.indexFormat = 3
        return r

    wrong = dict(result=all_wrong, maxDistance=gu.UNIT + 1, rounds=33, samples=29, mixed=5, flags=4, reserved=(1, 0, 0))
    mends = [("result", lambda: null_field("indexBuffer")), ("maxDistance", gu.UNIT), ("rounds", 32), ("samples", 28), ("mixed", 2), ("flags", 1), ("reserved", (0, 0, 0))]
    seen = []
    for what, mend in [(None, None)] + mends:
        if what:
            wrong[what] = mend
        rd = wrong["result"]()
        cd = gu.c_desc(wrong["maxDistance"], wrong["rounds"], wrong["samples"], 0, wrong["mixed"], wrong["flags"], wrong["reserved"])
        assert lib.dll.ommxMergeSimilarMicromaps(baker, C.byref(rd), C.byref(cd), PTR, None, None, None) == ot.INVALID_ARGUMENT
        seen.append(msgs[-1][1])
    assert seen == lines, (seen, lines)


def test_handles_and_the_empty_call(session):
    lib, baker, msgs = session
    rd, cd, info, out = result_desc(), gu.c_desc(), gu.MergeInfo(), C.c_void_p()
    call = lib.dll.ommxMergeSimilarMicromaps
    assert call(None, C.byref(rd), C.byref(cd), PTR, C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and not msgs
    assert call(baker, None, C.byref(cd), PTR, C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "deviceResult" in msgs[-1][1]
    assert call(baker, C.byref(rd), None, PTR, C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and "ommxMergeDesc" in msgs[-1][1]
    assert call(baker, C.byref(rd), C.byref(cd), None, None, None, None) == ot.INVALID_ARGUMENT and "outDeviceBlockRoots" in msgs[-1][1]
    # the first three in the documented order: every argument null at once names the result; an unset output comes before the desc's own checks
    assert call(baker, None, None, None, None, None, None) == ot.INVALID_ARGUMENT and msgs[-1][1] == msgs[0][1]
    assert call(baker, C.byref(rd), C.byref(gu.c_desc(rounds=33)), None, None, None, None) == ot.INVALID_ARGUMENT and msgs[-1][1] == msgs[2][1]
    assert len(msgs) == 5 and len({m[1] for m in msgs}) == 3 and all(m[0] == FATAL for m in msgs)
    # a handle that is no baker: the type is the handle's low three bits (4 is a texture's), judged before the handle is followed
    other = C.c_void_p((baker.value & ~7) | 4)
    assert call(other, C.byref(rd), C.byref(cd), PTR, C.byref(out), C.byref(info), None) == ot.INVALID_ARGUMENT and len(msgs) == 5
    # the limits themselves are accepted, and indexCount == 0 is SUCCESS without a launch, whatever the pointers are: zero info, an empty result
    empty = result_desc(ot.IDX_U8, index_count=0)
    for f in gu.COUNT_FIELDS:
        setattr(info, f, 9)
    info.absorbedPerRound[31] = 9
    assert call(baker, C.byref(empty), C.byref(gu.c_desc(gu.UNIT, 32, 28, 0xFFFFFFFF, 2, 1)), PTR, C.byref(out), C.byref(info), None) == ot.SUCCESS
    want = dict.fromkeys(gu.COUNT_FIELDS, 0)
    want["absorbedPerRound"] = [0] * 32
    assert gu.info_dict(info) == want and out.value
    e = cu.result_desc_of(lib.dll, out)
    assert (e.arrayDataSize, e.descArrayCount, e.indexCount, e.indexFormat) == (0, 0, 0, ot.IDX_U8)
    assert lib.dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
    assert call(baker, C.byref(empty), C.byref(cd), PTR, None, None, None) == ot.SUCCESS and len(msgs) == 5
