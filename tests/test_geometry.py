"""ommxExtractMicroGeometry / ommxExpandMicroNodes without a GPU: the header's vertex function and the cut of 64 as plain C++ under the sanitizers
(tests/native/geometry_check.cpp), the numpy restatement of the cut held to the definition by a second, recursive statement, the properties of a cut
on every pattern the GPU tests use, and every argument check of include/omm_mi355x_ext.h -- all of them are made before the device is touched."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import geometry_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3


def test_vertices_and_the_cut_of_64_as_host_code(tmp_path):
    """ommx_micro_vertices == orc_index2bary bit for bit, the centroid maps back, positive orientation, children 4j..4j+3 tile node j -- every index of
    levels 0..12; geo_cut64 == a scalar loop over the definition.  A stand-alone program under AddressSanitizer and UBSan."""
    exe = str(tmp_path / "geometry_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "omm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "geometry_check.cpp"), ot.oracle_path(), "-Wl,-rpath," + os.path.dirname(ot.oracle_path()), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert " 0 failures" in r.stdout and "geometry_check: 1" in r.stdout, r.stdout


GDESCS_2 = [gu.GDesc((0, 1, 0, 1), m, e) for m in (0, 1, gu.DROP) for e in (0, 1, 2, 12)] + [gu.GDesc((gu.DROP, 1, 0, 1), 1, 12)]


def test_restatement_equals_the_recursive_walk():
    """restate's block_cut == brute_cut: every 2-state block of levels 0..2 with two lists (exhaustive), seeded random 4-state blocks of levels 3 and 4
    with every mapping shape, at every emit level"""
    n = 0
    for level in (0, 1, 2):
        for word in range(1 << (4 ** level)):
            states = [(word >> i) & 1 for i in range(4 ** level)]
            for g in (GDESCS_2 if level < 2 else [GDESCS_2[word % len(GDESCS_2)]]):   # (level 2: 65536 words, the descs in turn)
                if g.max_emit > level and g.max_emit != 12:
                    continue
                assert [list(a) for a in gu.block_cut(states, level, g)] == gu.brute_cut(states, level, g), (level, word, g)
                n += 1
    rng = np.random.default_rng(11)
    maps = [(0, 1, 2, 3), (gu.DROP, 0, 1, 1), (0, 0, 0, 0), (2, 2, 0, 0), (gu.DROP,) * 4, (3, gu.DROP, 3, 1)]
    for level in (3, 4):
        for trial in range(60):
            run = 4 ** int(rng.integers(0, level + 1))
            states = np.repeat(rng.integers(0, 4, 4 ** level // run + 1), run)[:4 ** level]
            flips = rng.integers(0, 4 ** level, int(rng.integers(0, 4)))
            states[flips] = rng.integers(0, 4, len(flips))
            g = gu.GDesc(maps[trial % len(maps)], [0, 1, 2, 3, gu.DROP][trial % 5], [0, 1, 2, 3, 4, 0xFFFFFFFF][trial % 6])
            assert [list(a) for a in gu.block_cut(states, level, g)] == gu.brute_cut(states, level, g), (level, trial, g)
            n += 1
    assert n > 60000


def case_blocks():
    """(name, states, level, bits) of every block the GPU level cases use, up to level 9"""
    for level in (0, 1, 2, 3, 4, 5, 6, 7, 9):
        for bits in (1, 2):
            for name in gu.ALL_PATTERNS:
                yield "%s L%d b%d" % (name, level, bits), gu.pattern(name, level, bits), level, bits


def test_properties_of_the_restated_cut():
    """with DROP a list of its own nothing is lost: every micro-triangle is covered by exactly one node, the nodes' areas 4^-level add up to 1, and no
    four siblings of one class are all emitted (they would have merged); the dropped list is what a DROP mapping leaves out"""
    for name, states, level, bits in case_blocks():
        for emit in sorted({0, 1, max(level - 3, 0), level, 12}):
            for mapping, mixed in (((0, 1, 2, 3), 3), ((3, 0, 1, 1), 1), ((2, 2, 2, 2), 0)):
                cut = gu.block_cut(states, level, gu.GDesc(mapping, mixed, emit))
                assert (gu.covering(level, cut) == 1).all(), (name, emit, mapping)
                area = sum(float(np.sum(0.25 ** (np.asarray(c, np.int64) >> 24))) for c in cut)
                assert area == 1.0, (name, emit, mapping, area)        # dyadic: exact
                for c in cut:
                    c = np.asarray(c, np.int64)
                    lead = c[(c & 3) == 0]
                    full = np.isin(lead + 1, c) & np.isin(lead + 2, c) & np.isin(lead + 3, c) & ((lead >> 24) > 0)
                    assert not full.any(), (name, emit, mapping)
                # the same cut with list 3 dropped: lists 0..2 unchanged, nothing in list 3
                dropped = gu.block_cut(states, level, gu.GDesc(tuple(gu.DROP if v == 3 else v for v in mapping), gu.DROP if mixed == 3 else mixed, emit))
                assert all(np.array_equal(a, b) for a, b in zip(cut[:3], dropped[:3])) and len(dropped[3]) == 0


def test_restate_cut_on_the_tables():
    """the bounds table and the statistics table through restate_cut: skipped primitives are the ones the statistics skip, offsets close on the counts"""
    array_data, descs, index, _ = su.table_arrays()
    ref = gu.restate_cut(array_data, descs, index, gu.IDENTITY)
    assert ref["skipped"] == su.reference_stats(array_data, descs, index)["skipped"] == 8
    for k in range(4):
        assert ref["offsets"][k][-1] == ref["counts"][k] == len(ref["nodes"][k]) and (np.diff(ref["nodes"][k]["prim"].astype(np.int64)) >= 0).all()
    tb = lu.bounds_table(ot.IDX_U16)
    ref = gu.restate_cut(tb["array"], tb["descs"], [r[0] for r in tb["rows"]], gu.IDENTITY)
    assert ref["skipped"] == sum(1 for r in tb["rows"] if r[1] == lu.INVALID)


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


REFUSED = [
    ("unknown indexFormat", lambda: result_desc(index_format=3), lambda: gu.c_desc(gu.PRESET), "indexFormat"),
    ("listOfState 4", lambda: result_desc(), lambda: gu.c_desc(gu.GDesc((0, 4, 1, 1), 1, 12)), "listOfState"),
    ("listOfState 0xFE", lambda: result_desc(), lambda: gu.c_desc(gu.GDesc((0, 1, 1, 0xFE), 1, 12)), "listOfState"),
    ("mixedList 7", lambda: result_desc(), lambda: gu.c_desc(gu.GDesc((0, 1, 1, 1), 7, 12)), "mixedList"),
    ("reserved[0]", lambda: result_desc(), lambda: gu.c_desc(gu.PRESET, (1, 0, 0)), "reserved"),
    ("reserved[2]", lambda: result_desc(), lambda: gu.c_desc(gu.PRESET, (0, 0, 0x80)), "reserved"),
    ("null indexBuffer", lambda: null_field("indexBuffer"), lambda: gu.c_desc(gu.PRESET), "null array"),
    ("null descArray", lambda: null_field("descArray"), lambda: gu.c_desc(gu.PRESET), "null array"),
    ("null arrayData", lambda: null_field("arrayData"), lambda: gu.c_desc(gu.PRESET), "null array"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    _, make_result, make_desc, words = case
    counts = (C.c_uint64 * 4)(7, 7, 7, 7)
    r = lib.dll.ommxExtractMicroGeometry(baker, C.byref(make_result()), C.byref(make_desc()), None, counts, None, None)
    assert r == ot.INVALID_ARGUMENT
    assert len(msgs) == 1 and msgs[0][0] == FATAL and words in msgs[0][1], msgs


def test_handles_and_the_empty_result(session):
    lib, baker, msgs = session
    rd, gd, counts, skipped = result_desc(), gu.c_desc(gu.PRESET), (C.c_uint64 * 4)(7, 7, 7, 7), C.c_uint32(9)
    call = lib.dll.ommxExtractMicroGeometry
    assert call(None, C.byref(rd), C.byref(gd), None, counts, None, None) == ot.INVALID_ARGUMENT and not msgs
    assert call(baker, None, C.byref(gd), None, counts, None, None) == ot.INVALID_ARGUMENT and "deviceResult" in msgs[-1][1]
    assert call(baker, C.byref(rd), None, None, counts, None, None) == ot.INVALID_ARGUMENT and "ommxMicroGeometryDesc" in msgs[-1][1]
    assert call(baker, C.byref(rd), C.byref(gd), None, None, None, None) == ot.INVALID_ARGUMENT and "outCounts" in msgs[-1][1]
    assert len(msgs) == 3 and all(m[0] == FATAL for m in msgs) and list(counts) == [7, 7, 7, 7]
    # indexCount == 0: SUCCESS with zero counts and no launch, whatever the pointers are
    empty = result_desc(index_count=0)
    out = gu.MicroGeometryOutputs()
    assert call(baker, C.byref(empty), C.byref(gd), C.byref(out), counts, C.byref(skipped), None) == ot.SUCCESS
    assert list(counts) == [0, 0, 0, 0] and skipped.value == 0 and len(msgs) == 3


def test_expand_argument_checks():
    dll = gu.bind(C.CDLL(ot.product_path()))
    mesh = gu.MicroMeshDesc(PTR, 12, PTR, ot.IDX_U32, 4)
    assert dll.ommxExpandMicroNodes(PTR, 0, None, PTR, None, None) == ot.SUCCESS              # count 0: no launch
    assert dll.ommxExpandMicroNodes(PTR, 0, C.byref(mesh), PTR, PTR, None) == ot.SUCCESS
    assert dll.ommxExpandMicroNodes(PTR, 5, None, PTR, PTR, None) == ot.INVALID_ARGUMENT      # positions without a mesh
    for stride in (8, 13, 14, 18):
        bad = gu.MicroMeshDesc(PTR, stride, PTR, ot.IDX_U32, 4)
        assert dll.ommxExpandMicroNodes(PTR, 5, C.byref(bad), PTR, PTR, None) == ot.INVALID_ARGUMENT
    assert dll.ommxExpandMicroNodes(PTR, 5, C.byref(gu.MicroMeshDesc(PTR, 12, PTR, 3, 4)), PTR, PTR, None) == ot.INVALID_ARGUMENT
    assert dll.ommxExpandMicroNodes(PTR, 5, C.byref(gu.MicroMeshDesc(None, 12, PTR, ot.IDX_U32, 4)), PTR, PTR, None) == ot.INVALID_ARGUMENT
    assert dll.ommxExpandMicroNodes(None, 5, None, PTR, None, None) == ot.INVALID_ARGUMENT


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxMicroGeometryDesc), offsetof(ommxMicroGeometryDesc, mixedList), offsetof(ommxMicroGeometryDesc, maxEmitLevel),
           sizeof(ommxMicroNode), (size_t)OMMX_GEOMETRY_DROP);
    printf("%zu %zu %zu\n", sizeof(ommxMicroGeometryOutputs), offsetof(ommxMicroGeometryOutputs, capacity), offsetof(ommxMicroGeometryOutputs, primitiveOffsets));
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxMicroMeshDesc), offsetof(ommxMicroMeshDesc, positionStrideInBytes), offsetof(ommxMicroMeshDesc, indexBuffer),
           offsetof(ommxMicroMeshDesc, indexFormat), offsetof(ommxMicroMeshDesc, triangleCount));
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    a, b, c = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    G, O, M = gu.MicroGeometryDesc, gu.MicroGeometryOutputs, gu.MicroMeshDesc
    assert a == [C.sizeof(G), G.mixedList.offset, G.maxEmitLevel.offset, gu.NODE.itemsize, gu.DROP] == [12, 4, 8, 8, 255]
    assert b == [C.sizeof(O), O.capacity.offset, O.primitiveOffsets.offset] == [96, 32, 64]
    assert c == [C.sizeof(M), M.positionStrideInBytes.offset, M.indexBuffer.offset, M.indexFormat.offset, M.triangleCount.offset] == [32, 8, 16, 24, 28]
