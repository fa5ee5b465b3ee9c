"""ommxProfileMicromapLevels, ommxCoarsenMicromapLevels and ommxFitMicromap without a GPU: the counting of omm_amd/csrc/profile_count.h and the planner
of omm_amd/csrc/fit_plan.h as plain C++ under the sanitizers (tests/native/fit_check.cpp), the numpy and Python statements of tests/fit_util.py held
to loops over single states and to the native planner, the properties the header promises, the designed input on which the per-block plan provably
beats every global cap, the symbols and struct layouts, and every argument check -- all of them are made before the device is touched."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import ommtest as ot
import stats_util as su
import coarsen_util as cu
import fit_util as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3
SENTINEL = 0x5EED5EED


@pytest.fixture(scope="module")
def fit_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fit") / "fit_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "fit_check.cpp"), "-o", exe], check=True)
    return exe


def test_counting_and_planner_as_host_code(fit_check):
    """profile_count.h == a loop over single states (exhaustive on 8-field groups, planted random words, both formats, validity masks for 1, 4, 16 and 64
    fields with zeros and with garbage above); fit_plan.h == a planner that rescans every candidate at every step, on seeded tables that hold ties, zero
    weights, chain ends, free blocks and infeasible budgets.  A stand-alone program under AddressSanitizer and UBSan, run directly."""
    r = subprocess.run([fit_check], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert " 0 failures" in r.stdout and int(r.stdout.split("fit_check:")[1].split()[0]) > 500000, r.stdout


def test_python_plan_equals_the_native_plan(fit_check):
    """the tables the program plans, printed by it, through fit_util.restate_plan: feasibility, both sizes, the step count and every level"""
    out = subprocess.run([fit_check, "tables"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    tables, ties, infeasible = 0, 0, 0
    lines = iter(out.stdout.splitlines())
    for line in lines:
        if not line.startswith("table "):
            continue
        D, max_level, special, budget = (int(x) for x in line.split()[1:])
        shape, known, opaque, weights = [], [], [], []
        for _ in range(D):
            row = [int(x) for x in next(lines).split()[1:]]
            shape.append(((row[0] >> 2) & 0xFF, row[0] & 3) if row[0] >> 31 else None)
            weights.append(row[1])
            known.append(row[2::2])
            opaque.append(row[3::2])
        want = [int(x) for x in next(lines).split()[1:]]
        plan = fu.restate_plan(shape, known, opaque, weights, budget, max_level, bool(special))
        assert [int(plan["feasible"]), plan["unfitted"], plan["planned"], plan["steps"]] + plan["levels"] == want, (tables, plan, want)
        tables, ties, infeasible = tables + 1, ties + plan["ties"], infeasible + (not plan["feasible"])
    assert tables == 120 and ties > 0 and infeasible > 0


def test_profile_restatement_equals_the_loops():
    """known_counts (numpy) == brute_known_counts (loops over single states): every 2-state block of levels 0..2 exhaustively, planted blocks of levels
    0..4 in both formats; the weights against exact fractions"""
    n = 0
    for level in (0, 1, 2):
        for word in range(1 << (4 ** level)):
            states = [(word >> i) & 1 for i in range(4 ** level)]
            assert fu.known_counts(states, level) == fu.brute_known_counts(states, level)
            n += 1
    for seed in range(60):
        for level in range(5):
            for bits in (1, 2):
                states = cu.planted_states(level, bits, seed)
                got = fu.known_counts(states, level)
                assert got == fu.brute_known_counts(states.tolist(), level)
                assert all(got[0][t - 1] * 4 <= got[0][t] and got[1][t - 1] * 4 <= got[1][t] for t in range(1, level + 1)) and got[0][level + 1:] == [0] * (12 - level)
                assert got[0][level] == int((states < 2).sum()) and got[1][level] == int((states == 1).sum())
                n += 1
    assert n > 66000
    # the weights: exact, below 2^32, the largest in [2^31, 2^32); what is not finite and positive counts 0
    w = np.array([np.nan, -1.0, np.inf, 0.0, 1e-45, 3.4028234663852886e38, 1.5, -np.inf, 2.5e-39], np.float32)
    q, e = fu.weight_units(w)
    assert e == 127 and q == [0, 0, 0, 0, 0, (1 << 32) - (1 << 8), 0, 0, 0]
    q, e = fu.weight_units(w[[0, 4, 8]])          # subnormals alone: the largest is 2.5e-39
    assert e == -129 and q[0] == 0 and q[1] == 1 << (31 + 129 - 149) and (1 << 31) <= q[2] < (1 << 32)
    q, e = fu.weight_units(np.array([0.75, 0.1, 3.0], np.float32))
    assert e == 1 and q == [0.75 * 2 ** 30, int(float(np.float32(0.1)) * 2 ** 30), 3 << 30]
    assert fu.weight_units(np.array([np.nan, 0.0], np.float32)) == ([0, 0], 0) and fu.weight_units([]) == ([], 0)
    # the numpy statement used for a million weights == the exact one
    rng = np.random.default_rng(3)
    for scale in (1e-42, 1e-30, 1.0, 1e30):
        w = np.concatenate([w, (rng.random(500) * scale).astype(np.float32), rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32).view(np.float32)])
        q, e = fu.weight_units(w)
        qn, en = fu.weight_units_numpy(w)
        assert e == en and q == [int(x) for x in qn]


def _mixed_table(seed, count, max_level=4):
    rng = np.random.default_rng(seed)
    blocks = []
    for k in range(count):
        level, bits = int(rng.integers(0, max_level + 1)), int(rng.integers(1, 3))
        blocks.append((cu.planted_states(level, bits, seed * 100 + k), level, bits))
    array_data, descs = cu.table_of_blocks(blocks, first_offset=seed % 3, gap=seed % 2)
    index = np.concatenate([np.arange(count), rng.integers(-5, count + 1, 3 * count)])
    weights = (rng.random(len(index)) * 4 + 0.01).astype(np.float32)
    return array_data, descs, index, weights


def test_properties_of_the_model():
    """levels are monotone in the budget; result.arrayDataSize <= plannedArrayDataSize <= budget; a budget at or above the unfitted size takes no step and
    equals restate_coarsen at the cap; the step sequence of a tighter budget extends that of a looser one"""
    for seed in range(6):
        array_data, descs, index, weights = _mixed_table(seed, 12 + seed)
        unpacked = {}
        prof = fu.restate_profile(array_data, descs, index, weights if seed % 2 else None, unpacked=unpacked)
        for d in range(len(descs)):
            if prof["shape"][d] is not None:      # (the property holds up to the block's own level; above it the row is zero)
                assert all(int(prof["known"][d][t - 1]) * 4 <= int(prof["known"][d][t]) for t in range(1, prof["shape"][d][0] + 1))
                assert not prof["known"][d][prof["shape"][d][0] + 1:].any()
        for flags, cap in ((fu.NONE, 12), (fu.NO_SPECIAL, 3), (fu.NO_DEDUP, 2)):
            whole, res = fu.restate_fit(array_data, descs, index, ot.IDX_U16, 1 << 40, max_level=cap, flags=flags, profile=prof, unpacked=unpacked)
            assert whole["steps"] == 0 and whole["planned"] == whole["unfitted"]
            same = cu.restate_coarsen(array_data, descs, index, ot.IDX_U16, cap, 3, flags, unpacked=unpacked)
            cu.assert_same(res, same)
            assert res["info"] == same["info"] and same["info"]["arrayDataSize"] <= whole["unfitted"]
            last, last_steps = None, None
            for budget in sorted({0, 1, 5, whole["unfitted"] // 7, whole["unfitted"] // 3, whole["unfitted"] // 2, whole["unfitted"] - 1, whole["unfitted"]}, reverse=True):
                plan, res = fu.restate_fit(array_data, descs, index, ot.IDX_U16, max(budget, 0), max_level=cap, flags=flags, profile=prof, unpacked=unpacked)
                if not plan["feasible"]:
                    assert flags & fu.NO_SPECIAL and res is None
                    continue
                assert res["info"]["arrayDataSize"] <= plan["planned"] <= budget and plan["unfitted"] == whole["unfitted"]
                if last is not None:
                    assert all(a <= b for a, b in zip(plan["levels"], last)) and plan["stepped"][:len(last_steps)] == last_steps
                last, last_steps = plan["levels"], plan["stepped"]


def test_designed_input_beats_every_global_cap():
    """four blocks of uniform quadrants beside four of alternating states (fit_util.designed_blocks), level 4, 4-state: 64 bytes each.  The quadrant blocks
    keep their whole known share down to level 1 (1 byte); the alternating ones lose all of it at the first step.  At a budget of 4 * 64 + 4 bytes the plan
    takes the quadrant blocks to level 1 and leaves the others alone: the known share is everything.  A global cap that fits the same budget is level 3 or
    below, at which the alternating blocks know nothing: the share is a half.  The plan's share is at least the best cap's at every budget."""
    blocks = fu.designed_blocks(4, 2, 4)
    array_data, descs = cu.table_of_blocks(blocks)
    index = list(range(8))
    prof = fu.restate_profile(array_data, descs, index)
    full = fu.known_share(prof, [4] * 8)
    assert full == 8 * 4 ** 12 and [int(prof["known"][0][t]) for t in range(5)] == [0, 4, 16, 64, 256] and [int(prof["known"][7][t]) for t in range(5)] == [0, 0, 0, 0, 256]
    plan = fu.restate_plan(prof["shape"], prof["known"], prof["opaque"], prof["weights"], 4 * 64 + 4)
    assert plan["levels"] == [1] * 4 + [4] * 4 and plan["planned"] == 260 and fu.known_share(prof, plan["levels"]) == full
    cap, levels = fu.best_global_cap(prof, 4 * 64 + 4)
    assert cap == 3 and fu.known_share(prof, levels) * 2 == full
    strictly = 0
    for budget in range(0, 8 * 64 + 1, 4):
        plan = fu.restate_plan(prof["shape"], prof["known"], prof["opaque"], prof["weights"], budget)
        cap, levels = fu.best_global_cap(prof, budget)
        assert plan["feasible"] and fu.known_share(prof, plan["levels"]) >= fu.known_share(prof, levels)
        strictly += fu.known_share(prof, plan["levels"]) > fu.known_share(prof, levels)
    assert strictly > 60


# ---- the ABI ----
def test_symbols_are_exported():
    dll = C.CDLL(ot.product_path())
    out = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    for name in ("ommxProfileMicromapLevels", "ommxCoarsenMicromapLevels", "ommxFitMicromap"):
        assert hasattr(dll, name)
        assert any(line.split()[-1] == name and line.split()[-2] == "T" for line in out.splitlines() if line.strip()), name


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
#define O(t, f) offsetof(t, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %d\n", sizeof(ommxLevelProfileOutputs), O(ommxLevelProfileOutputs, knownCounts), O(ommxLevelProfileOutputs, knownOpaqueCounts),
           O(ommxLevelProfileOutputs, referenceCounts), O(ommxLevelProfileOutputs, blockWeights), OMMX_PROFILE_LEVELS);
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxLevelProfileInfo), O(ommxLevelProfileInfo, referencedBlocks), O(ommxLevelProfileInfo, skippedPrimitives),
           O(ommxLevelProfileInfo, weightExponent), O(ommxLevelProfileInfo, reserved));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxFitDesc), O(ommxFitDesc, maxArrayDataSize), O(ommxFitDesc, devicePrimitiveWeights), O(ommxFitDesc, maxSubdivisionLevel),
           O(ommxFitDesc, mixedState), O(ommxFitDesc, reserved), O(ommxFitDesc, flags));
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxFitInfo), O(ommxFitInfo, result), O(ommxFitInfo, unfittedArrayDataSize), O(ommxFitInfo, plannedArrayDataSize), O(ommxFitInfo, steps));
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    a, b, c, d = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    layout = lambda S: [C.sizeof(S)] + [getattr(S, f[0]).offset for f in S._fields_]
    assert a == layout(fu.LevelProfileOutputs) + [fu.LEVELS] == [32, 0, 8, 16, 24, 13]
    assert b == layout(fu.LevelProfileInfo) == [16, 0, 4, 8, 12]
    assert c == layout(fu.FitDesc) == [32, 0, 8, 16, 20, 21, 24]
    assert d == layout(fu.FitInfo) == [56, 0, 32, 40, 48]


# ---- the argument checks: refused before the device is touched, each with its log line ----
@pytest.fixture()
def session():
    lib = ot.Lib("product")
    fu.bind(lib.dll)
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


# (name, result, coarsen desc or None where the case is not the desc's, fit desc, words of the log line)
REFUSED = [
    ("unknown indexFormat", lambda: result_desc(index_format=3), lambda: cu.c_desc(4), lambda: fu.f_desc(100), "indexFormat"),
    ("mixedState 0", result_desc, lambda: cu.c_desc(4, mixed=0), lambda: fu.f_desc(100, mixed=0), "mixedState"),
    ("mixedState 4", result_desc, lambda: cu.c_desc(4, mixed=4), lambda: fu.f_desc(100, mixed=4), "mixedState"),
    ("flag bit 2", result_desc, lambda: cu.c_desc(4, flags=4), lambda: fu.f_desc(100, flags=4), "flags"),
    ("reserved[1]", result_desc, lambda: cu.c_desc(4, reserved=(0, 1, 0)), lambda: fu.f_desc(100, reserved=(0, 1, 0)), "reserved"),
    ("null indexBuffer", lambda: null_field("indexBuffer"), lambda: cu.c_desc(4), lambda: fu.f_desc(100), "null array"),
    ("null descArray", lambda: null_field("descArray"), lambda: cu.c_desc(4), lambda: fu.f_desc(100), "null array"),
    ("null arrayData", lambda: null_field("arrayData"), lambda: cu.c_desc(4), lambda: fu.f_desc(100), "null array"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    name, make_result, make_coarsen, make_fit, words = case
    calls = 0
    for want_result in (True, False):
        out, info = C.c_void_p(SENTINEL), cu.CoarsenInfo()
        info.skippedPrimitives = 77
        r = lib.dll.ommxCoarsenMicromapLevels(baker, C.byref(make_result()), PTR, C.byref(make_coarsen()), C.byref(out) if want_result else None, C.byref(info), None)
        calls += 1
        assert r == ot.INVALID_ARGUMENT and out.value == SENTINEL and info.skippedPrimitives == 77
        assert len(msgs) == calls and msgs[-1][0] == FATAL and words in msgs[-1][1] and ("ommxCoarsenDesc" in msgs[-1][1]) == (words in ("mixedState", "flags", "reserved")), msgs
        out, finfo = C.c_void_p(SENTINEL), fu.FitInfo()
        finfo.steps = 77
        r = lib.dll.ommxFitMicromap(baker, C.byref(make_result()), C.byref(make_fit()), PTR, C.byref(out) if want_result else None, C.byref(finfo), None)
        calls += 1
        assert r == ot.INVALID_ARGUMENT and out.value == SENTINEL and finfo.steps == 77
        assert len(msgs) == calls and msgs[-1][0] == FATAL and words in msgs[-1][1] and ("ommxFitDesc" in msgs[-1][1]) == (words in ("mixedState", "flags", "reserved")), msgs
    if words in ("indexFormat", "null array"):
        pinfo, outputs = fu.LevelProfileInfo(), fu.LevelProfileOutputs(PTR, PTR, PTR, PTR)
        pinfo.skippedPrimitives = 77
        r = lib.dll.ommxProfileMicromapLevels(baker, C.byref(make_result()), PTR, C.byref(outputs), C.byref(pinfo), None)
        assert r == ot.INVALID_ARGUMENT and pinfo.skippedPrimitives == 77 and len(msgs) == calls + 1 and msgs[-1][0] == FATAL and words in msgs[-1][1], msgs


def test_handles_and_the_empty_result(session):
    lib, baker, msgs = session
    rd, cd, fd, out = result_desc(), cu.c_desc(4), fu.f_desc(100), C.c_void_p(SENTINEL)
    cinfo, finfo, pinfo, outputs = cu.CoarsenInfo(), fu.FitInfo(), fu.LevelProfileInfo(), fu.LevelProfileOutputs(PTR, PTR, PTR, PTR)
    prof, coarsen, fit = lib.dll.ommxProfileMicromapLevels, lib.dll.ommxCoarsenMicromapLevels, lib.dll.ommxFitMicromap
    # no baker: nobody to tell
    assert prof(None, C.byref(rd), None, C.byref(outputs), C.byref(pinfo), None) == ot.INVALID_ARGUMENT
    assert coarsen(None, C.byref(rd), PTR, C.byref(cd), C.byref(out), C.byref(cinfo), None) == ot.INVALID_ARGUMENT
    assert fit(None, C.byref(rd), C.byref(fd), PTR, C.byref(out), C.byref(finfo), None) == ot.INVALID_ARGUMENT and not msgs
    # the null arguments, each with its line
    assert prof(baker, None, None, C.byref(outputs), C.byref(pinfo), None) == ot.INVALID_ARGUMENT and "deviceResult" in msgs[-1][1]
    assert prof(baker, C.byref(rd), None, None, None, None) == ot.INVALID_ARGUMENT and "outputs" in msgs[-1][1] and "outInfo" in msgs[-1][1]
    assert coarsen(baker, None, PTR, C.byref(cd), C.byref(out), C.byref(cinfo), None) == ot.INVALID_ARGUMENT and "deviceResult" in msgs[-1][1]
    assert coarsen(baker, C.byref(rd), PTR, None, C.byref(out), C.byref(cinfo), None) == ot.INVALID_ARGUMENT and "ommxCoarsenDesc" in msgs[-1][1]
    assert coarsen(baker, C.byref(rd), PTR, C.byref(cd), None, None, None) == ot.INVALID_ARGUMENT and "outResult" in msgs[-1][1] and "outInfo" in msgs[-1][1]
    assert fit(baker, None, C.byref(fd), PTR, C.byref(out), C.byref(finfo), None) == ot.INVALID_ARGUMENT and "deviceResult" in msgs[-1][1]
    assert fit(baker, C.byref(rd), None, PTR, C.byref(out), C.byref(finfo), None) == ot.INVALID_ARGUMENT and "ommxFitDesc" in msgs[-1][1]
    assert fit(baker, C.byref(rd), C.byref(fd), None, None, None, None) == ot.INVALID_ARGUMENT and "outDeviceBlockLevels" in msgs[-1][1]
    assert len(msgs) == 8 and all(m[0] == FATAL for m in msgs) and out.value == SENTINEL
    # a handle that is no baker: the type is the handle's low three bits (4 is a texture's), judged before the handle is followed
    other = C.c_void_p((baker.value & ~7) | 4)
    assert prof(other, C.byref(rd), None, C.byref(outputs), C.byref(pinfo), None) == ot.INVALID_ARGUMENT
    assert coarsen(other, C.byref(rd), PTR, C.byref(cd), C.byref(out), C.byref(cinfo), None) == ot.INVALID_ARGUMENT
    assert fit(other, C.byref(rd), C.byref(fd), PTR, C.byref(out), C.byref(finfo), None) == ot.INVALID_ARGUMENT and out.value == SENTINEL and len(msgs) == 8
    # indexCount == 0: SUCCESS without a launch, whatever the pointers are; the infos are zero, the results are empty and can be destroyed
    empty = result_desc(index_count=0)
    pinfo.referencedBlocks = pinfo.weightExponent = 9
    assert prof(baker, C.byref(empty), PTR, C.byref(outputs), C.byref(pinfo), None) == ot.SUCCESS
    assert [getattr(pinfo, f) for f in fu.PROFILE_INFO_FIELDS] == [0, 0, 0, 0]
    for call in ("coarsen", "fit"):
        out = C.c_void_p(SENTINEL)
        if call == "coarsen":
            cinfo.skippedPrimitives = 9
            assert coarsen(baker, C.byref(empty), PTR, C.byref(cd), C.byref(out), C.byref(cinfo), None) == ot.SUCCESS
            assert cu.info_dict(cinfo) == dict.fromkeys(cu.INFO_FIELDS, 0)
        else:
            finfo.steps = finfo.unfittedArrayDataSize = 9
            assert fit(baker, C.byref(empty), C.byref(fd), PTR, C.byref(out), C.byref(finfo), None) == ot.SUCCESS
            assert fu.fit_info_dict(finfo) == dict(unfittedArrayDataSize=0, plannedArrayDataSize=0, steps=0, result=dict.fromkeys(cu.INFO_FIELDS, 0))
        assert out.value not in (None, SENTINEL)
        pd = C.POINTER(ot.BakeResultDesc)()
        assert lib.dll.ommxGetDeviceBakeResultDesc(out, C.byref(pd)) == ot.SUCCESS
        e = pd.contents
        assert (e.arrayDataSize, e.descArrayCount, e.indexCount, e.descArrayHistogramCount, e.indexHistogramCount) == (0, 0, 0, 0, 0) and not e.arrayData
        assert lib.dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
    assert len(msgs) == 8
