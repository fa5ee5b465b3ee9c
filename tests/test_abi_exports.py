"""CPU-side checks of the drop-in boundary: the shared library loads without a GPU and exports every symbol that
include/*.h declares; struct layouts match the SDK's (sizes the reference itself asserts)."""
import ctypes as C
import os
import re
import pytest
import ommtest as ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = []
    for h in ("omm_mi355x.h", "omm_mi355x_ext.h"):
        src = open(os.path.join(ROOT, "include", h)).read()
        names += re.findall(r"OMM_MI355X_API\s+[\w\s\*]+?\b(omm\w+)\s*\(", src)
    return sorted(set(names))


def test_library_exports_every_declared_symbol():
    path = ot.product_path()
    if not os.path.exists(path):
        pytest.fail("libomm-lib.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` first")
    dll = C.CDLL(path)
    names = declared_symbols()
    assert len(names) >= 25, names
    missing = [n for n in names if not hasattr(dll, n)]
    assert not missing, missing
    dll.ommGetLibraryDesc.restype = C.c_uint32  # 3 bytes in a register
    v = dll.ommGetLibraryDesc()
    assert (v & 0xff, (v >> 8) & 0xff, (v >> 16) & 0xff) == (1, 9, 0)


def sdk_exports():
    return open(os.path.join(ROOT, "tests", "golden", "sdk_exports.txt")).read().split()


def test_every_export_of_the_sdk_library_is_present(tmp_path):
    """The SDK's libomm-lib exports the 25 OMM_API functions of its omm.h.  The drop-in exports the same set under
    the same SONAME, so a binary linked against the SDK library -- whichever of them it references -- loads against this one.
    The list is a committed fixture; it is re-derived from the SDK header where the reference checkout exists."""
    import subprocess
    names = sdk_exports()
    assert len(names) == 25
    ref_h = "/root/reference/libraries/omm-lib/include/omm.h"
    if os.path.exists(ref_h):
        src = open(ref_h).read()
        assert sorted(set(re.findall(r"OMM_API\s+\w+\s+(?:OMM_CALL\s+)?(omm\w+)\s*\(", src))) == names
    path = ot.product_path()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = {ln.split()[-1] for ln in dyn.splitlines() if " T " in ln}
    assert not [n for n in names if n not in exported]
    assert set(declared_symbols()) >= set(names)          # and every one of them is declared in include/omm_mi355x.h
    assert "libomm-lib.so" in subprocess.check_output(["readelf", "-d", path], text=True).split("SONAME")[1].splitlines()[0]
    # a program that references every one of the 25 symbols links against the drop-in and loads (no GPU needed: nothing is called)
    src = tmp_path / "all_symbols.c"
    src.write_text("#include <stdio.h>\n" + "".join("extern void %s(void);\n" % n for n in names) +
                   "int main(void) { void (*f[])(void) = { %s }; unsigned k = 0, i; for (i = 0; i < sizeof f / sizeof f[0]; ++i) k += f[i] != 0; printf(\"%%u\\n\", k); return 0; }\n"
                   % ", ".join(names))
    lib_dir = os.path.dirname(path)
    exe = str(tmp_path / "all_symbols")
    r = subprocess.run(["gcc", str(src), "-o", exe, "-L" + lib_dir, "-lomm-lib", "-Wl,-rpath," + lib_dir, "-Wl,--no-as-needed"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.check_output([exe], text=True).strip() == "25"


class _Blob(C.Structure):
    _fields_ = [("data", C.c_void_p), ("size", C.c_uint64)]


def test_gpu_baker_and_debug_entry_points_answer_like_the_sdk(tmp_path):
    """ommBakerType_GPU bakers are creatable (support/tests/test_basic.cpp:46-51); the SDK's GPU-baker / PNG-dump entry points validate their
    arguments like src/bake.cpp:262-336 and then answer NOT_IMPLEMENTED with a log line; ommDebugSaveBinaryToDisk writes the blob
    (debug_impl.cpp:654-670).  None of this touches the device."""
    NOT_IMPLEMENTED = 4
    lib = ot.Lib("product")
    dll = lib.dll
    msgs = []
    gpu = lib.create_baker(baker_type=0, callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    cpu = ot.Lib("product").create_baker()    # (a Lib keeps ONE callback object alive: the second baker comes from a second Lib)
    dummy = C.c_uint64(0)
    out = C.c_void_p(0x1234)
    dll.ommGpuCreatePipeline.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    assert dll.ommGpuCreatePipeline(None, C.byref(dummy), C.byref(out)) == ot.INVALID_ARGUMENT
    assert dll.ommGpuCreatePipeline(gpu, None, C.byref(out)) == ot.INVALID_ARGUMENT
    assert dll.ommGpuCreatePipeline(cpu, C.byref(dummy), C.byref(out)) == ot.INVALID_ARGUMENT           # "[Invalid Arg] - invalid baker type"
    assert dll.ommGpuCreatePipeline(gpu, C.byref(dummy), C.byref(out)) == NOT_IMPLEMENTED and not out.value
    assert msgs and msgs[-1][0] == 3 and "ommGpuCreatePipeline" in msgs[-1][1]
    dll.ommGpuDestroyPipeline.argtypes = [C.c_void_p, C.c_void_p]
    assert dll.ommGpuDestroyPipeline(gpu, None) == ot.INVALID_ARGUMENT
    assert dll.ommGpuDestroyPipeline(cpu, C.c_void_p(8)) == ot.INVALID_ARGUMENT
    for name in ("ommGpuGetPipelineDesc",):
        getattr(dll, name).argtypes = [C.c_void_p, C.c_void_p]
        assert getattr(dll, name)(None, None) == ot.INVALID_ARGUMENT
        assert getattr(dll, name)(C.c_void_p(8), None) == NOT_IMPLEMENTED
    for name in ("ommGpuGetPreDispatchInfo", "ommGpuDispatch"):
        getattr(dll, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        assert getattr(dll, name)(None, C.byref(dummy), None) == ot.INVALID_ARGUMENT
        assert getattr(dll, name)(C.c_void_p(8), None, None) == ot.INVALID_ARGUMENT
        assert getattr(dll, name)(C.c_void_p(8), C.byref(dummy), None) == NOT_IMPLEMENTED
    dll.ommGpuGetStaticResourceData.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
    n = C.c_size_t(0)
    assert dll.ommGpuGetStaticResourceData(11, None, C.byref(n)) == NOT_IMPLEMENTED
    dll.ommDebugSaveAsImages.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert dll.ommDebugSaveAsImages(cpu, None, None, C.byref(dummy)) == ot.INVALID_ARGUMENT
    assert dll.ommDebugSaveAsImages(cpu, C.byref(dummy), None, C.byref(dummy)) == NOT_IMPLEMENTED
    # ommDebugSaveBinaryToDisk
    dll.ommDebugSaveBinaryToDisk.argtypes = [C.c_void_p, C.POINTER(_Blob), C.c_char_p]
    payload = bytes(range(256)) * 3
    buf = C.create_string_buffer(payload, len(payload))
    blob = _Blob(C.cast(buf, C.c_void_p), len(payload))
    path = str(tmp_path / "blob.bin").encode()
    assert dll.ommDebugSaveBinaryToDisk(None, C.byref(blob), path) == ot.INVALID_ARGUMENT
    assert dll.ommDebugSaveBinaryToDisk(cpu, C.byref(blob), None) == ot.INVALID_ARGUMENT
    assert dll.ommDebugSaveBinaryToDisk(cpu, C.byref(blob), path) == ot.SUCCESS
    assert open(path, "rb").read() == payload
    assert dll.ommDebugSaveBinaryToDisk(gpu, C.byref(blob), str(tmp_path / "no_such_dir" / "x.bin").encode()) == ot.INVALID_ARGUMENT
    assert "Unable to save file" in msgs[-1][1] and msgs[-1][0] == 2
    # ommDebugGetStats2 argument checks (bake.cpp:359-362)
    st = ot.DebugStats()
    assert lib.fn("ommDebugGetStats2")(None, None, C.byref(st)) == ot.INVALID_ARGUMENT
    assert lib.fn("ommDebugGetStats2")(cpu, None, C.byref(st)) == ot.INVALID_ARGUMENT
    assert lib.destroy_baker(gpu) == ot.SUCCESS and lib.destroy_baker(cpu) == ot.SUCCESS


def test_struct_layouts():
    assert C.sizeof(ot.BakeInputDesc) == 136          # serialize_impl.cpp:86
    assert C.sizeof(ot.BakeResultDesc) == 80
    assert C.sizeof(ot.MicromapDesc) == 8 and C.sizeof(ot.UsageCount) == 8
    assert C.sizeof(ot.TextureDesc) == 24 and C.sizeof(ot.TextureMipDesc) == 24
    assert ot.BakeInputDesc.maxWorkloadSize.offset == 128 and ot.BakeInputDesc.subdivisionLevels.offset == 120
    assert ot.BakeInputDesc.maxSubdivisionLevel.offset == 112 and ot.BakeInputDesc.maxArrayDataSize.offset == 116


def test_host_side_argument_checks_need_no_gpu():
    """entry points reject bad handles before touching the device (bake.cpp:36-135)"""
    dll = C.CDLL(ot.product_path())
    assert dll.ommCreateBaker(None, None) == ot.INVALID_ARGUMENT
    assert dll.ommDestroyBaker(None) == ot.INVALID_ARGUMENT
    assert dll.ommCpuBake(None, None, None) == ot.INVALID_ARGUMENT
    assert dll.ommCpuDestroyBakeResult(None) == ot.INVALID_ARGUMENT
    assert dll.ommCpuGetBakeResultDesc(None, None) == ot.INVALID_ARGUMENT
    lib = ot.Lib("product")
    b = lib.create_baker(baker_type=0)               # ommBakerType_GPU bakers can be created but do not bake (test_basic.cpp:46-51)
    d = ot.default_bake_desc()
    assert lib.bake_raw(b, d)[0] == ot.INVALID_ARGUMENT
    assert lib.destroy_baker(b) == ot.SUCCESS
    b = lib.create_baker()
    assert lib.bake_raw(b, d)[0] == ot.INVALID_ARGUMENT   # no texture set
    assert lib.destroy_baker(b) == ot.SUCCESS


def test_no_cpu_fallback_without_a_gpu():
    """the product has no CPU path.  On a machine without a HIP device texture creation (the first call that
    needs HBM) fails loudly -- FAILURE + a Fatal log line -- instead of computing anything on the host."""
    hip = C.CDLL("libamdhip64.so")
    n = C.c_int(0)
    if hip.hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a HIP device is present: the fail-loudly path cannot be exercised here")
    import numpy as np
    lib = ot.Lib("product")
    msgs = []
    b = lib.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    t = lib.create_texture(b, [np.zeros((16, 16), np.float32)], expect=ot.FAILURE)
    assert t is None
    assert msgs and msgs[-1][0] == 3 and "no CPU fallback" in msgs[-1][1], msgs       # ommMessageSeverity_Fatal
    assert lib.destroy_baker(b) == ot.SUCCESS


def _build_example(std_args, out):
    import subprocess
    lib_dir = os.path.join(ROOT, "omm_amd", "lib")
    cmd = std_args + ["-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "minimal_sample.c"), "-o", out,
                      "-L" + lib_dir, "-lomm-lib", "-lm", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr


def test_header_is_valid_c99_and_cpp17_and_the_example_links(tmp_path):
    """include/omm_mi355x.h is what a C or C++ caller compiles against: examples/minimal_sample.c builds warning-free in both languages
    and links against the drop-in library"""
    _build_example(["gcc", "-std=c99", "-pedantic"], str(tmp_path / "sample_c"))
    _build_example(["g++", "-std=c++17", "-x", "c++"], str(tmp_path / "sample_cpp"))


def _abi_facts(include_dir, header, tmp_path, tag):
    import subprocess
    exe = str(tmp_path / ("abi_" + tag))
    subprocess.check_call(["g++", "-std=c++17", "-x", "c++", "-Wno-deprecated-declarations", "-I" + include_dir, "-DOMM_HEADER=" + header,
                           os.path.join(ROOT, "tests", "native", "abi_layout.c"), "-o", exe])
    return subprocess.check_output([exe], text=True)


def test_struct_layouts_and_enum_values_equal_the_sdk_header(tmp_path):
    """146 sizeof / offsetof / enumerator facts of the CPU-baker interface: include/omm_mi355x.h vs the SDK's omm.h (committed output of
    the same probe compiled against the SDK header; regenerated and re-checked when the reference checkout is present)"""
    mine = _abi_facts(os.path.join(ROOT, "include"), '"omm_mi355x.h"', tmp_path, "mine")
    golden = open(os.path.join(ROOT, "tests", "golden", "abi_layout_sdk.txt")).read()
    assert mine == golden
    sdk = "/root/reference/libraries/omm-lib/include"
    if os.path.exists(os.path.join(sdk, "omm.h")):
        assert _abi_facts(sdk, "<omm.h>", tmp_path, "sdk") == golden


def sdk_user_symbols():
    return open(os.path.join(ROOT, "tests", "golden", "sdk_user_symbols.txt")).read().split()


def test_sdk_header_user_links_against_the_drop_in(tmp_path):
    """A translation unit compiled against the SDK's OWN omm.h / omm.hpp (tests/native/sdk_user*.cpp) links against libomm-lib.so: every
    CPU-baker symbol it references resolves.  The symbols those units reference are a committed fixture (tests/golden/sdk_user_symbols.txt):
    a program that references exactly them links and loads.  Where the SDK headers exist the units themselves are compiled, linked and
    run, and their references are re-checked against the fixture."""
    import subprocess
    names = sdk_user_symbols()
    assert len(names) == 16 and set(names) <= set(sdk_exports()), names
    lib_dir = os.path.join(ROOT, "omm_amd", "lib")
    src = tmp_path / "sdk_user_symbols.c"
    src.write_text("#include <stdio.h>\n" + "".join("extern void %s(void);\n" % n for n in names) +
                   "int main(void) { void (*f[])(void) = { %s }; unsigned k = 0, i; for (i = 0; i < sizeof f / sizeof f[0]; ++i) k += f[i] != 0; printf(\"%%u\\n\", k); return 0; }\n"
                   % ", ".join(names))
    exe = str(tmp_path / "sdk_user_symbols")
    r = subprocess.run(["gcc", str(src), "-o", exe, "-L" + lib_dir, "-lomm-lib", "-Wl,-rpath," + lib_dir, "-Wl,--no-as-needed"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.check_output([exe], text=True).strip() == str(len(names))
    sdk = "/root/reference/libraries/omm-lib/include"
    if not os.path.exists(os.path.join(sdk, "omm.h")):
        return
    referenced = set()
    for unit in ("sdk_user", "sdk_user_hpp"):
        obj, exe = str(tmp_path / (unit + ".o")), str(tmp_path / unit)
        r = subprocess.run(["g++", "-std=c++17", "-Wno-deprecated-declarations", "-I" + sdk, "-c", os.path.join(ROOT, "tests", "native", unit + ".cpp"), "-o", obj],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        referenced |= {ln.split()[-1] for ln in subprocess.check_output(["nm", "-u", obj], text=True).splitlines() if ln.split()[-1].startswith("omm")}
        r = subprocess.run(["g++", obj, "-o", exe, "-L" + lib_dir, "-lomm-lib", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert sorted(referenced) == names
    assert subprocess.run([exe]).returncode == 0      # (the omm.hpp user) baker create/destroy and the argument checks need no GPU


def test_baker_knobs_are_per_baker_state_not_environment():
    """ommxSetBakerKnob (include/omm_mi355x_ext.h) replaces the getenv() hooks of earlier rounds: switches belong to ONE baker, out-of-range values and
    unknown knobs are refused, and the library never looks at the process environment (no getenv among its undefined symbols)."""
    import subprocess
    path = ot.product_path()
    dll = C.CDLL(path)
    dll.ommxSetBakerKnob.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    lib = ot.Lib("product")
    b = lib.create_baker()          # (no GPU needed: a baker is host state until its first texture)
    assert dll.ommxSetBakerKnob(b, ot.KNOB_RESERVED0, 6) == ot.SUCCESS            # (the retired test switch of rounds 1 - 5: accepted, no effect)
    assert dll.ommxSetBakerKnob(b, ot.KNOB_HELPER_AFFINITY, 1) == ot.SUCCESS and dll.ommxSetBakerKnob(b, ot.KNOB_HELPER_AFFINITY, 2) == ot.INVALID_ARGUMENT
    assert dll.ommxSetBakerKnob(b, ot.KNOB_ZERO_AHEAD, 1) == ot.SUCCESS and dll.ommxSetBakerKnob(b, ot.KNOB_ZERO_AHEAD, 2) == ot.INVALID_ARGUMENT
    assert dll.ommxSetBakerKnob(b, ot.KNOB_SHARD_CHUNK_BYTES, 100) == ot.INVALID_ARGUMENT
    assert dll.ommxSetBakerKnob(b, ot.KNOB_SHARD_CHUNK_BYTES, 4352) == ot.SUCCESS
    assert dll.ommxSetBakerKnob(b, ot.KNOB_STREAM_CHUNKS, 3) == ot.SUCCESS
    assert dll.ommxSetBakerKnob(b, ot.KNOB_STREAM_CHUNKS, 33) == ot.INVALID_ARGUMENT     # at most 32 ranges (two queue sections each)
    assert dll.ommxSetBakerKnob(b, ot.KNOB_GENERIC_PASS, 2) == ot.SUCCESS
    assert dll.ommxSetBakerKnob(b, ot.KNOB_GENERIC_PASS, 3) == ot.INVALID_ARGUMENT
    assert dll.ommxSetBakerKnob(b, ot.KNOB_RETAIN_MEMORY, 1) == ot.SUCCESS and dll.ommxSetBakerKnob(b, ot.KNOB_RETAIN_MEMORY, 2) == ot.INVALID_ARGUMENT
    dll.ommxTrimBaker.argtypes = [C.c_void_p]
    assert dll.ommxTrimBaker(b) == ot.SUCCESS and dll.ommxTrimBaker(None) == ot.INVALID_ARGUMENT
    assert dll.ommxSetBakerKnob(b, 99, 1) == ot.INVALID_ARGUMENT
    assert dll.ommxSetBakerKnob(None, ot.KNOB_STREAM_CHUNKS, 3) == ot.INVALID_ARGUMENT
    lib.destroy_baker(b)
    # the library's OWN objects do not read the environment (switches are baker knobs); the one getenv import of the shared object comes from the
    # rocPRIM headers inside the two kernel files that use its scans and sorts (ROCPRIM_USE_ATOMIC_BLOCK_ID; INTEGRATION.md says so)
    objdir = os.path.join(os.path.dirname(path), "obj")
    for o in ("omm_host.o", "host_tail.o", "bake_kernels.o"):
        if os.path.exists(os.path.join(objdir, o)):
            undefined = subprocess.check_output(["nm", "--undefined-only", os.path.join(objdir, o)], text=True)
            assert not any(w.split("@")[0] == "getenv" for w in undefined.split()), o


def test_poison_knob_argument_rules_and_its_counters_need_no_gpu():
    """ommxBakerKnob_PoisonMemory (knob 10) and ommxDebugGetPoisonedBytes: off, or bit 32 | a 32-bit word -- anything else is refused; knob 11 does
    not exist; a baker that never filled anything reports zeros; either output pointer may be null, the baker may not."""
    lib = ot.Lib("product")
    dll = lib.dll
    dll.ommxSetBakerKnob.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    dll.ommxDebugGetPoisonedBytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    assert ot.KNOB_POISON == 10
    b = lib.create_baker()
    for word in (0x00000000, 0x00000001, 0xFFFFFFFF, 0xA5A5A5A5):
        assert ot.poison(word) == (1 << 32) | word
        assert dll.ommxSetBakerKnob(b, ot.KNOB_POISON, ot.poison(word)) == ot.SUCCESS
    for bad in (1, 0xA5A5A5A5, 0xFFFFFFFF, 1 << 33, (1 << 33) | (1 << 32) | 5, 1 << 63):
        assert dll.ommxSetBakerKnob(b, ot.KNOB_POISON, bad) == ot.INVALID_ARGUMENT, hex(bad)
    assert dll.ommxSetBakerKnob(b, ot.KNOB_POISON, 0) == ot.SUCCESS
    assert dll.ommxSetBakerKnob(b, 11, 0) == ot.INVALID_ARGUMENT and dll.ommxSetBakerKnob(b, 11, ot.poison(0)) == ot.INVALID_ARGUMENT
    assert lib.poisoned_bytes(b) == (0, 0)
    one = C.c_uint64(77)
    assert dll.ommxDebugGetPoisonedBytes(b, C.byref(one), None) == ot.SUCCESS and one.value == 0
    one = C.c_uint64(77)
    assert dll.ommxDebugGetPoisonedBytes(b, None, C.byref(one)) == ot.SUCCESS and one.value == 0
    assert dll.ommxDebugGetPoisonedBytes(b, None, None) == ot.SUCCESS
    untouched = C.c_uint64(77)
    assert dll.ommxDebugGetPoisonedBytes(None, C.byref(untouched), C.byref(untouched)) == ot.INVALID_ARGUMENT and untouched.value == 77
    lib.destroy_baker(b)


def test_timings_struct_of_the_extension_header_matches_its_python_mirror():
    """ommxBakeTimings (include/omm_mi355x_ext.h) only ever grows at its end; ommxGetLastBakeTimingsSized reports the library's size of it, which must be
    the size of bench.py's ctypes mirror (a mirror that lags behind the header would read garbage through the unsized getter)."""
    import bench
    dll = C.CDLL(ot.product_path())
    dll.ommxGetLastBakeTimingsSized.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib = ot.Lib("product")
    b = lib.create_baker()
    n = C.c_size_t(0)
    tm = bench.BakeTimings()
    r = dll.ommxGetLastBakeTimingsSized(b, C.byref(tm), C.sizeof(tm), C.byref(n))
    assert r == ot.FAILURE            # no bake yet on this baker
    assert n.value == C.sizeof(bench.BakeTimings), (n.value, C.sizeof(bench.BakeTimings))
    assert dll.ommxGetLastBakeTimingsSized(None, C.byref(tm), C.sizeof(tm), None) == ot.INVALID_ARGUMENT
    lib.destroy_baker(b)
