"""The gather kernels of ommxCreateTextureDevice (omm_amd/csrc/texture_kernels.hip) without a GPU: the kernel source compiles as host C++ against a
shim of the HIP language (tests/native/hip_host_shim) and runs, lane by lane, under AddressSanitizer and the alignment sanitizer -- a stand-alone
program, tests/native/texture_gather_host.cpp.  Sources are exact-size heap blocks, so a load that starts before a mip's first pixel, ends behind
its last one, or is wider than its address allows stops the program; every layout path (the wide ones, the per-texel one, odd strides), offset,
tight / padded pitch and base alignment is run at the widths where groups, peels and ragged ends change, and all 65 536 halves are widened."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_paths_stay_inside_their_rows_and_extract_the_channel(tmp_path):
    exe = str(tmp_path / "texture_gather_host")
    native = os.path.join(ROOT, "tests", "native")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-mf16c", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function",
                        "-I" + os.path.join(native, "hip_host_shim"), "-I" + os.path.join(ROOT, "omm_amd", "csrc"),
                        os.path.join(native, "texture_gather_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    assert int(r.stdout.split()[1]) == 35 * 11 * 3 * 2 * 3
