"""The decode kernels of ommxCreateTextureBC7 (omm_amd/csrc/bc7_kernels.hip, bc7_decode.h) without a GPU: the kernel source compiles as host C++
against the shim of the HIP language (tests/native/hip_host_shim) and runs, lane by lane, under AddressSanitizer and the alignment sanitizer -- a
stand-alone program, tests/native/bc7_decode_host.cpp.  Sources and destinations are exact-size heap blocks, so a load outside a row of blocks, a
16-byte load that is not aligned, or a store at or beyond texel w * h stops the program.  It runs at the widths and heights where the aligned row
stores give way to per-texel stores, where the last block column / row is partial and where a second wave, workgroup or block-row group begins, with
a tight pitch and one padded by 16 bytes.  Most blocks are forced into the modes 4..7 (and some to the reserved byte 0): the program refuses to pass
unless every mode occurred at least 100 times.  Every texel is compared with a decoder written from the header's definition inside the program, bit by
bit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_stays_inside_its_blocks_and_texels_and_matches_the_definition(tmp_path):
    exe = str(tmp_path / "bc7_decode_host")
    native = os.path.join(ROOT, "tests", "native")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function",
                        "-Wno-unknown-pragmas", "-I" + os.path.join(native, "hip_host_shim"), "-I" + os.path.join(ROOT, "omm_amd", "csrc"),
                        os.path.join(native, "bc7_decode_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    assert int(r.stdout.split()[1]) == 16 * 8 * 2   # widths x heights x pitches
