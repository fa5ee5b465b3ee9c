"""The layout of the arrays that ommxCoarsenMicromap, ommxCombineMicromaps and ommxGatherMicromaps hand to the tail (omm_amd/csrc/rebuild_arrays.h)
without a GPU -- a stand-alone program, tests/native/rebuild_arrays_check.cpp, under AddressSanitizer and UBSan.  Items 0, 1, 255, 256, 257 and 65 537
x temporary storage of the scans of 0, 1 and 4096 bytes x scratch of the tail of 0 and 256 bytes, each carved from a null base (the size to reserve) and
over an exact-size heap block in which every slot is written end to end."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_arrays_are_aligned_disjoint_and_sized_as_by_hand(tmp_path):
    exe = str(tmp_path / "rebuild_arrays_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                        "-I" + os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "rebuild_arrays_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    # per shape: the allocation, the agreement of the passes, 9 slots x (aligned, same offset) + 8 neighbours, n + 1 elements, the adjacency, three sums
    assert int(r.stdout.split()[1]) == 6 * 3 * 2 * (2 + 9 * 2 + 8 + 1 + 1 + 3)
