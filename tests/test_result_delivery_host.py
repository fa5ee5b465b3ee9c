"""The integer rules of ommCpuBake's result delivery (omm_amd/csrc/host_expand.h) without a GPU: the carve of the device codec block, the cut of a codec
stream into the twelve slices it crosses the link in, the slice an expansion task has to wait for, and a stream of the scalar codec model delivered and
expanded in that order -- a stand-alone program, tests/native/result_delivery_check.cpp, under AddressSanitizer and UBSan.  Every figure is checked
against the arithmetic ommCpuBake did inline before these functions existed, restated in the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_codec_block_carve_slice_plan_and_task_order(tmp_path):
    exe = str(tmp_path / "result_delivery_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                        "-I" + os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "result_delivery_check.cpp"),
                        os.path.join(ROOT, "omm_amd", "csrc", "host_expand.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    # carve: 6 array sizes x 3 scratch sizes x with / without codes, 6 checks of the sizing pass each; 2 more over a heap block for the 5 sizes up to 32 MiB + 16
    carve = 6 * 3 * 2 * 6 + 5 * 3 * 2 * 2
    # slice plans: 8 block counts x 3 offset tables x 5 properties; per block count two corrupt tables rejected; an entry dipping inside a slice accepted
    # for the 5 block counts that have a slice of two blocks or more (13 and up)
    plans = 8 * 3 * 5 + 8 * 2 + 5
    # per task of 512 blocks the slice it waits for (1, 1, 1, 1, 1, 1, 2 and 13 tasks), per block count the tiling of the tasks
    tasks = (6 * 1 + 2 + 13) + 8
    round_trip = 2 * 2
    assert int(r.stdout.split()[1]) == carve + plans + tasks + round_trip
