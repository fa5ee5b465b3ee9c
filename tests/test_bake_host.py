"""The host-side rules of a bake (omm_amd/csrc/bake_host.h) without a GPU: index formats, histogram lists, the result descriptor, the layout of the raw
triangle upload and the carve of the working set -- a stand-alone program, tests/native/bake_host_check.cpp, under AddressSanitizer and UBSan.  The carve
is run twice per shape, from a null base (the size to reserve) and over an exact-size heap block that every slot is then filled in: a slot that is not
aligned, overlaps another, runs over the reservation, or breaks one of the two adjacency contracts (counters + digest table, the read-back span) stops it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bake_host_rules_and_working_set_carve(tmp_path):
    exe = str(tmp_path / "bake_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                        "-I" + os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "bake_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    index_formats = 6 * 4 + 2
    histograms = 2 * (2 + 4 + 6 + 28) + 2
    result_descs = 2 * 4 * 5
    raw_inputs = 10 * 3 * 3 * 2 * 6
    # per shape 4 checks per slot and 6 of the whole; 26 slots, 4 more sharded, 11 more streamed; one check per absent group
    carve = 5 * 2 * ((4 * 26 + 8) + (4 * 30 + 7) + (4 * 37 + 7) + (4 * 41 + 6))
    assert int(r.stdout.split()[1]) == index_formats + histograms + result_descs + raw_inputs + carve
