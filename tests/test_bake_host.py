"""The host-side rules of a bake (omm_amd/csrc/bake_host.h) without a GPU: index formats, histogram lists, the result descriptor, the layout of the raw
triangle upload and the carve of the working set -- a stand-alone program, tests/native/bake_host_check.cpp, under AddressSanitizer and UBSan.  The carve
is run twice per shape, from a null base (the size to reserve) and over an exact-size heap block that every slot is then filled in: a slot that is not
aligned, overlaps another, runs over the reservation, or breaks one of the two adjacency contracts (counters + digest table, the read-back span) stops it.
The decisions and layouts that bake_core's stages take from that header -- rank ranges, the ranges of a streamed result, the deferred generic pass, the
interleave stride, the carve of the states arena, the read-back slots -- are each held to the expression they replaced, restated in the program; so are
the rules of the sharded bake: rank validity, contribution stride, the chunk walk of the exchange, the exchange arena (carved and written like the
working set), each rank's share of the metadata sum, raw or stream, the cuts of the host scatter."""
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
    # the decisions and layouts of bake_core's stages, each against the expression it had inline:
    # worlds 1, 2, 3, 8, 16 (30 ranks): per rank the bounds, its range and 13 levels that start where the rank before ended; per world 13 levels that end with the list
    rank_ranges = 30 * (2 + 13) + 5 * 13
    # 38 sizes of the states x 3 micro-triangle counts x compressed transfer on / off, each over all its workloads; 2 threshold-straddling checks;
    # 3 forced counts x 38 sizes; the clamp of a forced count; the two anchors of the pricing
    stream_ranges = 38 * 3 * 2 + 2 + 3 * 38 + 1 + 2
    # 3 modes x 2 micro-triangle counts x (1 + 6 workloads); 2 of the modes' meaning; per storeBits 7 sizes and 3 at the cap
    generic_pass = 3 * 2 * 7 + 2 + 2 * (7 + 3)
    # cnt 3..4096 and 9 large ones: equal, coprime, in range; up to 4096 also a permutation
    interleave = 3 * (4094 + 9) + 4094
    # 3 sizes of the states x 3 queues x streamed on / off x 3 generic capacities, 4 checks each; the 16 shapes of at most 32 MiB are also written end to end
    states_carve = 3 * 3 * 2 * 3 * 4 + 16
    # read-back slots: 6 spans, 2 + 2 at the block size; launches: no / each / every level (15) + 3 values; 6 + 1 waits; 3 digest bounds
    readback_and_small = 6 + 2 + 2 + 15 + 3 + 6 + 1 + 3
    stages = rank_ranges + stream_ranges + generic_pass + interleave + states_carve + readback_and_small
    # the sharded bake's rules, each against the expression it had inline:
    # rank validity over worlds and ranks 0..17, 2 limits; the stride at 6 largest totals x 5 worlds, and the 6 strides themselves
    rank_and_stride = 18 * 18 + 2 + 6 * 5 + 6
    # 7 strides x 3 knob values: the chunk size, the walk against both loops it replaced, it tiles the stride, multiples of 256, at most 8 chunks; 3 of the sizes' meaning
    chunks = 7 * 3 * 5 + 3
    # exchange arena, async on / off x 3 worlds x 2 strides: the reservation, the offsets, both passes, the slots apart, each written end to end
    exchange_arena = 2 * 3 * 2 * 5
    # meta-sum share: 5 word counts x (30 ranks of 5 worlds + the 5 tilings); raw or stream at 6 stream sizes
    meta_share_and_send = 5 * (30 + 5) + 6
    # 7 lists of block sizes: the cuts against the loop they replaced, against the expected ones, and their properties
    scatter_cuts = 7 * 3
    sharded = rank_and_stride + chunks + exchange_arena + meta_share_and_send + scatter_cuts
    assert int(r.stdout.split()[1]) == index_formats + histograms + result_descs + raw_inputs + carve + stages + sharded
