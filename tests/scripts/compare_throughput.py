"""Time of the compare (not a test): ommxCompareMicromaps on two device results of the metric configuration (workloads c2: 1 M triangles, level 8,
4-state, baked through ommxBakeDevice) at two alpha cut-offs -- the pair of tests/scripts/combine_throughput.py -- info-only and with all three
outputs, next to the yardsticks taken in the same process: the info-only ommxCombineMicromaps of the same two sources (the same front and the same
bytes read; it stages blocks where this entry writes 64 bytes per pair) and ommxDebugGetStatsDevice of each source (one streaming read each).  One
process, warmed, HIP events around each call.

    python tests/scripts/compare_throughput.py [--config c2] [--tris N] [--reps 15] [--cutoffs 0.5,0.35] [--json out.json]

Prints per call the median / min / max ms, the compare's info and the read rate of the info-only call (both sources' arrayData bytes / its time).
Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` in a run of its own.  The script ends itself after --time-limit
seconds."""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import ommtest as ot  # noqa: E402
import workloads as wl  # noqa: E402
import lookup_util as lu  # noqa: E402
import combine_util as mu  # noqa: E402
import compare_util as pu  # noqa: E402
from lookup_throughput import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cutoffs", default="0.5,0.35")
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # SIGALRM's default action ends the process
    product = ot.Lib("product")
    dll = pu.bind(product.dll)
    hip = ot.Hip()
    hip.rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.rt.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.rt.hipEventDestroy.argtypes = [C.c_void_p]

    tex, uv, ix, lv, kw = wl.workload(a.config, a.tris)
    b = product.create_baker()
    level = kw.pop("level")
    bakes, textures = [], []
    for cutoff in (float(x) for x in a.cutoffs.split(",")):
        t = product.create_texture(b, [tex], alpha_cutoff=cutoff)   # (a texture's cut-off, which its summed-area table is built for, must be the bake's)
        textures.append(t)
        d = ot.make_desc(t, uv, ix, level, levels=lv, **dict(kw, alpha_cutoff=cutoff))
        bakes.append(lu.DeviceBake(product, hip, b, d, uv, ix, lv))
        r = bakes[-1].rdesc
        print("source at cut-off %.2f: %d triangles, %d OMMs, arrayData %.1f MiB" % (cutoff, r.indexCount, r.descArrayCount, r.arrayDataSize / 2**20))
    ra, rb = bakes[0].rdesc, bakes[1].rdesc
    rds = mu.pointer_array([ra, rb])
    st = ot.DebugStats()
    row = dict(config=a.config, triangles=ra.indexCount, source_bytes=[ra.arrayDataSize, rb.arrayDataSize], reps=a.reps)

    def report(name, fn):
        ms = timed(hip, fn, a.reps)
        med = float(np.median(ms))
        print("%-44s median %8.3f ms  (min %.3f, max %.3f, %d reps)" % (name, med, ms.min(), ms.max(), len(ms)))
        return dict(median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()))

    def stats_call(rd):
        assert dll.ommxDebugGetStatsDevice(b, C.byref(rd), None, None, C.byref(st), None, None) == ot.SUCCESS

    combine_desc, combine_info = mu.c_desc(2, 3), mu.CombineInfo()

    def combine_call():
        assert dll.ommxCombineMicromaps(b, rds, 2, C.byref(combine_desc), None, C.byref(combine_info), None) == ot.SUCCESS

    cd, info = pu.c_desc(), pu.CompareInfo()
    outputs = pu.Outputs(hip, ra.indexCount)

    def info_call():
        assert dll.ommxCompareMicromaps(b, C.byref(ra), C.byref(rb), C.byref(cd), None, C.byref(info), None) == ot.SUCCESS

    def full_call():
        assert dll.ommxCompareMicromaps(b, C.byref(ra), C.byref(rb), C.byref(cd), C.byref(outputs.c), C.byref(info), None) == ot.SUCCESS

    row["ommxDebugGetStatsDevice_A"] = report("ommxDebugGetStatsDevice, A", lambda: stats_call(ra))
    row["ommxDebugGetStatsDevice_B"] = report("ommxDebugGetStatsDevice, B", lambda: stats_call(rb))
    row["combine_info_only"] = report("ommxCombineMicromaps, info only", combine_call)
    info_call()
    got = pu.info_dict(info)
    print("compared: %d pairs (%d refined); primitives: %d identical, %d conflict, %d A weaker, %d B weaker, %d hint, %d skipped; first conflict %d" % (
        got["comparedPairs"], got["refinedPairs"], got["identicalPrimitives"], got["conflictPrimitives"], got["aWeakerPrimitives"], got["bWeakerPrimitives"],
        got["hintPrimitives"], got["skippedPrimitives"], got["firstConflictPrimitive"]))
    assert sum(sum(got["totals"], [])) == (ra.indexCount - got["skippedPrimitives"]) * pu.UNIT
    row["info"] = got
    row["info_only"] = report("ommxCompareMicromaps, info only", info_call)
    row["full"] = report("ommxCompareMicromaps, all outputs", full_call)
    row["read_GBps"] = (ra.arrayDataSize + rb.arrayDataSize) / row["info_only"]["median_ms"] / 1e6
    print("  info only / combine info only = %.2f,  read rate of the info-only call %.0f GB/s" % (
        row["info_only"]["median_ms"] / row["combine_info_only"]["median_ms"], row["read_GBps"]))
    outputs.close()
    for k in bakes:
        k.close()
    for t in textures:
        product.destroy_texture(b, t)
    product.destroy_baker(b)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
