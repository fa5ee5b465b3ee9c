"""Time of the combine (not a test): ommxCombineMicromaps on two device results of the metric configuration (workloads c2: 1 M triangles, level 8,
4-state, baked through ommxBakeDevice) at two alpha cut-offs, into the 4-state format, info-only and full, next to two yardsticks taken in the same
process: ommxCoarsenMicromap at cap 8 on one of the sources (nothing to reduce: it reads arrayData once and writes it twice, staging and output) and
ommxDebugGetStatsDevice (one streaming read).  One process, warmed, HIP events around each call.

    python tests/scripts/combine_throughput.py [--config c2] [--tris N] [--reps 15] [--cutoffs 0.5,0.35] [--json out.json]

Prints per call the median / min / max ms and the combine's info.  Kernel times (the streaming pass's HBM read rate is the sources' arrayData bytes /
time of combine_units): run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` in a run of its own.  The script ends itself after
--time-limit seconds."""
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
import coarsen_util as cu  # noqa: E402
import combine_util as mu  # noqa: E402
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
    dll = mu.bind(product.dll)
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
    rds = mu.pointer_array([k.rdesc for k in bakes])
    first = bakes[0].rdesc
    st = ot.DebugStats()
    row = dict(config=a.config, triangles=first.indexCount, source_bytes=[k.rdesc.arrayDataSize for k in bakes], reps=a.reps)

    def report(name, fn):
        ms = timed(hip, fn, a.reps)
        med = float(np.median(ms))
        print("%-44s median %8.3f ms  (min %.3f, max %.3f, %d reps)" % (name, med, ms.min(), ms.max(), len(ms)))
        return dict(median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()))

    def stats_call():
        assert dll.ommxDebugGetStatsDevice(b, C.byref(first), None, None, C.byref(st), None, None) == ot.SUCCESS

    coarsen_desc, coarsen_info = cu.c_desc(8, 3), cu.CoarsenInfo()

    def coarsen_call():
        out = C.c_void_p()
        assert dll.ommxCoarsenMicromap(b, C.byref(first), C.byref(coarsen_desc), C.byref(out), C.byref(coarsen_info), None) == ot.SUCCESS
        assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS

    cd, info = mu.c_desc(2, 3), mu.CombineInfo()

    def info_call():
        assert dll.ommxCombineMicromaps(b, rds, len(bakes), C.byref(cd), None, C.byref(info), None) == ot.SUCCESS

    def full_call():
        out = C.c_void_p()
        assert dll.ommxCombineMicromaps(b, rds, len(bakes), C.byref(cd), C.byref(out), C.byref(info), None) == ot.SUCCESS
        assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS

    row["ommxDebugGetStatsDevice"] = report("ommxDebugGetStatsDevice", stats_call)
    row["ommxCoarsenMicromap_8_full"] = report("ommxCoarsenMicromap to 8, full", coarsen_call)
    info_call()
    got = mu.info_dict(info)
    print("combined: arrayData %.1f MiB, %d OMMs; of %d tuples %d refined, %d uniform, %d duplicates; %d skipped" % (
        got["arrayDataSize"] / 2**20, got["descArrayCount"], got["combinedTuples"], got["refinedTuples"], got["uniformBlocks"], got["duplicateBlocks"],
        got["skippedPrimitives"]))
    row["info"] = got
    row["info_only"] = report("ommxCombineMicromaps, info only", info_call)
    row["full"] = report("ommxCombineMicromaps, full", full_call)
    print("  full / coarsening at cap 8 = %.2f,  info only / statistics = %.2f" % (
        row["full"]["median_ms"] / row["ommxCoarsenMicromap_8_full"]["median_ms"], row["info_only"]["median_ms"] / row["ommxDebugGetStatsDevice"]["median_ms"]))
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
