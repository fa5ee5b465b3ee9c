"""Time of the coarsening (not a test): ommxCoarsenMicromap on the metric configuration's device result (workloads c2: 1 M triangles, level 8, 4-state,
baked through ommxBakeDevice) at maxSubdivisionLevel 4, 6, 7 and 8 (nothing to reduce), info-only and full, next to the yardstick
ommxDebugGetStatsDevice -- the existing single streaming pass over the same arrayData and index buffer.  One process, warmed, HIP events around each call.

    python tests/scripts/coarsen_throughput.py [--config c2] [--tris N] [--reps 20] [--levels 4,6,7,8] [--json out.json]

Prints per call the median / min / max ms and per level the output's size and counts.  Kernel times (the reduction kernel's HBM read rate is
arrayData bytes / time of coarsen_units): run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` in a run of its own.  The script ends
itself after --time-limit seconds."""
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
from lookup_throughput import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--levels", default="4,6,7,8")
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # SIGALRM's default action ends the process
    product = ot.Lib("product")
    dll = cu.bind(product.dll)
    hip = ot.Hip()
    hip.rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.rt.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.rt.hipEventDestroy.argtypes = [C.c_void_p]

    tex, uv, ix, lv, kw = wl.workload(a.config, a.tris)
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    d = ot.make_desc(t, uv, ix, kw.pop("level"), levels=lv, **kw)
    bake = lu.DeviceBake(product, hip, b, d, uv, ix, lv)
    r = bake.rdesc
    print("result: %d triangles, %d OMMs, arrayData %.1f MiB" % (r.indexCount, r.descArrayCount, r.arrayDataSize / 2**20))
    st = ot.DebugStats()
    row = dict(config=a.config, triangles=r.indexCount, omms=r.descArrayCount, array_bytes=r.arrayDataSize, reps=a.reps, levels={})

    def stats_call():
        assert dll.ommxDebugGetStatsDevice(b, C.byref(r), None, None, C.byref(st), None, None) == ot.SUCCESS

    def report(name, fn):
        ms = timed(hip, fn, a.reps)
        med = float(np.median(ms))
        print("%-44s median %8.3f ms  (min %.3f, max %.3f, %d reps)" % (name, med, ms.min(), ms.max(), len(ms)))
        return dict(median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()))

    row["ommxDebugGetStatsDevice"] = report("ommxDebugGetStatsDevice", stats_call)
    for level in (int(x) for x in a.levels.split(",")):
        cd, info = cu.c_desc(level, 3), cu.CoarsenInfo()

        def info_call():
            assert dll.ommxCoarsenMicromap(b, C.byref(r), C.byref(cd), None, C.byref(info), None) == ot.SUCCESS

        def full_call():
            out = C.c_void_p()
            assert dll.ommxCoarsenMicromap(b, C.byref(r), C.byref(cd), C.byref(out), C.byref(info), None) == ot.SUCCESS
            assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS

        info_call()
        got = cu.info_dict(info)
        print("maxSubdivisionLevel %d: arrayData %.1f MiB, %d OMMs; of %d referenced blocks %d coarsened, %d uniform, %d duplicates" % (
            level, got["arrayDataSize"] / 2**20, got["descArrayCount"], got["referencedBlocks"], got["coarsenedBlocks"], got["uniformBlocks"], got["duplicateBlocks"]))
        entry = dict(info=got, info_only=report("ommxCoarsenMicromap to %d, info only" % level, info_call), full=report("ommxCoarsenMicromap to %d, full" % level, full_call))
        print("  info only / statistics = %.2f" % (entry["info_only"]["median_ms"] / row["ommxDebugGetStatsDevice"]["median_ms"]))
        row["levels"][str(level)] = entry
    bake.close()
    product.destroy_texture(b, t)
    product.destroy_baker(b)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
