"""Time of the gather (not a test): ommxGatherMicromaps on device results of the metric configuration (workloads c2: 1 M triangles, level 8, 4-state,
baked through ommxBakeDevice), info-only and full, next to the yardstick taken in the same process: ommxCoarsenMicromap at cap 12 on the same source,
which keeps every block and so moves the same bytes through the same tail.  One process, warmed, HIP events around each call.

    python tests/scripts/gather_throughput.py [--config c2] [--tris N] [--reps 15] [--cutoffs 0.5,0.35] [--json out.json]

    (a) one result, NULL selection        (b) the concatenation of the bakes at the two cut-offs        (c) every fourth primitive of the first bake
    (d) (a) again on a copy of the first bake whose arrayData lies one byte off a 16-byte boundary: the shifted path of gather_units

Prints per call the median / min / max ms and the gather's info.  Kernel times (the read rate of gather_units is the referenced blocks' bytes / its
time): run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` in a run of its own.  The script ends itself after --time-limit seconds."""
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
import gather_util as gt  # noqa: E402
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
    dll = gt.bind(product.dll)
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
    first = bakes[0].rdesc
    # the first bake again with its arrayData one byte off a 16-byte boundary
    lead = 17
    shifted_buf = hip.alloc(first.arrayDataSize + lead)
    hip.copy_dtod(C.c_void_p(shifted_buf.value + lead), first.arrayData, first.arrayDataSize)
    shifted = ot.BakeResultDesc.from_buffer_copy(first)
    shifted.arrayData = shifted_buf.value + lead
    every_fourth = np.arange(0, first.indexCount, 4)
    d_sel = hip.upload(gt.refs(np.stack([np.zeros(len(every_fourth), np.int64), every_fourth], 1)))
    row = dict(config=a.config, triangles=first.indexCount, source_bytes=[k.rdesc.arrayDataSize for k in bakes], reps=a.reps)

    def report(name, fn):
        ms = timed(hip, fn, a.reps)
        med = float(np.median(ms))
        print("%-52s median %8.3f ms  (min %.3f, max %.3f, %d reps)" % (name, med, ms.min(), ms.max(), len(ms)))
        return dict(median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()))

    coarsen_desc, coarsen_info = cu.c_desc(12, 3), cu.CoarsenInfo()

    def coarsen_call(full=True):
        out = C.c_void_p()
        assert dll.ommxCoarsenMicromap(b, C.byref(first), C.byref(coarsen_desc), C.byref(out) if full else None, C.byref(coarsen_info), None) == ot.SUCCESS
        if full:
            assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS

    info = gt.GatherInfo()

    def gather_call(rds, desc, full=True):
        out = C.c_void_p()
        assert dll.ommxGatherMicromaps(b, rds, len(rds), C.byref(desc), C.byref(out) if full else None, C.byref(info), None) == ot.SUCCESS
        if full:
            assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS

    one, both, off = mu.pointer_array([first]), mu.pointer_array([k.rdesc for k in bakes]), mu.pointer_array([shifted])
    everything, strided = gt.c_desc(), gt.c_desc(d_sel, len(every_fourth))
    row["ommxCoarsenMicromap_12_info"] = report("ommxCoarsenMicromap at cap 12, info only", lambda: coarsen_call(False))
    row["ommxCoarsenMicromap_12_full"] = report("ommxCoarsenMicromap at cap 12, full", coarsen_call)
    for key, name, rds, desc in (("a", "(a) one result", one, everything), ("b", "(b) concatenation of %d bakes" % len(bakes), both, everything),
                                 ("c", "(c) every fourth primitive", one, strided), ("d", "(d) one result at an odd address", off, everything)):
        gather_call(rds, desc, False)
        got = gt.info_dict(info)
        print("%s: %d primitives, arrayData %.1f MiB, %d OMMs; of %d blocks %d uniform, %d duplicates; %d skipped" % (
            name, got["primitiveCount"], got["arrayDataSize"] / 2**20, got["descArrayCount"], got["referencedBlocks"], got["uniformBlocks"],
            got["duplicateBlocks"], got["skippedPrimitives"]))
        row[key] = dict(info=got, info_only=report("ommxGatherMicromaps %s, info only" % name, lambda: gather_call(rds, desc, False)),
                        full=report("ommxGatherMicromaps %s, full" % name, lambda: gather_call(rds, desc)))
    yard = row["ommxCoarsenMicromap_12_full"]
    print("  (a) full / coarsening at cap 12 = %.2f  (the coarsening's own spread: %.3f ms; (a) - coarsening: %.3f ms)" % (
        row["a"]["full"]["median_ms"] / yard["median_ms"], yard["max_ms"] - yard["min_ms"], row["a"]["full"]["median_ms"] - yard["median_ms"]))
    hip.free(d_sel)
    hip.free(shifted_buf)
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
