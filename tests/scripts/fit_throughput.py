"""Time of the fit (not a test): on the metric configuration's device result (workloads c2: 1 M triangles, level 8, 4-state, baked through
ommxBakeDevice), in one process, warmed, HIP events around each call:

  ommxProfileMicromapLevels, next to its yardsticks ommxDebugGetStatsDevice and the info-only ommxCoarsenMicromap to level 0 (the existing pass with the
  same reduction depth, without the profile's counting);
  ommxFitMicromap at budgets of 1/2, 1/4 and 1/16 of arrayDataSize with the result's own triangle areas as weights, info-only and full, and its parts:
  the profile (above), the coarsening (ommxCoarsenMicromapLevels on the levels the fit returned), and what is left of the info-only call -- the
  read-back of 116 bytes per descriptor, the plan on the host and the upload of the levels;
  what a caller does without it: info-only ommxCoarsenMicromap from the result's finest level down until the size fits, then one full call at that cap;
  for each budget the knownAreaMetric (ommxDebugGetStatsDevice with the source's areas) and the size of both outputs.

    python tests/scripts/fit_throughput.py [--config c2] [--tris N] [--reps 20] [--fractions 2,4,16] [--json out.json]

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
import coarsen_util as cu  # noqa: E402
import fit_util as fu  # noqa: E402
from lookup_throughput import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fractions", default="2,4,16")
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # SIGALRM's default action ends the process
    product = ot.Lib("product")
    dll = fu.bind(product.dll)
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
    areas = C.c_void_p()
    assert dll.ommxGetDeviceBakeResultTriangleAreas(bake.out, C.byref(areas)) == ot.SUCCESS and areas.value
    print("result: %d triangles, %d OMMs, arrayData %.1f MiB" % (r.indexCount, r.descArrayCount, r.arrayDataSize / 2**20))
    st = ot.DebugStats()
    row = dict(config=a.config, triangles=r.indexCount, omms=r.descArrayCount, array_bytes=r.arrayDataSize, reps=a.reps, budgets={})

    def report(name, fn):
        ms = timed(hip, fn, a.reps)
        med = float(np.median(ms))
        print("%-58s median %8.3f ms  (min %.3f, max %.3f, %d reps)" % (name, med, ms.min(), ms.max(), len(ms)))
        return dict(median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()))

    def metric(rd):
        assert dll.ommxDebugGetStatsDevice(b, C.byref(rd), areas, None, C.byref(st), None, None) == ot.SUCCESS
        return float(st.knownAreaMetric)

    def stats_call():
        assert dll.ommxDebugGetStatsDevice(b, C.byref(r), None, None, C.byref(st), None, None) == ot.SUCCESS

    cinfo, pinfo = cu.CoarsenInfo(), fu.LevelProfileInfo()
    to_zero = cu.c_desc(0, 3)

    def coarsen_to_zero():
        assert dll.ommxCoarsenMicromap(b, C.byref(r), C.byref(to_zero), None, C.byref(cinfo), None) == ot.SUCCESS

    def profile_call(weights):
        def call():
            assert dll.ommxProfileMicromapLevels(b, C.byref(r), weights, None, C.byref(pinfo), None) == ot.SUCCESS
        return call

    row["source_metric"] = metric(r)
    print("knownAreaMetric of the source: %.6f" % row["source_metric"])
    row["ommxDebugGetStatsDevice"] = report("ommxDebugGetStatsDevice", stats_call)
    row["coarsen_to_0_info_only"] = report("ommxCoarsenMicromap to 0, info only", coarsen_to_zero)
    row["profile_unweighted"] = report("ommxProfileMicromapLevels, no weights", profile_call(None))
    row["profile"] = report("ommxProfileMicromapLevels, triangle areas", profile_call(areas))
    print("  profile / info-only coarsening to 0 = %.2f" % (row["profile"]["median_ms"] / row["coarsen_to_0_info_only"]["median_ms"]))

    levels = hip.alloc(max(r.descArrayCount, 16))
    finest = max(int(r.descArrayHistogram[k].subdivisionLevel) for k in range(r.descArrayHistogramCount))
    for fraction in (int(x) for x in a.fractions.split(",")):
        budget = r.arrayDataSize // fraction
        fd, finfo = fu.f_desc(budget, areas, 12, 3), fu.FitInfo()

        def fit_info():
            assert dll.ommxFitMicromap(b, C.byref(r), C.byref(fd), levels, None, C.byref(finfo), None) == ot.SUCCESS

        def fit_full():
            out = C.c_void_p()
            assert dll.ommxFitMicromap(b, C.byref(r), C.byref(fd), levels, C.byref(out), C.byref(finfo), None) == ot.SUCCESS
            assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS

        keep = cu.c_desc(12, 3)

        def levels_info():
            assert dll.ommxCoarsenMicromapLevels(b, C.byref(r), levels, C.byref(keep), None, C.byref(cinfo), None) == ot.SUCCESS

        # what a caller does without the fit: the finest global cap whose size fits, found by info-only calls, then built
        search = dict(cap=None, calls=0)

        def search_and_build():
            search["calls"] = 0
            for cap in range(finest, -1, -1):
                cd = cu.c_desc(cap, 3)
                assert dll.ommxCoarsenMicromap(b, C.byref(r), C.byref(cd), None, C.byref(cinfo), None) == ot.SUCCESS
                search["calls"] += 1
                if cinfo.arrayDataSize <= budget:
                    out = C.c_void_p()
                    assert dll.ommxCoarsenMicromap(b, C.byref(r), C.byref(cd), C.byref(out), C.byref(cinfo), None) == ot.SUCCESS
                    assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
                    search["cap"] = cap
                    return
            raise AssertionError("no cap fits")

        entry = dict(budget=budget)
        entry["fit_info_only"] = report("ommxFitMicromap to 1/%d, info only" % fraction, fit_info)
        entry["fit_full"] = report("ommxFitMicromap to 1/%d, full" % fraction, fit_full)
        entry["coarsen_levels_info_only"] = report("  its coarsening (ommxCoarsenMicromapLevels, info only)", levels_info)
        rest = entry["fit_info_only"]["median_ms"] - row["profile"]["median_ms"] - entry["coarsen_levels_info_only"]["median_ms"]
        entry["readback_plan_upload_ms"] = rest
        print("  read-back, plan on the host, upload (the rest of the info-only call): %.3f ms" % rest)
        entry["search_and_build"] = report("global caps: info-only search from the top + one full call", search_and_build)
        # both outputs
        out = C.c_void_p()
        assert dll.ommxFitMicromap(b, C.byref(r), C.byref(fd), levels, C.byref(out), C.byref(finfo), None) == ot.SUCCESS
        fitted = cu.result_desc_of(dll, out)
        entry["fit"] = dict(info=fu.fit_info_dict(finfo), metric=metric(fitted), histogram=np.bincount(hip.download(levels, r.descArrayCount), minlength=256)[:13].tolist())
        assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
        cd = cu.c_desc(search["cap"], 3)
        assert dll.ommxCoarsenMicromap(b, C.byref(r), C.byref(cd), C.byref(out), C.byref(cinfo), None) == ot.SUCCESS
        entry["cap"] = dict(level=search["cap"], calls=search["calls"], info=cu.info_dict(cinfo), metric=metric(cu.result_desc_of(dll, out)))
        assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
        print("  budget %.1f MiB: fit %.1f MiB (planned %.1f, %d steps), knownAreaMetric %.6f; best cap %d (%d info-only calls) %.1f MiB, knownAreaMetric %.6f" % (
            budget / 2**20, entry["fit"]["info"]["result"]["arrayDataSize"] / 2**20, entry["fit"]["info"]["plannedArrayDataSize"] / 2**20, entry["fit"]["info"]["steps"],
            entry["fit"]["metric"], search["cap"], search["calls"], entry["cap"]["info"]["arrayDataSize"] / 2**20, entry["cap"]["metric"]))
        print("  blocks per chosen level 0..12:", entry["fit"]["histogram"])
        row["budgets"][str(fraction)] = entry
    hip.free(levels)
    bake.close()
    product.destroy_texture(b, t)
    product.destroy_baker(b)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
