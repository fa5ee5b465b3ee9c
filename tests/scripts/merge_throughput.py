"""Saving and time of the near-duplicate merge (not a test): ommxMergeSimilarMicromaps on
  (a) the device result of the metric configuration (workloads c2: 1 M triangles, level 8, 4-state, baked through ommxBakeDevice),
  (b) the two-mesh scene array: ommxGatherMicromaps of (a) and a second bake at another alpha cut-off,
  (c) near-copy content: BASES triangles over a foliage texture, each COPIES times with Gaussian jitter of 0.3 texel on every vertex,
at limits of 1, 2, 5 and 10 % of a block with default rounds and samples: arrayDataSize, descArrayCount, absorbedPerRound and the knownAreaMetric
(ommxDebugGetStatsDevice with the source's areas) next to the unmerged numbers; the whole call, the info-only call and info-only calls of 1, 2, 4 and 8
rounds, next to two yardsticks on the same source in the same process: the info-only ommxCoarsenMicromap at cap 12 (the same front and tail without
rounds) and ommxCompareMicromaps(source, source) (one two-source streaming pass over the same bytes).  One process, warmed, HIP events around each
call.

    python tests/scripts/merge_throughput.py [--config c2] [--tris N] [--reps 5] [--near-copies 1000,100,6] [--json out.json]

Kernel times and counters: under `rocprofv3 --kernel-trace --stats` or `rocprofv3 --pmc`, each in a run of its own.  The script ends itself after
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
import compare_util as pu  # noqa: E402
import gather_util as gt  # noqa: E402
import merge_util as gu  # noqa: E402
from lookup_throughput import timed  # noqa: E402

PERCENTS = (1, 2, 5, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cutoffs", default="0.5,0.35")
    ap.add_argument("--near-copies", default="1000,100,6")
    ap.add_argument("--time-limit", type=int, default=500)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # SIGALRM's default action ends the process
    product = ot.Lib("product")
    dll = gu.bind(gt.bind(cu.bind(product.dll)))
    hip = ot.Hip()
    hip.rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.rt.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.rt.hipEventDestroy.argtypes = [C.c_void_p]
    b = product.create_baker()
    st = ot.DebugStats()
    rows = {}

    def report(name, fn):
        ms = timed(hip, fn, a.reps)
        med = float(np.median(ms))
        print("  %-50s median %9.3f ms  (min %.3f, max %.3f, %d reps)" % (name, med, ms.min(), ms.max(), len(ms)), flush=True)
        return dict(median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()))

    def metric(rd, areas):
        assert dll.ommxDebugGetStatsDevice(b, C.byref(rd), areas, None, C.byref(st), None, None) == ot.SUCCESS
        return float(st.knownAreaMetric)

    def measure(name, rd, areas, times=True):
        print("%s: %d primitives, %d OMMs, arrayData %.1f MiB, knownAreaMetric %.6f" % (
            name, rd.indexCount, rd.descArrayCount, rd.arrayDataSize / 2**20, metric(rd, areas) if areas else float("nan")), flush=True)
        row = dict(primitives=rd.indexCount, descArrayCount=rd.descArrayCount, arrayDataSize=rd.arrayDataSize, limits={})
        info = gu.MergeInfo()

        def call(percent, rounds=0, full=True):
            out = C.c_void_p()
            r = dll.ommxMergeSimilarMicromaps(b, C.byref(rd), C.byref(gu.c_desc(gu.UNIT * percent // 100, rounds)), None, C.byref(out) if full else None, C.byref(info), None)
            assert r == ot.SUCCESS, r
            return out if full else None

        for percent in PERCENTS:
            out = call(percent)
            got = gu.info_dict(info)
            known = metric(cu.result_desc_of(dll, out), areas) if areas else float("nan")
            assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
            print("  limit %2d %%: arrayData %.1f MiB, %d OMMs; of %d candidates %d absorbed %s, %d uniform, %d duplicates; knownAreaMetric %.6f" % (
                percent, got["arrayDataSize"] / 2**20, got["descArrayCount"], got["candidateBlocks"], got["absorbedBlocks"], got["absorbedPerRound"][:8],
                got["uniformBlocks"], got["duplicateBlocks"], known), flush=True)
            row["limits"][percent] = dict(info=got, knownAreaMetric=known)
        if times:
            coarsen_desc, coarsen_info, cd, cinfo = cu.c_desc(12, 3), cu.CoarsenInfo(), pu.c_desc(), pu.CompareInfo()
            row["coarsen_12_info_only"] = report("ommxCoarsenMicromap at cap 12, info only",
                                                 lambda: dll.ommxCoarsenMicromap(b, C.byref(rd), C.byref(coarsen_desc), None, C.byref(coarsen_info), None))
            row["compare_self"] = report("ommxCompareMicromaps(source, source), info only",
                                         lambda: dll.ommxCompareMicromaps(b, C.byref(rd), C.byref(rd), C.byref(cd), None, C.byref(cinfo), None))

            def full_call(percent):
                assert dll.ommxDestroyDeviceBakeResult(call(percent)) == ot.SUCCESS

            for percent in (1, 5):
                row["full_%d" % percent] = report("merge at %d %%, whole call" % percent, lambda: full_call(percent))
                row["info_%d" % percent] = report("merge at %d %%, info only" % percent, lambda: call(percent, full=False))
            for rounds in (1, 2, 4, 8):
                row["info_5_rounds_%d" % rounds] = report("merge at 5 %%, info only, %d round(s)" % rounds, lambda: call(5, rounds, False))
            per_round = (row["info_5_rounds_8"]["median_ms"] - row["info_5_rounds_1"]["median_ms"]) / 7
            print("  a round after the first: %.3f ms = %.2f x compare-self;  front, copy, one round and tail: %.3f ms" % (
                per_round, per_round / row["compare_self"]["median_ms"], row["info_5_rounds_1"]["median_ms"]), flush=True)
        rows[name] = row

    def areas_of(bake):
        areas = C.c_void_p()
        assert dll.ommxGetDeviceBakeResultTriangleAreas(bake.out, C.byref(areas)) == ot.SUCCESS and areas.value
        return areas

    # (c) first: it is small
    bases, copies, level = (int(x) for x in a.near_copies.split(","))
    if bases:
        size = 4096
        tex = ot.foliage_texture(3, size, size, 64)
        base, _ = ot.random_triangles(5, bases, 0.02, 0.05, 0.95)
        uv = np.repeat(base.reshape(bases, 3, 2), copies, axis=0)
        uv = (uv + np.random.default_rng(5).normal(0.0, 0.3 / size, uv.shape)).astype(np.float32).reshape(-1, 2)
        ix = np.arange(len(uv), dtype=np.uint32)
        t = product.create_texture(b, [tex])
        bake = lu.DeviceBake(product, hip, b, ot.make_desc(t, uv, ix, level, alpha_cutoff=0.5, fmt=ot.FMT_4STATE), uv, ix)
        measure("(c) %d x %d near-copies at level %d" % (bases, copies, level), bake.rdesc, areas_of(bake))
        bake.close()
        product.destroy_texture(b, t)

    tex, uv, ix, lv, kw = wl.workload(a.config, a.tris)
    level = kw.pop("level")
    bakes, textures = [], []
    for cutoff in (float(x) for x in a.cutoffs.split(",")):
        t = product.create_texture(b, [tex], alpha_cutoff=cutoff)   # (a texture's cut-off, which its summed-area table is built for, must be the bake's)
        textures.append(t)
        d = ot.make_desc(t, uv, ix, level, levels=lv, **dict(kw, alpha_cutoff=cutoff))
        bakes.append(lu.DeviceBake(product, hip, b, d, uv, ix, lv))
    measure("(a) %s" % a.config, bakes[0].rdesc, areas_of(bakes[0]))
    if len(bakes) > 1:
        gathered, ginfo = C.c_void_p(), gt.GatherInfo()
        rds = mu.pointer_array([k.rdesc for k in bakes])
        assert dll.ommxGatherMicromaps(b, rds, len(bakes), C.byref(gt.c_desc()), C.byref(gathered), C.byref(ginfo), None) == ot.SUCCESS
        measure("(b) gather of %d bakes" % len(bakes), cu.result_desc_of(dll, gathered), None, times=False)
        assert dll.ommxDestroyDeviceBakeResult(gathered) == ot.SUCCESS
    for k in bakes:
        k.close()
    for t in textures:
        product.destroy_texture(b, t)
    product.destroy_baker(b)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
