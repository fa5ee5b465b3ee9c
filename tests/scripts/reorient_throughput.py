"""Time of the re-orientation (not a test): ommxReorientMicromap on one device result of the metric configuration (workloads c2: 1 M triangles, level 8,
4-state, baked through ommxBakeDevice), info-only and full, next to the floor taken in the same process: ommxGatherMicromaps on the same single source,
which is the same pipeline with a copy in the place of the permutation.  One process, warmed, HIP events around each call.

    python tests/scripts/reorient_throughput.py [--config c2] [--tris N] [--reps 15] [--json out.json]

    (0) every orientation 0, through the desc (items: one per descriptor)      (0p) the same as a byte per primitive (items: six per descriptor)
    (1) every orientation 1                (3) every orientation 3             (r) a random orientation 0..5 per BLOCK, given per primitive: every
    primitive of a block has the block's orientation, so the output has the source's size (independent orientations per primitive would ask for up to
    six images of every block -- at the metric size more than a 32-bit descriptor offset can express, which the call refuses)

Prints per call the median / min / max ms and the call's info.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` in
a run of its own.  The script ends itself after --time-limit seconds."""
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
import gather_util as gt  # noqa: E402
import reorient_util as rt  # noqa: E402
from lookup_throughput import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # SIGALRM's default action ends the process
    product = ot.Lib("product")
    dll = rt.bind(gt.bind(product.dll))
    hip = ot.Hip()
    hip.rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.rt.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.rt.hipEventDestroy.argtypes = [C.c_void_p]

    tex, uv, ix, lv, kw = wl.workload(a.config, a.tris)
    b = product.create_baker()
    level = kw.pop("level")
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    bake = lu.DeviceBake(product, hip, b, ot.make_desc(t, uv, ix, level, levels=lv, **kw), uv, ix, lv)
    src = bake.rdesc
    print("source: %d triangles, %d OMMs, arrayData %.1f MiB" % (src.indexCount, src.descArrayCount, src.arrayDataSize / 2**20))
    n = src.indexCount
    rng = np.random.default_rng(1)
    entries = np.asarray(bake.host.index).astype(np.int64)
    per_block = rng.integers(0, 6, max(src.descArrayCount, 1)).astype(np.uint8)
    bytes_of = {"0p": np.zeros(n, np.uint8), "r": np.where(entries >= 0, per_block[np.maximum(entries, 0)], 0).astype(np.uint8)}
    device = {k: hip.upload(v) for k, v in bytes_of.items()}
    row = dict(config=a.config, triangles=n, source_bytes=src.arrayDataSize, reps=a.reps)

    def report(name, fn):
        ms = timed(hip, fn, a.reps)
        med = float(np.median(ms))
        print("%-60s median %8.3f ms  (min %.3f, max %.3f, %d reps)" % (name, med, ms.min(), ms.max(), len(ms)))
        return dict(median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()))

    ginfo, one, everything = gt.GatherInfo(), mu.pointer_array([src]), gt.c_desc()

    def gather_call(full=True):
        out = C.c_void_p()
        assert dll.ommxGatherMicromaps(b, one, 1, C.byref(everything), C.byref(out) if full else None, C.byref(ginfo), None) == ot.SUCCESS
        if full:
            assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS

    info = rt.ReorientInfo()

    def reorient_call(desc, full=True):
        out = C.c_void_p()
        assert dll.ommxReorientMicromap(b, C.byref(src), C.byref(desc), C.byref(out) if full else None, C.byref(info), None) == ot.SUCCESS
        if full:
            assert dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS

    row["gather"] = dict(info_only=report("ommxGatherMicromaps, one result, info only", lambda: gather_call(False)),
                         full=report("ommxGatherMicromaps, one result, full", gather_call))
    floor = row["gather"]["full"]["median_ms"]
    cases = (("0", "(0) orientation 0 through the desc", rt.c_desc(None, 0)), ("0p", "(0p) orientation 0 per primitive", rt.c_desc(device["0p"])),
             ("1", "(1) orientation 1 through the desc", rt.c_desc(None, 1)), ("3", "(3) orientation 3 through the desc", rt.c_desc(None, 3)),
             ("r", "(r) a random orientation per block", rt.c_desc(device["r"])))
    for key, name, desc in cases:
        reorient_call(desc, False)
        got = rt.info_dict(info)
        print("%s: arrayData %.1f MiB, %d OMMs; of %d blocks %d re-oriented, %d uniform, %d duplicates; %d skipped" % (
            name, got["arrayDataSize"] / 2**20, got["descArrayCount"], got["referencedBlocks"], got["reorientedBlocks"], got["uniformBlocks"],
            got["duplicateBlocks"], got["skippedPrimitives"]))
        row[key] = dict(info=got, info_only=report("ommxReorientMicromap %s, info only" % name, lambda: reorient_call(desc, False)),
                        full=report("ommxReorientMicromap %s, full" % name, lambda: reorient_call(desc)))
        print("  full / gather = %.2f" % (row[key]["full"]["median_ms"] / floor))
    for p in device.values():
        hip.free(p)
    bake.close()
    product.destroy_texture(b, t)
    product.destroy_baker(b)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
