"""Time of the geometry extraction (not a test): ommxExtractMicroGeometry and ommxExpandMicroNodes on the metric configuration's device result (workloads
c2: 1 M triangles, level 8, 4-state, baked through ommxBakeDevice), next to the yardstick ommxDebugGetStatsDevice -- the existing single streaming pass
over the same arrayData and index buffer.  One process, warmed, HIP events around each call.

    python tests/scripts/geometry_throughput.py [--config c2] [--tris N] [--reps 20] [--json out.json]

Prints per call the median / min / max ms, the records per list and the bytes the full call writes.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -d <dir> -- python ...` in a run of its own.  The script ends itself after --time-limit seconds."""
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
import geometry_util as gu  # noqa: E402
from lookup_throughput import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # SIGALRM's default action ends the process
    product = ot.Lib("product")
    dll = gu.bind(product.dll)
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
    T = r.indexCount
    print("result: %d triangles, %d OMMs, arrayData %.1f MiB" % (T, r.descArrayCount, r.arrayDataSize / 2**20))
    gd = gu.c_desc(gu.PRESET)
    counts, skipped, st = (C.c_uint64 * 4)(), C.c_uint32(), ot.DebugStats()

    def stats_call():
        assert dll.ommxDebugGetStatsDevice(b, C.byref(r), None, None, C.byref(st), None, None) == ot.SUCCESS

    def count_call():
        assert dll.ommxExtractMicroGeometry(b, C.byref(r), C.byref(gd), None, counts, C.byref(skipped), None) == ot.SUCCESS

    count_call()
    n = list(counts)
    o = gu.MicroGeometryOutputs()
    bufs = []
    for k in range(4):
        bufs += [hip.alloc(8 * n[k]), hip.alloc(8 * (T + 1))]
        o.nodes[k], o.capacity[k], o.primitiveOffsets[k] = bufs[-2].value, n[k], bufs[-1].value
    written = sum(8 * c for c in n) + 4 * 8 * (T + 1)

    def full_call():
        assert dll.ommxExtractMicroGeometry(b, C.byref(r), C.byref(gd), C.byref(o), counts, None, None) == ot.SUCCESS

    mesh_pos = hip.upload(np.concatenate([uv.astype(np.float32), np.zeros((len(uv), 1), np.float32)], axis=1))
    mesh_ix = hip.upload(ix.astype(np.uint32))
    mesh = gu.MicroMeshDesc(mesh_pos, 12, mesh_ix, ot.IDX_U32, T)
    out_bary, out_pos = hip.alloc(24 * n[0]), hip.alloc(36 * n[0])
    full_call()

    def expand_call():
        assert dll.ommxExpandMicroNodes(o.nodes[0], n[0], C.byref(mesh), out_bary, out_pos, None) == ot.SUCCESS
        assert hip.rt.hipDeviceSynchronize() == 0

    row = dict(config=a.config, triangles=T, omms=r.descArrayCount, array_bytes=r.arrayDataSize, records=n, skipped=skipped.value, bytes_written=written,
               reps=a.reps)
    print("records per list %r, skipped %d, the full call writes %.1f MB, the expansion of list 0 %.1f MB" % (n, skipped.value, written / 1e6, 60 * n[0] / 1e6))
    for name, fn in (("ommxDebugGetStatsDevice", stats_call), ("ommxExtractMicroGeometry count-only", count_call),
                     ("ommxExtractMicroGeometry full", full_call), ("ommxExpandMicroNodes list 0", expand_call)):
        ms = timed(hip, fn, a.reps)
        med = float(np.median(ms))
        print("%-38s median %8.3f ms  (min %.3f, max %.3f, %d reps)" % (name, med, ms.min(), ms.max(), len(ms)))
        row[name] = dict(median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()))
    print("count-only / statistics = %.2f" % (row["ommxExtractMicroGeometry count-only"]["median_ms"] / row["ommxDebugGetStatsDevice"]["median_ms"]))
    for p in bufs + [mesh_pos, mesh_ix, out_bary, out_pos]:
        hip.free(p)
    bake.close()
    product.destroy_texture(b, t)
    product.destroy_baker(b)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
