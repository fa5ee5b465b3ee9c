"""Time of the device statistics (not a test): ommxDebugGetStatsDevice2 on the metric configuration's result (workloads c2: 1 M triangles, level 8,
4-state, baked through ommxBakeDevice), HIP events around each call after a warm-up, next to the only route without it: the device-to-host copy of
the three arrays plus the host's ommDebugGetStats over the copy (ommDebugGetStats2 minus the areas, which a device result could not supply).

    python tests/scripts/stats_throughput.py [--config c2] [--reps 10] [--host-reps 1] [--json out.json]

Prints the call's median / min / max ms and the bytes per second it moves, counting the bytes the algorithm needs (arrayData once, the descriptors,
the index buffer twice, the areas).  Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` separately; stats_count_blocks
reads arrayDataSize bytes.  The script ends itself after --time-limit seconds."""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import ommtest as ot  # noqa: E402
import workloads as wl  # noqa: E402
import lookup_util as lu  # noqa: E402
import stats_util as su  # noqa: E402
from lookup_throughput import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1, help="timed runs of the download + host statistics (seconds each at c2; 0 = skip)")
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # SIGALRM's default action ends the process
    product = ot.Lib("product")
    dll = su.bind(product.dll)
    hip = ot.Hip()
    hip.rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.rt.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.rt.hipEventDestroy.argtypes = [C.c_void_p]

    tex, uv, ix, lv, kw = wl.workload(a.config)
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    d = ot.make_desc(t, uv, ix, kw.pop("level"), levels=lv, **kw)
    bake = lu.DeviceBake(product, hip, b, d, uv, ix, lv)
    r = bake.rdesc
    isz = {ot.IDX_U8: 1, ot.IDX_U16: 2, ot.IDX_U32: 4}[r.indexFormat]
    print("result: %d triangles, %d OMMs, arrayData %.1f MiB, %d-byte index entries" % (r.indexCount, r.descArrayCount, r.arrayDataSize / 2**20, isz))
    st = ot.DebugStats()

    def device_call():
        assert dll.ommxDebugGetStatsDevice2(b, bake.out, C.byref(st)) == ot.SUCCESS
    ms = timed(hip, device_call, a.reps)
    need = r.arrayDataSize + 8 * r.descArrayCount + 2 * isz * r.indexCount + 4 * r.indexCount
    med = float(np.median(ms))
    print("ommxDebugGetStatsDevice2   median %8.3f ms  (min %.3f, max %.3f, %d reps)  %.1f MB needed -> %.0f GB/s over the whole call"
          % (med, ms.min(), ms.max(), len(ms), need / 1e6, need / (med * 1e-3) / 1e9))
    print("  ", dict(zip(su.INT_FIELDS, su.int_fields(st))), "knownAreaMetric %.9g" % st.knownAreaMetric)
    row = dict(config=a.config, triangles=r.indexCount, omms=r.descArrayCount, array_bytes=r.arrayDataSize, bytes_needed=need,
               device_median_ms=med, device_min_ms=float(ms.min()), device_max_ms=float(ms.max()), reps=len(ms),
               fields=su.int_fields(st), known_area_metric=float(st.knownAreaMetric))

    # the route without the device statistics: download the arrays, then the host loop
    host_ms, copy_ms = [], []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        arrays = [hip.download(r.arrayData, r.arrayDataSize), hip.download(r.descArray, 8 * r.descArrayCount), hip.download(r.indexBuffer, isz * r.indexCount)]
        t1 = time.perf_counter()
        hd = ot.BakeResultDesc.from_buffer_copy(r)
        hd.arrayData, hd.descArray, hd.indexBuffer = arrays[0].ctypes.data, C.cast(arrays[1].ctypes.data, C.POINTER(ot.MicromapDesc)), arrays[2].ctypes.data
        hs = ot.DebugStats()
        assert product.fn("ommDebugGetStats")(b, C.byref(hd), C.byref(hs)) == ot.SUCCESS
        t2 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        host_ms.append((t2 - t1) * 1e3)
        assert su.int_fields(hs) == su.int_fields(st), (su.int_fields(hs), su.int_fields(st))
    if host_ms:
        print("download + ommDebugGetStats   copy %.1f ms (pageable destination) + host loop %.1f ms (median of %d); integer fields equal the device's"
              % (float(np.median(copy_ms)), float(np.median(host_ms)), len(host_ms)))
        row.update(download_ms=float(np.median(copy_ms)), host_stats_ms=float(np.median(host_ms)))
    bake.close()
    product.destroy_texture(b, t)
    product.destroy_baker(b)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
