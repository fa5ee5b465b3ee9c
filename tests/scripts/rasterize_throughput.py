"""Time of the texture-space view (not a test): ommxRasterizeMicromap on the metric configuration's result (workloads c2: 1 M triangles, level 8,
4-state, baked through ommxBakeDevice) over [0, 1]^2 at 4096^2 and 8192^2 -- all outputs, the picture alone and info only -- and on the foliage
cards (large triangles) at 4096^2; next to it, as context and not as a gate (the work differs), ommxLookupOpacity on as many primitive-sorted hits
as the smaller image has pixels.  One process, warmed, HIP events around each call.

    python tests/scripts/rasterize_throughput.py [--sizes 4096,8192] [--reps 9] [--tris N] [--configs c2,cards] [--json out.json]

Prints per call the median / min / max ms and the pixels per second, and the info of each scene.  Kernel times: run it under
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
import rasterize_util as ru  # noqa: E402
from lookup_throughput import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--configs", default="c2,cards")
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # SIGALRM's default action ends the process
    product = ot.Lib("product")
    dll = ru.bind(lu.bind(product.dll))
    hip = ot.Hip()
    hip.rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.rt.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.rt.hipEventDestroy.argtypes = [C.c_void_p]
    sizes = [int(s) for s in a.sizes.split(",")]
    rows = []
    b = product.create_baker()

    def report(name, fn, pixels):
        ms = timed(hip, fn, a.reps, warmup=2)
        med = float(np.median(ms))
        rows.append(dict(case=name, median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()), pixels=pixels))
        print("%-46s median %8.3f ms  (min %.3f, max %.3f, %d reps)  %.2f G pixels/s" % (name, med, ms.min(), ms.max(), len(ms), pixels / med / 1e6))

    for config in a.configs.split(","):
        tex, uv, ix, lv, kw = wl.workload(config, a.tris)
        t = product.create_texture(b, [tex], alpha_cutoff=0.5)
        d = ot.make_desc(t, uv, ix, kw.pop("level"), levels=lv, **kw)
        bake = lu.DeviceBake(product, hip, b, d, uv, ix, lv)
        r = bake.rdesc
        print("%s: %d triangles, %d OMMs, arrayData %.1f MiB" % (config, r.indexCount, r.descArrayCount, r.arrayDataSize / 2**20))
        for size in (sizes if config == "c2" else sizes[:1]):
            pixels = size * size
            bufs = {name: hip.alloc(pixels * ru.OUT_BYTES[name]) for name in ru.OUTPUTS}
            info = ru.RasterInfo()
            desc = ru.c_desc((0.0, 0.0, 1.0, 1.0), size, size)

            def call(names, want_info=True):
                o = ru.RasterOutputs(*[bufs[n] if n in names else None for n in ru.OUTPUTS])
                got = dll.ommxRasterizeMicromap(b, C.byref(bake.ddesc), C.byref(r), C.byref(desc), C.byref(o) if names else None,
                                                C.byref(info) if want_info else None, None)
                assert got == ot.SUCCESS, got

            call(ru.OUTPUTS)
            got = ru.info_dict(info)
            print("  %d^2: %s" % (size, got))
            assert got["coveredPixels"] == sum(got["pixelsPerState"]) + got["invalidPixels"]
            rows.append(dict(case="%s %d info" % (config, size), info=got))
            report("%s %d^2, all outputs" % (config, size), lambda: call(ru.OUTPUTS), pixels)
            report("%s %d^2, picture only" % (config, size), lambda: call(("rgba",), False), pixels)
            report("%s %d^2, info only" % (config, size), lambda: call(()), pixels)
            for p in bufs.values():
                hip.free(p)
        if config == "c2":   # the context: as many primitive-sorted hits as the smaller image has pixels
            n = sizes[0] * sizes[0]
            rng = np.random.default_rng(1)
            hits = np.empty(n, lu.HIT)
            hits["prim"] = np.sort(rng.integers(0, ix.size // 3, n, dtype=np.uint32))
            w = rng.random((n, 2), dtype=np.float32)
            fold = w.sum(axis=1) > 1.0
            w[fold] = 1.0 - w[fold]
            hits["u"], hits["v"] = w[:, 0], w[:, 1]
            dh, dout = hip.upload(hits), hip.alloc(n)
            report("ommxLookupOpacity, %d sorted hits" % n, lambda: dll.ommxLookupOpacity(C.byref(r), dh, n, dout, 0, None), n)
            hip.free(dh)
            hip.free(dout)
        bake.close()
        product.destroy_texture(b, t)
    product.destroy_baker(b)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
