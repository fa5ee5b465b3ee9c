"""Throughput of the micromap consumer (not a test): ommxLookupOpacity and ommxResolveHits on the metric configuration's result (workloads c2:
1 M triangles, level 8, 4-state, baked through ommxBakeDevice), 2^26 hits per call, HIP events around each call after a warm-up.

    python tests/scripts/lookup_throughput.py [--hits-log2 26] [--reps 10] [--json out.json]

Prints one line per case: median / min / max ms, hits/s, and the bytes the algorithm needs per hit (hit record 12 B + index entry + 8-byte descriptor
+ state byte + output byte; resolve adds, for a hit that samples the texture, three vertex indices, three texture coordinates and the texels of
the filter).  Kernel times for the same calls: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` separately."""
import argparse
import ctypes as C
import json
import os
import sys
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import ommtest as ot  # noqa: E402
import workloads as wl  # noqa: E402
import lookup_util as lu  # noqa: E402


def timed(hip, fn, reps, warmup=3):
    rt = hip.rt
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert rt.hipEventCreate(C.byref(e)) == 0
    for _ in range(warmup):
        fn()
    assert rt.hipDeviceSynchronize() == 0
    ms = []
    for _ in range(reps):
        assert rt.hipEventRecord(ev[0], None) == 0
        fn()
        assert rt.hipEventRecord(ev[1], None) == 0
        assert rt.hipEventSynchronize(ev[1]) == 0
        t = C.c_float()
        assert rt.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
        ms.append(t.value)
    for e in ev:
        rt.hipEventDestroy(e)
    return np.array(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits-log2", type=int, default=26)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    product = ot.Lib("product")
    dll = lu.bind(product.dll)
    hip = ot.Hip()
    hip.rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.rt.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.rt.hipEventDestroy.argtypes = [C.c_void_p]

    tex, uv, ix, lv, kw = wl.workload("c2")
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    d = ot.make_desc(t, uv, ix, kw.pop("level"), levels=lv, **kw)
    bake = lu.DeviceBake(product, hip, b, d, uv, ix, lv)
    r = bake.rdesc
    ntri = ix.size // 3
    isz = {ot.IDX_U8: 1, ot.IDX_U16: 2, ot.IDX_U32: 4}[r.indexFormat]
    print("result: %d triangles, %d OMMs, arrayData %.1f MiB, %d-byte index entries" % (ntri, r.descArrayCount, r.arrayDataSize / 2**20, isz))

    n = 1 << a.hits_log2
    rng = np.random.default_rng(1)
    hits = np.empty(n, lu.HIT)
    hits["prim"] = rng.integers(0, ntri, n, dtype=np.uint32)
    w = rng.random((n, 2), dtype=np.float32)
    fold = w.sum(axis=1) > 1.0                                 # uniform over the triangle
    w[fold] = 1.0 - w[fold]
    hits["u"], hits["v"] = w[:, 0], w[:, 1]
    sorted_hits = hits.copy()
    sorted_hits["prim"] = np.sort(hits["prim"])
    d_rand, d_sorted, d_out = hip.upload(hits), hip.upload(sorted_hits), hip.alloc(n)
    lookup_bytes = 12 + isz + 8 + 1 + 1
    rows = []

    def report(name, ms, bytes_per_hit, extra=""):
        med = float(np.median(ms))
        row = dict(case=name, hits=n, median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()), hits_per_s=n / (med * 1e-3),
                   bytes_per_hit=bytes_per_hit, gbytes_per_s=n * bytes_per_hit / (med * 1e-3) / 1e9)
        rows.append(row)
        print("%-22s median %8.3f ms  (min %.3f, max %.3f, %d reps)  %.2f G hits/s  %d B/hit -> %.0f GB/s%s"
              % (name, med, ms.min(), ms.max(), len(ms), row["hits_per_s"] / 1e9, bytes_per_hit, row["gbytes_per_s"], extra))
        return row

    for name, dh in (("lookup_random", d_rand), ("lookup_sorted", d_sorted)):
        ms = timed(hip, lambda: dll.ommxLookupOpacity(C.byref(r), dh, n, d_out, 0, None), a.reps)
        report(name, ms, lookup_bytes)

    def resolve(dh):
        assert dll.ommxResolveHits(b, C.byref(bake.ddesc), C.byref(r), dh, n, d_out, 0, None) == ot.SUCCESS
    for name, dh in (("resolve_random", d_rand), ("resolve_sorted", d_sorted)):
        ms = timed(hip, lambda: resolve(dh), a.reps)
        out = hip.download(d_out, n)
        share = float(((out & 8) != 0).mean())
        # a sampled hit also reads 3 x 4-byte vertex indices, 3 x 8-byte texture coordinates and 4 one-byte texels (Linear)
        row = report(name, ms, lookup_bytes, "  texture sampled for %.2f %% of the hits (%.2f %% skipped it)" % (100 * share, 100 * (1 - share)))
        row["sampled_share"] = share
        row["bytes_per_sampled_hit_extra"] = 3 * 4 + 3 * 8 + 4
    for p in (d_rand, d_sorted, d_out):
        hip.free(p)
    bake.close()
    product.destroy_texture(b, t)
    product.destroy_baker(b)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(config="c2 (1 M triangles, level 8, 4-state, ommxBakeDevice)", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
