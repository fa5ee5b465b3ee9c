"""Time of ommxCreateTextureDevice (not a test): textures of 4096^2 and 8192^2 texels made from RGBA8, RGBA16F and packed UNORM8 images that live in HBM, with
and without a summed-area table, next to ommCpuCreateTexture of the extracted channel from (pageable) host memory -- the same resulting texture.
Wall clock around each call (both calls return with the texture complete), best of --reps in one process after one warm-up call.

    python tests/scripts/texture_device_throughput.py [--sizes 4096 8192] [--reps 5] [--json out.json]

Before any timing is printed the serialized blob (texels and tables) of every device-made texture is compared with the host-made one's by digest.
Bytes per second count what the gather needs: the source rows once, the texels once.  The script asserts that the device route is not slower than
the host route for the same texture, and ends itself after --time-limit seconds."""
import argparse
import hashlib
import json
import os
import signal
import sys
import time
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import ommtest as ot  # noqa: E402
import sat_util as su  # noqa: E402
import texture_device_util as tu  # noqa: E402

SOURCES = [("RGBA8.a", tu.UNORM8, 4, 3), ("RGBA16F.a", tu.FP16, 8, 6), ("R8", tu.UNORM8, 1, 0)]


def best_ms(call, reps):
    call()   # warm-up: pools, code objects
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out), out


def digest(lib, baker, tex):
    return hashlib.blake2b(su.serialize_texture(lib, baker, tex, 0), digest_size=16).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=540)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    signal.alarm(a.time_limit)   # SIGALRM's default action ends the process
    product = ot.Lib("product")
    tu.bind(product.dll)
    hip = ot.Hip()
    b = product.create_baker()
    rows = []
    for n in a.sizes:
        alpha8 = ot.foliage_texture(1234, n, n, feature=64)
        assert alpha8.dtype == np.uint8
        alpha16 = (alpha8.astype(np.float32) / np.float32(255)).astype(np.float16)
        host = {tu.UNORM8: alpha8, tu.FP16: alpha16.astype(np.float32)}
        want = {}
        for fmt, mip in host.items():
            t = product.create_texture(b, [mip], alpha_cutoff=0.5, disable_zorder=True)
            want[fmt] = digest(product, b, t)
            product.destroy_texture(b, t)
        host_ms = {}
        for fmt, mip in host.items():
            for cutoff in (0.5, -1.0):
                def host_call():
                    product.destroy_texture(b, product.create_texture(b, [mip], alpha_cutoff=cutoff, disable_zorder=True))
                host_ms[(fmt, cutoff)] = best_ms(host_call, a.reps)[0]
        lines = []
        for name, fmt, stride, offset in SOURCES:
            bits = alpha8 if fmt == tu.UNORM8 else alpha16.view(np.uint16)
            cb = tu.CHANNEL_BYTES[fmt]
            img = np.full((n, n, stride // cb), 0x7E01 if fmt == tu.FP16 else 0x55, tu.SOURCE_DTYPE[fmt])   # the other channels: NaN / other bytes
            img[:, :, offset // cb] = bits
            base = hip.upload(img)
            del img
            mip = (n, n, 0, base.value)
            t = tu.create(product, b, tu.make_desc(fmt, stride, offset, [mip], 0.5, True))
            got = digest(product, b, t)
            product.destroy_texture(b, t)
            assert got == want[fmt], "%s at %d^2: the device-made texture's blob differs from the host-made one's" % (name, n)
            for cutoff in (0.5, -1.0):
                desc = tu.make_desc(fmt, stride, offset, [mip], cutoff, True)

                def device_call():
                    product.destroy_texture(b, tu.create(product, b, desc))
                ms = best_ms(device_call, a.reps)[0]
                moved = n * n * stride + n * n * (1 if fmt == tu.UNORM8 else 4)
                rows.append(dict(size=n, source=name, table=cutoff >= 0, device_ms=ms, host_ms=host_ms[(fmt, cutoff)], gather_bytes=moved))
                lines.append("%5d^2  %-9s table %-3s  ommxCreateTextureDevice %8.3f ms   ommCpuCreateTexture of the channel %8.3f ms   gather moves %.0f MB (%.0f GB/s over the whole call)"
                             % (n, name, "yes" if cutoff >= 0 else "no", ms, host_ms[(fmt, cutoff)], moved / 1e6, moved / (ms * 1e-3) / 1e9))
            hip.free(base)
        print("\n".join(lines), flush=True)   # (after every digest of this size has been compared)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    slower = [r for r in rows if r["device_ms"] > r["host_ms"]]
    assert not slower, "the device route is slower than the host route: %r" % slower
    product.destroy_baker(b)


if __name__ == "__main__":
    main()
