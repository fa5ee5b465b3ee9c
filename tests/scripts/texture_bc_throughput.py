"""Time of ommxCreateTextureBC / ommxCreateTextureBCDevice (not a test): textures of 4096^2 and 8192^2 texels made from BC1, BC3 and BC4 blocks, with and
without a summed-area table, on both entries, next to two yardsticks measured in the same run:
  * ommxCreateTextureDevice from a packed image of the resulting texel type and size in HBM (R8 for BC1, R32F for BC3 / BC4): it writes the same bytes
    and reads more;
  * the route without these calls: decode on the CPU, then ommCpuCreateTexture.  The CPU decoder is Pillow's (its C decoder for DDS files, which gives
    bytes) where Pillow imports, the numpy reference decoder of tests/block_texture_util.py otherwise; neither is a tuned decoder.
Wall clock around each whole call plus the texture's destruction (every call returns with the texture complete), best of --reps in one process after one
warm-up call; all timings of the BC device entry are kept so that its spread can be read.

    python tests/scripts/texture_bc_throughput.py [--sizes 4096 8192] [--reps 5] [--json out.json]

Before any timing is printed the serialized blob (texels and tables) of every block-made texture is compared by digest with that of the texture
ommCpuCreateTexture makes from the numpy-decoded texels.  The script ends itself after --time-limit seconds."""
import argparse
import hashlib
import io
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
import block_texture_util as bu  # noqa: E402

try:
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
except ImportError:
    Image = None

FORMATS = [("BC1", bu.BC1), ("BC3", bu.BC3), ("BC4", bu.BC4)]


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


def decode_in_strips(fmt, blocks, n):
    """the numpy reference decoder, 64 rows of blocks at a time (its intermediates are 64-bit)"""
    out = np.empty((n, n), np.uint8 if fmt in (bu.BC1, bu.BC2) else np.float32)
    for r0 in range(0, blocks.shape[0], 64):
        r1 = min(r0 + 64, blocks.shape[0])
        out[4 * r0:4 * r1] = bu.decode(fmt, 0, blocks[r0:r1], n, 4 * (r1 - r0))
    return out


def cpu_decode(fmt, blocks, n):
    """-> the alpha as the array a user would hand to ommCpuCreateTexture"""
    if Image is None:
        return decode_in_strips(fmt, blocks, n)
    img = Image.open(io.BytesIO(bu.dds_bytes(fmt, blocks, n, n)))
    img.load()
    return np.ascontiguousarray(np.array(img.getchannel("A") if fmt != bu.BC4 else img))


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
    bu.bind(product.dll)
    hip = ot.Hip()
    b = product.create_baker()
    decoder = "Pillow" if Image is not None else "numpy"
    rows = []
    for n in a.sizes:
        assert n % 4 == 0
        lines = []
        for name, fmt in FORMATS:
            blocks = bu.random_blocks(fmt, n, n, seed=n + fmt)
            texels = decode_in_strips(fmt, blocks, n)
            t = product.create_texture(b, [texels], alpha_cutoff=0.5, disable_zorder=True)
            want = digest(product, b, t)
            product.destroy_texture(b, t)
            dev_blocks = bu.DeviceBlocks(hip, blocks)
            host_blocks = bu.HostBlocks(blocks)
            packed = hip.upload(texels)
            packed_fmt = tu.UNORM8 if texels.dtype == np.uint8 else tu.FP32
            for device, src in ((True, dev_blocks), (False, host_blocks)):
                t = bu.create(product, b, bu.make_desc(fmt, 0, [src.mip(n, n)], 0.5, True), device)
                got = digest(product, b, t)
                product.destroy_texture(b, t)
                assert got == want, "%s at %d^2 (%s entry): the block-made texture's blob differs from the host-made one's" % (name, n, "device" if device else "host")
            t0 = time.perf_counter()
            decoded = cpu_decode(fmt, blocks, n)
            decode_ms = (time.perf_counter() - t0) * 1e3
            for cutoff in (0.5, -1.0):
                bc_dev = bu.make_desc(fmt, 0, [dev_blocks.mip(n, n)], cutoff, True)
                bc_host = bu.make_desc(fmt, 0, [host_blocks.mip(n, n)], cutoff, True)
                pk = tu.make_desc(packed_fmt, 0, 0, [(n, n, 0, packed.value)], cutoff, True)
                dev_ms, dev_all = best_ms(lambda: product.destroy_texture(b, bu.create(product, b, bc_dev, True)), a.reps)
                host_ms = best_ms(lambda: product.destroy_texture(b, bu.create(product, b, bc_host, False)), a.reps)[0]
                packed_ms, packed_all = best_ms(lambda: product.destroy_texture(b, tu.create(product, b, pk)), a.reps)
                create_ms = best_ms(lambda: product.destroy_texture(b, product.create_texture(b, [decoded], alpha_cutoff=cutoff, disable_zorder=True)), a.reps)[0]
                rows.append(dict(size=n, format=name, table=cutoff >= 0, bc_device_ms=dev_ms, bc_device_all_ms=dev_all, bc_host_ms=host_ms, packed_device_ms=packed_ms,
                                 packed_device_all_ms=packed_all, cpu_decoder=decoder, cpu_decode_ms=decode_ms, cpu_create_ms=create_ms, block_bytes=int(blocks.size),
                                 texel_bytes=int(texels.nbytes)))
                lines.append("%5d^2  %s table %-3s  BCDevice %7.3f ms (max of %d: %7.3f)   BC (host blocks) %7.3f ms   ommxCreateTextureDevice of packed %s %7.3f ms (max %7.3f)   "
                             "%s decode %8.1f ms + ommCpuCreateTexture %7.3f ms"
                             % (n, name, "yes" if cutoff >= 0 else "no", dev_ms, a.reps, max(dev_all), host_ms, "R8" if packed_fmt == tu.UNORM8 else "R32F", packed_ms, max(packed_all),
                                decoder, decode_ms, create_ms))
            dev_blocks.free()
            hip.free(packed)
        print("\n".join(lines), flush=True)   # (after every digest of this size has been compared)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    product.destroy_baker(b)


if __name__ == "__main__":
    main()
