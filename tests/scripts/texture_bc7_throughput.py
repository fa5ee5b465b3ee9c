"""Time of ommxCreateTextureBC7 / ommxCreateTextureBC7Device (not a test): textures of 4096^2 and 8192^2 texels made from BC7 blocks, with and without a
summed-area table, on both entries, next to two yardsticks measured in the same run:
  * ommxCreateTextureBCDevice of a BC3 image of the same size: per block it also reads 16 bytes, but writes 64 bytes of fp32 where BC7 writes 16;
  * ommxCreateTextureDevice from the packed R8 image of the decoded bytes in HBM: it writes the same bytes and reads as many.
The BC7 image is a 1024^2 image of forced-mode random blocks (tests/bc7_util.py: at least half of the blocks in the modes 4..7, all modes mixed inside
every wave) repeated over the size, so that the reference decode of 65 536 blocks serves every size.  Wall clock around each whole call plus the
texture's destruction (every call returns with the texture complete), best of --reps in one process after one warm-up call; all timings of the BC7
device entry are kept so that its spread can be read.

    python tests/scripts/texture_bc7_throughput.py [--sizes 4096 8192] [--reps 5] [--json out.json]

Before any timing is printed the serialized blob (texels and tables) of every block-made texture is compared by digest with that of the texture
ommCpuCreateTexture makes from the reference-decoded bytes.  The script ends itself after --time-limit seconds."""
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
import block_texture_util as bu  # noqa: E402
import bc7_util as b7  # noqa: E402

TILE = 1024


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
    bu.bind(product.dll)
    b7.bind(product.dll)
    hip = ot.Hip()
    b = product.create_baker()
    tile_blocks = b7.random_blocks(TILE, TILE, seed=7)
    tile_texels = b7.decode(tile_blocks, TILE, TILE)
    rows = []
    for n in a.sizes:
        assert n % TILE == 0
        blocks = np.ascontiguousarray(np.tile(tile_blocks, (n // TILE, n // TILE, 1)))
        texels = np.ascontiguousarray(np.tile(tile_texels, (n // TILE, n // TILE)))
        t = product.create_texture(b, [texels], alpha_cutoff=0.5, disable_zorder=True)
        want = digest(product, b, t)
        product.destroy_texture(b, t)
        dev_blocks, host_blocks = bu.DeviceBlocks(hip, blocks), bu.HostBlocks(blocks)
        bc3_blocks = bu.DeviceBlocks(hip, bu.random_blocks(bu.BC3, n, n, seed=n))
        packed = hip.upload(texels)
        for device, src in ((True, dev_blocks), (False, host_blocks)):
            t = b7.create(product, b, b7.make_desc([src.mip(n, n)], 0.5, True), device)
            got = digest(product, b, t)
            product.destroy_texture(b, t)
            assert got == want, "%d^2 (%s entry): the block-made texture's blob differs from the host-made one's" % (n, "device" if device else "host")
        lines = []
        for cutoff in (0.5, -1.0):
            d_dev, d_host = b7.make_desc([dev_blocks.mip(n, n)], cutoff, True), b7.make_desc([host_blocks.mip(n, n)], cutoff, True)
            d_bc3 = bu.make_desc(bu.BC3, 0, [bc3_blocks.mip(n, n)], cutoff, True)
            pk = tu.make_desc(tu.UNORM8, 0, 0, [(n, n, 0, packed.value)], cutoff, True)
            dev_ms, dev_all = best_ms(lambda: product.destroy_texture(b, b7.create(product, b, d_dev, True)), a.reps)
            host_ms = best_ms(lambda: product.destroy_texture(b, b7.create(product, b, d_host, False)), a.reps)[0]
            bc3_ms, bc3_all = best_ms(lambda: product.destroy_texture(b, bu.create(product, b, d_bc3, True)), a.reps)
            packed_ms, packed_all = best_ms(lambda: product.destroy_texture(b, tu.create(product, b, pk)), a.reps)
            rows.append(dict(size=n, table=cutoff >= 0, bc7_device_ms=dev_ms, bc7_device_all_ms=dev_all, bc7_host_ms=host_ms, bc3_device_ms=bc3_ms, bc3_device_all_ms=bc3_all,
                             packed_r8_device_ms=packed_ms, packed_r8_device_all_ms=packed_all, block_bytes=int(blocks.size), texel_bytes=int(texels.nbytes)))
            lines.append("%5d^2  table %-3s  BC7Device %7.3f ms (max of %d: %7.3f)   BC7 (host blocks) %7.3f ms   BCDevice of BC3 %7.3f ms (max %7.3f)   "
                         "ommxCreateTextureDevice of packed R8 %7.3f ms (max %7.3f)"
                         % (n, "yes" if cutoff >= 0 else "no", dev_ms, a.reps, max(dev_all), host_ms, bc3_ms, max(bc3_all), packed_ms, max(packed_all)))
        for p in (dev_blocks, bc3_blocks):
            p.free()
        hip.free(packed)
        print("\n".join(lines), flush=True)   # (after every digest of this size has been compared)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    product.destroy_baker(b)


if __name__ == "__main__":
    main()
