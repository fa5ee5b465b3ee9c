"""Every device entry on memory that ommxBakerKnob_PoisonMemory has filled with a word: the scratch and result blocks of the baker's device pool and
the working set of a bake are handed out as the last user left them, and each entry trusts a memset or a kernel to write what it reads
(tests/README_poison.md: the ledger, region by region, and kernel -> case).  Here every entry runs under each of the four words of
poison_cases.WORDS and is held, byte for byte, to the model or the oracle that its own GPU file already uses -- never to the product's unpoisoned run.
A derived entry first meets a decoy (equal counts, every block the same uniform block), then the real source: the real call's scratch is the decoy's,
with the word on top.

Positive controls, so that a hook that does nothing cannot pass: the bytes behind every output array of a derived result, up to the next 4096-byte
boundary of its pool block, hold the word (PoisonedDll looks when the helper destroys the result); the pool counter grows by at least the rounded
sizes of those arrays; the working-set counter grows across every bake; with the knob off both counters stand still.

Concurrent callers are supported by the code (a call owns its PoolBlocks, DevPool and the arena pool lock, the fill's counters are atomics), so that
family is here.  No test tries to make the device fault."""
import ctypes as C
import threading
import traceback
import numpy as np
import pytest
import bench
import blobfmt
import ommtest as ot
import poison_cases as pc
import coarsen_util as cu
import combine_util as bu_combine
import gather_util as gu
import reorient_util as rt
import compare_util as pu
import merge_util as mu
import geometry_util as geo
import fit_util as fu
import rasterize_util as ru
import lookup_util as lu
import stats_util as su
import sat_util
import texture_device_util as tu
import block_texture_util as btu
import bc7_util as b7
from test_gpu_parity import both
from test_fit_gpu import profile_and_check, levels_and_check, fit_and_check
from test_stats_gpu import table_and_check
from test_rasterize_gpu import Session, checker_texture
import test_texture_bc_gpu
import test_texture_bc7_gpu

pytestmark = pytest.mark.gpu
JOIN_SECONDS = 120
POISONED = pytest.mark.parametrize("word", pc.WORDS, ids=pc.WORD_IDS)


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    d = product.dll
    for m in (cu, bu_combine, gu, rt, pu, mu, geo, fu, ru, lu, su):
        m.bind(d)
    return d


def word_bytes(word, start, count):
    """`count` bytes of memory filled with `word`, from byte offset `start` of a block (blocks are 256-byte aligned)"""
    return np.resize(np.roll(np.frombuffer(np.uint32(word).tobytes(), np.uint8), -(start % 4)), count)


class PoisonedDll:
    """The product library as the helpers of the other GPU files take it, with one addition: when a helper destroys a device result, the bytes behind
    each of its arrays up to the next 4096-byte boundary (inside the pool block: capacities are multiples of 4096) must still hold the word."""

    def __init__(self, dll, hip, word):
        self._dll, self._hip, self._word = dll, hip, word
        self.rounded, self.tails = 0, 0

    def __getattr__(self, name):
        return getattr(self._dll, name)

    def check_tails(self, handle):
        rd = cu.result_desc_of(self._dll, handle)
        isz = np.dtype(su.INDEX_DTYPE[rd.indexFormat]).itemsize
        for name, ptr, size in (("arrayData", rd.arrayData, rd.arrayDataSize), ("descArray", C.cast(rd.descArray, C.c_void_p).value, 8 * rd.descArrayCount),
                                ("indexBuffer", rd.indexBuffer, isz * rd.indexCount)):
            if not ptr or not size:
                continue
            end = (size + 4095) // 4096 * 4096
            self.rounded += end
            if end > size:
                got = self._hip.download(C.c_void_p(ptr + size), end - size)
                want = word_bytes(self._word, size, end - size)
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, "%s: %d bytes behind the array do not hold the word, first at +%d: 0x%02X" % (name, bad.size, bad[0], got[bad[0]])
                self.tails += 1

    def ommxDestroyDeviceBakeResult(self, handle):
        self.check_tails(handle)
        return self._dll.ommxDestroyDeviceBakeResult(handle)


class Poisoned:
    """one poisoned baker and the controls on its counters"""

    def __init__(self, product, dll, hip, word):
        self.product, self.hip, self.word = product, hip, word
        self.baker = product.create_baker()
        assert product.poisoned_bytes(self.baker) == (0, 0)
        product.set_knob(self.baker, ot.KNOB_POISON, ot.poison(word))
        self.dll = PoisonedDll(dll, hip, word)

    def counters(self):
        return self.product.poisoned_bytes(self.baker)

    def leak(self):
        """the baker is not destroyed at the end of the test (a thread that outlived its time limit may still use it)"""
        self.leaked = True

    def close(self, results=True):
        if getattr(self, "leaked", False):
            return
        pool, ws = self.counters()
        if results:
            assert self.dll.tails > 0, "no result array was looked at"
        assert pool >= self.dll.rounded and pool > 0, (pool, self.dll.rounded)
        self.product.destroy_baker(self.baker)


@pytest.fixture()
def pb(product, dll, hip, word):
    p = Poisoned(product, dll, hip, word)
    yield p
    p.close()


@pytest.fixture()
def pb_plain(product, dll, hip, word):
    """for the entries that make no device result"""
    p = Poisoned(product, dll, hip, word)
    yield p
    p.close(results=False)


def sources(hip, arrays, index_format, array_align=16):
    return cu.Source(hip, arrays[0], arrays[1], arrays[2], index_format, array_align=array_align)


class Pairs:
    """decoy and real source of poison_cases in each index format, closed together"""

    def __init__(self, hip, pair=None, formats=pc.INDEX_FORMATS, seed=0):
        self.open = []
        self.items = []
        decoy, real = pair if pair else pc.derived_pair(seed)
        for f in formats:
            d, r = sources(hip, decoy, f), sources(hip, real, f)
            self.open += [d, r]
            self.items.append((f, d, r))

    def __iter__(self):
        return iter(self.items)

    def close(self):
        for s in self.open:
            s.close()


# ---- derived entries: decoy first, then the real source, on one poisoned baker ----
COARSEN_CAPS = (0, 3, 4, 7, 8, 12)          # below a lane's 256 micro-triangles, at and above a wave's share, the unit level, nothing coarsened


@POISONED
def test_coarsen(pb, hip, word):
    """ommxCoarsenMicromap / ommxCoarsenMicromapLevels: info-only and full call per source (coarsen_and_check), then the per-block levels as the side input"""
    pairs = Pairs(hip)
    try:
        for k, (f, decoy, real) in enumerate(pairs):
            for cap in COARSEN_CAPS:
                for flags in (cu.NONE, cu.NO_SPECIAL | cu.NO_DEDUP):
                    cu.coarsen_and_check(pb.dll, hip, pb.baker, decoy, cap, 2 + k % 2, flags)
                    ref = cu.coarsen_and_check(pb.dll, hip, pb.baker, real, cap, 2 + k % 2, flags)
                    assert ref["info"]["skippedPrimitives"] == 2
            # the pool counter across ONE info-only call and ONE full call (the same scratch blocks): the difference is the result's three arrays, each
            # rounded up to 4096 at the least
            pool0 = pb.counters()[0]
            r, info, none = cu.coarsen(pb.dll, pb.baker, real.rd, 4, want_result=False)
            pool1 = pb.counters()[0]
            r2, info2, h = cu.coarsen(pb.dll, pb.baker, real.rd, 4)
            pool2 = pb.counters()[0]
            assert (r, r2) == (ot.SUCCESS, ot.SUCCESS) and none is None and info == info2
            rd = cu.result_desc_of(pb.dll, h)
            isz = np.dtype(su.INDEX_DTYPE[rd.indexFormat]).itemsize
            arrays = sum((n + 4095) // 4096 * 4096 for n in (rd.arrayDataSize, 8 * rd.descArrayCount, isz * rd.indexCount))
            assert rd.arrayDataSize and (pool2 - pool1) - (pool1 - pool0) >= arrays, (pool0, pool1, pool2, arrays)          # (a reused block may be larger)
            assert pb.dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS
            own = (np.arange(len(real.host[1])) * 5 % 11).astype(np.int64)
            levels_and_check(pb.dll, hip, pb.baker, decoy, own[::-1].copy(), 12, 3, cu.NO_SPECIAL | cu.NO_DEDUP)
            levels_and_check(pb.dll, hip, pb.baker, real, own, 12, 3, cu.NO_SPECIAL | cu.NO_DEDUP)
            levels_and_check(pb.dll, hip, pb.baker, real, own, 6, 2)
    finally:
        pairs.close()


@POISONED
def test_combine(pb, hip, word):
    """ommxCombineMicromaps of two and of three sources in different index formats"""
    a, b = Pairs(hip, seed=0), Pairs(hip, seed=50)
    try:
        (_, da, ra), (_, db, rb), (_, dc, rc) = a.items[0], b.items[1], a.items[2]
        for fmt, mixed in ((ot.FMT_2STATE, 2), (ot.FMT_4STATE, 3)):
            bu_combine.combine_and_check(pb.dll, hip, pb.baker, [da, db], fmt, mixed)
            bu_combine.combine_and_check(pb.dll, hip, pb.baker, [ra, rb], fmt, mixed)
            bu_combine.combine_and_check(pb.dll, hip, pb.baker, [da, db, dc], fmt, mixed)
            bu_combine.combine_and_check(pb.dll, hip, pb.baker, [ra, rb, rc], fmt, mixed)
    finally:
        a.close()
        b.close()


@POISONED
def test_gather(pb, hip, word):
    """ommxGatherMicromaps: everything of two sources, and a selection with repeats, a source and a primitive out of range"""
    a, b = Pairs(hip, seed=0), Pairs(hip, seed=50)
    try:
        for k in range(3):
            (_, da, ra), (_, db, rb) = a.items[k], b.items[(k + 1) % 3]
            T = len(ra.host[2])
            sel = [(0, 0), (1, 3), (0, T - 1), (2, 0), (1, T), (0, 5), (1, 3), (0, 7), (1, 9), (0, 10), (1, 0)]
            for flags in (0, gu.NO_SPECIAL | gu.NO_DEDUP):
                gu.gather_and_check(pb.dll, hip, pb.baker, [da, db], None, flags)
                gu.gather_and_check(pb.dll, hip, pb.baker, [ra, rb], None, flags)
                gu.gather_and_check(pb.dll, hip, pb.baker, [da, db], sel, flags)
                ref = gu.gather_and_check(pb.dll, hip, pb.baker, [ra, rb], sel, flags)
                assert ref["info"]["skippedPrimitives"] >= 2
    finally:
        a.close()
        b.close()


@POISONED
def test_reorient(pb, hip, word):
    """ommxReorientMicromap: one orientation for all, and one per primitive through all six"""
    pairs = Pairs(hip)
    try:
        for f, decoy, real in pairs:
            T = len(real.host[2])
            each = (np.arange(T) % 6).astype(np.uint8)
            for orient in (4, each):
                for flags in (0, rt.NO_SPECIAL | rt.NO_DEDUP):
                    rt.reorient_and_check(pb.dll, hip, pb.baker, decoy, orient, flags=flags)
                    rt.reorient_and_check(pb.dll, hip, pb.baker, real, orient, flags=flags)
    finally:
        pairs.close()


@POISONED
def test_merge(pb, hip, word):
    """ommxMergeSimilarMicromaps: info-only, roots-only and full call (merge_and_check) at levels 1, 2, 3, 5, 6, 7 with one level-8 block, and leaders of 1,
    64 and 65 members; before each a decoy of uniform blocks and one of equal mixed blocks"""
    limit = mu.UNIT * 4 // 100
    levels = pc.merge_levels_real()
    a, d, i, family = pc.merge_leaders_real()
    for real, fmt, kw in ((levels, ot.IDX_U8, dict(seed=5)), ((a, d, i), ot.IDX_U16, dict(rounds=1, samples=pc.MERGE_BUCKET["samples"], seed=pc.MERGE_BUCKET["seed"]))):
        srcs = [sources(hip, pc.decoy_of(real[1], real[2]), fmt, 1), sources(hip, pc.merge_equal_decoy(real[1], real[2]), fmt, 1), sources(hip, real, fmt, 1)]
        try:
            for mixed in (2, 3):
                for s in srcs:
                    ref = mu.merge_and_check(pb.dll, hip, pb.baker, s, limit, mixed=mixed, **kw)
            assert ref["info"]["absorbedBlocks"] > 0
        finally:
            for s in srcs:
                s.close()
    sizes = np.bincount(ref["roots"])
    assert sorted((sizes[sizes > 0] - 1).tolist()) == list(pc.MERGE_LEADERS)


@POISONED
def test_profile_and_fit(pb, hip, word):
    """ommxProfileMicromapLevels (no result), then ommxFitMicromap: info-only, full call and its identity with ommxCoarsenMicromapLevels (fit_and_check)"""
    deep = Pairs(hip, formats=[ot.IDX_U16])          # (a block above level 8: the second pass of the profile)
    try:
        for _, decoy_s, real_s in deep:
            profile_and_check(pb.dll, hip, pb.baker, decoy_s)
            ref = profile_and_check(pb.dll, hip, pb.baker, real_s)
            assert ref["info"]["skippedPrimitives"] == 2
    finally:
        deep.close()
    array_data, descs, index, weights = pc.fit_real()
    real = (array_data, descs, index)
    for f in pc.INDEX_FORMATS:
        decoy_s, real_s = sources(hip, pc.decoy_of(descs, index), f, 1), sources(hip, real, f, 1)
        dev = hip.upload(weights)
        try:
            profile_and_check(pb.dll, hip, pb.baker, decoy_s, weights)
            prof = profile_and_check(pb.dll, hip, pb.baker, real_s, weights)
            profile_and_check(pb.dll, hip, pb.baker, decoy_s)
            profile_and_check(pb.dll, hip, pb.baker, real_s)
            floor = fu.restate_plan(prof["shape"], prof["known"], prof["opaque"], prof["weights"], 0, 12, True)
            low, top = floor["planned"], floor["unfitted"]
            dprof = fu.restate_profile(*pc.decoy_of(descs, index), weights, unpacked=decoy_s.unpacked)
            for budget in ((low + top) // 2, low + 7):
                fit_and_check(pb.dll, hip, pb.baker, decoy_s, 1 << 20, weights, dev, dprof)
                plan, _ = fit_and_check(pb.dll, hip, pb.baker, real_s, budget, weights, dev, prof)
                assert plan["steps"] > 0
        finally:
            hip.free(dev)
            decoy_s.close()
            real_s.close()


@POISONED
def test_compare(pb_plain, hip, word):
    """ommxCompareMicromaps: info-only, outputs-only, full and single-output calls (compare_and_check); a source against a coarser relative and against itself"""
    pb = pb_plain
    a, b = Pairs(hip, seed=0), Pairs(hip, seed=50)
    try:
        for k in range(3):
            (_, da, ra), (_, db, rb) = a.items[k], b.items[(k + 1) % 3]
            for force2 in (False, True):
                pu.compare_and_check(pb.dll, hip, pb.baker, da, db, force2)
                ref = pu.compare_and_check(pb.dll, hip, pb.baker, ra, rb, force2)
                assert len(ref["relations"]) == len(ra.host[2])
            pu.compare_and_check(pb.dll, hip, pb.baker, ra, ra)
    finally:
        a.close()
        b.close()


def stats_and_check(dll, hip, baker, arrays, index_format, stream=None):
    """test_stats_gpu.table_and_check (every output of ommxDebugGetStatsDevice against stats_util.reference_stats) on a source of poison_cases"""
    array_data, descs, index = arrays
    areas = (0.25 + (np.arange(len(index)) % 7) / 8).astype(np.float32)
    return table_and_check(dll, hip, baker, index_format, array_data, descs, index, areas, stream)


@POISONED
def test_stats(pb_plain, hip, word):
    pb = pb_plain
    decoy, real = pc.derived_pair()
    for f in pc.INDEX_FORMATS:
        stats_and_check(pb.dll, hip, pb.baker, decoy, f)
        ref = stats_and_check(pb.dll, hip, pb.baker, real, f)
        assert ref["skipped"] == 2


@POISONED
def test_geometry(pb_plain, hip, word):
    """ommxExtractMicroGeometry: the count-only call and the full call (extract_and_check)"""
    pb = pb_plain
    decoy, real = pc.derived_pair()
    for f, g in zip(pc.INDEX_FORMATS, (geo.IDENTITY, geo.PRESET, geo.IDENTITY)):
        geo.extract_and_check(pb.dll, hip, pb.baker, decoy[0], decoy[1], decoy[2], f, g)
        ref = geo.extract_and_check(pb.dll, hip, pb.baker, real[0], real[1], real[2], f, g)
        assert ref["skipped"] == 2 and sum(ref["counts"]) > 0


@POISONED
def test_rasterize(pb_plain, product, hip, word):
    """ommxRasterizeMicromap: ten descriptors under six primitives; images whose triangle boxes fall to a lane (21 x 9), a wave (63 x 33: 2079 pixels, no
    multiple of a wave) and the grid (385 x 97), without and with HighlightReuse (the `lowest` table)"""
    pb = pb_plain
    s = Session(product, hip, pb.baker)
    try:
        uv, ix = pc.raster_mesh()
        u8 = checker_texture(16, 8)
        scenes = [s.scene(tex, uv, ix, ru.HostResult.of(pc.raster_result(equal)[0]), addr=ot.WRAP)
                  for equal, tex in ((True, u8), (False, u8), (False, (u8 / np.float32(255)).astype(np.float32)))]          # (the last: the FP32 shade)
        for w, h in pc.RASTER_IMAGES:
            for flags in (0, ru.HIGHLIGHT_REUSE):
                for dev in scenes:
                    ref = ru.check(pb.dll, hip, dev, pc.RASTER_VIEW, w, h, flags=flags)
                assert ref["info"]["coveredPixels"] > 0 and ref["info"]["drawnPrimitives"] == pc.RASTER_PRIMS
    finally:
        s.close()


# ---- circulation: blocks handed from one operation to another, results alive across them, a trim in the middle ----
@POISONED
def test_circulation(pb, product, hip, word):
    decoy, real = pc.derived_pair()
    other = pc.derived_real(seed=50)
    dll, baker = pb.dll, pb.baker
    s = Session(product, hip, baker)
    srcs = [sources(hip, real, ot.IDX_U16), sources(hip, other, ot.IDX_U32), sources(hip, decoy, ot.IDX_U8)]
    kept = []
    try:
        uv, ix = pc.raster_mesh()
        dev = s.scene(checker_texture(), uv, ix, ru.HostResult.of(pc.raster_result(False)[0]))
        ru.check(dll, hip, dev, (0.0, 0.0, 1.0, 1.0), *pc.RASTER_IMAGE)
        r, info, h = cu.coarsen(dll, baker, srcs[0].rd, 4)
        want = srcs[0].model(4)
        assert (r, info) == (ot.SUCCESS, want["info"])
        kept.append((h, want))
        pu.compare_and_check(dll, hip, baker, srcs[0], srcs[1])
        mu.merge_and_check(dll, hip, baker, srcs[1], mu.UNIT * 4 // 100, seed=2)
        kept.append(gu.gather_and_check(dll, hip, baker, [srcs[2], srcs[0]], keep=True)[::-1])
        assert product.dll.ommxTrimBaker(baker) == ot.SUCCESS
        stats_and_check(dll, hip, baker, real, ot.IDX_U8)
        kept.append(rt.reorient_and_check(dll, hip, baker, srcs[1], 3, keep=True)[::-1])
        gu.gather_and_check(dll, hip, baker, [srcs[0], srcs[1]])
        cu.coarsen_and_check(dll, hip, baker, srcs[1], 2)
        ru.check(dll, hip, dev, (0.0, 0.0, 1.0, 1.0), 65, 5)
        for k in (1, 2, 0):          # alive across everything above, destroyed out of order: still the model's bytes, and the word behind them
            h, want = kept[k]
            cu.assert_same(cu.download_result(dll, hip, h), want)
            assert dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS
            kept[k] = None
        geo.extract_and_check(dll, hip, baker, real[0], real[1], real[2], ot.IDX_U16, geo.IDENTITY)
    finally:
        for k in kept:
            if k:
                product.dll.ommxDestroyDeviceBakeResult(k[0])
        for x in srcs:
            x.close()
        s.close()


# ---- concurrent callers ----
@POISONED
def test_four_threads_on_one_baker(pb, hip, word):
    """coarsen and gather on streams of their own, compare and statistics on the null stream: four threads, three rounds each, every answer held to its
    model.  A thread that is still running after the time limit fails the test."""
    a, b = Pairs(hip, seed=0), Pairs(hip, seed=50)
    streams = [hip.stream_create(non_blocking=True), hip.stream_create(non_blocking=True)]
    dlls = [PoisonedDll(pb.dll._dll, hip, word) for _ in range(4)]
    errors = []
    real0 = pc.derived_real(seed=0)

    def body(k):
        try:
            for round_ in range(3):
                if k == 0:
                    cu.coarsen_and_check(dlls[0], hip, pb.baker, a.items[0][1 + round_ % 2], 3 + round_, stream=streams[0])
                elif k == 1:
                    gu.gather_and_check(dlls[1], hip, pb.baker, [a.items[1][2], b.items[1][2]], stream=streams[1])
                elif k == 2:
                    pu.compare_and_check(dlls[2], hip, pb.baker, a.items[2][2], b.items[2][2], bool(round_ % 2))
                else:
                    stats_and_check(dlls[3], hip, pb.baker, real0, pc.INDEX_FORMATS[round_])
        except BaseException:          # noqa: BLE001  (an assertion of a helper: reported by the test)
            errors.append((k, traceback.format_exc()))

    threads = [threading.Thread(target=body, args=(k,), daemon=True) for k in range(4)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_SECONDS)
        assert not any(t.is_alive() for t in threads), "a caller thread is still running"
        assert not errors, errors
        for d in dlls:
            pb.dll.rounded += d.rounded
            pb.dll.tails += d.tails
    finally:
        if any(t.is_alive() for t in threads):
            pb.leak()          # a caller may still be inside an entry: its baker, sources and streams stay
        else:
            for st in streams:
                hip.stream_destroy(st)
            a.close()
            b.close()


# ---- textures ----
SAT_SHAPES = [(513, 257, 1), (300, 129, 0), (257, 257, 0), (64, 65, 1), (513, 257, 0), (1, 200, 0)]          # test_sat_gpu.test_sat_scratch_block_reused_dirty


@POISONED
def test_summed_area_tables(pb_plain, product, word):
    """the shapes of test_sat_scratch_block_reused_dirty back to back on a poisoned baker (all above the cut-off before random ones), textures alive together;
    then a two-mip chain in both tilings"""
    pb = pb_plain
    alive = []
    try:
        for n, (w, h, kind) in enumerate(SAT_SHAPES):
            tex = sat_util.contents(w, h, False, seed=40 + n)[kind][1]
            alive.append((tex, product.create_texture(pb.baker, [tex], alpha_cutoff=sat_util.CUTOFF, disable_zorder=True)))
        for tex, t in alive:
            parsed = blobfmt.parse_blob(sat_util.serialize_texture(product, pb.baker, t, 0))
            sat_util.check_tables(parsed["inputs"][0]["texture"], [tex], sat_util.CUTOFF, True)
    finally:
        for tex, t in alive:
            product.destroy_texture(pb.baker, t)
    base = sat_util.contents(130, 66, False, seed=9)[0][1]
    half = sat_util.contents(65, 33, False, seed=10)[0][1]
    for disable_zorder in (True, False):
        sat_util.tables_of(product, pb.baker, [base, half], 0.3, disable_zorder, compress_modes=(0,))


@POISONED
def test_block_compressed_textures(pb_plain, product, hip, word):
    """one BC3 and one BC7 texture of 37 x 21 texels (partial last block column and row) through the device and the host entry, checked as their own GPU
    files check them: the serialized blob of the texture ommCpuCreateTexture makes from the reference decoder's texels, and sat_util's tables"""
    pb = pb_plain
    w, h = 37, 21
    blocks = btu.random_blocks(btu.BC3, w, h, seed=5)
    mips = [btu.decode(btu.BC3, 0, blocks, w, h)]
    blocks7 = b7.random_blocks(w, h, seed=6)
    mips7 = [b7.decode(blocks7, w, h)]
    cutoff = 0.5
    for disable_zorder in (True, False):
        want = tu.host_blobs(product, pb.baker, mips, cutoff, disable_zorder)
        want7 = tu.host_blobs(product, pb.baker, mips7, cutoff, disable_zorder)
        for device in (True, False):
            src = btu.DeviceBlocks(hip, blocks) if device else btu.HostBlocks(blocks)
            src7 = btu.DeviceBlocks(hip, blocks7) if device else btu.HostBlocks(blocks7)
            try:
                test_texture_bc_gpu._made_and_checked(product, pb.baker, btu.make_desc(btu.BC3, 0, [src.mip(w, h)], cutoff, disable_zorder), device, mips, cutoff,
                                                      disable_zorder, want, "bc3 poisoned")
                test_texture_bc7_gpu._made_and_checked(product, pb.baker, b7.make_desc([src7.mip(w, h)], cutoff, disable_zorder), device, mips7, cutoff,
                                                       disable_zorder, want7, "bc7 poisoned")
            finally:
                if device:
                    src.free()
                    src7.free()


@POISONED
def test_textures_from_device_images(pb_plain, product, hip, word):
    """ommxCreateTextureDevice (texture_gather): the alpha of RGBA8, the last channel of RGBA16F and packed FP32, 65 x 5 texels (a ragged row end and peeled
    first texels), as test_texture_device_gpu.py checks them"""
    pb = pb_plain
    w, h, cutoff = 65, 5, 0.5
    for n, (fmt, stride, offset) in enumerate(((tu.UNORM8, 4, 3), (tu.FP16, 8, 6), (tu.FP32, 4, 0))):
        bits = tu.channel_bits(fmt, w, h, seed=20 + n)
        mips = [tu.texels_of(fmt, bits)]
        for disable_zorder in (True, False):
            want = tu.host_blobs(product, pb.baker, mips, cutoff, disable_zorder)
            src = tu.Source(hip, fmt, stride, offset, bits, pad_elems=n)
            tex = tu.create(product, pb.baker, tu.make_desc(fmt, stride, offset, [src.mip], cutoff, disable_zorder))
            try:
                tu.check_texture(product, pb.baker, tex, mips, cutoff, disable_zorder, want, tu.layout_id((fmt, stride, offset)) + " poisoned")
            finally:
                product.destroy_texture(pb.baker, tex)
                src.free()


# ---- bakes ----
class CountingProduct:
    """the product library as test_gpu_parity.both takes it; reads the baker's counters before `both` destroys the baker"""

    def __init__(self, product):
        self._p, self.seen = product, []

    def __getattr__(self, name):
        return getattr(self._p, name)

    def destroy_baker(self, baker):
        self.seen.append(self._p.poisoned_bytes(baker))
        return self._p.destroy_baker(baker)


_BAKES = {}


def bake_case(name):
    if not _BAKES:
        _BAKES.update(pc.bake_cases())
    return _BAKES[name]


def both_poisoned(product, oracle, case, word, extra_knobs=()):
    p = CountingProduct(product)
    r = both(p, oracle, case["mips"], case["uv"], case["ix"], case["level"], sat=case["sat"], levels=case["levels"],
             knobs=[(ot.KNOB_POISON, ot.poison(word))] + list(case["knobs"]) + list(extra_knobs), **{k: v for k, v in case["kw"].items() if k != "levels"})
    assert len(p.seen) == 1 and p.seen[0][1] > 0 and p.seen[0][0] > 0, p.seen          # the working set and the texture's blocks were filled
    return r


@POISONED
@pytest.mark.parametrize("name", [n for n in pc.BAKE_NAMES if n != "max-array-data-size"])
def test_bake_against_the_oracle(product, oracle, name, word):
    both_poisoned(product, oracle, bake_case(name), word)


def bake_on(lib, baker, case, run=None):
    """one bake of a case on an existing baker -> BakeResult"""
    t = lib.create_texture(baker, case["mips"], alpha_cutoff=0.5 if case["sat"] else -1.0)
    try:
        d = ot.make_desc(t, case["uv"], case["ix"], case["level"], levels=case["levels"], **{k: v for k, v in case["kw"].items() if k != "levels"})
        if case["max_array"] is not None:
            d.maxArrayDataSize = case["max_array"]
        return run(baker, d) if run else lib.bake(baker, d)
    finally:
        lib.destroy_texture(baker, t)


def oracle_result(oracle, case):
    b = oracle.create_baker()
    try:
        return bake_on(oracle, b, case)
    finally:
        oracle.destroy_baker(b)


@POISONED
def test_bake_under_a_size_budget(pb_plain, product, oracle, word):
    """maxArrayDataSize (test_gpu_parity.both has no way to set it: the same comparison, spelled out)"""
    pb = pb_plain
    case = bake_case("max-array-data-size")
    want = oracle_result(oracle, case)
    before = pb.counters()
    got = bake_on(product, pb.baker, case)
    assert got.same_as(want), got.diff(want)
    assert got.array_data.size <= case["max_array"] and pb.counters()[1] > before[1]


@POISONED
def test_every_bake_entry(pb_plain, product, oracle, hip, word):
    """one case through ommCpuBake, ommxBakeDevice, the streamed result in 3 ranges, the four-phase sharded API at world 2 and ommxBakerKnob_Devices = 2, all on
    ONE poisoned baker and each against the oracle; the working-set counter grows across every one of them"""
    pb = pb_plain
    case = pc.entry_case()
    want = oracle_result(oracle, case)
    uv, ix = case["uv"], case["ix"]

    def grown(run):
        before = pb.counters()[1]
        r = bake_on(product, pb.baker, case, run)
        assert pb.counters()[1] > before
        return r

    r = grown(None)
    assert r.same_as(want), r.diff(want)
    r = grown(lambda b, d: ot.bake_device(product, hip, b, d, uv, ix, case["levels"]))
    assert r.same_as(want), ("ommxBakeDevice", r.diff(want))
    product.set_knob(pb.baker, ot.KNOB_STREAM_CHUNKS, 3)
    r = grown(None)
    tm = bench.get_timings(product, pb.baker)
    product.set_knob(pb.baker, ot.KNOB_STREAM_CHUNKS, 0)
    assert r.same_as(want), ("streamed", r.diff(want))
    assert tm.streamChunks == 3 and tm.streamedBytes > 0, (tm.streamChunks, tm.streamedBytes)
    two = dict(case, kw=dict(case["kw"], fmt=ot.FMT_2STATE))          # (2-state items of 512 bytes: the other digest of a streamed range)
    want2 = oracle_result(oracle, two)
    product.set_knob(pb.baker, ot.KNOB_STREAM_CHUNKS, 3)
    r = bake_on(product, pb.baker, two)
    tm = bench.get_timings(product, pb.baker)
    product.set_knob(pb.baker, ot.KNOB_STREAM_CHUNKS, 0)
    assert r.same_as(want2), ("streamed, 2-state", r.diff(want2))
    assert tm.streamChunks == 3 and tm.streamedBytes > 0, (tm.streamChunks, tm.streamedBytes)
    ranks = grown(lambda b, d: ot.bake_sharded_simulated(product, hip, b, d, uv, ix, 2, case["levels"]))
    for k, r in enumerate(ranks):
        assert r.same_as(want), ("sharded, rank %d" % k, r.diff(want))
    product.set_knob(pb.baker, ot.KNOB_DEVICES, 2)
    r = grown(None)
    tm = bench.get_timings(product, pb.baker)
    product.set_knob(pb.baker, ot.KNOB_DEVICES, 0)
    assert r.same_as(want), ("two devices", r.diff(want))
    assert tm.devices == 2


@POISONED
def test_a_larger_bake_before_a_smaller_one(pb_plain, product, oracle, word):
    """the second bake's working set is the first one's memory, with the word on top"""
    pb = pb_plain
    for case in pc.back_to_back_cases():
        want = oracle_result(oracle, case)
        before = pb.counters()[1]
        got = bake_on(product, pb.baker, case)
        assert got.same_as(want), got.diff(want)
        assert pb.counters()[1] > before


# ---- the knob off ----
def test_knob_off_fills_nothing(product, oracle, dll, hip):
    """a derived entry, a texture and a bake with the knob off (never set; set and cleared again): both counters stay where they were"""
    b = product.create_baker()
    case = bake_case("linear")
    decoy, real = pc.derived_pair()
    src = sources(hip, real, ot.IDX_U16)
    want = oracle_result(oracle, case)
    try:
        cu.coarsen_and_check(dll, hip, b, src, 3)
        assert bake_on(product, b, case).same_as(want)
        assert product.poisoned_bytes(b) == (0, 0)
        product.set_knob(b, ot.KNOB_POISON, ot.poison(0xA5A5A5A5))
        cu.coarsen_and_check(dll, hip, b, src, 3)
        assert bake_on(product, b, case).same_as(want)
        on = product.poisoned_bytes(b)
        assert on[0] > 0 and on[1] > 0
        product.set_knob(b, ot.KNOB_POISON, 0)
        cu.coarsen_and_check(dll, hip, b, src, 3)
        assert bake_on(product, b, case).same_as(want)
        assert product.poisoned_bytes(b) == on
    finally:
        src.close()
        product.destroy_baker(b)
