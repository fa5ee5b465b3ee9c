"""ommxDebugGetStatsDevice / ommxDebugGetStatsDevice2 / ommxGetDeviceBakeResultTriangleAreas on the GPU: the hand-built table of the bounds rule with
canaries around every output, the host's 32-bit products, real bakes against ommCpuBake + ommDebugGetStats2, determinism and the argument checks."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    return su.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


class Image:
    """One device allocation that holds every array of a call, inputs and outputs, each at the alignment its C type asks for and no more, the gaps and
    the outputs pre-filled with random bytes (padding that reads like data).  After the call every byte outside the outputs must be what it was."""

    def __init__(self, hip, seed=3):
        self.hip, self.parts, self.size, self.rng = hip, {}, 0, np.random.default_rng(seed)

    def add(self, name, nbytes, align, misalign, data=None, output=False):
        """place `nbytes` at an address that is `misalign` modulo 2 * align (aligned for the type, not for anything wider), 24 - 39 bytes behind the last part"""
        at = self.size + 24
        at += (misalign - at) % (2 * align)
        self.parts[name] = (at, nbytes, data, output)
        self.size = at + nbytes

    def upload(self):
        self.size += 40
        self.before = self.rng.integers(0, 256, self.size, dtype=np.uint8)
        for at, n, data, _ in self.parts.values():
            if data is not None:
                self.before[at:at + n] = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.base = self.hip.upload(self.before)
        assert self.base.value % 256 == 0
        return self

    def ptr(self, name):
        return C.c_void_p(self.base.value + self.parts[name][0])

    def download(self):
        self.after = self.hip.download(self.base, self.size)
        return self

    def out(self, name, dtype):
        at, n, _, _ = self.parts[name]
        return self.after[at:at + n].copy().view(dtype)

    def assert_only_outputs_changed(self, written=None):
        keep = np.ones(self.size, bool)
        for name, (at, n, _, output) in self.parts.items():
            if output and (written is None or name in written):
                keep[at:at + n] = False
        bad = np.nonzero((self.before != self.after) & keep)[0]
        assert bad.size == 0, "bytes outside the outputs changed, first at %d of %d" % (bad[0], self.size)

    def free(self):
        self.hip.free(self.base)


def table_image(hip, index_format, array_data, descs, index, areas):
    D, T = len(descs), len(index)
    raw = np.zeros(D, dtype=[("o", "<u4"), ("l", "<u2"), ("f", "<u2")])
    raw["o"], raw["l"], raw["f"] = descs[:, 0], descs[:, 1], descs[:, 2]
    idx = index.astype(su.INDEX_DTYPE[index_format])
    im = Image(hip)
    im.add("array", array_data.size, 1, 1, array_data)
    im.add("descs", 8 * D, 4, 4, raw)
    im.add("index", idx.nbytes, idx.itemsize, idx.itemsize, idx)
    im.add("areas", 4 * T, 4, 4, areas)
    im.add("stateCounts", 16 * D, 4, 4, output=True)
    im.add("referenceCounts", 4 * D, 4, 4, output=True)
    im.add("knownFraction", 4 * T, 4, 4, output=True)
    im.upload()
    rd = ot.BakeResultDesc()
    rd.arrayData, rd.arrayDataSize = im.ptr("array"), array_data.size
    rd.descArray, rd.descArrayCount = C.cast(im.ptr("descs"), C.POINTER(ot.MicromapDesc)), D
    rd.indexBuffer, rd.indexCount, rd.indexFormat = im.ptr("index"), T, index_format
    return im, rd, idx


def outputs_of(im, names=("stateCounts", "referenceCounts", "knownFraction")):
    o = su.DeviceStatsOutputs()
    for n in names:
        setattr(o, n, im.ptr(n))
    return o


def table_and_check(dll, hip, baker, index_format, array_data, descs, index, areas, stream=None):
    """one call with every output on hand-built arrays in an Image, against stats_util.reference_stats: the eight integers, the skipped count, the three
    arrays byte for byte, the metric within an ulp, and nothing written outside the outputs -> the reference's answer"""
    ref = su.reference_stats(array_data, descs, index, areas)
    im, rd, _ = table_image(hip, index_format, array_data, descs, index, areas)
    try:
        st, skipped = ot.DebugStats(), C.c_uint32(12345)
        o = outputs_of(im)
        assert dll.ommxDebugGetStatsDevice(baker, C.byref(rd), im.ptr("areas"), C.byref(o), C.byref(st), C.byref(skipped), stream) == ot.SUCCESS
        im.download()
        got = su.int_fields(st)
        print("fields", got, "skipped", skipped.value, "metric %r (reference %r)" % (st.knownAreaMetric, float(ref["metric"])))
        assert got == ref["fields"]
        assert skipped.value == ref["skipped"]
        assert np.array_equal(im.out("stateCounts", np.uint32).reshape(-1, 4), ref["state_counts"])
        assert np.array_equal(im.out("referenceCounts", np.uint32), ref["refs"])
        assert np.array_equal(im.out("knownFraction", np.uint32), ref["known_fraction"].view(np.uint32))   # bit for bit: one IEEE division
        assert su.ulp_distance(st.knownAreaMetric, ref["metric"]) <= 1
        im.assert_only_outputs_changed()
    finally:
        im.free()
    return ref


@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32])
def test_hand_built_table(dll, hip, baker, index_format):
    """well-formed blocks of levels 0 - 3 in both formats at odd offsets, a level-7 block across byte 16384 of the array, a level-9 block of several
    segments; descriptors that fail the bounds rule (level 13, formats 0 and 3, a block ending one byte past arrayDataSize), which get zero counts and
    whose primitives are skipped; the four specials, -5 and descArrayCount; blocks referenced 0, 1 and 3 times"""
    array_data, descs, index, areas = su.table_arrays()
    ref = table_and_check(dll, hip, baker, index_format, array_data, descs, index, areas)
    assert ref["skipped"] == 8 and ref["refs"][0] == 3 and ref["refs"][8] == 1 and ref["refs"][7] == 0 and not ref["state_counts"][su.TABLE_WELL_FORMED:].any()


@pytest.mark.parametrize("references", [300, 600])
def test_32_bit_products(dll, hip, baker, references):
    """One level-12 2-state block (2 MiB) of random bytes, every primitive selects it: the totals are the host's (uint32_t)(references * count), wrapped.
    With 300 references both products (about 2.5e9) still fit 32 bits, so wrapped and exact coincide; the 600-reference case is there so that they differ."""
    rng = np.random.default_rng(references)
    array_data = rng.integers(0, 256, su.block_bytes(12, 1), dtype=np.uint8)
    counts = su.block_counts(array_data, 0, 12, 1)
    descs = np.array([(0, 12, 1)], np.int64)
    index = np.zeros(references, np.int64)
    im, rd, _ = table_image(hip, ot.IDX_U16, array_data, descs, index, np.ones(references, np.float32))
    try:
        st = ot.DebugStats()
        assert dll.ommxDebugGetStatsDevice(baker, C.byref(rd), None, None, C.byref(st), None, None) == ot.SUCCESS
        wrapped = [(references * int(c)) & 0xFFFFFFFF for c in counts]
        exact = [references * int(c) for c in counts]
        print("counts", counts.tolist(), "wrapped", wrapped, "exact", exact, "got", su.int_fields(st))
        assert (st.totalTransparent, st.totalOpaque, st.totalUnknownTransparent, st.totalUnknownOpaque) == tuple(wrapped)
        assert su.int_fields(st)[4:] == (0, 0, 0, 0) and st.knownAreaMetric == 0.0
        if references == 600:
            assert wrapped[:2] != exact[:2]
        im.download().assert_only_outputs_changed(written=())
    finally:
        im.free()


# ---- real bakes ----
BAKE_TRIS = 2000


@pytest.fixture(scope="module")
def bake_inputs():
    tex = ot.foliage_texture(7, 512, 512)
    uv, ix = ot.random_triangles(21, BAKE_TRIS, 0.08)
    uv = uv.reshape(BAKE_TRIS, 3, 2).copy()
    levels = (np.arange(BAKE_TRIS) * 7 % 13 % 7).astype(np.uint8)   # 0..6
    for t in range(7, BAKE_TRIS, 8):            # every eighth triangle repeats an earlier one, level included: blocks with several references
        uv[t], levels[t] = uv[(t // 2) | 1], levels[(t // 2) | 1]
    return tex, uv.reshape(-1, 2), ix, levels


@pytest.mark.parametrize("sat", [True, False], ids=["sat", "nosat"])
@pytest.mark.parametrize("fmt", [ot.FMT_2STATE, ot.FMT_4STATE], ids=["2state", "4state"])
def test_real_bake_against_the_host_path(product, dll, hip, bake_inputs, fmt, sat):
    """2000 random triangles on a 512^2 foliage texture, levels 0 - 6 per triangle: ommCpuBake + ommDebugGetStats2 against ommxBakeDevice +
    ommxDebugGetStatsDevice2.  A: all integer fields equal.  B: knownAreaMetric within 4 * (T + 4) * 2^-24 (tests/test_stats_reference.py).  C: the device
    metric is the float64 value of the downloaded arrays and areas to one fp32 ulp.  D: the areas the device result hands out are the host result's,
    bit for bit -- the host result does not hand its areas out, so they are restated from the input UVs in the fp32 operations of the bake's
    setup, and the host's metric (B) depends on them.  E: the same bake with EnableNearDuplicateDetection has areas too."""
    tex, uv, ix, levels = bake_inputs
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5 if sat else -1.0)
    try:
        for flags in (ot.FLAG_THREADS, ot.FLAG_THREADS | ot.FLAG_NEAR_DUP):
            d = ot.make_desc(t, uv, ix, 6, fmt=fmt, levels=levels, flags=flags, promo=ot.PROMO_NEAREST)
            host = product.bake(b, d)
            bake = lu.DeviceBake(product, hip, b, d, uv, ix, levels)
            try:
                st = ot.DebugStats()
                assert dll.ommxDebugGetStatsDevice2(b, bake.out, C.byref(st)) == ot.SUCCESS
                p_areas = C.c_void_p()
                assert dll.ommxGetDeviceBakeResultTriangleAreas(bake.out, C.byref(p_areas)) == ot.SUCCESS and p_areas.value
                areas = hip.download(p_areas, 4 * BAKE_TRIS, np.float32)
                # D
                p = uv.reshape(BAKE_TRIS, 6).astype(np.float32)
                v0x, v0y, v1x, v1y = p[:, 4] - p[:, 0], p[:, 5] - p[:, 1], p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
                nz = v0x * v1y - v1x * v0y
                want_areas = np.float32(0.5) * np.sqrt(nz * nz)
                assert np.array_equal(areas.view(np.uint32), want_areas.view(np.uint32))
                if flags & ot.FLAG_NEAR_DUP:
                    assert su.int_fields(st) == su.int_fields(host.stats2)     # E (the merged result's statistics agree as well)
                    continue
                assert host.same_as(bake.host), host.diff(bake.host)
                h = host.stats2
                bound = su.host_metric_bound(BAKE_TRIS)
                ref = su.reference_stats(bake.host.array_data, bake.host.descs, bake.host.index, areas)
                print("host", su.int_fields(h), h.knownAreaMetric, "device", su.int_fields(st), st.knownAreaMetric, "float64", float(ref["metric"]),
                      "|host - device| %.3g, bound %.3g" % (abs(h.knownAreaMetric - st.knownAreaMetric), bound), "blocks", len(bake.host.descs),
                      "most references", int(ref["refs"].max()))
                assert ref["refs"].max() > 1 and ref["skipped"] == 0
                assert su.int_fields(st) == su.int_fields(h) == ref["fields"]                      # A
                assert abs(st.knownAreaMetric - h.knownAreaMetric) <= bound                        # B
                assert su.ulp_distance(st.knownAreaMetric, ref["metric"]) <= 1                     # C
            finally:
                bake.close()
    finally:
        product.destroy_texture(b, t)
        product.destroy_baker(b)


# ---- determinism and plumbing ----
def test_determinism_stream_and_optional_arguments(dll, hip, baker):
    array_data, descs, index, areas = su.table_arrays(seed=9)
    ref = su.reference_stats(array_data, descs, index, areas)
    im, rd, _ = table_image(hip, ot.IDX_U32, array_data, descs, index, areas)
    stream = hip.stream_create(non_blocking=True)
    try:
        def call(areas_ptr, outputs, st, skipped=None, s=None):
            return dll.ommxDebugGetStatsDevice(baker, C.byref(rd), areas_ptr, outputs, C.byref(st), skipped, s)
        # two calls, identical bytes: the struct and every output
        a, b2 = ot.DebugStats(), ot.DebugStats()
        o = outputs_of(im)
        assert call(im.ptr("areas"), C.byref(o), a) == ot.SUCCESS
        first = im.download().after.copy()
        assert call(im.ptr("areas"), C.byref(o), b2) == ot.SUCCESS
        assert bytes(a) == bytes(b2) and np.array_equal(first, im.download().after)
        assert su.int_fields(a) == ref["fields"] and su.ulp_distance(a.knownAreaMetric, ref["metric"]) <= 1
        # a stream of the caller (non-blocking: not ordered against the null stream); the call synchronises it
        c, skipped = ot.DebugStats(), C.c_uint32()
        assert call(im.ptr("areas"), C.byref(o), c, C.byref(skipped), stream) == ot.SUCCESS
        assert bytes(c) == bytes(a) and skipped.value == ref["skipped"] and np.array_equal(first, im.download().after)
        # NULL outputs, NULL members, NULL areas
        e = ot.DebugStats()
        assert call(None, None, e) == ot.SUCCESS
        assert su.int_fields(e) == ref["fields"] and e.knownAreaMetric == 0.0
        only = su.DeviceStatsOutputs()
        only.knownFraction = im.ptr("knownFraction")
        f = ot.DebugStats()
        assert call(im.ptr("areas"), C.byref(only), f) == ot.SUCCESS and bytes(f) == bytes(a)
        assert np.array_equal(first, im.download().after)
        # zero areas: the host's 0 / 0
        zeros = hip.upload(np.zeros(len(index), np.float32))
        g = ot.DebugStats()
        assert call(zeros, None, g) == ot.SUCCESS
        hip.free(zeros)
        assert np.isnan(g.knownAreaMetric) and su.int_fields(g) == ref["fields"]
        # indexCount == 0: success, nothing launched, nothing written
        rd0 = ot.BakeResultDesc.from_buffer_copy(rd)
        rd0.indexCount = 0
        z, skipped = ot.DebugStats(), C.c_uint32(7)
        z.totalOpaque = 99
        assert dll.ommxDebugGetStatsDevice(baker, C.byref(rd0), None, C.byref(o), C.byref(z), C.byref(skipped), None) == ot.SUCCESS
        assert su.int_fields(z) == (0,) * 8 and z.knownAreaMetric == 0.0 and skipped.value == 0
        assert np.array_equal(first, im.download().after)
        # argument checks
        bad = ot.BakeResultDesc.from_buffer_copy(rd)
        bad.indexFormat = 3
        x = ot.DebugStats()
        assert dll.ommxDebugGetStatsDevice(baker, C.byref(bad), None, None, C.byref(x), None, None) == ot.INVALID_ARGUMENT
        assert dll.ommxDebugGetStatsDevice(None, C.byref(rd), None, None, C.byref(x), None, None) == ot.INVALID_ARGUMENT
        assert dll.ommxDebugGetStatsDevice(baker, None, None, None, C.byref(x), None, None) == ot.INVALID_ARGUMENT
        assert dll.ommxDebugGetStatsDevice(baker, C.byref(rd), None, None, None, None, None) == ot.INVALID_ARGUMENT
        assert dll.ommxDebugGetStatsDevice2(baker, None, C.byref(x)) == ot.INVALID_ARGUMENT
        assert dll.ommxGetDeviceBakeResultTriangleAreas(None, C.byref(C.c_void_p())) == ot.INVALID_ARGUMENT
        im.assert_only_outputs_changed()
    finally:
        hip.stream_destroy(stream)
        im.free()


def test_device_copy_of_a_host_bake_and_a_sharded_result(product, dll, hip):
    """a desc the caller filled with device copies of an ommCpuBake result is accepted and answers like the host; a result of the sharded entry points
    carries no areas: the accessor yields NULL and ommxDebugGetStatsDevice2 answers with the integer fields and metric 0"""
    tex = ot.kat_texture("circle", 256, 256)
    uv, ix = ot.random_triangles(3, 64, 0.2)
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    try:
        d = ot.make_desc(t, uv, ix, 5, promo=ot.PROMO_FORCE_OPAQUE, addr=ot.WRAP)
        host = product.bake(b, d)
        arrays = lu.host_arrays_of(host)
        dev = [hip.upload(a) for a in arrays]
        rd = ot.BakeResultDesc()
        rd.arrayData, rd.arrayDataSize = dev[0], host.array_data.size
        rd.descArray, rd.descArrayCount = C.cast(dev[1], C.POINTER(ot.MicromapDesc)), len(host.descs)
        rd.indexBuffer, rd.indexCount, rd.indexFormat = dev[2], host.index.size, host.index_format
        st = ot.DebugStats()
        assert dll.ommxDebugGetStatsDevice(b, C.byref(rd), None, None, C.byref(st), None, None) == ot.SUCCESS
        assert su.int_fields(st) == su.int_fields(host.stats) and sum(su.int_fields(st)) > 0
        for p in dev:
            hip.free(p)
        # one rank of a "sharded" bake of world size 1 through the four-call interface
        import omm_amd.sharded as sh
        sdll = sh.bind(product.dll)
        d_uv, d_ix = hip.upload(uv), hip.upload(ix)
        dd = ot.BakeInputDesc.from_buffer_copy(d)
        dd.texCoords, dd.indexBuffer = d_uv, d_ix
        h = C.c_void_p()
        assert sdll.ommxShardedBegin(b, C.byref(dd), 0, 1, C.byref(h)) == ot.SUCCESS
        w, n = C.c_void_p(), C.c_uint64()
        assert sdll.ommxShardedGetMeta(h, C.byref(w), C.byref(n)) == ot.SUCCESS
        c, nb, stride = C.c_void_p(), C.c_uint64(), C.c_uint64()
        assert sdll.ommxShardedTail(h, C.byref(c), C.byref(nb), C.byref(stride)) == ot.SUCCESS
        gathered = hip.alloc(max(stride.value, 16))    # the "all-gather" of one rank
        hip.copy_dtod(gathered, c, stride.value)
        out = C.c_void_p()
        assert sdll.ommxShardedFinish(h, gathered, C.byref(out)) == ot.SUCCESS
        p_areas = C.c_void_p(1)
        assert dll.ommxGetDeviceBakeResultTriangleAreas(out, C.byref(p_areas)) == ot.SUCCESS and not p_areas.value
        s2 = ot.DebugStats()
        assert dll.ommxDebugGetStatsDevice2(b, out, C.byref(s2)) == ot.SUCCESS
        assert su.int_fields(s2) == su.int_fields(host.stats) and s2.knownAreaMetric == 0.0
        assert product.dll.ommxDestroyDeviceBakeResult(out) == ot.SUCCESS
        assert sdll.ommxShardedDestroy(h) == ot.SUCCESS
        for p in (d_uv, d_ix, gathered):
            hip.free(p)
    finally:
        product.destroy_texture(b, t)
        product.destroy_baker(b)
