"""The micromap consumer on the MI355X: ommxLookupOpacity (lookup_opacity kernel) and ommxResolveHits (resolve_hits kernel).

  agreement   device lookup == ommxLookupOpacityHost == a numpy decode of the host (ommCpuBake) result, byte for byte
  meaning     at points strictly inside micro-triangles whose state is known, the plain alpha test (IgnoreMicromap) gives that state
  resolution  known hits are answered from the OMM (texture untouched), unknown ones by the texture; overall == the plain alpha test
  bounds      malformed results, primitives past the index buffer or past the mesh, and arbitrary float barycentrics read what the host reads
              (OMMX_OPACITY_INVALID where the header says so), from arrays followed by valid-looking padding inside one allocation
  edges       vertices, edge midpoints and points an ulp off the cell diagonal read a micro-triangle whose closure holds them
  launches    counts around the block size and the grid stride, canaries around the output, a stream of the caller
  sampler     resolve_hits' own instantiation of the classifier's sampler: sizes that are not powers of two, mips, cut-offs, mappings, Border
              under Linear, 8- and 16-bit mesh indices, unaligned texture coordinates, against the numpy sampler of lookup_util"""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import workloads as wl
import lookup_util as lu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(product):
    return lu.bind(product.dll), ot.Hip()


def bake_both(product, hip, tex, uv, ix, levels=None, sat=True, **kw):
    """ommCpuBake and ommxBakeDevice of one desc; both results must be identical"""
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=kw.get("alpha_cutoff", 0.5) if sat else -1.0)
    d = ot.make_desc(t, uv, ix, kw.pop("level"), levels=levels, **kw)
    host = product.bake(b, d, want_stats=False)
    dev = lu.DeviceBake(product, hip, b, d, uv, ix, levels)
    assert host.same_as(dev.host), host.diff(dev.host)
    return b, t, d, host, dev


def release(product, b, t, dev):
    dev.close()
    product.destroy_texture(b, t)
    product.destroy_baker(b)


def query_points(rng, res, max_centroid_tris=3000, interior=200000, centroid_cap=1 << 20):
    """centroids of every micro-triangle of up to `max_centroid_tris` primitives (at most `centroid_cap` micro-triangles), plus random interior
    points of random micro-triangles of all primitives -> (prims, micro index, u, v)"""
    lv, has = lu.prim_levels(res)
    n = len(lv)
    prims, micro = [], []
    budget = centroid_cap
    for p in rng.permutation(n)[:max_centroid_tris]:
        k = 4 ** int(lv[p])
        if k > budget:
            continue
        budget -= k
        prims.append(np.full(k, p, np.int64))
        micro.append(np.arange(k, dtype=np.int64))
    pc, mc = np.concatenate(prims), np.concatenate(micro)
    cu, cv = lu.centroid_points(lu.micro_vertices(mc, lv[pc]))
    pr = rng.integers(0, n, interior)
    mr = (rng.random(interior) * (4.0 ** lv[pr])).astype(np.int64)
    ru, rv = lu.interior_points(rng, lu.micro_vertices(mr, lv[pr]))
    return np.concatenate([pc, pr]), np.concatenate([mc, mr]), np.concatenate([cu, ru]), np.concatenate([cv, rv])


def hits_of(prims, u, v):
    h = np.empty(len(prims), lu.HIT)
    h["prim"], h["u"], h["v"] = prims, u, v
    return h


def check_agreement(dll, hip, host_res, dev):
    rng = np.random.default_rng(11)
    prims, micro, u, v = query_points(rng, host_res)
    hits = hits_of(prims, u, v)
    expect = lu.numpy_states(host_res, prims, micro).astype(np.uint8)
    hdesc = lu.result_desc_over(lu.host_arrays_of(host_res), host_res.index_format)
    for flags in (0, lu.FORCE_2STATE):
        on_host = lu.lookup_host(dll, hdesc, hits, flags)
        on_dev = lu.lookup_device(dll, hip, dev.rdesc, hits, flags)
        want = expect if flags == 0 else np.where(expect >= 2, expect - 2, expect).astype(np.uint8)
        assert np.array_equal(on_host, want), np.nonzero(on_host != want)[0][:10]
        assert np.array_equal(on_dev, on_host), np.nonzero(on_dev != on_host)[0][:10]
    return len(hits)


AGREEMENT_CASES = {
    # per-triangle levels 0..12, 4-state, device tail, special indices on, 16-bit index output
    "levels0-12_4state": dict(fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS),
    "levels0-12_2state_nospecial_32bit": dict(fmt=ot.FMT_2STATE, flags=ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL | ot.FLAG_FORCE32),
    "levels0-12_4state_8bit": dict(fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS | ot.FLAG_ALLOW8),
    # the host tail (near-duplicate merging)
    "levels0-12_4state_hosttail": dict(fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS | ot.FLAG_NEAR_DUP),
    "levels0-12_2state_hosttail_budget": dict(fmt=ot.FMT_2STATE, flags=ot.FLAG_THREADS, budget=200000),
}


@pytest.mark.parametrize("case", sorted(AGREEMENT_CASES))
def test_lookup_agrees_with_host_decode(product, env, case):
    dll, hip = env
    kw = dict(AGREEMENT_CASES[case])
    budget = kw.pop("budget", None)
    n = 60 if "8bit" in case else 150
    tex = ot.foliage_texture(31, 512, 512, feature=24)
    uv, ix = ot.random_triangles(32, n, 12.0 / 512)
    uv[:3 * 4] = np.nan                                   # unresolved triangles (special index unresolvedTriState, or an OMM when specials are off)
    levels = (ot.hash_u32(np.arange(n) + 5) % 13).astype(np.uint8)
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    d = ot.make_desc(t, uv, ix, 12, levels=levels, addr=ot.WRAP, promo=ot.PROMO_NEAREST, **kw)
    if budget is not None:
        d.maxArrayDataSize = budget
    host = product.bake(b, d, want_stats=False)
    dev = lu.DeviceBake(product, hip, b, d, uv, ix, levels)
    try:
        assert host.same_as(dev.host), host.diff(dev.host)
        if "8bit" in case:
            assert host.index_format == ot.IDX_U8
        if "32bit" in case:
            assert host.index_format == ot.IDX_U32
        assert (host.index < 0).any() or "nospecial" in case
        check_agreement(dll, hip, host, dev)
    finally:
        release(product, b, t, dev)


@pytest.mark.parametrize("which", ["c1_full", "c2_slice"])
def test_lookup_agrees_on_benchmark_configurations(product, env, which):
    dll, hip = env
    if which == "c1_full":
        tex, uv, ix, lv, kw = wl.workload("c1")
    else:
        tex, uv, ix, lv, kw = wl.workload("c2")
        uv, ix, lv = wl.subset(uv, ix, lv, 0, 50000)
    b, t, d, host, dev = bake_both(product, hip, tex, uv, ix, lv, **kw)
    try:
        check_agreement(dll, hip, host, dev)
    finally:
        release(product, b, t, dev)


MEANING_CASES = [(addr, ot.LINEAR) for addr in (ot.WRAP, ot.MIRROR, ot.CLAMP, ot.MIRROR_ONCE)] + \
                [(addr, ot.NEAREST) for addr in (ot.WRAP, ot.MIRROR, ot.CLAMP, ot.BORDER, ot.MIRROR_ONCE)]


@pytest.mark.parametrize("texkind", ["foliage", "noise"])
@pytest.mark.parametrize("sat", [True, False])
@pytest.mark.parametrize("addr,filt", MEANING_CASES)
def test_known_states_mean_what_the_texture_says(product, env, texkind, sat, addr, filt):
    """4-state, Nearest promotion, no near-duplicate merging, no size budget.  At random points strictly inside micro-triangles whose state
    is known, the plain alpha test (IgnoreMicromap) must give that state; ommxResolveHits answers known hits from the OMM without the texture
    and unknown ones from the texture, and equals the plain alpha test everywhere.  Texture coordinates in all three formats, 12-byte stride."""
    dll, hip = env
    seed = 100 * addr + 10 * filt + (1 if sat else 0) + (5 if texkind == "noise" else 0)
    tex = ot.foliage_texture(seed, 1024, 1024, feature=48) if texkind == "foliage" else ot.value_noise(seed, 1024, 1024, octaves=4, base_cell=64)
    n = 3000
    uvf, ix = ot.random_triangles(seed, n, 16.0 / 1024, lo=-0.3, hi=1.3)
    uv_fmt = (ot.UV32_FLOAT, ot.UV16_FLOAT, ot.UV16_UNORM)[seed % 3]
    if uv_fmt == ot.UV16_UNORM:
        uvf = (uvf * np.float32(0.6) + np.float32(0.2)).astype(np.float32)   # into [0, 1] without clipping (clipped triangles would be degenerate)
    raw, uv_read = lu.uv_encoded(uvf, uv_fmt)
    levels = (3 + ot.hash_u32(np.arange(n) + seed) % 4).astype(np.uint8)
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5 if sat else -1.0)
    d = ot.make_desc(t, raw, ix, 6, levels=levels, addr=addr, filt=filt, promo=ot.PROMO_NEAREST, flags=ot.FLAG_THREADS, uv_format=uv_fmt,
                     border_alpha=0.75)
    d.texCoordStrideInBytes = 12
    dev = lu.DeviceBake(product, hip, b, d, raw, ix, levels)
    try:
        res = dev.host
        rng = np.random.default_rng(seed)
        lv, has = lu.prim_levels(res)
        m = 400000
        prims = rng.integers(0, n, m)
        micro = (rng.random(m) * (4.0 ** lv[prims])).astype(np.int64)
        u, v = lu.interior_points(rng, lu.micro_vertices(micro, lv[prims]))
        hits = hits_of(prims, u, v)
        state = lu.lookup_device(dll, hip, dev.rdesc, hits)
        assert np.array_equal(state, lu.numpy_states(res, prims, micro).astype(np.uint8))
        plain = lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits, lu.IGNORE_MICROMAP)
        assert ((plain & 8) != 0).all() and np.array_equal((plain >> 1) & 3, state)
        # the sampler: the kernel's alpha test == a numpy restatement of it, except within 1e-6 of the cut-off
        tu, tv = lu.hit_tex_coords(uv_read, ix, prims, u, v)
        alpha = lu.sample_alpha(tex, tu, tv, addr, filt, 0.75)
        near = np.abs(alpha.astype(np.float64) - 0.5) <= 1e-6
        assert np.array_equal((plain & 1)[~near], (alpha > np.float32(0.5))[~near].astype(np.uint8))
        known = state < 2
        # Finding: a zero-area triangle (the bake's degenerate rule, fp32 area < 1e-9; here half-float texture coordinates
        # collapse a few) gets no texel vote under the Nearest filter -- the conservative raster's strict inside test admits no texel -- so its
        # state says nothing about the texture.  The oracle does the same.  Those hits are set aside under Nearest only, and counted.
        q = uv_read[ix.reshape(-1, 3)].reshape(-1, 6)
        area = np.float32(0.5) * np.abs(q[:, 0] * (q[:, 3] - q[:, 5]) + q[:, 2] * (q[:, 5] - q[:, 1]) + q[:, 4] * (q[:, 1] - q[:, 3]))
        degenerate = (area.astype(np.float64) < 1e-9)[prims] if filt == ot.NEAREST else np.zeros(m, bool)
        checked = known & ~near & ~degenerate
        bad = checked & ((plain & 1) != state)
        print("%s sat=%d addr=%d filt=%d uv=%d: %d known hits checked, %d excluded (alpha within 1e-6 of the cut-off), %d on degenerate triangles "
              "(Nearest), %d unknown" % (texkind, sat, addr, filt, uv_fmt, int(checked.sum()), int((known & near).sum()), int((known & degenerate).sum()),
                                         int((~known).sum())))
        assert known.sum() > m // 4
        assert not bad.any(), "known state contradicted by the texture at %d points, e.g. hit %r state %d alpha %r" % (
            int(bad.sum()), hits[np.nonzero(bad)[0][0]], state[np.nonzero(bad)[0][0]], alpha[np.nonzero(bad)[0][0]])
        # resolution
        out = lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits)
        assert np.array_equal(out[known], (state | (state << 1))[known])
        assert np.array_equal(out[~known], plain[~known])
        same = ~(known & ~checked)   # every hit except the known ones set aside above
        assert np.array_equal((out & 1)[same], (plain & 1)[same])
        f2 = lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits, lu.FORCE_2STATE)
        s2 = np.where(state >= 2, state - 2, state).astype(np.uint8)
        assert np.array_equal(f2, s2 | (s2 << 1))
    finally:
        release(product, b, t, dev)


def test_resolve_refuses_what_the_bake_refuses(product, env):
    dll, hip = env
    tex = ot.foliage_texture(3, 256, 256, feature=16)
    uv, ix = ot.random_triangles(4, 50, 10.0 / 256)
    b, t, d, host, dev = bake_both(product, hip, tex, uv, ix, None, level=4, addr=ot.WRAP)
    b2 = product.create_baker()
    t2 = product.create_texture(b2, [tex], alpha_cutoff=0.5)
    try:
        hits = hits_of(np.arange(50), np.full(50, 0.2, np.float32), np.full(50, 0.3, np.float32))
        ok = lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits)
        assert (ok != lu.INVALID).all()
        import ctypes as C
        def call(desc, baker=b, flags=0):
            return dll.ommxResolveHits(baker, C.byref(desc), C.byref(dev.rdesc), None, 0, None, flags, None)
        bad = ot.BakeInputDesc.from_buffer_copy(dev.ddesc)
        bad.alphaCutoff = 0.25                               # differs from the texture's cut-off: INVALID_ARGUMENT, as ommxBakeDevice
        assert call(bad) == ot.INVALID_ARGUMENT
        bad = ot.BakeInputDesc.from_buffer_copy(dev.ddesc)
        bad.runtimeSamplerDesc.filter = 2                    # filter not set: FAILURE, as ommxBakeDevice
        assert call(bad) == ot.FAILURE
        other = ot.BakeInputDesc.from_buffer_copy(dev.ddesc)
        other.texture = t2                                   # a texture of another baker
        assert call(other) == ot.INVALID_ARGUMENT
        assert call(dev.ddesc, flags=4) == ot.INVALID_ARGUMENT
        assert call(dev.ddesc) == ot.SUCCESS                 # count == 0: nothing launched
    finally:
        product.destroy_texture(b2, t2)
        product.destroy_baker(b2)
        release(product, b, t, dev)


# ---- the bounds rule on the device ----
def resolve_expectation(state, out, flags):
    """what ommxResolveHits may answer for hits whose lookup answer is `state` (0..3 or INVALID), apart from the texture's verdict in bit 0"""
    valid = state != lu.INVALID
    assert (out[~valid] == lu.INVALID).all(), "an invalid hit was answered"
    s = state[valid].astype(np.uint8)
    o = out[valid]
    assert (o != lu.INVALID).all()
    if flags & lu.FORCE_2STATE:
        s = np.where(s >= 2, s - 2, s).astype(np.uint8)
    assert np.array_equal((o >> 1) & 3, s)
    sampled = np.ones(len(s), bool) if flags & lu.IGNORE_MICROMAP else s >= 2
    assert np.array_equal((o & 8) != 0, sampled)           # unknown hits (all hits under IgnoreMicromap) sampled the texture: bit 3
    assert np.array_equal((o & 1)[~sampled], s[~sampled])   # known hits: bit 0 is the state
    assert (o >> 4 == 0).all()


@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32])
def test_bounds_rule_on_the_device(product, env, index_format):
    """lookup_util.bounds_table through lookup_opacity and resolve_hits.  The three arrays lie in one device allocation, each followed by padding
    that looks valid (index entries 0, descs of a valid block, state bytes != 0), and every out-of-range value is near: a kernel without one
    of the checks would read the padding and answer a plausible state, not fault.  device == ommxLookupOpacityHost == the table."""
    dll, hip = env
    table = lu.bounds_table(index_format)
    buf, res, i_off, d_off, a_off = lu.bounds_arena(table)
    tex = ot.foliage_texture(3, 256, 256, feature=16)
    uv, ix = ot.random_triangles(4, 64, 10.0 / 256)
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    d = ot.make_desc(t, uv, ix, 4, addr=ot.WRAP)
    dev = lu.DeviceBake(product, hip, b, d, uv, ix)
    arena = hip.upload(buf)
    try:
        base = ot.BakeResultDesc.from_buffer_copy(res.desc)
        base.arrayData, base.indexBuffer = arena.value + a_off, arena.value + i_off
        base.descArray = C.cast(arena.value + d_off, C.POINTER(ot.MicromapDesc))
        seen = 0
        for name, fields, prims, expect, near in lu.bounds_variants(table):
            hits = lu.bounds_hits(prims)
            assert (prims[near].astype(np.int64) < 64).all()
            for flags in (0, lu.FORCE_2STATE):
                want = np.where((expect == 2) | (expect == 3), expect - 2, expect).astype(np.uint8) if flags else expect
                on_host = lu.lookup_host(dll, lu.with_fields(res.desc, **fields), hits, flags)
                assert np.array_equal(on_host, want), (name, flags, on_host, want)
                on_dev = lu.lookup_device(dll, hip, lu.with_fields(base, **fields), hits[near], flags)
                assert np.array_equal(on_dev, want[near]), (name, flags, on_dev, want[near])
            for flags in (0, lu.FORCE_2STATE, lu.IGNORE_MICROMAP):
                out = lu.resolve_device(dll, hip, b, dev.ddesc, lu.with_fields(base, **fields), hits[near], flags)
                resolve_expectation(expect[near], out, flags)
            seen += int(near.sum())
        assert seen >= 60
    finally:
        hip.free(arena)
        release(product, b, t, dev)


def test_resolve_primitive_beyond_the_mesh(product, env):
    """a desc whose mesh has fewer triangles than the result has index entries: hits on primitives >= the mesh's triangle count are answered
    from the OMM where it knows and read 0xFF where the texture would be needed.  Indices and texture coordinates lie in one allocation, the
    declared part followed by indices 0 and coordinates (0.5, 0.5): a kernel that fetched them anyway would answer from the texture."""
    dll, hip = env
    n, num = 60, 35
    tex = ot.foliage_texture(8, 512, 512, feature=24)
    uv, ix = ot.random_triangles(9, n, 16.0 / 512)
    levels = (3 + ot.hash_u32(np.arange(n) + 9) % 4).astype(np.uint8)
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    d = ot.make_desc(t, uv, ix, 6, levels=levels, addr=ot.WRAP, promo=ot.PROMO_NEAREST)
    dev = lu.DeviceBake(product, hip, b, d, uv, ix, levels)
    buf, i_off, t_off = lu.mesh_arena(uv, ix, num)
    arena = hip.upload(buf)
    try:
        short = ot.BakeInputDesc.from_buffer_copy(dev.ddesc)
        short.indexBuffer, short.texCoords, short.indexCount, short.texCoordStrideInBytes = arena.value + i_off, arena.value + t_off, 3 * num, 8
        assert dev.rdesc.indexCount == n
        rng = np.random.default_rng(9)
        lv, has = lu.prim_levels(dev.host)
        prims = rng.integers(0, n, 40000)
        micro = (rng.random(len(prims)) * (4.0 ** lv[prims])).astype(np.int64)
        u, v = lu.interior_points(rng, lu.micro_vertices(micro, lv[prims]))
        hits = hits_of(prims, u, v)
        state = lu.lookup_device(dll, hip, dev.rdesc, hits)
        assert np.array_equal(state, lu.numpy_states(dev.host, prims, micro).astype(np.uint8))
        beyond, known = prims >= num, state < 2
        assert (beyond & known).sum() > 100 and (beyond & ~known).sum() > 100       # both kinds of hit occur past the mesh
        for flags in (0, lu.IGNORE_MICROMAP, lu.FORCE_2STATE):
            whole = lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits, flags)
            out = lu.resolve_device(dll, hip, b, short, dev.rdesc, hits, flags)
            assert (whole != lu.INVALID).all()
            assert np.array_equal(out[~beyond], whole[~beyond])
            needs_texture = ~known if flags == 0 else (np.ones(len(hits), bool) if flags == lu.IGNORE_MICROMAP else np.zeros(len(hits), bool))
            assert (out[beyond & needs_texture] == lu.INVALID).all()
            assert np.array_equal(out[beyond & ~needs_texture], whole[beyond & ~needs_texture])
    finally:
        hip.free(arena)
        release(product, b, t, dev)


@pytest.mark.parametrize("level", [1, 4, 6, 9, 12])
def test_any_float_reads_on_the_device_what_it_reads_on_the_host(env, level):
    """random 32-bit patterns for u and v (NaN, infinities, denormals, huge values) against the digit result: device == host byte for byte,
    and the index the states spell is below 4^level"""
    dll, hip = env
    res = lu.digit_result(level)
    dr = lu.DeviceResult(hip, res.array, res.descs.view(np.uint8), res.index, ot.IDX_U32)
    try:
        rng = np.random.default_rng(50 + level)
        bits = rng.integers(0, 1 << 32, size=(2, 50000), dtype=np.uint64).astype(np.uint32)
        # random patterns hold NaNs and denormals but hardly ever an infinity (2 patterns of 2^32): the named values go in explicitly, every
        # one paired with every other in (u, v) -- the (Inf, -Inf) pair among them
        named = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA00000,      # +-Inf, quiet and signalling NaNs
                          0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF,                  # +-0, smallest and largest denormals
                          0x7F7FFFFF, 0xFF7FFFFF, 0x3F7FFFFF, 0x3F800000, 0x3F800001, 0x3F000000], np.uint32)   # +-FLT_MAX, 1.0 -/+ one ulp, 0.5
        k = len(named)
        bits[0, :k * k], bits[1, :k * k] = np.repeat(named, k), np.tile(named, k)
        u, v = bits[0].view(np.float32), bits[1].view(np.float32)
        for a in (u, v):
            assert np.isposinf(a).any() and np.isneginf(a).any() and np.isnan(a).any()
            assert ((a != 0) & (np.abs(a) < np.float32(1.1754944e-38))).any() and (np.abs(a) == np.float32(3.4028235e38)).any()
            assert (a[k * k:] != a[k * k:]).any()   # NaNs among the random patterns too
        assert (np.isposinf(u) & np.isneginf(v)).any() and (np.isneginf(u) & np.isposinf(v)).any()
        hits = lu.digit_hits(level, u, v)
        on_host = lu.lookup_host(dll, res.desc, hits)
        on_dev = lu.lookup_device(dll, hip, dr.rdesc, hits)
        assert np.array_equal(on_dev, on_host), np.nonzero(on_dev != on_host)[0][:10]
        assert (lu.digits_to_index(level, on_dev, len(u)) < 4 ** level).all()
    finally:
        dr.close()


# ---- edge and vertex hits ----
@pytest.mark.parametrize("level", range(13))
def test_edge_and_vertex_hits_on_the_device(env, level):
    """every vertex and edge midpoint (exact in fp32) of the micro-triangles of a level -- all of them, or 16 384 random ones -- and the points
    one ulp to either side of the cell diagonal: device == host, and the micro-triangle read is one whose closure, computed in float64 from
    the forward decode, holds the point (tests/native/lookup_check.cpp makes that check of the host code only)"""
    dll, hip = env
    rng = np.random.default_rng(40 + level)
    micro = lu.edge_level_sample(rng, level)
    u, v = lu.edge_and_vertex_points(micro, level)
    res = lu.digit_result(level)
    dr = lu.DeviceResult(hip, res.array, res.descs.view(np.uint8), res.index, ot.IDX_U32)
    try:
        hits = lu.digit_hits(level, u, v)
        on_host = lu.lookup_host(dll, res.desc, hits)
        on_dev = lu.lookup_device(dll, hip, dr.rdesc, hits)
        assert np.array_equal(on_dev, on_host), np.nonzero(on_dev != on_host)[0][:10]
        beyond = lu.check_index_is_a_holder(level, u, v, lu.digits_to_index(level, on_dev, len(u)))
        print("level %d: %d points, %d of them an ulp beyond the edge u + v = 1" % (level, len(u), beyond))
    finally:
        dr.close()


# ---- launch shapes ----
COUNTS = [1, 255, 256, 257, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 3 * (1 << 20) + 17]   # the block is 256 lanes, the grid stride 2^20


@pytest.fixture(scope="module")
def shapes_bake(product, env):
    dll, hip = env
    n = 150
    tex = ot.foliage_texture(31, 512, 512, feature=24)
    uv, ix = ot.random_triangles(32, n, 12.0 / 512)
    levels = (ot.hash_u32(np.arange(n) + 5) % 10).astype(np.uint8)
    b = product.create_baker()
    t = product.create_texture(b, [tex], alpha_cutoff=0.5)
    d = ot.make_desc(t, uv, ix, 12, levels=levels, addr=ot.WRAP, promo=ot.PROMO_NEAREST)
    dev = lu.DeviceBake(product, hip, b, d, uv, ix, levels)
    yield b, dev, n
    release(product, b, t, dev)


def check_launch_shape(dll, hip, shapes_bake, count, stream):
    b, dev, n = shapes_bake
    rng = np.random.default_rng(count)
    hits = hits_of(rng.integers(0, n + 2, count), rng.random(count, np.float32), rng.random(count, np.float32))   # two primitives past the index buffer
    want = lu.lookup_host(dll, dev.hdesc, hits)
    got = lu.guarded_call(hip, hits, lambda h, o, k, s: dll.ommxLookupOpacity(C.byref(dev.rdesc), h, k, o, 0, s), stream)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    got = lu.guarded_call(hip, hits, lambda h, o, k, s: dll.ommxResolveHits(b, C.byref(dev.ddesc), C.byref(dev.rdesc), h, k, o, 0, s), stream)
    piece = 1 << 19   # pieces <= 2^20: every piece is a launch without a second trip of the grid stride
    parts = np.concatenate([lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits[lo:lo + piece]) for lo in range(0, count, piece)])
    assert np.array_equal(got, parts), np.nonzero(got != parts)[0][:10]
    resolve_expectation(want, got, 0)
    if count >= 1 << 20:
        assert (want == lu.INVALID).any() and (want < 2).any() and (want >= 2).any()


@pytest.mark.parametrize("count", COUNTS)
def test_launch_shapes(env, shapes_bake, count):
    """both kernels at counts around the block size and the grid stride: every answer equals the host decode (lookup) or a run of the same
    hits in pieces (resolve), and the bytes before and after out[0, count) keep their canary value"""
    dll, hip = env
    check_launch_shape(dll, hip, shapes_bake, count, None)


def test_launch_on_a_stream_of_the_caller(env, shapes_bake):
    """the same counts on a stream the test creates.  The stream is non-blocking, so it does not order against the null stream the test's
    copies use, and only that stream is synchronised before the answers are read: a launch that ignored the stream argument would be unordered"""
    dll, hip = env
    stream = hip.stream_create(non_blocking=True)
    try:
        for count in COUNTS:
            check_launch_shape(dll, hip, shapes_bake, count, stream)
    finally:
        hip.stream_destroy(stream)


# ---- the sampler paths of resolve_hits ----
@pytest.mark.parametrize("name", lu.sampler_case_names())
def test_resolve_sampler_paths(product, env, name):
    """The plain alpha test (IgnoreMicromap) and the resolution assertions of test_known_states_mean_what_the_texture_says over the cases of
    lookup_util.sampler_case: Linear x Border on either side of the cut-off, textures that are not square or not powers of two under all five
    address modes and both filters (triangle centres in [-1.3, 2.3): mirror flips and several wraps), a mip chain whose lower mips are
    inverted, cut-offs 0.3 and 0.7, the four other LessEqual / Greater mappings, 16- and 8-bit mesh indices with shared vertices, and
    UV32_FLOAT texture coordinates at a base and a stride that are not multiples of 4.  The reference is lookup_util.sample_alpha: the
    kernel's fp32 texel coordinate and weights, a float64 blend.  Hits with |alpha - cutoff| <= 1e-6 are not compared; at most 0.1 % of a
    case's hits may be such (a condition on the cases, checked without a GPU in tests/test_lookup.py)."""
    dll, hip = env
    c = lu.sampler_case(name)
    alpha, near = lu.reference_alpha(c)
    assert near.sum() <= lu.BAND_CAP * len(near), int(near.sum())
    le, gt, m = c["le"], c["gt"], c["m"]
    b = product.create_baker()
    t = product.create_texture(b, c["mips"], alpha_cutoff=c["cutoff"])
    d = ot.make_desc(t, c["raw"], c["ix"], 6, levels=c["levels"], addr=c["addr"], filt=c["filt"], promo=ot.PROMO_NEAREST, flags=ot.FLAG_THREADS,
                     uv_format=c["uv_format"], border_alpha=c["border"], alpha_cutoff=c["cutoff"], le=le, gt=gt)
    d.texCoordStrideInBytes = c["stride"]
    dev = lu.DeviceBake(product, hip, b, d, c["raw"], c["ix"], c["levels"], uv_offset=c["uv_offset"])
    try:
        res = dev.host
        lv, has = lu.prim_levels(res)
        assert np.array_equal(lv[has], c["levels"][has])       # the hits were made for these levels
        prims, micro = c["prims"], c["micro"]
        hits = hits_of(prims, c["u"], c["v"])
        state = lu.lookup_device(dll, hip, dev.rdesc, hits)
        assert np.array_equal(state, lu.numpy_states(res, prims, micro).astype(np.uint8))
        plain = lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits, lu.IGNORE_MICROMAP)
        assert ((plain & 8) != 0).all() and np.array_equal((plain >> 1) & 3, state)
        # the sampler: bit 0 follows the mapped state of the numpy alpha test, st & 1
        st = np.where(alpha > np.float64(np.float32(c["cutoff"])), gt, le)
        wrong = ~near & ((plain & 1) != (st & 1))
        assert not wrong.any(), "%d hits answered against the reference, e.g. hit %r alpha %r" % (int(wrong.sum()), hits[wrong][0], alpha[wrong][0])
        known = state < 2
        q = c["uv_read"][c["ix"].reshape(-1, 3)].reshape(-1, 6)
        area = np.float32(0.5) * np.abs(q[:, 0] * (q[:, 3] - q[:, 5]) + q[:, 2] * (q[:, 5] - q[:, 1]) + q[:, 4] * (q[:, 1] - q[:, 3]))
        degenerate = (area.astype(np.float64) < 1e-9)[prims] if c["filt"] == ot.NEAREST else np.zeros(m, bool)   # 
        checked = known & ~near & ~degenerate
        bad = checked & ((plain & 1) != state)
        print("%s: %d known hits checked, %d of %d hits in the band, %d on degenerate triangles (Nearest), %d unknown; %d of %d triangles were "
              "slivers and re-drawn" % (name, int(checked.sum()), int(near.sum()), m, int((known & degenerate).sum()), int((~known).sum()),
                                        c["slivers"], c["ntris"]))
        if le < 2 and gt < 2 and c["kind"] != "mips":
            assert known.sum() > m // 4
        elif le >= 2 and gt >= 2:
            assert not known.any()                              # both answers of the cut-off are Unknown*: the OMM knows nothing
        elif c["kind"] != "mips":
            assert known.sum() > m // 16 and (state[known] == (le if le < 2 else gt)).all()
        assert not bad.any(), "known state contradicted by the texture at %d points, e.g. hit %r state %d alpha %r" % (
            int(bad.sum()), hits[np.nonzero(bad)[0][0]], state[np.nonzero(bad)[0][0]], alpha[np.nonzero(bad)[0][0]])
        # resolution
        out = lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits)
        assert np.array_equal(out[known], (state | (state << 1))[known])
        assert np.array_equal(out[~known], plain[~known])
        same = ~(known & ~checked)
        assert np.array_equal((out & 1)[same], (plain & 1)[same])
        f2 = lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits, lu.FORCE_2STATE)
        s2 = np.where(state >= 2, state - 2, state).astype(np.uint8)
        assert np.array_equal(f2, s2 | (s2 << 1))
    finally:
        release(product, b, t, dev)


def test_uploaded_host_result_answers_like_the_device_result(product, env):
    """the documented use of include/omm_mi355x_ext.h: device copies of an ommCpuBake result in a desc the caller fills give, through both
    kernels, the bytes the desc of ommxGetDeviceBakeResultDesc gives"""
    dll, hip = env
    n = 150
    tex = ot.foliage_texture(31, 512, 512, feature=24)
    uv, ix = ot.random_triangles(32, n, 12.0 / 512)
    levels = (ot.hash_u32(np.arange(n) + 5) % 13).astype(np.uint8)
    b, t, d, host, dev = bake_both(product, hip, tex, uv, ix, levels, level=12, addr=ot.WRAP, promo=ot.PROMO_NEAREST)
    up = lu.DeviceResult(hip, *lu.host_arrays_of(host), host.index_format)
    try:
        assert up.rdesc.arrayData != dev.rdesc.arrayData and up.rdesc.indexCount == dev.rdesc.indexCount == n
        prims, micro, u, v = query_points(np.random.default_rng(12), host)
        hits = hits_of(prims, u, v)
        expect = lu.numpy_states(host, prims, micro).astype(np.uint8)
        assert (expect >= 2).any() and (expect < 2).any()
        for flags in (0, lu.FORCE_2STATE):
            mine = lu.lookup_device(dll, hip, up.rdesc, hits, flags)
            assert np.array_equal(mine, lu.lookup_device(dll, hip, dev.rdesc, hits, flags))
            assert np.array_equal(mine, expect if flags == 0 else np.where(expect >= 2, expect - 2, expect))
        for flags in (0, lu.FORCE_2STATE, lu.IGNORE_MICROMAP):
            mine = lu.resolve_device(dll, hip, b, dev.ddesc, up.rdesc, hits, flags)
            assert np.array_equal(mine, lu.resolve_device(dll, hip, b, dev.ddesc, dev.rdesc, hits, flags))
            resolve_expectation(expect, mine, flags)
    finally:
        up.close()
        release(product, b, t, dev)
