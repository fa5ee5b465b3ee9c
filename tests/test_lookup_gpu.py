"""The micromap consumer on the MI355X: ommxLookupOpacity (lookup_opacity kernel) and ommxResolveHits (resolve_hits kernel).

  agreement   device lookup == ommxLookupOpacityHost == a numpy decode of the host (ommCpuBake) result, byte for byte
  meaning     at points strictly inside micro-triangles whose state is known, the plain alpha test (IgnoreMicromap) gives that state
  resolution  known hits are answered from the OMM (texture untouched), unknown ones by the texture; overall == the plain alpha test
Only valid results and in-range primitives reach the GPU here; out-of-range handling is proved on the host (tests/test_lookup.py)."""
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


def uv_encoded(uv, fmt):
    """texture coordinates in `fmt` with a 12-byte stride, and the float32 values the bake reads back"""
    n = len(uv)
    raw = np.zeros((n, 12), np.uint8)
    if fmt == ot.UV32_FLOAT:
        raw[:, :8] = np.ascontiguousarray(uv, np.float32).view(np.uint8).reshape(n, 8)
        return raw, uv.astype(np.float32)
    if fmt == ot.UV16_UNORM:
        q = np.clip(np.round(uv * 65535.0), 0, 65535).astype(np.uint16)
        raw[:, :4] = q.view(np.uint8).reshape(n, 4)
        return raw, (q.astype(np.float32) * np.float32(1.5259021896696421759314870504694e-5)).astype(np.float32)
    q = uv.astype(np.float16)
    raw[:, :4] = q.view(np.uint8).reshape(n, 4)
    return raw, q.astype(np.float32)


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
    raw, uv_read = uv_encoded(uvf, uv_fmt)
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
