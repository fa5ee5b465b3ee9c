"""The tail of a bake -- PromoteToSpecialIndices, DeduplicateExact, MicromapSpatialSort and Serialize (bake_cpu_impl.cpp:1432-1472, 1031-1066, 1707-1754,
1756-1920) -- at its digest, sort-key and placement edges: a numpy restatement of the stage and the case builders of tests/test_tail_reference.py
(oracle + numpy, no GPU) and tests/test_tail_gpu.py (HIP library vs oracle, and the library's result against the restatement).

The restatement starts from the per-work-item states of a bake, decoded from the oracle's result for the same input with special indices and duplicate
detection disabled and 32-bit indices forced (every triangle then keeps its own block, found through the index buffer), and produces everything the
caller sees: special indices, digests, representatives, the descriptor order, offsets, arrayData, the index buffer in its format and both histograms.
Floats are float32 with one rounding per operation, conversions as x86 cvttss2si does them (setup_cases.cvt_i32).  Four deliberately wrong variants of
the sort key show that the case families can notice a subtly wrong kernel:
  recip    the centroid as sum * float32(1 / 3)
  reorder  the sum as p0 + (p1 + p2)
  fused    the cell from float64: (p0 + p1 + p2) / 3 * 8192 in double, rounded to float32 once
  sat      a saturating float -> int conversion in place of the integer indefinite (INT_MIN)

A case is a dict: name, tex (2-D array), uv ((3 T, 2) float32, unshared vertices), gmax, levels (per triangle or None), fmt, flags, filt, addr, promo,
rejection, le, gt (the states of alpha <= cutoff and alpha > cutoff)."""
import atexit
import functools
from collections import Counter
import numpy as np
import xxhash
import ommtest as ot
import setup_cases as sc
import lookup_util as lu

F = np.float32
RAW_FLAGS = ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL | ot.FLAG_NO_DEDUP | ot.FLAG_FORCE32
EVERY_FLAGS = ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL | ot.FLAG_NO_DEDUP          # every work item emits a block; the index format follows the triangle count
KEY_VARIANTS = ["recip", "reorder", "fused", "sat"]
RANK_MAX, RANK_CHUNK, PLACE_TILE = 16384, 4096, 1024                            # tail_kernels.hip: kRankMax, kRankChunk, kPlaceTile
FORMATS = [ot.FMT_2STATE, ot.FMT_4STATE]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------
def cvt_sat(x):
    """a saturating conversion (the `sat` variant): NaN -> 0, out of range -> INT_MIN / INT_MAX"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        t = np.trunc(np.where(np.isnan(x), F(0), x)).astype(np.float64)
    return np.clip(t, -2147483648.0, 2147483647.0).astype(np.int64)


def cell(a, b, c, variant=None):
    """the 8192-grid cell of one centroid coordinate: (a + b + c) / 3.f, times 8192.f, cvttss2si, MirrorOnce (|q + 0.5| truncated), clamp
    (bake_cpu_impl.cpp:1731-1748, util/texture.h:84-87)"""
    a, b, c = (np.asarray(v, F) for v in (a, b, c))
    cvt = cvt_sat if variant == "sat" else sc.cvt_i32
    with np.errstate(all="ignore"):
        if variant == "fused":
            q = ((a.astype(np.float64) + b.astype(np.float64) + c.astype(np.float64)) / 3.0 * 8192.0).astype(F)
        else:
            s = a + (b + c) if variant == "reorder" else (a + b) + c
            cen = s * (F(1) / F(3)) if variant == "recip" else s / F(3)
            q = F(8192) * cen
        qi = cvt(q)
        m = cvt(np.abs(qi.astype(F) + F(0.5)))
    return np.clip(m, 0, 8191)


def spread16(x):
    x = np.asarray(x, np.uint64)
    for s, m in ((8, 0x00FF00FF), (4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555)):
        x = (x | (x << np.uint64(s))) & np.uint64(m)
    return x


def sort_key(p, level, variant=None):
    """level << 60 | Morton(cell of u, cell of v), u in the even bits"""
    p = np.asarray(p, F).reshape(-1, 6)
    mx, my = cell(p[:, 0], p[:, 2], p[:, 4], variant), cell(p[:, 1], p[:, 3], p[:, 5], variant)
    return (np.asarray(level, np.uint64) << np.uint64(60)) | spread16(mx) | (spread16(my) << np.uint64(1))


def block_bytes(level, bits):
    return np.maximum(1, (4 ** np.asarray(level, np.int64) * bits) >> 3)


def digest_of_states(row):
    """CalcDigest (:374-377): XXH64, seed 42, over one byte per micro-triangle, UT folded into UO"""
    row = np.asarray(row, np.uint8)
    return xxhash.xxh64_intdigest(np.where(row == ot.UT, ot.UO, row).astype(np.uint8).tobytes(), seed=42)


def digests_of_rows(S):
    """digest_of_states of every row of an (m, n) array"""
    m, n = S.shape
    buf = np.where(S == ot.UT, ot.UO, S).astype(np.uint8).tobytes()
    return np.array([xxhash.xxh64_intdigest(buf[i * n:(i + 1) * n], seed=42) for i in range(m)], np.uint64)


def pack_states(S, bits):
    """(m, 4^L) states -> (m, block bytes) as Serialize packs them (:1800-1830): state u at bit u * bits, least significant first"""
    S = np.asarray(S, np.uint8)
    m, n = S.shape
    if bits == 1:
        out = np.packbits(S & 1, axis=1, bitorder="little")
    elif n < 4:
        out = S[:, :1].copy()
    else:
        q = S.reshape(m, n // 4, 4)
        out = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
    return np.ascontiguousarray(out, np.uint8)


def unpack_block(blk, n, bits):
    """(m, block bytes) -> (m, n) states"""
    blk = np.asarray(blk, np.uint8)
    if bits == 1:
        return np.unpackbits(blk, axis=1, bitorder="little")[:, :n]
    return np.stack([(blk >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(len(blk), -1)[:, :n]


def triangle_levels(case):
    T = len(case["uv"]) // 3
    if case["levels"] is None:
        return np.full(T, case["gmax"], np.int64)
    lv = np.asarray(case["levels"], np.int64)
    return np.where(lv <= 12, lv, case["gmax"])


def tail_inputs(case, raw, flags=None):
    """what the tail of `case` under `flags` starts from: the work items (first occurrences of (coordinates, level) in triangle order, every triangle its
    own with duplicate detection disabled), their states from `raw` (the oracle's result of the case under RAW_FLAGS), UVs and levels, and the
    triangle-to-item map.  States come grouped by level: groups[L] = (item numbers ascending, (m, 4^L) uint8)"""
    flags = case["flags"] if flags is None else flags
    bits = 2 if case["fmt"] == ot.FMT_4STATE else 1
    p = np.ascontiguousarray(case["uv"], F).reshape(-1, 6)
    T = len(p)
    level = triangle_levels(case)
    assert not sc.invalid(p).any() and raw.index_format == ot.IDX_U32 and len(raw.index) == T and (raw.index >= 0).all(), case["name"]
    first = sc.first_occurrence(p, level, np.zeros(T, bool), dedup=not flags & ot.FLAG_NO_DEDUP)
    owners = np.nonzero(first == np.arange(T))[0]
    number = np.full(T, -1, np.int64)
    number[owners] = np.arange(len(owners))
    tri_item = number[first]
    d = raw.descs[raw.index[owners].astype(np.int64)]
    assert np.array_equal(d[:, 1], level[owners]), case["name"]
    groups = {}
    for L in sorted(set(level[owners].tolist())):
        ids = np.nonzero(level[owners] == L)[0]
        nb = int(block_bytes(L, bits))
        blk = raw.array_data[d[ids, 0][:, None] + np.arange(nb)[None, :]]
        groups[L] = (ids, unpack_block(blk, 4 ** L, bits))
    return dict(groups=groups, uv=p[owners], level=level[owners], tri_item=tri_item, bits=bits, fmt=case["fmt"], T=T)


def restate_tail(inp, flags, rejection=0.0, unresolved=ot.SPECIAL_FUO, variant=None):
    """promotion and rejection, digest, first occurrence, the descending sort of (level << 60 | morton, item), offsets as running sums of the block
    sizes, arrayData, the index buffer in its format, both histograms.  `variant`: a wrong sort key (KEY_VARIANTS)"""
    groups, level, bits, T = inp["groups"], inp["level"], inp["bits"], inp["T"]
    I = len(level)
    special = np.zeros(I, np.int64)
    digest = np.zeros(I, np.uint64)
    known = np.zeros(I, np.int64)
    uniform = np.zeros(I, bool)
    rejected = np.zeros(I, bool)
    frac = np.zeros(I, F)
    rej = F(rejection)
    for L, (ids, S) in groups.items():
        uniform[ids] = (S == S[:, :1]).all(axis=1)
        known[ids] = (S <= ot.O).sum(axis=1)
        frac[ids] = known[ids].astype(F) / F(4 ** L)
        common = S[:, 0].astype(np.int64)
        eq = uniform[ids].copy()
        if rej > 0:                                   # (NaN, -0.0 and negative thresholds compare false: nothing is rejected)
            r = ~eq & (frac[ids] < rej)
            rejected[ids] = r
            common = np.where(r, ot.UT, common)
            eq |= r
        if not flags & ot.FLAG_NO_SPECIAL:
            special[ids] = np.where(eq, -common - 1, 0)
        digest[ids] = digests_of_rows(S)
    rep = np.arange(I, dtype=np.int64)
    if not flags & ot.FLAG_NO_DEDUP:                  # the first item with a digest keeps the block; special items enter the map like every other
        seen = {}
        for i, dg in enumerate(digest.tolist()):
            rep[i] = seen.setdefault(dg, i)
    emitted = np.nonzero((special == 0) & (rep == np.arange(I)))[0]
    key = sort_key(inp["uv"][emitted], level[emitted], variant)
    order = emitted[np.lexsort((emitted, key))[::-1]]                       # descending by (key, item)
    sizes = block_bytes(level[order], bits)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(order) else np.zeros(0, np.int64)
    total = int(sizes.sum())
    assert total <= 0xFFFFFFFF
    array = np.zeros(total, np.uint8)
    slot = np.full(I, -1, np.int64)
    slot[order] = np.arange(len(order))
    for L, (ids, S) in groups.items():
        keep = slot[ids] >= 0
        if keep.any():
            packed = pack_states(S[keep], bits)
            array[offsets[slot[ids[keep]]][:, None] + np.arange(packed.shape[1])[None, :]] = packed
    descs = np.stack([offsets, level[order], np.full(len(order), inp["fmt"])], axis=1).astype(np.int64).reshape(-1, 3)
    value = np.where(special != 0, special, slot)
    tri_item = inp["tri_item"]
    index = np.where(tri_item >= 0, value[rep[np.maximum(tri_item, 0)]], unresolved).astype(np.int64)
    if flags & ot.FLAG_ALLOW8 and T <= 127 and not flags & ot.FLAG_FORCE32:
        index_format, index = ot.IDX_U8, index.astype(np.int8)
    elif T <= 32767 and not flags & ot.FLAG_FORCE32:
        index_format, index = ot.IDX_U16, index.astype(np.int16)
    else:
        index_format, index = ot.IDX_U32, index.astype(np.int32)
    owner = rep[tri_item[tri_item >= 0]]
    owner = owner[slot[owner] >= 0]
    array_hist = [(c, L, inp["fmt"]) for L, c in sorted(Counter(level[order].tolist()).items())]
    index_hist = [(c, L, inp["fmt"]) for L, c in sorted(Counter(level[owner].tolist()).items())]
    return dict(special=special, digest=digest, rep=rep, order=order, descs=descs, array=array, index=index, index_format=index_format, array_hist=array_hist,
                index_hist=index_hist, known=known, frac=frac, uniform=uniform, rejected=rejected, key=key, emitted=emitted,
                small=int((sizes < 16).sum()))


def check_result(case, res, rs):
    """a library's result equals the restatement's: descriptors (offset, level, format), arrayData, index buffer and format, both histograms"""
    name = case["name"]
    assert len(res.descs) == len(rs["descs"]), (name, len(res.descs), len(rs["descs"]))
    if len(rs["descs"]):
        bad = np.nonzero((np.asarray(res.descs).reshape(-1, 3) != rs["descs"]).any(axis=1))[0]
        assert bad.size == 0, (name, "%d descriptors differ, first %d: got %r want %r" % (bad.size, bad[0], res.descs[bad[0]], rs["descs"][bad[0]]))
    assert res.index_format == rs["index_format"], (name, res.index_format, rs["index_format"])
    assert res.index.dtype == rs["index"].dtype and np.array_equal(res.index, rs["index"]), (name, np.nonzero(res.index != rs["index"])[0][:8])
    assert np.array_equal(res.array_data, rs["array"]), (name, res.array_data.size, rs["array"].size)
    assert [tuple(int(v) for v in h) for h in res.array_hist] == rs["array_hist"], (name, res.array_hist, rs["array_hist"])
    assert [tuple(int(v) for v in h) for h in res.index_hist] == rs["index_hist"], (name, res.index_hist, rs["index_hist"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# running a case
# ---------------------------------------------------------------------------------------------------------------------------------------------
def make_case(name, tex, uv, gmax, *, levels=None, fmt=ot.FMT_4STATE, flags=EVERY_FLAGS, filt=ot.NEAREST, addr=ot.WRAP, promo=ot.PROMO_NEAREST, rejection=0.0, le=ot.T, gt=ot.O):
    uv = np.ascontiguousarray(np.asarray(uv, F).reshape(-1, 2))
    return dict(name=name, tex=tex, uv=uv, ix=np.arange(len(uv), dtype=np.uint32), gmax=gmax, levels=None if levels is None else np.ascontiguousarray(levels, np.uint8),
                fmt=fmt, flags=flags, filt=filt, addr=addr, promo=promo, rejection=float(rejection), le=le, gt=gt)


def desc_kw(case, flags=None, rejection=None):
    """the keyword arguments of ommtest.make_desc (and of test_gpu_parity.both) for a case"""
    return dict(fmt=case["fmt"], addr=case["addr"], filt=case["filt"], promo=case["promo"], flags=case["flags"] if flags is None else flags,
                levels=case["levels"], rejection=case["rejection"] if rejection is None else rejection, le=case["le"], gt=case["gt"])


_ORACLE_TEXTURE = {}


def release_oracle_texture():
    """destroys the kept texture and baker (at the next texture, and when the process ends)"""
    if _ORACLE_TEXTURE:
        _ORACLE_TEXTURE["lib"].destroy_texture(_ORACLE_TEXTURE["baker"], _ORACLE_TEXTURE["handle"])
        _ORACLE_TEXTURE["lib"].destroy_baker(_ORACLE_TEXTURE["baker"])
        _ORACLE_TEXTURE.clear()


atexit.register(release_oracle_texture)


def _oracle_texture(lib, tex):
    """the oracle's baker and texture object of the array used last, kept for the next bake over the same array (the summed-area table of an 8192^2
    texture costs more than the bakes of family D over it)"""
    if _ORACLE_TEXTURE.get("tex") is not tex:
        release_oracle_texture()
        b = lib.create_baker()
        _ORACLE_TEXTURE.update(lib=lib, tex=tex, baker=b, handle=lib.create_texture(b, [tex], alpha_cutoff=0.5))
    return _ORACLE_TEXTURE["baker"], _ORACLE_TEXTURE["handle"]


def bake(lib, case, flags=None, rejection=None, knobs=(), inspect=None):
    """one bake of the case; inspect(baker) runs behind it, while the baker still lives"""
    keep = lib.which == "oracle" and not knobs
    if keep:
        b, t = _oracle_texture(lib, case["tex"])
    else:
        b = lib.create_baker()
        for k, v in knobs:
            lib.set_knob(b, k, v)
        t = lib.create_texture(b, [case["tex"]], alpha_cutoff=0.5)
    d = ot.make_desc(t, case["uv"], case["ix"], case["gmax"], **desc_kw(case, flags, rejection))
    r = lib.bake(b, d)
    if inspect:
        inspect(b)
    if not keep:
        lib.destroy_texture(b, t)
        lib.destroy_baker(b)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------
# textures and the cheap triangles of families K and P
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def checker(n=256):
    """a 1-texel checker: with the Nearest filter no triangle of a texel or more is uniform above level 0"""
    yy, xx = np.mgrid[0:n, 0:n]
    return np.ascontiguousarray(((xx % 2) == (yy % 2)).astype(np.uint8) * 255)


def cheap_triangles(seed, n, extent=1.5 / 256, lo=0.0, hi=1.0):
    """n small triangles (a texel and a half of the 256^2 checker) with unshared vertices at seeded random places"""
    uv, _ = ot.random_triangles(seed, n, extent, lo=lo, hi=hi)
    return uv.reshape(-1, 6)


def stepped_levels(n, top=2, step=1000):
    """levels that change every `step` items: 0, 1, ..., top, 0, ..."""
    return ((np.arange(n) // step) % (top + 1)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family K: the sort key
# ---------------------------------------------------------------------------------------------------------------------------------------------
EDGE_K = [0, 1, 2, 4095, 4096, 8191, 8192, 8193, -1, -2, -4096, -8191, -8192, -8193]


def expected_cell(q):
    """the cell of a product 8192 * c = q, written out independently of `cell`: truncate toward zero, mirror once (-k -> k - 1), clamp"""
    t = int(np.trunc(np.float64(q)))
    return min(max(t if t >= 0 else -t - 1, 0), 8191)


def triangle_with_centroid(c, rng, other, axis, extent=F(2.0 ** -12)):
    """a non-degenerate triangle whose restated centroid along `axis` is exactly the float32 c (searched through the restatement); the other axis
    carries an ordinary coordinate near `other`"""
    c = F(c)
    with np.errstate(all="ignore"):
        for attempt in range(64):
            n = 512
            a = (c + (rng.random(n).astype(F) - F(0.5)) * extent).astype(F)
            b = (c + (rng.random(n).astype(F) - F(0.5)) * extent).astype(F)
            if attempt & 1:                                    # a + b == 0 exactly: the only way to a centroid far below the vertices' spacing
                b = -a
            third = (F(3) * c - (a + b)).astype(F)
            for d in range(-3, 4):
                t3 = third
                for _ in range(abs(d)):
                    t3 = np.nextafter(t3, F(np.inf) if d > 0 else F(-np.inf))
                cen = ((a + b) + t3) / F(3)
                hit = np.nonzero(cen.view(np.uint32) == c.view(np.uint32))[0]
                if c == 0:
                    hit = np.nonzero((cen == 0) & (np.signbit(cen) == np.signbit(c)))[0]
                for h in hit:
                    o = F(other) + (rng.random(3).astype(F) - F(0.5)) * extent
                    tri = np.zeros(6, F)
                    tri[axis::2] = [a[h], b[h], t3[h]]
                    tri[1 - axis::2] = o
                    if not sc.degenerate(tri.reshape(1, 6))[0]:
                        return tri
    raise AssertionError("no triangle with centroid %r" % c)


@functools.lru_cache(maxsize=None)
def k1_edge_triangles():
    """[(triangle, axis, k, side, product)]: for every k of EDGE_K and both axes, centroids whose 8192 * c is the largest float32 below k (side -1), k
    itself (0) and the smallest above (+1); and centroids inside (-1 / 8192, 1 / 8192), the double-width cell that truncation toward zero makes"""
    rng = np.random.default_rng(8192)
    out = []
    for axis in (0, 1):
        for k in EDGE_K:
            for side in (-1, 0, 1):
                q = F(k)
                if side:
                    q = np.nextafter(q, F(np.inf) if side > 0 else F(-np.inf))
                    if k == 0:
                        q = F(side * 2.0 ** -100)             # (the floats next to 0 are denormal and their centroid is not representable: a tiny normal product stands in)
                c = F(q / F(8192))
                assert F(8192) * c == q
                out.append((triangle_with_centroid(c, rng, 0.3 + 0.05 * axis, axis), axis, k, side, float(q)))
        for q in (-0.999, -0.5, -0.001, 0.001, 0.5, 0.999):
            c = F(F(q) / F(8192))
            out.append((triangle_with_centroid(c, rng, 0.6, axis), axis, 0, 2, float(F(8192) * c)))
    return out


def k1_case(fmt):
    tris = k1_edge_triangles()
    uv = np.array([t[0] for t in tris], F)
    plain = cheap_triangles(41, 200, extent=2.0 ** -11, lo=-1.2, hi=1.2)
    lv = (np.arange(len(uv) + len(plain)) % 3).astype(np.uint8)
    lv[:len(uv)] = 1                                            # the edge triangles share a level: only their cells order them
    return make_case("k1-edges-fmt%d" % fmt, checker(), np.concatenate([uv, plain]), 2, levels=lv, fmt=fmt)


@functools.lru_cache(maxsize=None)
def k2_rounding_triangles(want=(("recip", 50), ("reorder", 50), ("fused", 20))):
    """{variant: (n, 6) triangles whose restated key differs from the variant's}: centroids aimed at cell edges k / 8192 along u (v: an ordinary place),
    vertices a few cells apart, the third vertex within a few float32 spacings of 3 k / 8192 minus the other two"""
    rng = np.random.default_rng(1 << 13)
    found = {v: [] for v, _ in want}
    for _ in range(8):
        n = 200000
        k = rng.integers(1024, 8192, n).astype(F)
        edge = k / F(8192)
        a = (edge + (rng.random(n).astype(F) - F(0.5)) * F(2.0 ** -11)).astype(F)
        b = (edge + (rng.random(n).astype(F) - F(0.5)) * F(2.0 ** -11)).astype(F)
        c = (F(3) * edge - a - b).astype(F)
        c = (c.view(np.int32) + rng.integers(-2, 3, n).astype(np.int32)).view(F)
        v = rng.random((n, 3)).astype(F) * F(2.0 ** -11) + rng.random(n).astype(F)[:, None] * F(0.9)
        p = np.stack([a, v[:, 0], b, v[:, 1], c, v[:, 2]], axis=1).astype(F)
        p = p[~sc.degenerate(p)]
        for var, need in want:
            if len(found[var]) < 2 * need:
                moved = (cell(p[:, 0], p[:, 2], p[:, 4], var) != cell(p[:, 0], p[:, 2], p[:, 4])) & (cell(p[:, 1], p[:, 3], p[:, 5], var) == cell(p[:, 1], p[:, 3], p[:, 5]))
                found[var].extend(p[moved][:2 * need - len(found[var])])
        if all(len(found[v]) >= 2 * need for v, need in want):
            break
    return {v: np.array(found[v], F).reshape(-1, 6) for v, _ in want}


def k2_case(fmt):
    """the searched triangles among 2 000 ordinary ones.  A cell that moves by one changes the order only if somebody sits between the two keys, so every
    searched triangle has two witnesses, small triangles in the middle of its right cell and of the cell its variant would give: it ties with one of
    them.  The witnesses come earlier in the input than the searched triangles, so the tie is decided for the searched triangle (descending item
    index) and a wrong cell moves it behind a witness"""
    found = k2_rounding_triangles()
    special = np.concatenate([found[v] for v in ("recip", "reorder", "fused")])
    variant = sum([[v] * len(found[v]) for v in ("recip", "reorder", "fused")], [])
    rng = np.random.default_rng(5)
    witnesses = []
    for t, v in zip(special, variant):
        cv = int(cell(t[1], t[3], t[5])[()])
        for cu in (int(cell(t[0], t[2], t[4])[()]), int(cell(t[0], t[2], t[4], v)[()])):
            d = (rng.random((3, 2)) - 0.5) * (0.5 / 8192.0)
            witnesses.append((np.array([(cu + 0.5) / 8192.0, (cv + 0.5) / 8192.0]) + d).reshape(-1))
    plain = cheap_triangles(43, 2000, extent=2.0 ** -11)
    front = np.concatenate([plain[:1000], np.array(witnesses, F)])
    back = np.concatenate([plain[1000:], special])
    uv = np.concatenate([front[rng.permutation(len(front))], back[rng.permutation(len(back))]])
    c = make_case("k2-rounding-fmt%d" % fmt, checker(), uv, 1, fmt=fmt)
    c["searched"] = {v: len(found[v]) for v in found}
    return c


TIE_GROUPS = [2, 63, 64, 65, 300]


def k3_case(fmt, padded):
    """groups of 2, 63, 64, 65 and 300 triangles of different shapes with one level and one cell each, interleaved in input order with triangles of
    other cells and levels; `padded`: further triangles behind them take the candidate count past the counting path's limit"""
    rng = np.random.default_rng(33)
    tris, lv, group = [], [], []
    for g, size in enumerate(TIE_GROUPS):
        cu, cv = (1000 + 517 * g + 0.5) / 8192.0, (3000 - 211 * g + 0.5) / 8192.0        # cell centres
        for _ in range(size):
            d = (rng.random((3, 2)) - 0.5) * (0.6 / 8192.0)                                # the centroid stays within 0.3 cells of the centre
            tris.append((np.array([cu, cv]) + d).reshape(-1))
            lv.append(g % 3)
            group.append(g)
    tris = np.array(tris, F)
    other = cheap_triangles(47, 3 * len(tris), extent=2.0 ** -11)
    n = len(tris) + len(other)
    slots = np.sort(np.random.default_rng(7).permutation(n)[:len(tris)])                   # where the group triangles sit in input order
    uv, levels, grp = np.zeros((n, 6), F), np.zeros(n, np.uint8), np.full(n, -1, np.int64)
    mask = np.zeros(n, bool)
    mask[slots] = True
    order_in = np.random.default_rng(9).permutation(len(tris))                             # the groups interleave each other too
    uv[mask], levels[mask], grp[mask] = tris[order_in], np.array(lv, np.uint8)[order_in], np.array(group)[order_in]
    uv[~mask], levels[~mask] = other, (np.arange(len(other)) % 3).astype(np.uint8)
    if padded:
        pad = cheap_triangles(49, RANK_MAX + 700 - n, extent=2.0 ** -11)
        uv, levels, grp = np.concatenate([uv, pad]), np.concatenate([levels, (np.arange(len(pad)) % 3).astype(np.uint8)]), np.concatenate([grp, np.full(len(pad), -1)])
    c = make_case("k3-ties-fmt%d-%s" % (fmt, "sort" if padded else "count"), checker(), uv, 2, levels=levels, fmt=fmt)
    c["group"] = grp
    return c


def tie_groups_hold(case, order, inp):
    """every group of a k3 case: one level, one key, its descriptors adjacent and in descending item order.  order: descriptor -> work item"""
    slot = np.full(len(inp["level"]), -1)
    slot[order] = np.arange(len(order))
    key = sort_key(inp["uv"], inp["level"])
    sizes = []
    for g in range(len(TIE_GROUPS)):
        items = np.nonzero(case["group"] == g)[0]               # (no duplicates: item = triangle)
        sizes.append(len(items))
        assert len(set(key[items].tolist())) == 1 and len(set(inp["level"][items].tolist())) == 1
        assert (key == key[items[0]]).sum() == len(items)       # nobody else in the group's cell at its level
        s = slot[items]
        assert np.array_equal(np.sort(s), np.arange(s.min(), s.min() + len(items)))
        assert np.array_equal(order[s.min():s.min() + len(items)], items[::-1])
        assert np.any(np.diff(items) > 1)                        # interleaved with other triangles in input order
    assert sizes == TIE_GROUPS


def k4_case(fmt):
    """per-triangle levels 0 - 5 and 0xF (the global level, 4): blocks of 1, 1, 2, 8, 32, 128 bytes in 2-state and 1, 1, 4, 16, 64, 256 in 4-state"""
    n = 420
    uv = cheap_triangles(51, n, extent=3.0 / 256)
    lv = (np.arange(n) * 5 % 7).astype(np.uint8)
    lv[lv == 6] = 0xF
    return make_case("k4-levels-fmt%d" % fmt, checker(), uv, 4, levels=lv, fmt=fmt)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family P: placement counts
# ---------------------------------------------------------------------------------------------------------------------------------------------
P_COUNTS = [1, 2, 31, 32, 33, 1023, 1024, 1025, 2047, 2049, 3073, 4095, 4096, 4097, 8191, 8193, 16383, 16384, 16385, 17408, 17409, 32769]
P_PARTIAL = [(16385, 1), (16385, 1024), (16385, 16384), (20000, 1), (20000, 1024), (20000, 16384)]
LEVEL_MODES = ["one-level", "stepped"]


def p_all_case(n, mode, fmt):
    """n candidates, all emitted (special indices and duplicate detection off: the candidate bound is the item count)"""
    uv = cheap_triangles(1000 + n, n, extent=2.0 ** -11)
    lv = None if mode == "one-level" else stepped_levels(n)
    return make_case("p-all-%d-%s-fmt%d" % (n, mode, fmt), checker(), uv, 1, levels=lv, fmt=fmt)


PARTIAL_KINDS = ["duplicates", "uniform"]
POOL_SIZE = 26000
_PICKS = {}


@functools.lru_cache(maxsize=None)
def _p_pool():
    """triangles of three texels on the checker at places that are multiples of 2^-14 inside [0, 1/4)^2: moved by multiples of the checker's period
    (2^-7) every coordinate stays exact, so a moved copy classifies like the original"""
    uv = cheap_triangles(77, POOL_SIZE, extent=3.0 / 256, lo=0.03, hi=0.22)
    return (np.round(uv.astype(np.float64) * 16384) / 16384).astype(F)


def p_picks(oracle, fmt, L):
    """pool triangles that are non-uniform at level L with pairwise different digests, by the oracle's decode (one bake per format and level)"""
    if (fmt, L) not in _PICKS:
        probe = make_case("p-pool-L%d-fmt%d" % (L, fmt), checker(), _p_pool(), L, fmt=fmt, flags=RAW_FLAGS)
        rs = restate_tail(tail_inputs(probe, bake(oracle, probe)), RAW_FLAGS)
        _, firsts = np.unique(rs["digest"], return_index=True)
        firsts = np.sort(firsts)
        _PICKS[(fmt, L)] = firsts[~rs["uniform"][firsts]]
    return _PICKS[(fmt, L)]


def p_partial_case(oracle, n, emitted, mode, fmt, kind):
    """n candidates of which `emitted` keep a block, special indices and duplicate detection on.  The emitting triangles come from the pool (level 3; in
    mode "stepped" the level changes to 4 and back every 1000 of them) and sit evenly spread over the input.  kind "duplicates": every other
    triangle is a copy of an emitting one moved by whole periods of the checker -- other coordinates, so a work item of its own, the same states, so
    an exact duplicate by digest; all candidates are non-uniform.  kind "uniform": every other triangle is a level-0 triangle, uniform by
    construction and promoted to a special index."""
    pool = _p_pool()
    e = np.arange(emitted)
    base_level = np.full(emitted, 3, np.int64) if mode == "one-level" else 3 + (e // 1000) % 2
    base = np.zeros((emitted, 6), F)
    for L in sorted(set(base_level.tolist())):
        picks, m = p_picks(oracle, fmt, L), base_level == L
        assert len(picks) >= m.sum(), ("the pool holds %d distinct non-uniform blocks at level %d, %d needed" % (len(picks), L, m.sum()))
        base[m] = pool[picks[:m.sum()]]
    pos = np.linspace(0, n - 1, emitted).astype(np.int64) if emitted > 1 else np.array([n // 3])
    assert len(np.unique(pos)) == emitted
    uv, lv = np.zeros((n, 6), F), np.zeros(n, np.uint8)
    rest = np.setdiff1d(np.arange(n), pos)
    uv[pos], lv[pos] = base, base_level
    j = np.arange(len(rest))
    if kind == "duplicates":
        q = j // emitted + 1
        shift = np.stack([(q % 256), (q // 256)], axis=1).astype(F) * F(2.0 ** -7)
        uv[rest] = (base[j % emitted].reshape(-1, 3, 2) + shift[:, None, :]).reshape(-1, 6)
        lv[rest] = base_level[j % emitted]
    else:
        uv[rest] = cheap_triangles(79 + n, len(rest), extent=2.0 ** -11)
    c = make_case("p-partial-%d-%d-%s-%s-fmt%d" % (n, emitted, mode, kind, fmt), checker(), uv, 4, levels=lv, fmt=fmt, flags=ot.FLAG_THREADS)
    c["emitted"], c["emit_pos"] = emitted, pos
    return c


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family R: promotion and rejection
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise(n=512):
    return np.ascontiguousarray((ot.value_noise(11, n, n, octaves=4, base_cell=32) * 255).astype(np.uint8))


def r1_case(fmt, flags=ot.FLAG_THREADS, rejection=0.0):
    """300 triangles over noise at per-triangle levels 2 - 5, Linear filter: items of every known count"""
    uv, _ = ot.random_triangles(97, 300, 0.06)
    lv = (2 + ot.hash_u32(np.arange(300) + 3) % 4).astype(np.uint8)
    return make_case("r1-fmt%d-flags%x-rej%r" % (fmt, flags, rejection), noise(), uv, 5, levels=lv, fmt=fmt, flags=flags, filt=ot.LINEAR, rejection=rejection)


R1_FLAGS = [ot.FLAG_THREADS, ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL]
R1_ODD = [1.0, 1.5, float(np.float32(1e-45)), -0.0, -1.0, float("nan")]


def r1_pairs(rs, level):
    """six (k, N) pairs of non-uniform items of the 4-state bake, spread over the levels: per level the smallest k above 0 that leaves an item
    strictly below it, then the medians of levels 3 and 5"""
    out = []
    by_level = {}
    for L in (2, 3, 4, 5):
        ks = np.unique(rs["known"][(level == L) & ~rs["uniform"]])
        by_level[L] = ks
        mid = ks[(ks > ks.min())]
        out.append((int(mid[0]), 4 ** L))
    for L in (3, 5):
        ks = by_level[L]
        k = int(ks[len(ks) // 2])
        if (k, 4 ** L) not in out and k > ks.min():
            out.append((k, 4 ** L))
        else:
            out.append((int(ks[-1]), 4 ** L))
    return out


def r1_thresholds(pairs):
    """[(threshold, (k, N) or None)]: float32(k / N), the float below, the float above; then the odd ones"""
    out = []
    for k, n in pairs:
        t = F(k) / F(n)
        out += [(float(t), (k, n)), (float(np.nextafter(t, F(-np.inf))), None), (float(np.nextafter(t, F(np.inf))), None)]
    return out + [(t, None) for t in R1_ODD]


@functools.lru_cache(maxsize=None)
def halves():
    """64 x 64 texels, the left half transparent, the right half opaque"""
    t = np.zeros((64, 64), np.uint8)
    t[:, 32:] = 255
    return t


R2_STATES = {ot.FMT_2STATE: [(ot.T, ot.O), (ot.O, ot.T)], ot.FMT_4STATE: [(ot.T, ot.O), (ot.UT, ot.UO), (ot.UO, ot.UT), (ot.T, ot.UO)]}
R2_FIRST_AT = [255, 65600]


def r2_states(fmt, first_at):
    """every pair of states at the workgroup edge; beyond 65 536 items, where only the item number is new, the plain pair and the pair that shares a digest"""
    return R2_STATES[fmt] if first_at < 65536 else R2_STATES[fmt][:2]


def r2_case(fmt, le, gt, first_at, flags=ot.FLAG_THREADS):
    """uniform work items of the states `le` (left half) and `gt` (right half) at levels 0 - 8, three rounds of them at different places, between
    non-uniform level-1 triangles that straddle the halves.  `first_at` of those come first, so the first uniform items are work items first_at (for 255:
    the last lane of a workgroup of 256) and first_at + 1 (the first lane of the next); then uniform and non-uniform triangles alternate.  Every
    triangle has coordinates of its own: work item = triangle.  c["side"]: 0 / 1 for a uniform triangle in the left / right half, -1 for the others"""
    uni, side, lv = [], [], []
    for rnd in range(3):
        for L in range(9):
            for s in ((0, 1) if (L + rnd) % 2 == 0 else (1, 0)):               # both input orders of the two states of a level
                k = len(uni)
                x, y = (0.06 if s == 0 else 0.62) + 0.004 * (k % 64), 0.1 + 0.012 * (k // 2)
                uni.append([x, y, x + 0.05, y + 0.01, x + 0.02, y + 0.06])
                side.append(s)
                lv.append(L)
    n_fill = first_at + len(uni)
    k = np.arange(n_fill)
    a, y = (0.03 + 0.04 * (k % 97) / 97.0), 0.05 + 0.85 * k / n_fill
    fill = np.stack([0.5 - a, y, 0.5 + a, y, 0.5 + 0.01 * (k % 3), y + a], axis=1)
    n = n_fill + len(uni)
    uv, levels, sd = np.zeros((n, 6)), np.ones(n, np.uint8), np.full(n, -1, np.int64)
    upos = np.concatenate([[first_at, first_at + 1], first_at + 3 + 2 * np.arange(len(uni) - 2)])
    mask = np.zeros(n, bool)
    mask[upos] = True
    uv[mask], levels[mask], sd[mask] = np.array(uni), np.array(lv, np.uint8), np.array(side)
    uv[~mask] = fill
    c = make_case("r2-fmt%d-le%d-gt%d-first%d-flags%x" % (fmt, le, gt, first_at, flags), halves(), uv, 8, levels=levels, fmt=fmt, flags=flags, filt=ot.LINEAR, addr=ot.CLAMP, le=le, gt=gt)
    c["side"] = sd
    return c


def r2_statements(case, index, rs=None):
    """the direct statements on the index buffer of an r2 case: every uniform triangle carries the value of the first triangle of its level and 3-state
    class; with special indices that value is the first one's special index (where, by the restatement, no earlier non-uniform item shares its
    digest); without, one block per class"""
    side, level = case["side"], np.asarray(case["levels"], np.int64)
    state = np.where(side == 0, case["le"], case["gt"])
    cls = np.where(state == ot.UT, ot.UO, state)
    index = np.asarray(index, np.int64)
    firsts = {}
    for t in np.nonzero(side >= 0)[0]:
        f = firsts.setdefault((int(level[t]), int(cls[t])), t)
        assert index[t] == index[f], (case["name"], t, f)
        if not case["flags"] & ot.FLAG_NO_SPECIAL and (rs is None or rs["rep"][f] == f):
            assert index[t] == -int(state[f]) - 1, (case["name"], t, index[t], state[f])
        if case["flags"] & ot.FLAG_NO_SPECIAL:
            assert index[t] >= 0
    values = [int(index[f]) for f in firsts.values()]
    if case["flags"] & ot.FLAG_NO_SPECIAL and rs is not None:
        own = [f for f in firsts.values() if rs["rep"][f] == f]
        assert len({int(index[f]) for f in own}) == len(own)
    return len(firsts), values


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family D: digests
# ---------------------------------------------------------------------------------------------------------------------------------------------
# (level, format, item count): streams of 1, 4 and 16 bytes and every tail of the short-stream branch; 256- and 512-byte blocks around the workgroup
# edges of the LDS form (64 items); 1 KiB and 2 KiB blocks around the workgroup edge of the chain form (16 items) and the chain / LDS choice (2048 items)
D1_SMALL = [(L, f, 150) for L in (0, 1, 2, 3, 4) for f in FORMATS] + [(5, ot.FMT_2STATE, 150)]
D1_LDS = [(5, ot.FMT_4STATE, n) for n in (1, 63, 64, 65, 129)] + [(6, ot.FMT_2STATE, n) for n in (1, 63, 64, 65, 129)]
D1_CHAIN = [(6, ot.FMT_4STATE, n) for n in (1, 15, 16, 17, 2047, 2048, 2049)] + [(7, ot.FMT_2STATE, n) for n in (1, 15, 16, 17, 2047, 2048, 2049)]
D1_CASES = D1_SMALL + D1_LDS + D1_CHAIN


@functools.lru_cache(maxsize=None)
def foliage():
    return ot.foliage_texture(17, 1024, 1024, feature=24)


_D1_POOL = {}


class RawSubset:
    """the part of a RAW_FLAGS result that belongs to some of its triangles: what tail_inputs reads of a result"""

    def __init__(self, raw, keep):
        self.index, self.descs, self.array_data, self.index_format = raw.index[keep], raw.descs, raw.array_data, raw.index_format


def d1_case(oracle, level, fmt, n):
    """n work items of one level over 24-texel foliage; from level 5 on every one of them non-uniform (the first n such of a candidate list, by the
    oracle's decode), so that the device's active list of the level holds exactly n items.  The case carries the candidates' decode as its "raw" result"""
    big = n >= 1000
    key = (level, fmt, big)
    if key not in _D1_POOL:
        m = 150 if level <= 4 else (2400 if big else 208)
        uv, _ = ot.random_triangles(900 + level, m, (90.0 if big else 60.0) / 1024)
        c = make_case("d1-pool", foliage(), uv, level, fmt=fmt, flags=ot.FLAG_THREADS, filt=ot.LINEAR, promo=ot.PROMO_FORCE_OPAQUE)
        raw = bake(oracle, c, flags=RAW_FLAGS)
        keep = np.arange(m) if level <= 4 else np.nonzero(~restate_tail(tail_inputs(c, raw, RAW_FLAGS), RAW_FLAGS)["uniform"])[0]
        _D1_POOL[key] = (c, raw, keep)
    c, raw, keep = _D1_POOL[key]
    keep = keep[:n]
    assert len(keep) == n, (level, fmt, n, len(keep))
    sub = make_case("d1-L%d-fmt%d-%d" % (level, fmt, n), foliage(), c["uv"].reshape(-1, 6)[keep], level, fmt=fmt, flags=ot.FLAG_THREADS, filt=ot.LINEAR, promo=ot.PROMO_FORCE_OPAQUE)
    sub["raw"] = RawSubset(raw, keep)
    return sub


D1_MULTI_COUNTS = {3: 100, 5: 100, 6: 2700, 7: 100, 8: 40}


def d1_multi_level_case():
    """five levels at once: 3 (16 bytes, the small form); 5 (256 bytes) and 6 (1 KiB, but more than 2048 items: not the chain form) as two segments
    of the multi-level LDS launch; 7 and 8 (4 and 16 KiB, few items) as two segments of the multi-level chain launch: both blockStart searches"""
    lv = np.concatenate([np.full(c, L, np.uint8) for L, c in D1_MULTI_COUNTS.items()])
    lv = lv[np.argsort(ot.hash_u32(np.arange(len(lv)) + 9), kind="stable")]
    uv, _ = ot.random_triangles(931, len(lv), 60.0 / 1024)
    return make_case("d1-multi", foliage(), uv, 8, levels=lv, fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS, filt=ot.LINEAR, promo=ot.PROMO_FORCE_OPAQUE)


def block_digests(raw, case):
    """Counter of XXH64 over the decoded blocks of the non-uniform work items of a RAW_FLAGS result"""
    rs = restate_tail(tail_inputs(case, raw, RAW_FLAGS), RAW_FLAGS)
    return Counter(rs["digest"][~rs["uniform"]].tolist()), rs


# ---- near twins and true twins ----
TWIN_S = 6                       # texels per micro-triangle leg: texel (1, 1) from the right-angle corner lies strictly inside the micro-triangle
TWIN_LEVELS = {ot.FMT_4STATE: [2, 3, 4, 5, 6, 7, 8, 9], ot.FMT_2STATE: [3, 4, 5, 6, 7, 8]}


def twin_unit(level, fmt):
    """micro-triangles per swept unit: a packed byte to level 5 (4-state) / 6 (2-state), 16 bytes above"""
    per_byte = 4 if fmt == ot.FMT_4STATE else 8
    return per_byte if level <= (5 if fmt == ot.FMT_4STATE else 6) else 16 * per_byte


@functools.lru_cache(maxsize=None)
def twin_layout(level, need_down=True):
    """(texture, E, defect for upright targets, defect for flipped targets, origin of the untouched triangle).  The pattern -- opaque, a transparent
    column every 12 texels -- does not change under vertical moves or horizontal moves by 12 texels, so a right triangle with legs of E = 6 * 2^level
    texels classifies the same wherever such a move puts it: micro-triangles whose columns are 0 - 5 (mod 12) are opaque, the others touch a
    transparent column.  Two single transparent texels (defects) break that: a triangle moved so that a defect lies strictly inside one opaque
    micro-triangle differs from the untouched one in that micro-triangle and nowhere else"""
    E = TWIN_S * 2 ** level
    W = 1 << int(np.ceil(np.log2((4 if need_down else 2) * E + 64)))
    H = 1 << int(np.ceil(np.log2(2 * E + 64)))
    tex = np.full((H, W), 255, np.uint8)
    tex[:, np.arange(W) % 12 == 9] = 0
    yd = E + 8
    d_up, d_down = (E + 12 + 1, yd), (3 * E + 36 + 4, yd)
    tex[d_up[1], d_up[0]] = 0
    if need_down:
        tex[d_down[1], d_down[0]] = 0
    return tex, E, d_up, d_down, (0, yd + 16)


def twin_triangle(tex, E, origin):
    H, W = tex.shape
    x, y = origin
    return np.array([x / W, y / H, (x + E) / W, y / H, x / W, (y + E) / H], F)


def twin_units(level, fmt):
    """first micro-triangle of every swept unit: every unit to level 7; the first and the last unit of every 256-byte chunk at level 8 and of every
    1 KiB chunk at level 9"""
    n, unit = 4 ** level, twin_unit(level, fmt)
    if level <= 7:
        return list(range(0, n, unit))
    per_byte = 4 if fmt == ot.FMT_4STATE else 8
    chunk = (256 if level == 8 else 1024) * per_byte
    return sorted({c0 for c in range(0, n, chunk) for c0 in (c, c + chunk - unit)})


@functools.lru_cache(maxsize=None)
def twin_targets(level, fmt):
    """one opaque micro-triangle per swept unit: (bird-curve index, texel strictly inside it relative to the triangle's origin, upright)"""
    n, unit = 4 ** level, twin_unit(level, fmt)
    idx = np.arange(n)
    v = lu.micro_vertices(idx, np.full(n, level))
    corner = np.rint(v[:, 0] * 2 ** level).astype(np.int64) * TWIN_S          # the right-angle corner in texels from the origin
    up = v[:, 1, 0] > v[:, 0, 0]
    lo = np.where(up, corner[:, 0], corner[:, 0] - TWIN_S)                     # first column of the micro-triangle
    clear = lo % 12 == 0
    out = []
    for u0 in twin_units(level, fmt):
        ok = np.nonzero(clear[u0:u0 + unit] & up[u0:u0 + unit])[0]                 # an upright one where the unit has one: then one defect serves
        j = u0 + int(ok[0] if len(ok) else np.nonzero(clear[u0:u0 + unit])[0][0])
        t = corner[j] + (1 if up[j] else -2)
        out.append((j, (int(t[0]), int(t[1])), bool(up[j])))
    return out


def twin_case(level, fmt, part=0, parts=1, true_twins=False, first="untouched"):
    """the untouched triangle and one moved copy per swept unit (of this part of the units), each with a defect inside another opaque micro-triangle:
    near twins, every one a descriptor of its own.  true_twins: the copies are moved so that no defect comes near: exact duplicates by digest, one
    descriptor, every triangle pointing at the lowest work item.  first: the untouched triangle leads the input or ends it"""
    all_targets = twin_targets(level, fmt)
    tex, E, d_up, d_down, home = twin_layout(level, not all(up for j, t, up in all_targets))
    targets = all_targets[part::parts]
    tris = []
    for k, (j, t, up) in enumerate(targets):
        if true_twins:
            origin = (12 * (k % ((tex.shape[1] - E) // 12)), home[1] + (k // 64) % 8)
        else:
            d = d_up if up else d_down
            origin = (d[0] - t[0], d[1] - t[1])
        tris.append(twin_triangle(tex, E, origin))
    a = twin_triangle(tex, E, home)
    uv = np.array(([a] + tris) if first == "untouched" else (tris + [a]), F)
    if true_twins:
        uv = np.unique(uv, axis=0)[np.random.default_rng(level).permutation(len(np.unique(uv, axis=0)))]
    c = make_case("twins-L%d-fmt%d-part%d-%s-%s" % (level, fmt, part, "true" if true_twins else "near", first), tex, uv, level, fmt=fmt, flags=ot.FLAG_THREADS,
                  promo=ot.PROMO_FORCE_TRANSPARENT)
    c["targets"] = [j for j, t, up in targets]
    c["untouched"] = 0 if first == "untouched" else len(uv) - 1
    return c


def twin_parts(level):
    """slices of a level's units, so that the oracle's side of one case stays short"""
    return {8: 4, 9: 8}.get(level, 1)


TWIN_CASES = [(L, f, p) for f in FORMATS for L in TWIN_LEVELS[f] for p in range(twin_parts(L))]


def twin_differences(case, inp):
    """per moved copy: the micro-triangles in which its states differ from the untouched triangle's"""
    (L, (ids, S)), = inp["groups"].items()
    a = S[case["untouched"]]
    return [np.nonzero(S[i] != a)[0] for i in range(len(S)) if i != case["untouched"]]


@functools.lru_cache(maxsize=None)
def _ut_uo_pool():
    uv, _ = ot.random_triangles(411, 6000, 0.02)
    lv = (1 + ot.hash_u32(np.arange(6000) + 1) % 2).astype(np.uint8)
    return uv.reshape(-1, 6), lv


def ut_uo_case(oracle, pairs=12):
    """work items whose blocks differ only by UT against UO in some micro-triangles (one digest, different bytes): found in the oracle's decode of 6000
    small level-1 and level-2 triangles over noise under the Nearest promotion, which yields both unknown states.  Returns the case of the pairs'
    triangles (the second members first in one half of the pairs) between 200 other triangles of the pool, and the pairs as triangle numbers"""
    uv, lv = _ut_uo_pool()
    probe = make_case("ut-uo-pool", noise(), uv, 2, levels=lv, fmt=ot.FMT_4STATE, flags=RAW_FLAGS, filt=ot.LINEAR)
    inp = tail_inputs(probe, bake(oracle, probe))
    rs = restate_tail(inp, RAW_FLAGS)
    rows = {}
    for L, (ids, S) in inp["groups"].items():
        for i, row in zip(ids.tolist(), S):
            rows[i] = row
    by_digest, found, taken = {}, [], set()
    for i in range(len(uv)):
        if rs["uniform"][i] or not (rows[i] <= ot.O).any():
            continue
        dg = int(rs["digest"][i])
        if dg in taken:
            continue
        for j in by_digest.setdefault(dg, []):
            if not np.array_equal(rows[i], rows[j]):
                found.append((j, i))
                taken.add(dg)
                break
        else:
            by_digest[dg].append(i)
        if len(found) == pairs:
            break
    others = [i for i in range(len(uv)) if int(rs["digest"][i]) not in taken][:200]
    order = list(others)
    for k, (a, b) in enumerate(found):
        first, second = (a, b) if k % 2 == 0 else (b, a)
        order.insert(7 * k, first)
        order.append(second)
    c = make_case("ut-uo-pairs", noise(), uv[order], 2, levels=lv[order], fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS, filt=ot.LINEAR)
    pos = {t: n for n, t in enumerate(order)}
    c["pairs"] = [tuple(sorted((pos[a], pos[b]))) for a, b in found]
    return c


# ---- near twins that share their level-5 preview (the early list of a streamed bake) ----
EARLY_LEVEL, EARLY_PERIOD, EARLY_COPIES = 6, 512, 3          # (eight periods: a power of two wide, so that every coordinate is exact)


@functools.lru_cache(maxsize=None)
def _early_tile():
    """one period: an opaque disc on a transparent ground, eight periods side by side"""
    yy, xx = np.mgrid[0:EARLY_PERIOD, 0:EARLY_PERIOD]
    tile = np.where((xx - 200) ** 2 + (yy - 200) ** 2 < 150 ** 2, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.tile(tile, (1, 8)))


def _disc_twins(oracle, name, copies, gt, wanted):
    """a level-6 right triangle over the disc of period 0 and `copies` copies of it over the next periods, each with one texel made transparent
    strictly inside a level-6 micro-triangle that lies wholly inside the disc.  wanted(k) says whether copy k needs a micro-triangle whose level-5
    ancestor touches the disc's edge (the block changes in that micro-triangle, the level-5 preview does not) or one whose ancestor lies inside the
    disc as well.  60 other level-6 triangles spread the input over the ranges.  Returns (texture, twins, others, changed micro-triangles)"""
    L, P = EARLY_LEVEL, EARLY_PERIOD
    tile = _early_tile()
    E = TWIN_S * 2 ** L
    home = (8, 8)
    kw = dict(fmt=ot.FMT_4STATE, flags=RAW_FLAGS, promo=ot.PROMO_FORCE_TRANSPARENT, gt=gt)
    a = twin_triangle(tile, E, home)
    states = {}
    for lvl in (L, 5):
        probe = make_case("%s-probe%d" % (name, lvl), tile, a, lvl, **kw)
        states[lvl] = tail_inputs(probe, bake(oracle, probe))["groups"][lvl][1][0]
    idx = np.arange(4 ** L)
    v = lu.micro_vertices(idx, np.full(4 ** L, L))
    corner = np.rint(v[:, 0] * 2 ** L).astype(np.int64) * TWIN_S
    up = v[:, 1, 0] > v[:, 0, 0]
    texel = corner + np.where(up, 1, -2)[:, None] + np.array(home)[None, :]
    inside = (states[L] == gt) & (tile[texel[:, 1], texel[:, 0]] == 255)
    ancestor = states[5][idx >> (2 * (L - 5))]
    pools = {True: np.nonzero(inside & (ancestor == ot.UT))[0], False: np.nonzero(inside & (ancestor == gt))[0]}
    tex = tile.copy()
    twins, picks = [a], []
    for k in range(copies):
        pool = pools[bool(wanted(k))]
        u = int(pool[(len(pool) - 1) * (k + 1) // (copies + 1)])
        picks.append(u)
        tex[texel[u, 1], texel[u, 0] + (k + 1) * P] = 0
        twins.append(twin_triangle(tex, E, (home[0] + (k + 1) * P, home[1])))
    rng = np.random.default_rng(66)
    others = [twin_triangle(tex, E, (int(x), int(y))) for x, y in zip(rng.integers(0, tex.shape[1] - E, 60), rng.integers(20, 120, 60))]
    return tex, twins, others, picks


def early_twin_case(oracle):
    """a streamed bake classifies early every item of level >= 6 whose level-5 preview is mixed and shared with another item.  Here: the untouched
    triangle and three copies that differ from it in one level-6 micro-triangle each and share its preview.  c["twins"]: the four triangles;
    c["targets"]: the changed micro-triangles"""
    tex, twins, others, picks = _disc_twins(oracle, "early", EARLY_COPIES, ot.O, lambda k: True)
    uv = np.array(others[:20] + twins[:2] + others[20:40] + twins[2:] + others[40:], F)
    c = make_case("early-twins", tex, uv, EARLY_LEVEL, fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS, promo=ot.PROMO_FORCE_TRANSPARENT)
    c["twins"], c["targets"] = [20, 21, 42, 43], picks
    return c


UT_UO_COPIES = 6


def ut_uo_streamed_case(oracle):
    """level-6 blocks that differ only by UT against UO, so that they stream: alpha above the cut-off maps to UO (alphaCutoffGreater), below to T,
    unknown micro-triangles are forced to UT.  The untouched triangle over the disc holds all three; each of six copies has one micro-triangle
    inside the disc turned from UO to UT by a transparent texel: one digest, different bytes.  Three copies share the untouched triangle's level-5
    preview (a streamed bake classifies them early), three do not.  A copy leads the input, the untouched triangle follows 20 triangles later, the
    other copies lie further on: the first copy keeps the block.  c["twins"]: their triangles in input order; c["targets"]: per twin the changed
    micro-triangle, None for the untouched one"""
    tex, twins, others, picks = _disc_twins(oracle, "ut-uo", UT_UO_COPIES, ot.UO, lambda k: k % 2 == 0)
    uv = np.array(twins[1:2] + others[:20] + twins[:1] + twins[2:4] + others[20:40] + twins[4:] + others[40:], F)
    c = make_case("ut-uo-streamed", tex, uv, EARLY_LEVEL, fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS, promo=ot.PROMO_FORCE_TRANSPARENT, gt=ot.UO)
    c["twins"], c["targets"] = [0, 21, 22, 23, 44, 45, 46], [picks[0], None] + picks[1:]
    return c
