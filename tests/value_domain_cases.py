"""Case list of test_value_domain_gpu.py: bakes whose texel values, cut-offs and UV coordinates leave the range every other generator of the suite
stays in (alpha in [0, 1], cut-offs 0.25 .. 0.8, |pixel coordinate| < 2^31).  Plain module, no fixtures; the audits (test_edge_prefilter_audit.py,
test_region_curve_audit.py) bake the same inputs through the audit build of the oracle.

An INPUT is a texture (one or two mips) with its cut-off; every input is baked along five PATHS, each chosen by construction:
    fast7     level 7 on triangles of 20 .. 60 texels: micro-triangles smaller than a texel, the single-texel pass
    gen5k1    level 5 on triangles of 32 .. 128 texels (micro-triangles of 1 .. 4 texels across), the generic pass inside the persistent launch
    gen5k2    the same triangles, the deferred generic pass
    coarse0   level 0 on triangles of 0.5 .. 0.9 UV: one micro-triangle over much of the texture
    coarse3   level 3 on the same triangles: the coarse / tile path, summed-area-table queries over large rectangles
Triangle centres lie in UV [-0.3, 1.3], so part of every stream reaches over the texture's edge (a seam joins the last row / column to the first under Wrap,
to itself under Clamp, to borderAlpha under Border).  Filter, format, promotion, address mode, borderAlpha and -- where the input leaves it open -- the
summed-area table rotate with the input and the path; test_value_domain_gpu.py::test_case_list_coverage proves what the pick reaches, without a GPU.

Level-0 bakes and inputs whose texels all lie on one side of the cut-off (UNORM8 with cut-off >= 1.0) run with DisableSpecialIndices, so that their triangles
get a block the comparison can look at instead of a special index.  An all-NaN texture keeps special indices: it is the one case that must produce nothing else.

Dropped from parity (the reference's behaviour is undefined there, DESIGN.md "documented fences"): Mirror and MirrorOnce addressing of pixel coordinates
beyond the int range -- util/texture.h negates / takes abs() of INT_MIN."""
import numpy as np
import ommtest as ot
import sat_util as su

F = np.float32
ADDRS = [ot.WRAP, ot.CLAMP, ot.BORDER]
ADDR_NAMES = {ot.WRAP: "wrap", ot.CLAMP: "clamp", ot.BORDER: "border"}
FILTERS = [ot.LINEAR, ot.NEAREST]
FORMATS = [ot.FMT_2STATE, ot.FMT_4STATE]
PROMOS = [ot.PROMO_NEAREST, ot.PROMO_FORCE_OPAQUE, ot.PROMO_FORCE_TRANSPARENT]
BORDER_KINDS = ["cutoff", "cutoff+ulp", "cutoff-ulp", "-2", "7"]
SHAPES = [(64, 64), (96, 80), (32, 32), (128, 128)]          # (w, h)
PATHS = ["fast7", "gen5k1", "gen5k2", "coarse0", "coarse3"]
NO_SPECIAL = ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL
QNAN, SNAN, NEG_NAN = 0x7FC00000, 0x7FA00000, 0xFFC00001


def bits_f32(word):
    return np.array([word], np.uint32).view(np.float32)[0]


def base_field(seed, w, h):
    """the one smooth field: value noise with cells of 8 and 4 texels, stretched around its median (0.5 after the stretch), clipped to [0, 1]: half the texels on
    either side of 0.5, plateaus at 0 and 1"""
    t = ot.value_noise(seed, w, h, octaves=2, base_cell=8)
    return np.clip((t - F(np.median(t))) * F(3.0) + F(0.5), F(0), F(1)).astype(np.float32)


def border_alpha(kind, cutoff):
    c = F(cutoff)
    return float({"cutoff": c, "cutoff+ulp": su.ulp_up(c), "cutoff-ulp": su.ulp_down(c), "-2": F(-2.0), "7": F(7.0)}[kind])


# ---- FP32 value families ----
def plateau_texture(base, cutoff):
    """blocks of 4 x 4 texels: the cut-off, one ulp above, one ulp below (cut-off 0: also -0.0 against +0.0) and ordinary texels; horizontal neighbours differ
    by one kind, vertical ones by two, so every kind has an edge with every other and whole cells have four equal corners"""
    c = F(cutoff)
    kinds = [c, su.ulp_up(c), su.ulp_down(c)] + ([F(-0.0)] if c == 0 else [])
    h, w = base.shape
    by, bx = np.mgrid[0:h, 0:w] // 4
    k = (bx + 2 * by) % (len(kinds) + 1)
    out = (base - F(0.5) if c == 0 else base).astype(np.float32)
    for i, v in enumerate(kinds):
        out[k == i] = v
    return np.ascontiguousarray(out)


def scaled_plateau_texture(base, cutoff, scale):
    """the cut-off, +-1 and +3 ulp, +-1e-3 and +-0.03 of it in blocks of 2 x 2 texels beside texels up to `scale` away on either side: cells with a corner next
    to the cut-off whose S = |ha| + |hb| + |hc| + |hd| is thousands -- where an error bound that does not scale with the patch is too small"""
    c = F(cutoff)
    vals = [c, su.ulp_up(c), su.ulp_down(c), su.ulp_up(su.ulp_up(su.ulp_up(c))), c + F(1e-3), c - F(1e-3), c + F(0.03), c - F(0.03)]
    h, w = base.shape
    by, bx = np.mgrid[0:h, 0:w] // 2
    k = (bx * 3 + by * 5) % (len(vals) + 4)
    out = ((base - F(0.5)) * F(2 * scale) + c).astype(np.float32)
    for i, v in enumerate(vals):
        out[k == i] = v
    return np.ascontiguousarray(out)


def with_value(base, arrangement, value, seed):
    """`value` (a float32, possibly a NaN with a payload) put into the base field: single texels (3 %), row 0 in full, the last column in full, 2 x 2 blocks
    (one of them over the corner texel 0, 0).  Row 0 and the last column are what a seam joins to ordinary texels."""
    out = base.copy()
    h, w = out.shape
    word = np.array([value], np.float32).view(np.uint32)[0]
    u = out.view(np.uint32)
    if arrangement == "single":
        mask = ot.hash_u32(np.arange(w * h, dtype=np.int64) + seed * 7919).reshape(h, w) % 100 < 3
        u[mask] = word
    elif arrangement == "row":
        u[0, :] = word
    elif arrangement == "col":
        u[:, w - 1] = word
    elif arrangement == "block":
        for (x, y) in [(0, 0), (w // 2, h // 3), (w // 3, h // 2 + 1), (w - 2, h - 2), (5, h - 7)]:
            u[y:y + 2, x:x + 2] = word
    else:
        raise ValueError(arrangement)
    return out


def nan_bits_texture(base):
    """quiet, signalling and sign-bit-set NaNs as single texels among ordinary ones (the bit patterns survive: written through a uint32 view)"""
    out = base.copy()
    h, w = out.shape
    sel = ot.hash_u32(np.arange(w * h, dtype=np.int64) + 4242).reshape(h, w) % 40
    u = out.view(np.uint32)
    for i, word in enumerate([QNAN, SNAN, NEG_NAN]):
        u[sel == i] = word
    return out


def halve(t):
    return ((t[0::2, 0::2] + t[1::2, 0::2]) + t[0::2, 1::2] + t[1::2, 1::2]) * F(0.25)


# ---- UNORM8 ----
UNORM8_KS = [1, 127, 128, 254]


def unorm8_texture(k, w, h, seed):
    """bytes k - 1, k, k + 1 (clipped to 0 .. 255): the left half in plateaus of 3 x 3 texels, the right half as 1-texel noise"""
    vals = np.array(sorted({max(k - 1, 0), k, min(k + 1, 255)}), np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    blocks = ot.hash_u32(((x // 3) + (y // 3) * 1000 + seed * 77).astype(np.int64)) % len(vals)
    noise = ot.hash_u32((x + y * 1000 + seed * 131 + 500000).astype(np.int64)) % len(vals)
    return np.ascontiguousarray(vals[np.where(x < w // 2, blocks, noise)])


def unorm8_cutoffs():
    """[(name, k of the texture, cut-off)]: 0.0, 1.0, k * (1 / 255) in float32 -- the value Load() produces, so texel == cut-off exactly -- and one above 1.0"""
    out = [("c0", 0, F(0.0)), ("c1", 255, F(1.0))]
    out += [("k%d" % k, k, F(k) * F(1.0 / 255.0)) for k in UNORM8_KS]
    out += [("c1.5", 254, F(1.5))]
    return out


# ---- inputs ----
def inputs():
    """[dict(name, family, index, mips, cutoff, sat (True / False / None = picked per bake), flags, special_only)]"""
    out = []

    def add(name, family, mips, cutoff, sat=None, flags=ot.FLAG_THREADS, special_only=False):
        out.append(dict(name=name, family=family, index=len(out), mips=[np.ascontiguousarray(m) for m in mips], cutoff=float(F(cutoff)), sat=sat, flags=flags,
                        special_only=special_only))

    def base(i):
        w, h = SHAPES[i % len(SHAPES)]
        return base_field(40 + i, w, h)

    b = base(0); add("sdf-c0", "sdf", [(b - F(0.5)) * F(100)], 0.0, sat=True)
    b = base(1); add("sdf-neg", "sdf", [(b - F(0.5)) * F(100)], -3.0, sat=True)      # a negative cut-off: the texture gets no table whatever `sat` says
    # (two of each of the next three, on consecutive indices: the rotation of bakes_of() then gives every path of the family both filters)
    for k, suffix in enumerate(("", "-b")):
        b = base(2 + k); add("hdr" + suffix, "hdr", [b * F(1e4)], 100.0)
    for k, suffix in enumerate(("", "-b")):
        b = base(4 + k); add("huge" + suffix, "huge", [((b.astype(np.float64) - 0.5) * 6e38).astype(np.float32)], 0.0)      # (6e38 is no float32: the product is formed in float64)
    for k, suffix in enumerate(("", "-b")):
        b = base(6 + k); add("denormal" + suffix, "denormal", [b * F(1e-40)], 5e-41)
    b = base(8); add("plateau-0.5", "plateau", [plateau_texture(b, 0.5)], 0.5)
    b = base(9); add("plateau-0.0", "plateau", [plateau_texture(b, 0.0)], 0.0)
    n = 10
    for vname, v in (("nan", F(np.nan)), ("pinf", F(np.inf)), ("ninf", F(-np.inf))):
        for arr in ("single", "row", "col", "block"):
            add("%s-%s" % (vname, arr), "nonfinite", [with_value(base(n), arr, v, n)], 0.5); n += 1
    add("nan-bits", "nonfinite", [nan_bits_texture(base(n))], 0.5); n += 1
    add("all-nan", "nonfinite", [np.full((64, 64), np.nan, np.float32)], 0.5, special_only=True); n += 1
    m0 = base_field(40 + n, 64, 64)
    m1 = with_value(with_value(with_value(halve(m0), "single", F(np.nan), n), "row", F(np.inf), n), "col", F(-np.inf), n)
    add("mip1-nonfinite", "nonfinite", [m0, m1], 0.5, sat=False); n += 1
    for (name, k, c) in unorm8_cutoffs():
        w, h = SHAPES[n % len(SHAPES)]
        add("unorm8-" + name, "unorm8", [unorm8_texture(k, w, h, n)], c, flags=NO_SPECIAL if c >= 1.0 else ot.FLAG_THREADS); n += 1
    # plateaus at the cut-off inside HDR- and SDF-scale values (appended: the indices above, and with them every rotation, stay as they are)
    add("hdr-plateau", "plateau", [scaled_plateau_texture(base_field(91, 96, 80), 100.0, 1e4)], 100.0); n += 1
    add("sdf-plateau", "plateau", [scaled_plateau_texture(base_field(93, 128, 128), 0.0, 100.0)], 0.0); n += 1
    return out


def tris(seed, n, ext_lo, ext_hi, lo=-0.3, hi=1.3):
    """n triangles, unshared vertices: centre ~ U[lo, hi)^2, vertices = centre + U(-e/2, e/2)^2 with e ~ U[ext_lo, ext_hi) per triangle"""
    e = ot.uniform01(seed, n, 9) * F(ext_hi - ext_lo) + F(ext_lo)
    cx = ot.uniform01(seed, n, 0) * F(hi - lo) + F(lo)
    cy = ot.uniform01(seed, n, 1) * F(hi - lo) + F(lo)
    uv = np.empty((n, 3, 2), np.float32)
    for v in range(3):
        uv[:, v, 0] = cx + (ot.uniform01(seed, n, 2 + 2 * v) - F(0.5)) * e
        uv[:, v, 1] = cy + (ot.uniform01(seed, n, 3 + 2 * v) - F(0.5)) * e
    return uv.reshape(-1, 2), np.arange(3 * n, dtype=np.uint32)


def path_triangles(path, index, w, h):
    """(uv, ix, level, knobs) of one path over a w x h texture"""
    s = float(max(w, h))
    if path == "fast7":
        return tris(8000 + index, 40, 20.0 / s, 60.0 / s) + (7, ())
    if path in ("gen5k1", "gen5k2"):
        return tris(8100 + index, 40, 32.0 / s, 128.0 / s) + (5, ((ot.KNOB_GENERIC_PASS, 1 if path == "gen5k1" else 2),))
    if path in ("coarse0", "coarse3"):
        return tris(8200 + index, 60, 0.5, 0.9) + (0 if path == "coarse0" else 3, ())
    raise ValueError(path)


def bakes_of(inp):
    """[dict(path, uv, ix, level, knobs, sat, kw)] of one input; kw goes to ommtest.make_desc"""
    i = inp["index"]
    h, w = inp["mips"][0].shape
    out = []
    for p, path in enumerate(PATHS):
        uv, ix, level, knobs = path_triangles(path, i, w, h)
        # the rotation: over the five paths of ONE input every filter, format, promotion and address mode occurs, and so it does over the inputs of one path
        addr = ADDRS[(i + p + p // 3) % 3]
        bkind = BORDER_KINDS[(2 * i + p) % 5]
        sat = inp["sat"] if inp["sat"] is not None else bool((i + p // 2) % 2)
        kw = dict(filt=FILTERS[(i + p) % 2], fmt=FORMATS[(i + (p + 1) // 2) % 2], promo=PROMOS[(i + p) % 3], addr=addr,
                  border_alpha=border_alpha(bkind, inp["cutoff"]), flags=NO_SPECIAL if level == 0 else inp["flags"])
        out.append(dict(path=path, uv=uv, ix=ix, level=level, knobs=knobs, sat=sat, border_kind=bkind, kw=kw))
    return out


def run_input(both, product, oracle, inp):
    """every bake of one input through `both` (test_gpu_parity.both: product == oracle on every array, histogram and ommDebugGetStats2)"""
    for b in bakes_of(inp):
        both(product, oracle, inp["mips"], b["uv"], b["ix"], b["level"], sat=b["sat"], cutoff=inp["cutoff"], knobs=b["knobs"], **b["kw"])


# ---- UV values ----
UV_TEX_SEED, UV_CUTOFF = 77, 0.5


def uv_texture():
    return base_field(UV_TEX_SEED, 64, 64)


def zero_sign_triangles():
    """pairs of triangles whose coordinates differ only in the sign of a zero -- (0.0, 0.25) against (-0.0, 0.25) -- next to each other in the stream; every
    fifth pair has all three vertices on an axis (a degenerate item).  The reference hashes +-0 to 0: a pair is ONE work item, owned by its first triangle."""
    n = 20
    uv, _ = tris(8300, n, 0.3, 0.8, lo=0.0, hi=0.6)
    t = np.abs(uv.reshape(n, 3, 2))
    for i in range(n):
        axis = i & 1
        t[i, i % 3, axis] = 0.0                      # one vertex on an axis
        if i % 4 == 1:
            t[i, (i + 1) % 3, 1 - axis] = 0.0        # ... a second one on the other axis
        if i % 5 == 4:
            t[i, :, axis] = 0.0                      # all three on one axis
    pairs = np.empty((n, 2, 3, 2), np.float32)
    pairs[:, 0] = t
    neg = t.copy(); neg[neg == 0.0] = F(-0.0)
    pairs[:, 1] = neg
    pairs[1::2] = pairs[1::2, ::-1]                  # in every other pair the -0.0 triangle comes first
    uv = pairs.reshape(-1, 2)
    assert np.array_equal(uv.reshape(n, 2, 6)[:, 0], uv.reshape(n, 2, 6)[:, 1]) and not np.array_equal(np.signbit(uv.reshape(n, 2, 6)[:, 0]), np.signbit(uv.reshape(n, 2, 6)[:, 1]))
    return uv, np.arange(uv.shape[0], dtype=np.uint32)


def tiny_triangles():
    """40 ordinary triangles with one vertex moved to denormal / tiny coordinates (1e-40, 1e-30, with either sign), and 10 that lie entirely within [0, 1e-30]"""
    uv, _ = tris(8400, 40, 0.3, 0.8, lo=0.1, hi=0.7)
    t = uv.reshape(40, 3, 2)
    small = [F(1e-40), F(1e-30), F(-1e-40), F(-1e-30), F(0.0)]
    for i in range(40):
        t[i, i % 3] = (small[i % 5], small[(i // 5) % 5])
    tiny = np.empty((10, 3, 2), np.float32)
    for i in range(10):
        tiny[i] = [(0.0, 0.0), (F(1e-30) * F(i + 1) / F(10), F(1e-40) * F(i)), (F(1e-40) * F(3 * i), F(1e-30) * F(10 - i) / F(10))]
    uv = np.concatenate([t.reshape(-1, 2), tiny.reshape(-1, 2)]).astype(np.float32)
    return uv, np.arange(uv.shape[0], dtype=np.uint32)


OVERFLOW_SIZE = 64          # texture width = height of the overflow cases
INT_LIMIT = 2.0 ** 31


def grid_triangles(seed, n, ox, oy, kmax):
    """n triangles on the float32 grid at the offsets: vertex = offset + k * ulp(offset), k in 0 .. kmax (a random triangle shifted by such an offset
    collapses to a point); triangles whose three grid points are collinear are replaced by a fixed right triangle"""
    ulx, uly = np.spacing(F(abs(ox))), np.spacing(F(abs(oy)))
    k = (ot.hash_u32(np.arange(n * 6, dtype=np.int64) + seed * 1000003) % (kmax + 1)).reshape(n, 3, 2).astype(np.int64)
    area2 = (k[:, 1, 0] - k[:, 0, 0]) * (k[:, 2, 1] - k[:, 0, 1]) - (k[:, 2, 0] - k[:, 0, 0]) * (k[:, 1, 1] - k[:, 0, 1])
    k[area2 == 0] = [[0, 0], [kmax, 0], [0, kmax]]
    uv = np.empty((n, 3, 2), np.float64)
    uv[:, :, 0] = ox + np.sign(ox) * k[:, :, 0] * float(ulx)
    uv[:, :, 1] = oy + np.sign(oy) * k[:, :, 1] * float(uly)
    uv32 = uv.astype(np.float32)
    assert np.array_equal(uv32.astype(np.float64), uv)       # on the grid: nothing was rounded
    return uv32.reshape(-1, 2), np.arange(3 * n, dtype=np.uint32)


def overflow_cases():
    """[dict(name, regime, uv, ix, level, addr)] over the 64 x 64 texture.
    (a) every pixel coordinate below 2^31 - 2^16 in magnitude, every UV above the 16384 threshold of the single-texel pass;
    (b) every pixel coordinate of every vertex at or above 2^32 in magnitude: every float -> int conversion of the bake gives INT_MIN."""
    out = []
    s = float(OVERFLOW_SIZE)
    two25 = 2.0 ** 25
    specs = [("a-2p22", "a", 2.0 ** 22, 2.0 ** 22, 6, 3), ("a-neg", "a", -(2.0 ** 22), 2.0 ** 21, 6, 4), ("a-near-limit", "a", two25 - 1024.0 - 16.0, -(two25 - 1024.0 - 16.0), 3, 4),
             ("b-pos", "b", 2.0 ** 26, 2.0 ** 27, 5, 3), ("b-neg", "b", -(2.0 ** 26), -(2.0 ** 28), 5, 4), ("b-mixed-axes", "b", 2.0 ** 30, -(2.0 ** 26), 5, 3)]
    for n, (name, regime, ox, oy, kmax, level) in enumerate(specs):
        if name == "a-near-limit":   # towards zero from just under the limit: k counts downwards in magnitude
            uv, ix = grid_triangles(8500 + n, 40, ox - np.sign(ox) * 2 * kmax, oy - np.sign(oy) * 2 * kmax, kmax)
        else:
            uv, ix = grid_triangles(8500 + n, 40, ox, oy, kmax)
        for a, addr in enumerate(ADDRS):
            out.append(dict(name="%s-%s" % (name, ADDR_NAMES[addr]), regime=regime, uv=uv, ix=ix, level=level, addr=addr,
                            filt=FILTERS[(n + a) % 2], fmt=FORMATS[(n + a // 2) % 2], promo=PROMOS[(n + a + 2) % 3], sat=bool((n + a) % 2)))
        check_overflow_rules(uv, regime, s)
    return out


def check_overflow_rules(uv, regime, size):
    """the safety rules of the overflow cases, in float64, for every vertex pair of every triangle: no triangle has pixel coordinates on both sides of 2^31 or of
    -2^31 in either axis (a loop bound pair (valid, INT_MIN) is not an input of this suite), and each regime is what it says"""
    p = uv.astype(np.float64).reshape(-1, 3, 2) * size           # pixel coordinates; the kernels' "- 0.5" and floor / ceil move them by less than 2
    for axis in (0, 1):
        for i in range(3):
            for j in range(3):
                a, b = p[:, i, axis], p[:, j, axis]
                assert not np.any((a < INT_LIMIT) & (b >= INT_LIMIT)), "a triangle straddles 2^31"
                assert not np.any((a >= -INT_LIMIT) & (b < -INT_LIMIT)), "a triangle straddles -2^31"
    if regime == "a":
        assert np.all(np.abs(p) <= INT_LIMIT - 2.0 ** 16) and np.all(np.abs(uv.astype(np.float64)) > 16384.0)
    else:
        assert np.all(np.abs(p) >= 2.0 ** 32)


def uv_cases():
    """[dict(name, group, uv, ix, level, levels, kw, knobs)] over uv_texture(), cut-off 0.5"""
    out = []
    zu, zi = zero_sign_triangles()
    nz = zi.size // 3
    same, diff = None, (np.arange(nz) % 2 * 2 + 3).astype(np.uint8)          # per-triangle levels 3 / 5: the two triangles of a pair differ
    for name, levels, flags in (("same-level", same, ot.FLAG_THREADS), ("same-level-nodedup", same, ot.FLAG_THREADS | ot.FLAG_NO_DEDUP),
                                ("levels-differ", diff, ot.FLAG_THREADS), ("levels-differ-nodedup", diff, ot.FLAG_THREADS | ot.FLAG_NO_DEDUP)):
        out.append(dict(name="zero-" + name, group="zero", uv=zu, ix=zi, level=5, levels=levels, knobs=(),
                        kw=dict(flags=flags, addr=ot.WRAP, filt=ot.LINEAR, fmt=ot.FMT_2STATE if flags & ot.FLAG_NO_DEDUP else ot.FMT_4STATE, promo=ot.PROMO_NEAREST), sat=True))
    tu, ti = tiny_triangles()
    for n, (filt, addr, level) in enumerate([(ot.LINEAR, ot.WRAP, 5), (ot.NEAREST, ot.CLAMP, 3), (ot.LINEAR, ot.BORDER, 7)]):
        out.append(dict(name="tiny-%d" % n, group="tiny", uv=tu, ix=ti, level=level, levels=None, knobs=(),
                        kw=dict(flags=ot.FLAG_THREADS, addr=addr, filt=filt, fmt=FORMATS[(n + 1) % 2], promo=PROMOS[n], border_alpha=0.4), sat=bool(n % 2)))
    # (far outside the texture Clamp and Border read one value, and where the float32 grid of the vertices is a whole UV unit or coarser every micro-triangle
    #  vertex wraps to the same texel: such triangles are uniform, and DisableSpecialIndices gives each a block to compare; regime (a) under Wrap on a finer
    #  grid is mixed and keeps the default)
    for c in overflow_cases():
        out.append(dict(name="overflow-" + c["name"], group="overflow-" + c["regime"], uv=c["uv"], ix=c["ix"], level=c["level"], levels=None, knobs=(),
                        kw=dict(flags=ot.FLAG_THREADS if (c["addr"] == ot.WRAP and float(np.spacing(np.abs(c["uv"]).max())) < 1.0) else NO_SPECIAL, addr=c["addr"], filt=c["filt"], fmt=c["fmt"], promo=c["promo"],
                                border_alpha=0.7), sat=c["sat"]))
    return out


def run_uv_case(both, product, oracle, case, tex=None):
    tex = uv_texture() if tex is None else tex
    return both(product, oracle, [tex], case["uv"], case["ix"], case["level"], sat=case["sat"], cutoff=UV_CUTOFF, knobs=case["knobs"], levels=case["levels"], **case["kw"])


# ---- what the coverage test and the audits need of the oracle alone ----
def oracle_bake(lib, mips, uv, ix, level, sat, cutoff, levels=None, **kw):
    b = lib.create_baker()
    t = lib.create_texture(b, mips, alpha_cutoff=cutoff if sat else -1.0)
    res = lib.bake(b, ot.make_desc(t, uv, ix, level, alpha_cutoff=cutoff, levels=levels, **kw))
    lib.destroy_texture(b, t)
    lib.destroy_baker(b)
    return res


def block_states(res):
    """set of (format, state) over every micro-triangle of every block of a result"""
    out = set()
    bits = np.unpackbits(res.array_data, bitorder="little")
    for (ofs, level, fmt) in res.descs:
        n = 4 ** int(level)
        b = bits[8 * int(ofs): 8 * int(ofs) + n * int(fmt)].reshape(n, int(fmt))
        states = b[:, 0] if fmt == 1 else b[:, 0] + 2 * b[:, 1]
        out |= {(int(fmt), int(s)) for s in np.unique(states)}
    return out
