"""Case list of test_small_textures_gpu.py: bakes over textures smaller than the kernels' own windows, thin and long ones, and mip chains
down to 1x1.  Every shape runs with every address mode, every extent and every level; the filter and SAT on / off are a seeded pick per bake
(as test_gpu_parity._fuzz_case picks), the texture format alternates.  What the pick must still cover is asserted by
test_small_textures_gpu.py::test_case_list_coverage, without a GPU."""
import numpy as np
import ommtest as ot

# (w, h)
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5),        # tiny
          (31, 33), (33, 31),                            # around the 32x32 window of classify_tiles
          (63, 65),                                      # around a 64 edge
          (1, 4096), (4096, 1), (5, 1000)]               # thin and long
ADDRS = [ot.WRAP, ot.MIRROR, ot.CLAMP, ot.BORDER, ot.MIRROR_ONCE]
ADDR_NAMES = ["wrap", "mirror", "clamp", "border", "mirror_once"]
UV_LO, UV_HI = -3.5, 4.5
LOW_LEVELS, HIGH_LEVELS = [0, 2, 5], [6, 7]
CUTOFF = 0.5
BORDER_ALPHA = 0.4


def _h(seed, k):
    return int(ot.hash_u32(np.array([seed * 193 + k], dtype=np.int64))[0])


def noise_texture(seed, w, h, fp32):
    """value noise whose cells are 3 texels and 1 texel, stretched around its own median, which lands on the cut-off: features of 1-3 texels, half the texels
    on either side however few there are, most rectangles mixed"""
    t = ot.value_noise(seed, w, h, octaves=2, base_cell=3)
    t = np.clip((t - np.float32(np.median(t))) * np.float32(3.0) + np.float32(0.5), np.float32(0), np.float32(1)).astype(np.float32)
    return np.ascontiguousarray(t if fp32 else (t * np.float32(255)).astype(np.uint8))


def extents(w, h):
    """UV extents of the triangles and how many: about one texel, about the whole texture, about 3 UV units (at low levels one micro-triangle's
    texel rectangle wraps the texture more than once and no level of the hierarchy is free of seams)"""
    return [("texel", 1.5 / max(w, h), 60), ("texture", 1.0, 60), ("wraps", 3.0, 20)]


def bakes_of(case_index, w, h):
    """[(extent name, extent, triangles, level, filter, sat, knobs)] of one (shape, address mode) case"""
    out = []
    for e, (name, ext, n) in enumerate(extents(w, h)):
        for li, level in enumerate(LOW_LEVELS + (HIGH_LEVELS if name != "wraps" else [])):
            filt = [ot.LINEAR, ot.NEAREST][_h(case_index, 30 + 8 * e + li) % 2]
            sat = bool(_h(case_index, 70 + 8 * e + li) % 2)
            # level 7: both homes of the generic texel-loop pass (ommxBakerKnob_GenericPass), as test_micro_triangles_of_several_texels runs them
            for knobs in ([((ot.KNOB_GENERIC_PASS, 1),), ((ot.KNOB_GENERIC_PASS, 2),)] if level == 7 else [()]):
                out.append((name, ext, n, level, filt, sat, knobs))
    return out


def cases():
    """[(id, index, (w, h), addr, fp32)]: every shape with every address mode; the texture format alternates along the list"""
    out = []
    for s, (w, h) in enumerate(SHAPES):
        for a, addr in enumerate(ADDRS):
            i = s * len(ADDRS) + a
            out.append(("%dx%d-%s" % (w, h, ADDR_NAMES[a]), i, (w, h), addr, bool((s + a) & 1)))
    return out


def triangles(case_index, e, n, ext):
    return ot.random_triangles(5000 + 7 * case_index + e, n, ext, lo=UV_LO, hi=UV_HI)


def run_case(both, product, oracle, case):
    """every bake of one case through `both` (test_gpu_parity.both: product == oracle on every array, histogram and ommDebugGetStats2)"""
    _, i, (w, h), addr, fp32 = case
    tex = noise_texture(300 + i, w, h, fp32)
    names = [x[0] for x in extents(w, h)]
    for (name, ext, n, level, filt, sat, knobs) in bakes_of(i, w, h):
        uv, ix = triangles(i, names.index(name), n, ext)
        both(product, oracle, [tex], uv, ix, level, sat=sat, cutoff=CUTOFF, knobs=knobs, addr=addr, filt=filt,
             border_alpha=BORDER_ALPHA, promo=[ot.PROMO_NEAREST, ot.PROMO_FORCE_OPAQUE, ot.PROMO_FORCE_TRANSPARENT][(i + level) % 3])


# ---- mip chains ----
def halve(t):
    """next mip: box filter over the 2x2 (at a dimension of 1: 2x1 / 1x2) blocks that exist; an odd last row / column is dropped (300x200 -> ... -> 37x25 -> 18x12)"""
    h, w = t.shape
    nh, nw = max(1, h // 2), max(1, w // 2)
    f = t.astype(np.float32)
    rows = (f[0:2 * nh:2] + f[1:2 * nh:2]) * np.float32(0.5) if h > 1 else f
    out = (rows[:, 0:2 * nw:2] + rows[:, 1:2 * nw:2]) * np.float32(0.5) if w > 1 else rows
    return np.ascontiguousarray(out.astype(np.float32) if t.dtype == np.float32 else (out + np.float32(0.5)).astype(np.uint8))


def chain(w, h, fp32, seed):
    mips = [noise_texture(seed, w, h, fp32)]
    while mips[-1].shape != (1, 1):
        mips.append(halve(mips[-1]))
    return mips


CHAINS = [("pow2", 64, 64, [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]),
          ("odd", 300, 200, [(300, 200), (150, 100), (75, 50), (37, 25), (18, 12), (9, 6), (4, 3), (2, 1), (1, 1)])]


def chain_cases():
    """[(id, name, w, h, sat, addr, fp32)]"""
    out = []
    for c, (name, w, h, _) in enumerate(CHAINS):
        for s, sat in enumerate([True, False]):
            for a, addr in enumerate([ot.WRAP, ot.CLAMP]):
                out.append(("%s-%s-%s" % (name, "sat" if sat else "nosat", ADDR_NAMES[ADDRS.index(addr)]), name, w, h, sat, addr, bool((c + s + a) & 1)))
    return out


def run_chain_case(both, product, oracle, case):
    _, name, w, h, sat, addr, fp32 = case
    mips = chain(w, h, fp32, 900 + w)
    for e, (ext, n, level) in enumerate([(1.5 / w, 60, 5), (0.15, 60, 5), (1.0, 60, 6), (3.0, 20, 2)]):
        uv, ix = ot.random_triangles(7000 + e, n, ext, lo=UV_LO, hi=UV_HI)
        both(product, oracle, mips, uv, ix, level, sat=sat, cutoff=CUTOFF, addr=addr, filt=[ot.LINEAR, ot.NEAREST][e & 1],
             border_alpha=BORDER_ALPHA, promo=ot.PROMO_NEAREST)
