"""Shared by tests/test_poisoned_memory_gpu.py and tests/test_poison_cases.py: the fill words of ommxBakerKnob_PoisonMemory and the case lists of the
poisoned runs, built without a device.  Every derived entry gets a PAIR of sources of equal descriptor and primitive counts: a decoy whose blocks are all
the same uniform block (every mark set, one hash key, every item uniform), and the real source whose blocks are all different.  The decoy goes first on
the poisoned baker, so that the scratch block of the real call is the decoy's, filled with the word on top.  tests/README_poison.md has the ledger."""
import numpy as np
import ommtest as ot
import coarsen_util as cu
import merge_util as mu
import lookup_util as lu

WORDS = [0x00000000, 0x00000001, 0xFFFFFFFF, 0xA5A5A5A5]
WORD_IDS = ["w%08X" % w for w in WORDS]
INDEX_FORMATS = [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32]

# (level, bits): two blocks below a byte, one byte, 8 bytes, 16 bytes, the unit level of the per-block kernels (4^8 micro-triangles) in both formats, one above it
DERIVED_SHAPES = [(0, 2), (1, 1), (1, 2), (3, 1), (3, 2), (8, 1), (8, 2), (9, 2)]
SIZE_CLASSES = {"below a byte": lambda n: n < 8, "one byte": lambda n: n == 8, "8 bytes": lambda n: n == 64, "16 bytes": lambda n: n == 128,
                "unit": lambda n: n in (4 ** 8, 2 * 4 ** 8), "above the unit": lambda n: n > 2 * 4 ** 8}
UNIFORM_AT, INVALID_AT = 4, 6          # positions among the descriptors of the real source: a uniform block and an invalid descriptor BETWEEN live ones
DECOY_BLOCK = (np.full(64, 2, np.uint8), 3, 2)


def block_bits(level, bits):
    return bits * 4 ** level


def derived_blocks(seed=0, shapes=DERIVED_SHAPES):
    """one planted block per shape, all different -> [(states, level, bits)]"""
    return [(mixed_planted(level, bits, 11 + seed + 100 * k), level, bits) for k, (level, bits) in enumerate(shapes)]


def mixed_planted(level, bits, seed):
    """coarsen_util.planted_states of the first seed from `seed` on whose block is not uniform as a whole (three in ten are; a level-0 block always is)"""
    while True:
        s = cu.planted_states(level, bits, seed)
        if level == 0 or not (s == s[0]).all():
            return s
        seed += 1


def derived_real(seed=0, shapes=DERIVED_SHAPES):
    """-> (array_data, descs (D, 3), index): the blocks of derived_blocks with a uniform block at UNIFORM_AT (it stages no block: a special index), a
    descriptor of level 13 at INVALID_AT (its primitive is skipped) and a last block that no primitive selects; the four special indices, the entry
    descArrayCount (skipped), and block 0 under two primitives"""
    blocks = derived_blocks(seed, shapes)
    blocks.insert(UNIFORM_AT, (np.full(16, 1, np.uint8), 2, 2))
    blocks.append((mixed_planted(2, 2, 900 + seed), 2, 2))          # unselected
    array_data, descs = cu.table_of_blocks(blocks)
    descs = np.insert(descs, INVALID_AT, [0, 13, 2], axis=0)
    D = len(descs)
    index = list(range(D - 1)) + [-1, -2, -3, -4, D, 0]
    return array_data, descs, np.array(index, np.int64)


def decoy_of(descs, index):
    """the decoy of a source: as many descriptors, each over its own copy of DECOY_BLOCK, and as many primitives, every one of them on a descriptor"""
    D = len(descs)
    array_data, ddescs = cu.table_of_blocks([DECOY_BLOCK] * D)
    dindex = np.arange(len(index)) % D
    return array_data, ddescs, dindex.astype(np.int64)


def derived_pair(seed=0, shapes=DERIVED_SHAPES):
    """-> (decoy, real), each (array_data, descs, index)"""
    real = derived_real(seed, shapes)
    return decoy_of(real[1], real[2]), real


def valid_rows(array_data, descs):
    """the descriptors that pass the bounds rule (level <= 12, format 1 or 2, inside the array)"""
    return [d for d, (o, l, f) in enumerate(np.asarray(descs).tolist()) if l <= 12 and f in (1, 2) and o + (block_bits(l, f) + 7) // 8 <= len(array_data)]


def packed_blocks(array_data, descs):
    """(level, format, bytes) of every valid descriptor"""
    return [(int(descs[d][1]), int(descs[d][2]), bytes(array_data[int(descs[d][0]):int(descs[d][0]) + (block_bits(int(descs[d][1]), int(descs[d][2])) + 7) // 8]))
            for d in valid_rows(array_data, descs)]


def all_equal(array_data, descs):
    return len(valid_rows(array_data, descs)) == len(descs) and len(set(packed_blocks(array_data, descs))) == 1


def all_distinct(array_data, descs):
    p = packed_blocks(array_data, descs)
    return len(set(p)) == len(p)


def is_uniform(level, fmt, data):
    b = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")[:block_bits(level, fmt)]
    s = b if fmt == 1 else b[0::2] + 2 * b[1::2]
    return bool((s == s[0]).all())


# ---- merge: levels on either side of each switch, leaders of 1, 64 and 65 members ----
MERGE_LEVELS = [1, 2, 3, 5, 6, 7]
MERGE_LEADERS = (1, 64, 65)
MERGE_BUCKET = dict(level=3, samples=4, seed=3)


def merge_levels_real():
    """three near copies at each of MERGE_LEVELS and ONE level-8 block, a 2-state and a level-0 block between them; specials and a bad entry"""
    blocks = [(mixed_planted(3, 1, 5), 3, 1), (np.array([2], np.uint8), 0, 2)]
    for level in MERGE_LEVELS:
        blocks += mu.near_copies(level, 3, 0.03, 40 + level)
    blocks.append((mixed_planted(8, 2, 48), 8, 2))
    array_data, descs = cu.table_of_blocks(blocks, first_offset=2)
    D = len(descs)
    index = np.concatenate([np.arange(D), np.arange(D)[::-1], [-1, -3, D]])
    return array_data, descs, index.astype(np.int64)


def merge_leaders_real():
    """leaders with 1, 64 and 65 members at level 3, all blocks different (a member differs from its base in one of the 60 fields that round 0 does
    not sample: level 2, with 12 such fields, has no room for 65 different members)"""
    from test_merge_gpu import _bucket_source
    blocks, family = _bucket_source(MERGE_BUCKET["level"], MERGE_LEADERS, MERGE_BUCKET["samples"], MERGE_BUCKET["seed"], distinct=True)
    array_data, descs = cu.table_of_blocks(blocks, first_offset=1)
    index = np.concatenate([np.arange(len(descs)), [0, 0, -2]])
    return array_data, descs, index.astype(np.int64), family


def merge_equal_decoy(descs, index):
    """a second decoy for the merge: as many descriptors over copies of ONE mixed block (all duplicates of each other, one hash key, nothing uniform)"""
    D = len(descs)
    array_data, ddescs = cu.table_of_blocks([(mixed_planted(2, 2, 77), 2, 2)] * D)
    return array_data, ddescs, (np.arange(len(index)) % D).astype(np.int64)


# ---- fit: blocks of levels 0..5 in both formats, weights that differ ----
FIT_SHAPES = [(level, bits) for level in range(6) for bits in (1, 2)]


def fit_real():
    array_data, descs, index = derived_real(seed=300, shapes=FIT_SHAPES)
    weights = (1 + np.arange(len(index)) % 5).astype(np.float32) / 4
    return array_data, descs, index, weights


# ---- rasterize: more descriptors than primitives, a pixel count that is no multiple of 64 ----
RASTER_IMAGE = (63, 33)
RASTER_IMAGES = [(21, 9), RASTER_IMAGE, (385, 97)]          # the boxes of the six triangles: 64 pixels or fewer (a lane), 4096 or fewer (a wave), more (the grid)
RASTER_PRIMS = 6
RASTER_VIEW = (0.0, 0.0, 1.0, 1.0)


def raster_mesh():
    """six triangles, one per cell of a 3 x 2 grid over [-0.1, 1.1]^2 -> (uv (18, 2), ix)"""
    from test_rasterize_gpu import tiles
    return tiles(RASTER_PRIMS, 3, lo=-0.1, size=1.2)


def raster_blocks(equal):
    """ten blocks (levels 0..4, both formats) for six primitives: random states, or ten copies of one uniform block"""
    rng = np.random.default_rng(12)
    if equal:
        return [DECOY_BLOCK] * 10
    return [(rng.integers(0, 1 << bits, 4 ** level).astype(np.uint8), level, bits) for level in (0, 1, 2, 3, 4) for bits in (1, 2)]


def raster_result(equal):
    array, descs = cu.table_of_blocks(raster_blocks(equal), first_offset=1, gap=2)
    index = np.array([9, 7, -2, 5, 3, 8]) if not equal else np.arange(RASTER_PRIMS)
    return lu.Result(array, [tuple(d) for d in descs.tolist()], index, ot.IDX_U16), array, descs


# ---- bakes: one case per path that carves or queues differently, from the families' own builders ----
BAKE_NAMES = ["nearest", "linear", "level9-joined-chunk", "level5-queue", "unsliced-0-4", "generic-pass-1", "generic-pass-2", "tail-sort-16385",
              "tail-counting-1025", "pending-levels", "near-duplicates", "max-array-data-size"]


def _of_case(case, knobs=()):
    import tail_cases as tc
    return dict(mips=case.get("mips") or [case["tex"]], uv=case["uv"], ix=case["ix"], level=case["gmax"], kw=tc.desc_kw(case), knobs=list(knobs), max_array=None,
                sat=True, levels=case["levels"])


def bake_cases():
    """name -> dict(mips, uv, ix, level, kw (ommtest.make_desc's keywords), knobs, max_array (maxArrayDataSize or None), sat, levels)"""
    import tail_cases as tc
    import classify_cases as cc
    import kat_cases
    uv, ix = ot.random_triangles(41, 60, 0.1)
    noise = (ot.value_noise(11, 256, 256, octaves=4, base_cell=32) * 255).astype(np.uint8)
    plain = dict(mips=[noise], uv=uv, ix=ix, level=4, knobs=[], max_array=None, sat=True, levels=None)
    out = {}
    out["nearest"] = dict(plain, kw=dict(filt=ot.NEAREST, addr=ot.CLAMP, promo=ot.PROMO_NEAREST))
    out["linear"] = dict(plain, kw=dict(filt=ot.LINEAR, addr=ot.WRAP, promo=ot.PROMO_FORCE_OPAQUE))
    out["level9-joined-chunk"] = _of_case(cc.variant(cc.j_case("sum-64"), mode="table"))
    out["level5-queue"] = _of_case(cc.m5_case(5, mode="linear"))
    out["unsliced-0-4"] = _of_case(cc.s_case(2, cc.s_counts(2)[-1], ot.FMT_4STATE, True, mode="linear"))
    out["generic-pass-1"] = _of_case(cc.b_case("sum-64", "linear"), [(ot.KNOB_GENERIC_PASS, 1)])
    out["generic-pass-2"] = _of_case(cc.b_case("sum-64", "linear"), [(ot.KNOB_GENERIC_PASS, 2)])
    out["tail-sort-16385"] = _of_case(tc.p_all_case(16385, "stepped", ot.FMT_4STATE))
    out["tail-counting-1025"] = _of_case(tc.p_all_case(1025, "stepped", ot.FMT_2STATE))
    puv = uv.reshape(-1, 3, 2).copy()
    puv[3, 1] = puv[3, 0]                                   # degenerate triangles under dynamic subdivision: their levels come from the host
    puv[17] = puv[17, 0]
    puv[40, 2] = puv[40, 1]
    out["pending-levels"] = dict(plain, uv=np.ascontiguousarray(puv.reshape(-1, 2)), level=5, kw=dict(filt=ot.LINEAR, addr=ot.WRAP, promo=ot.PROMO_FORCE_OPAQUE, dyn_scale=2.0))
    hexagons = ot.kat_texture("hexagons", 1024, 1024)
    huv, hix = kat_cases.hex_grid()
    out["near-duplicates"] = dict(mips=[hexagons], uv=huv, ix=hix, level=4, knobs=[], max_array=None, sat=False, levels=None,
                                  kw=dict(addr=ot.CLAMP, promo=ot.PROMO_NEAREST, flags=ot.FLAG_THREADS | ot.FLAG_NEAR_DUP))
    uv2, ix2 = ot.random_triangles(777, 60, 0.2)
    out["max-array-data-size"] = dict(mips=[hexagons], uv=uv2, ix=ix2, level=5, knobs=[], max_array=4000, sat=True, levels=None,
                                      kw=dict(addr=ot.WRAP, promo=ot.PROMO_FORCE_OPAQUE))
    assert list(out) == BAKE_NAMES
    return out


def entry_case():
    """the bake of ommxBakeDevice, of the streamed result (3 ranges), of the sharded API (world 2) and of ommxBakerKnob_Devices = 2: work items of
    levels 6 and 5 with special indices on (a bake streams only then), Linear"""
    uv, ix = ot.random_triangles(55, 24, 0.2)
    noise = (ot.value_noise(5, 256, 256, octaves=3, base_cell=16) * 255).astype(np.uint8)
    levels = np.where(np.arange(24) % 3 == 2, 5, 6).astype(np.uint8)          # (level 5 in 4 states: 256 bytes, the streamed bake's digest of the levels below 6)
    return dict(mips=[noise], uv=uv, ix=ix, level=6, knobs=[], max_array=None, sat=True, levels=levels,
                kw=dict(filt=ot.LINEAR, addr=ot.WRAP, promo=ot.PROMO_FORCE_OPAQUE, flags=ot.FLAG_THREADS | ot.FLAG_NO_DEDUP))


def back_to_back_cases():
    """a larger bake before a smaller one on one baker: the second one's working set is the first one's memory"""
    import tail_cases as tc
    return [_of_case(tc.p_all_case(4097, "stepped", ot.FMT_4STATE)), _of_case(tc.p_all_case(33, "one-level", ot.FMT_2STATE))]
