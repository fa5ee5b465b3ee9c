"""The way into and out of the serial host tail (omm_amd/csrc/omm_host.cpp: gather_host_items, run_host_tail_for, upload_host_tail, RcclBake::host_tail) on
the device: a subset of the families of tests/host_tail_cases.py, both formats, through ommCpuBake (statistics included), ommxBakeDevice and the one-call
sharded bake at worlds 1, 2, 3 and 8 (ranks as threads, collectives written in tests/test_shard_gpu.py).  Every result equals the oracle's, byte for byte.
tests/test_host_tail_reference.py proves without a GPU what the cases cover and puts host_tail.cpp itself under the same comparison."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import tail_cases as tc
import host_tail_cases as hc
import test_shard_gpu as sg
from test_shard_gpu import hip, dll                                   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
FOUR, TWO = ot.FMT_4STATE, ot.FMT_2STATE


def oracle_result(oracle, case, **knobs):
    return hc.bake(oracle, case, want_stats=True, **knobs)


def device_bake(product, hip, baker, tex, case, **knobs):
    d = hc.make_desc(tex, case, **knobs)
    return ot.bake_device(product, hip, baker, d, case["uv"], case["ix"], case["levels"])


def through_the_abi(product, oracle, hip, case, variants=({},)):
    """per variant: ommCpuBake with statistics and ommxBakeDevice, on one baker, equal to the oracle's result.  -> the oracle's results"""
    refs = [oracle_result(oracle, case, **v) for v in variants]
    b = product.create_baker()
    t = product.create_texture(b, [case["tex"]], alpha_cutoff=0.5)
    try:
        for v, ref in zip(variants, refs):
            got = product.bake(b, hc.make_desc(t, case, **v), want_stats=True)
            assert got.same_as(ref), (case["name"], v, "ommCpuBake", got.diff(ref))
            dev = device_bake(product, hip, b, t, case, **v)
            assert dev.same_as(ref), (case["name"], v, "ommxBakeDevice", dev.diff(ref))
    finally:
        product.destroy_texture(b, t)
        product.destroy_baker(b)
    return refs


def low_level_tiles(seed=5):
    """items of levels 0, 1 and 2 -- device slots of 16 bytes that hold 1, 1 and 4 (4-state) or 1, 1 and 2 (2-state) bytes, the 1-bit states of a partial
    byte -- of every base, mixed and uniform, near pairs among them"""
    rng = np.random.default_rng(seed)
    tiles = []
    for k in range(6):
        for L in (0, 1, 2):
            d = hc.pick(rng, L, int(rng.integers(0, max(1, 4 ** L // 2))), "O")
            tiles += [hc.tile(L, d, "OT"[k % 2], 6 + k, 7), hc.tile(L, hc.pick(rng, L, min(k % 3, int(hc.clear_micro(L).sum()))))]
            if L == 2:
                tiles.append(hc.tile(L, d + hc.pick(rng, L, 1, "O", avoid=d), "OT"[k % 2], 7, 6 + k))
    return tiles


def deep_case(fmt, **knobs):
    """test_host_tail_reference.test_c_deep_drop_beside_an_item_that_keeps_its_level: a budget walk whose order no tie leaves open"""
    base, promo = ("O", ot.PROMO_FORCE_TRANSPARENT) if fmt == FOUR else ("T", ot.PROMO_FORCE_OPAQUE)
    return hc.painted("deep-fmt%d" % fmt, [hc.tile(5, (5,), base), hc.tile(2, (0, 5, 10), base, 9, 9)], fmt, promo=promo, **knobs)


def plateau_case(fmt, **knobs):
    """level 7 and level 8 items over the halves texture, Linear: large transparent and opaque plateaus with the step between them inside the triangle, so
    the states of one item come from settled tiles, settled groups and classified groups at once; near copies (moved along the step) and level 2 - 3 items"""
    rows, lv = [], []
    for k, L in enumerate((7, 8, 7, 8, 7, 3, 2, 3)):
        x, y, w = 0.18 + 0.01 * (k % 3), 0.05 + 0.09 * k, 0.55 + 0.01 * (k // 3)
        rows.append([x, y, x + w, y + 0.01 * (k % 2), x + 0.1, y + 0.2])
        lv.append(L)
    c = tc.make_case("plateaus-fmt%d" % fmt, tc.halves(), np.array(rows, np.float32), 8, levels=np.array(lv, np.uint8), fmt=fmt, flags=knobs.pop("flags", hc.NEAR),
                     filt=ot.LINEAR, addr=ot.CLAMP, promo=ot.PROMO_FORCE_OPAQUE)
    c.update(knobs)
    return c


# ---- the families through both entry points ----
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_no_reduction_equals_the_device_tail(product, oracle, hip, fmt):
    """T0: per-triangle levels 0 - 5 and 0xF, and the low-level items, under a budget nothing reaches, with and without special indices"""
    for case in (tc.k4_case(fmt), hc.painted("t0-low-fmt%d" % fmt, low_level_tiles(), fmt, shuffle=1)):
        refs = through_the_abi(product, oracle, hip, case, [{"budget": hc.NO_REDUCTION}, {"budget": hc.NO_REDUCTION, "flags": case["flags"] | ot.FLAG_NO_SPECIAL}, {}])
        assert refs[0].same_as(refs[2])


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_low_level_items_under_every_reducer(product, oracle, hip, fmt):
    """levels 0, 1 and 2 with the LSH (factor 0.3, so that level 1 has a radius above 1), brute force, a budget of 1 (everything ends at level 0 in whatever
    order the walk goes: budgets in between meet tied keys among these small items), and all three with special indices off"""
    case = hc.painted("low-fmt%d" % fmt, low_level_tiles(), fmt, shuffle=2, factor=0.3)
    variants = [{"flags": f | s, "budget": b} for f in (hc.NEAR, hc.NEAR | hc.BRUTE) for s in (0, ot.FLAG_NO_SPECIAL) for b in (hc.NO_BUDGET, 1)]
    refs = through_the_abi(product, oracle, hip, case, variants)
    assert fmt == TWO or len(refs[0].descs) < len(oracle_result(oracle, case, flags=ot.FLAG_THREADS).descs)


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_mixed_levels_near_duplicates_and_budgets(product, oracle, hip, fmt):
    """N, B and C with levels 1 - 6 in one bake"""
    case = hc.painted("mixed-fmt%d" % fmt, hc.mixed_levels_tiles(2), fmt, shuffle=2)
    through_the_abi(product, oracle, hip, case, [{"flags": hc.NEAR}, {"flags": hc.NEAR | hc.BRUTE}, {"flags": hc.NEAR, "budget": 1}, {"budget": 1}, {"budget": 0}])
    through_the_abi(product, oracle, hip, deep_case(fmt), [{"budget": b} for b in (261, 260, 69, 68, 67, 21, 20, 19)])
    if fmt == TWO:
        refs = through_the_abi(product, oracle, hip, hc.painted("two-state-3", [hc.tile(3, (1, 13, 29), "T"), hc.tile(2, (), "T", 7, 7)], TWO, promo=ot.PROMO_FORCE_OPAQUE), [{"budget": 17}, {"budget": 16}])
        assert refs[1].array_data.tolist() == [0x9B, 0x00]


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_items_from_settled_tiles_settled_groups_and_classified_groups(product, oracle, hip, fmt):
    """the host tail reads states that settled tiles, settled groups and the per-micro-triangle classification wrote, of one bake.  A host-tail bake leaves
    the classification's counters out of ommxBakeTimings, so they are read behind an ordinary bake of the same case on the same baker type: the
    classification does not depend on the reducer flags.  Five items of levels 7 and 8 are 3 * 4 + 2 * 16 = 44 tiles"""
    case = plateau_case(fmt)
    raw = oracle_result(oracle, case, flags=tc.RAW_FLAGS)
    assert set(raw.descs[:, 1].tolist()) == {2, 3, 7, 8}
    b = product.create_baker()
    t = product.create_texture(b, [case["tex"]], alpha_cutoff=0.5)
    try:
        product.bake(b, hc.make_desc(t, case, flags=ot.FLAG_THREADS))
        tm = sg.timings(product, b)
    finally:
        product.destroy_texture(b, t)
        product.destroy_baker(b)
    counters = dict(activeItems=tm.activeItems, openTiles=tm.openTiles, openTileMicroTriangles=tm.openTileMicroTriangles, fineMicroTriangles=tm.fineMicroTriangles)
    print(case["name"], counters)
    assert 0 < tm.openTiles < 44, counters                               # some tiles settle as a whole, some stay open
    assert 0 < tm.fineMicroTriangles < tm.openTileMicroTriangles, counters   # of the open tiles' micro-triangles some settle with their group, the others are classified one by one
    through_the_abi(product, oracle, hip, case, [{}, {"flags": hc.NEAR | hc.BRUTE}, {"budget": 1}, {"budget": hc.NO_REDUCTION, "flags": ot.FLAG_THREADS}])


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_all_items_uniform_and_all_triangles_invalid(product, oracle, hip, fmt):
    tiles = [hc.tile(L, (), b, 6 + L, 7) for L in (0, 1, 2, 3, 5) for b in "OT"] + [hc.tile(2, tuple(range(16)), "O", 9, 9)]
    case = hc.painted("uniform-fmt%d" % fmt, tiles, fmt)
    variants = [{"flags": hc.NEAR | s, "budget": b} for s in (0, ot.FLAG_NO_SPECIAL) for b in (hc.NO_BUDGET, 1)]
    refs = through_the_abi(product, oracle, hip, case, variants)
    assert len(refs[0].descs) == 0 and len(refs[1].descs) == 0 and len(refs[2].descs) > 0
    uv = case["uv"].copy()
    uv[0::3, 0] = np.nan
    case["uv"] = uv
    refs = through_the_abi(product, oracle, hip, case, variants)
    assert all(len(r.descs) == 0 and (r.index == ot.SPECIAL_FUO).all() for r in refs)


# (triangles, Allow8, Force32) -> index format (bake_cpu_impl.cpp:1872-1902), written out
INDEX_FORMATS = [(127, False, False, ot.IDX_U16), (127, True, False, ot.IDX_U8), (127, False, True, ot.IDX_U32), (127, True, True, ot.IDX_U32),
                 (128, False, False, ot.IDX_U16), (128, True, False, ot.IDX_U16), (128, False, True, ot.IDX_U32), (128, True, True, ot.IDX_U32),
                 (32767, False, False, ot.IDX_U16), (32767, True, False, ot.IDX_U16), (32767, False, True, ot.IDX_U32), (32767, True, True, ot.IDX_U32),
                 (32768, False, False, ot.IDX_U32), (32768, True, False, ot.IDX_U32), (32768, False, True, ot.IDX_U32), (32768, True, True, ot.IDX_U32)]


@pytest.mark.parametrize("count,allow8,force32,want", INDEX_FORMATS)
def test_index_format_of_a_host_tail_result(product, oracle, hip, count, allow8, force32, want):
    """run_host_tail_for narrows the index in place, host_result_from_tail and upload_host_tail copy it: 127 / 128 / 32 767 / 32 768 triangles x Allow8 x
    Force32 through ommCpuBake and ommxBakeDevice.  127 / 128: painted level-2 items under the LSH and a budget of 1, special indices among the values;
    32 767 / 32 768: cheap triangles of levels 0 - 2 under a budget nothing reaches"""
    extra = (ot.FLAG_ALLOW8 if allow8 else 0) | (ot.FLAG_FORCE32 if force32 else 0)
    if count < 1000:
        rng = np.random.default_rng(count)
        tiles = [hc.tile(2, hc.pick(rng, 2, int(rng.integers(0, 5)), "O"), "OT"[k % 2], 6 + k % 9, 6 + k // 9) for k in range(count)]
        refs = through_the_abi(product, oracle, hip, hc.painted("index-%d" % count, tiles, flags=hc.NEAR | extra), [{}, {"budget": 1}])
        assert (refs[0].index < 0).any() and (refs[0].index >= 0).any()
    else:
        case = tc.p_all_case(count, "stepped", FOUR)
        refs = through_the_abi(product, oracle, hip, case, [{"budget": hc.NO_REDUCTION, "flags": case["flags"] | extra}])
        assert len(refs[0].descs) == count
    assert all(r.index_format == want and len(r.index) == count for r in refs)


def test_host_tail_and_ordinary_bakes_alternate_on_one_baker(product, oracle, hip):
    """pool blocks reused: ordinary bake, host-tail bake, ordinary, device-resident host-tail bake, ..., three rounds on one baker"""
    case = hc.painted("alternate", hc.mixed_levels_tiles(5), shuffle=5)
    variants = [{"flags": ot.FLAG_THREADS}, {"flags": hc.NEAR}, {"flags": ot.FLAG_THREADS, "budget": 1}, {"flags": hc.NEAR | hc.BRUTE, "budget": 0}]
    refs = [oracle_result(oracle, case, **v) for v in variants]
    b = product.create_baker()
    t = product.create_texture(b, [case["tex"]], alpha_cutoff=0.5)
    try:
        for rnd in range(3):
            for v, ref in zip(variants, refs):
                got = product.bake(b, hc.make_desc(t, case, **v), want_stats=True) if (rnd + len(v)) % 2 else device_bake(product, hip, b, t, case, **v)
                assert got.same_as(ref), (rnd, v, got.diff(ref))
    finally:
        product.destroy_texture(b, t)
        product.destroy_baker(b)


def test_near_duplicates_without_duplicate_detection_are_refused(product, oracle):
    case = hc.painted("refused", [hc.tile(2, (1,), "O"), hc.tile(2, (1, 2), "O", 7, 7)], flags=hc.NEAR | ot.FLAG_NO_DEDUP)
    for lib in (oracle, product):
        assert hc.bake(lib, case, expect=ot.INVALID_ARGUMENT) is None


# ---- ranks ----
class Reduced(sg.Baked):
    """test_shard_gpu.Baked with the case's budget and factor in the desc"""

    def __init__(self, product, hip, case, knobs=()):
        super().__init__(product, hip, case, knobs)
        flags, budget, factor, rejection = hc.knobs_of(case)
        self.desc.maxArrayDataSize = self.host_desc.maxArrayDataSize = budget
        self.desc.nearDuplicateDeduplicationFactor = self.host_desc.nearDuplicateDeduplicationFactor = factor


def rank_cases(fmt):
    """the cases of the rank test.  An N, a B, a C and an N + C case, each twice: painted items of levels 0 - 6, and the level-7 / 8 plateau items with
    levels 2 and 3 (the two need different textures and filters).  `tiny`: three items, so whole ranks own nothing.  `few`: one level-5 and one level-4
    item among thirty of level 2, levels with fewer items than ranks.  Two budgets of deep_case.  The budgets are 1, under which every order of the walk
    ends with everything at level 0, and deep_case's, whose walk no tie leaves open"""
    out = []
    for name, knobs in (("n", dict(flags=hc.NEAR)), ("b", dict(flags=hc.NEAR | hc.BRUTE)), ("c", dict(flags=ot.FLAG_THREADS, budget=1)), ("nc", dict(flags=hc.NEAR, budget=1))):
        out.append(hc.painted("ranks-%s-fmt%d" % (name, fmt), low_level_tiles(7)[:20] + hc.mixed_levels_tiles(6), fmt, shuffle=6, **knobs))
        out.append(plateau_case(fmt, **knobs))
    rng = np.random.default_rng(3)
    a = hc.pick(rng, 3, 20, "O")
    out.append(hc.painted("ranks-tiny-fmt%d" % fmt, [hc.tile(3, a, "O"), hc.tile(3, a + hc.pick(rng, 3, 1, "O", avoid=a), "O", 7, 7), hc.tile(1, (2,), "T")], fmt, flags=hc.NEAR))
    few = [hc.tile(2, hc.pick(rng, 2, 3 + k % 5, "O"), "OT"[k % 2], 6 + k % 8, 6 + k // 8) for k in range(30)] + [hc.tile(5, hc.pick(rng, 5, 300, "O"), "O"), hc.tile(4, hc.pick(rng, 4, 70, "O"), "O")]
    out.append(hc.painted("ranks-few-fmt%d" % fmt, few, fmt, flags=hc.NEAR, budget=1, shuffle=3))
    out += [deep_case(fmt, budget=b) for b in (68, 20)]
    return out


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_ranks_merge_their_states_by_a_sum(product, oracle, hip, dll, monkeypatch, fmt, world):
    """every rank classifies its share into zeroed states and the shares are summed as uint32 words: every rank's result equals the oracle's (and so the
    world-1 result), on items of every level 0 - 8, 1-bit and under-16-byte slots included.  Every rank bakes on a fresh baker, whose memory may well be
    zero already, so from world 2 on every case runs a second time with ommxBakerKnob_Poison: pool and working set are then filled with 0xA5A5A5A5 before
    the bake, and a share that the rank does not own stays zero only if the bake zeroes it"""
    monkeypatch.setattr(sg, "Baked", Reduced)
    for case in rank_cases(fmt):
        ref = oracle_result(oracle, case)
        for knobs in [()] + ([((ot.KNOB_POISON, ot.poison(0xA5A5A5A5)),)] if world > 1 else []):
            run = sg.one_call(product, hip, dll, case, world, knobs)
            sg.all_equal(run["results"], ref, (case["name"], knobs))


def test_fences_of_the_host_tail(product, oracle, hip, dll):
    """the caller-driven four-phase protocol answers NOT_IMPLEMENTED for a bake with a reducer; ommxBakerKnob_Devices leaves such a bake on one device"""
    case = hc.painted("fences", hc.mixed_levels_tiles(1), flags=hc.NEAR, budget=1)
    B = Reduced(product, hip, case)
    try:
        for r, world in ((0, 1), (1, 2)):
            h = C.c_void_p()
            assert dll.ommxShardedBegin(B.baker, C.byref(B.desc), r, world, C.byref(h)) == ot.NOT_IMPLEMENTED and not h.value
    finally:
        B.close()
    ref = oracle_result(oracle, case)
    b = product.create_baker()
    product.set_knob(b, ot.KNOB_DEVICES, 2)
    t = product.create_texture(b, [case["tex"]], alpha_cutoff=0.5)
    got = product.bake(b, hc.make_desc(t, case), want_stats=True)
    devices = sg.timings(product, b).devices
    product.destroy_texture(b, t)
    product.destroy_baker(b)
    assert got.same_as(ref), got.diff(ref)
    assert devices != 2, devices                                        # (a bake that went to two devices says so: test_shard_gpu.test_multi_device_bake)
