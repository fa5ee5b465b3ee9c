"""No GPU: every case list of tests/test_poisoned_memory_gpu.py (tests/poison_cases.py) held to what it claims, with the numpy models and the oracle
alone -- decoy and real source of equal counts, the decoy's blocks all equal and uniform, the real ones all different, every named size class, level and
kind of index entry present, the merge leaders of 1, 64 and 65 members, the shapes of the rasterized image, and for the bakes the path each case is
there for.  The oracle's side of every bake is printed and bounded at 3 s."""
import time
import numpy as np
import pytest
import ommtest as ot
import poison_cases as pc
import coarsen_util as cu
import merge_util as mu
import fit_util as fu
import stats_util as su
import classify_cases as cc
import tail_cases as tc

ORACLE_SECONDS = 3.0


def test_words_contradict_every_initialisation_twice():
    """a zero fill is contradicted by every word but 0, a 0xFF fill by every word but 0xFFFFFFFF; 1 stays in bounds as a mark, count or index"""
    assert pc.WORDS == [0x00000000, 0x00000001, 0xFFFFFFFF, 0xA5A5A5A5] and len(set(pc.WORD_IDS)) == 4
    assert sum(w != 0 for w in pc.WORDS) >= 2 and sum(w != 0xFFFFFFFF for w in pc.WORDS) >= 2
    assert ot.poison(0) == 1 << 32 and ot.poison(0xFFFFFFFF) == 0x1FFFFFFFF


@pytest.mark.parametrize("seed", [0, 50])
def test_derived_pair(seed):
    decoy, real = pc.derived_pair(seed)
    (da, dd, di), (ra, rd, ri) = decoy, real
    assert len(dd) == len(rd) <= 127 and len(di) == len(ri)          # equal counts; every index format can name every descriptor
    assert pc.all_equal(da, dd) and all(pc.is_uniform(*b) for b in pc.packed_blocks(da, dd)) and (di >= 0).all() and (di < len(dd)).all()
    assert pc.all_distinct(ra, rd)
    valid = pc.valid_rows(ra, rd)
    assert len(valid) == len(rd) - 1 and pc.INVALID_AT not in valid and 0 < pc.INVALID_AT < len(rd) - 1          # an invalid descriptor between live ones
    bits = {pc.block_bits(int(rd[d][1]), int(rd[d][2])) for d in valid}
    for name, holds in pc.SIZE_CLASSES.items():
        assert any(holds(n) for n in bits), name
    assert {int(rd[d][2]) for d in valid} == {1, 2}
    uniform = [d for d, b in zip(valid, pc.packed_blocks(ra, rd)) if pc.is_uniform(*b) and b[0] > 0]
    assert uniform == [pc.UNIFORM_AT] and pc.UNIFORM_AT - 1 in valid and pc.UNIFORM_AT + 1 in valid          # an item that stages no block between live ones
    entries = ri.tolist()
    assert {-1, -2, -3, -4} <= set(entries) and len(rd) in entries and entries.count(0) == 2          # specials, a skipped primitive, a block under two
    assert len(rd) - 1 not in entries and len(rd) - 1 in valid                                          # an unselected descriptor
    ref = cu.restate_coarsen(ra, rd, ri, ot.IDX_U8, 12)
    assert ref["info"]["skippedPrimitives"] == 2 and ref["info"]["uniformBlocks"] >= 1 and ref["info"]["referencedBlocks"] == len(valid) - 1
    for cap in (0, 3, 4, 7, 8):
        assert cu.restate_coarsen(ra, rd, ri, ot.IDX_U8, cap)["info"]["coarsenedBlocks"] == sum(int(rd[d][1]) > cap for d in valid[:-1])


def test_merge_cases():
    limit = mu.UNIT * 4 // 100
    a, d, i = pc.merge_levels_real()
    assert pc.all_distinct(a, d) and len(pc.valid_rows(a, d)) == len(d) <= 127
    levels = [int(l) for l in d[:, 1]]
    assert {1, 2, 3, 5, 6, 7} <= set(levels) and levels.count(8) == 1 and 4 not in levels and max(levels) == 8
    ref = mu.restate_merge(a, d, i, ot.IDX_U8, limit, seed=5)
    assert ref["info"]["absorbedBlocks"] > 0 and ref["info"]["skippedPrimitives"] == 1
    a, d, i, family = pc.merge_leaders_real()
    assert pc.all_distinct(a, d) and [family.count(k) - 1 for k in range(3)] == list(pc.MERGE_LEADERS)
    ref = mu.restate_merge(a, d, i, ot.IDX_U16, limit, rounds=1, samples=pc.MERGE_BUCKET["samples"], seed=pc.MERGE_BUCKET["seed"])
    sizes = np.bincount(ref["roots"])
    assert sorted((sizes[sizes > 0] - 1).tolist()) == [1, 64, 65] and ref["info"]["absorbedPerRound"][0] == 130
    for real in (pc.merge_levels_real(), (a, d, i)):
        for decoy in (pc.decoy_of(real[1], real[2]), pc.merge_equal_decoy(real[1], real[2])):
            assert len(decoy[1]) == len(real[1]) and len(decoy[2]) == len(real[2]) and pc.all_equal(decoy[0], decoy[1])
    eq = pc.merge_equal_decoy(d, i)
    assert not any(pc.is_uniform(*b) for b in pc.packed_blocks(eq[0], eq[1]))


def test_fit_case():
    a, d, i, w = pc.fit_real()
    assert pc.all_distinct(a, d) and len(d) <= 127 and len(w) == len(i) and len(set(w.tolist())) == 5
    assert {(int(l), int(f)) for o, l, f in d[pc.valid_rows(a, d)].tolist()} >= set(pc.FIT_SHAPES)
    prof = fu.restate_profile(a, d, i, w)
    floor = fu.restate_plan(prof["shape"], prof["known"], prof["opaque"], prof["weights"], 0, 12, True)
    low, top = floor["planned"], floor["unfitted"]
    assert floor["feasible"] and low + 7 < (low + top) // 2 < top
    for budget in ((low + top) // 2, low + 7):
        plan, ref = fu.restate_fit(a, d, i, ot.IDX_U8, budget, w, profile=prof)
        assert plan["feasible"] and plan["steps"] > 0 and ref["info"]["arrayDataSize"] <= budget


def test_raster_case():
    from test_rasterize_gpu import box_pixels, LANE_BOX, WAVE_BOX
    uv, ix = pc.raster_mesh()
    boxes = [[box_pixels(t, pc.RASTER_VIEW, w, h) for t in uv.reshape(-1, 3, 2)] for w, h in pc.RASTER_IMAGES]
    assert 0 < max(boxes[0]) <= LANE_BOX < min(boxes[1]) and max(boxes[1]) <= WAVE_BOX < min(boxes[2])          # one image per coverage kernel
    w, h = pc.RASTER_IMAGE
    assert (w * h) % 64 and (w * h) % 256 and w * h > 256                                   # several workgroups, the last one partly filled
    for equal in (True, False):
        res, array, descs = pc.raster_result(equal)
        assert len(descs) == 10 > pc.RASTER_PRIMS == len(res.index)
        assert pc.all_equal(array, descs) if equal else pc.all_distinct(array, descs)


def test_statistics_and_geometry_read_the_derived_pair():
    decoy, real = pc.derived_pair()
    ref = su.reference_stats(real[0], real[1], real[2], np.ones(len(real[2]), np.float32))
    assert ref["skipped"] == 2 and ref["refs"][0] == 2 and ref["refs"][-1] == 0 and not ref["state_counts"][pc.INVALID_AT].any()
    ref = su.reference_stats(decoy[0], decoy[1], decoy[2])
    assert ref["skipped"] == 0 and (ref["state_counts"][:, 2] == 64).all()


@pytest.fixture(scope="module")
def bakes():
    return pc.bake_cases()


def oracle_bake(oracle, case):
    t0 = time.perf_counter()
    b = oracle.create_baker()
    t = oracle.create_texture(b, case["mips"], alpha_cutoff=0.5 if case["sat"] else -1.0)
    d = ot.make_desc(t, case["uv"], case["ix"], case["level"], levels=case["levels"], **{k: v for k, v in case["kw"].items() if k != "levels"})
    if case["max_array"] is not None:
        d.maxArrayDataSize = case["max_array"]
    r = oracle.bake(b, d)
    oracle.destroy_texture(b, t)
    oracle.destroy_baker(b)
    return r, time.perf_counter() - t0


@pytest.mark.parametrize("name", pc.BAKE_NAMES)
def test_bake_case_is_what_its_name_says(oracle, bakes, name):
    case = bakes[name]
    r, seconds = oracle_bake(oracle, case)
    T = len(case["ix"]) // 3
    print("oracle side of %s: %.2f s, %d blocks, %d bytes, %d primitives" % (name, seconds, len(r.descs), r.array_data.size, T))
    assert seconds < ORACLE_SECONDS and len(r.index) == T
    kw = case["kw"]
    levels = [case["level"]] * T if case["levels"] is None else [int(x) for x in case["levels"]]
    if name in ("nearest", "linear"):
        assert kw["filt"] == (ot.NEAREST if name == "nearest" else ot.LINEAR) and len(r.descs) > 8
    elif name == "level9-joined-chunk":
        c = cc.variant(cc.j_case("sum-64"), mode="table")
        s = cc.restate_schedule(c)
        assert levels == [9] and [len(k["members"]) for k in s["chunks"]] == [2] and s["deterministic"] and len(r.descs) == 1
    elif name == "level5-queue":
        s = cc.restate_schedule(cc.m5_case(5, mode="linear"))
        assert set(levels) == {5} and len(s["small"]) == 5 and not s["records"]          # the 1024-tile queue alone
    elif name == "unsliced-0-4":
        assert max(levels) <= 4 and T > 128 and len(r.descs) > 64                          # more than one workgroup of unsliced items
    elif name.startswith("generic-pass"):
        c = cc.b_case("sum-64", "linear")
        leg = float(cc.B_TRI[1, 0] - cc.B_TRI[0, 0]) * cc.B_SIZE
        assert case["knobs"] == [(ot.KNOB_GENERIC_PASS, int(name[-1]))] and leg / 2 ** max(levels) > 1 and len(r.descs) == 1          # micro-triangles of several texels
    elif name == "tail-sort-16385":
        assert T == 16385 and len(r.descs) == 16385 and kw["flags"] == tc.EVERY_FLAGS          # every item a candidate: one past the counting path's 16 384
    elif name == "tail-counting-1025":
        assert T == 1025 and len(r.descs) == 1025 and kw["flags"] == tc.EVERY_FLAGS
    elif name == "pending-levels":
        tri = case["uv"].reshape(-1, 3, 2).astype(np.float64)
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        area2 = np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
        assert kw["dyn_scale"] > 0 and int((area2 == 0).sum()) == 3 and len(set(r.descs[:, 1].tolist())) > 1          # degenerate triangles: levels from the host
    elif name == "near-duplicates":
        plain, _ = oracle_bake(oracle, dict(case, kw=dict(kw, flags=ot.FLAG_THREADS)))
        assert kw["flags"] & ot.FLAG_NEAR_DUP and 0 < len(r.descs) < len(plain.descs)          # the merge took blocks away
    elif name == "max-array-data-size":
        plain, _ = oracle_bake(oracle, dict(case, max_array=None))
        assert r.array_data.size <= case["max_array"] < plain.array_data.size
    else:
        raise AssertionError(name)


def test_entry_and_back_to_back_cases(oracle):
    case = pc.entry_case()
    r, seconds = oracle_bake(oracle, case)
    print("oracle side of the entry case: %.2f s, %d blocks, %d bytes" % (seconds, len(r.descs), r.array_data.size))
    flags = case["kw"]["flags"]
    assert sorted(set(case["levels"].tolist())) == [5, 6] and int((case["levels"] == 6).sum()) >= 6
    assert seconds < ORACLE_SECONDS and len(r.descs) >= 6 and not flags & ot.FLAG_NO_SPECIAL and case["kw"]["filt"] == ot.LINEAR          # several items: three ranges cut
    sizes = []
    for c in pc.back_to_back_cases():
        r, seconds = oracle_bake(oracle, c)
        print("oracle side of a back-to-back bake: %.2f s, %d blocks" % (seconds, len(r.descs)))
        assert seconds < ORACLE_SECONDS and len(r.descs) == len(c["ix"]) // 3
        sizes.append(len(c["ix"]) // 3)
    assert sizes[0] > 100 * sizes[1]                                                       # the larger one first
