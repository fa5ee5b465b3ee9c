"""ommxProfileMicromapLevels, ommxCoarsenMicromapLevels and ommxFitMicromap on the GPU.  Every case is compared with the statements of
tests/fit_util.py byte for byte -- counts, weights, levels, arrayData, descArray, the index buffer, both histograms and the info fields; there is no
tolerance anywhere.  The shapes are the tier edges of the counting pass (a lane's 256 micro-triangles, part of a wave, a workgroup's unit of 4^8, several
units, the second pass above level 8), not a workload."""
import ctypes as C
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import fit_util as fu
import kat_cases
import kat_runner

pytestmark = pytest.mark.gpu

FORMATS = pytest.mark.parametrize("bits", [1, 2], ids=["2state", "4state"])


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    return fu.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def profile_and_check(dll, hip, baker, src, weights=None, stream=None):
    """the profile of a coarsen_util.Source against the model (weights: host float32 or None) -> the model's answer"""
    a, d, i = src.host
    size = None
    if src.declared:
        size, D, T = src.declared
        d, i = d[:D], i[:T]
    ref = fu.restate_profile(a, d, i, weights, size, src.unpacked)
    dev = hip.upload(np.asarray(weights, np.float32)) if weights is not None else None
    try:
        r, got, info = fu.profile(dll, hip, baker, src.rd, dev, stream)
        assert r == ot.SUCCESS and info == ref["info"], (r, info, ref["info"])
        fu.assert_profile(got, ref)
        assert src.unchanged()
    finally:
        if dev is not None:
            hip.free(dev)
    return ref


def state_counts(dll, hip, baker, rd):
    """ommxDebugGetStatsDevice's stateCounts -> (D, 4) uint32"""
    buf = hip.alloc(16 * max(rd.descArrayCount, 1))
    try:
        outputs, st = su.DeviceStatsOutputs(buf.value, None, None), ot.DebugStats()
        assert dll.ommxDebugGetStatsDevice(baker, C.byref(rd), None, C.byref(outputs), C.byref(st), None, None) == ot.SUCCESS
        return hip.download(buf, 16 * rd.descArrayCount, np.uint32).reshape(-1, 4)
    finally:
        hip.free(buf)


# ---- the profile: every tier edge ----
@FORMATS
def test_profile_every_level_up_to_9(dll, hip, baker, bits):
    """one block per level 0..9: a lane's share, part of a wave, a wave, a workgroup's unit, four units and the second pass; the t = L row equals T + O
    and O of the statistics' stateCounts; a second call returns the same bytes"""
    blocks = [(cu.planted_states(level, bits, seed=3), level, bits) for level in range(10)]
    array_data, descs = cu.table_of_blocks(blocks)
    src = cu.Source(hip, array_data, descs, list(range(10)), ot.IDX_U8, array_align=16)
    try:
        ref = profile_and_check(dll, hip, baker, src)
        assert (ref["known"].sum(axis=0)[:10] > 0).all() and (ref["opaque"].sum(axis=0)[:10] > 0).all()          # (known groups at every level)
        assert bits == 1 or sum(0 < ref["known"][l][l] < 4 ** l for l in range(10)) >= 5
        counts = state_counts(dll, hip, baker, src.rd)
        for l in range(10):
            assert (counts[l][0] + counts[l][1], counts[l][1]) == (ref["known"][l][l], ref["opaque"][l][l])
        r1, a1, i1 = fu.profile(dll, hip, baker, src.rd)
        r2, a2, i2 = fu.profile(dll, hip, baker, src.rd)
        assert r1 == r2 == ot.SUCCESS and i1 == i2 and all(a1[k].tobytes() == a2[k].tobytes() for k in a1)
    finally:
        src.close()


@FORMATS
def test_profile_level_12(dll, hip, baker, bits):
    """a level-12 block (256 units, four levels in the second pass) beside a level-10 block (16 units, two), one of them selected twice"""
    seed = 5 if bits == 1 else 4          # (blocks with known groups left at every level from 2 up, and not all of them)
    blocks = [(cu.planted_states(12, bits, seed), 12, bits), (cu.planted_states(10, bits, seed), 10, bits)]
    array_data, descs = cu.table_of_blocks(blocks)
    src = cu.Source(hip, array_data, descs, [0, 1, 0], ot.IDX_U32, array_align=256)
    try:
        ref = profile_and_check(dll, hip, baker, src)
        assert ref["refs"].tolist() == [2, 1] and ref["weights"].tolist() == [2, 1]
        top = 1 if bits == 2 else 0          # (a 2-state block knows all of its own level)
        assert all(0 < ref["known"][0][t] < 4 ** t for t in range(2, 12 + top)) and all(0 < ref["known"][1][t] < 4 ** t for t in range(2, 10 + top))
    finally:
        src.close()


@FORMATS
def test_profile_at_odd_addresses(dll, hip, baker, bits):
    """level-8 and level-9 blocks at offset % 16 of 3 and 8, and one-byte blocks (levels 0 and 1) whose unused bits are set: ignored"""
    blocks = [(cu.planted_states(level, bits, seed=level), level, bits) for level in (8, 0, 9, 1, 1, 0)]
    for first, gap in ((3, 0), (8, 16)):
        array_data, descs = cu.table_of_blocks(blocks, first_offset=first, gap=gap, filler=0xFF)
        for d in (1, 3, 4, 5):                     # garbage above the fields of the one-byte blocks
            array_data[descs[d, 0]] |= (0xFF << (bits * 4 ** int(descs[d, 1]))) & 0xFF
        src = cu.Source(hip, array_data, descs, [0, 1, 2, 3, 4, 5], ot.IDX_U16, array_align=16)
        try:
            profile_and_check(dll, hip, baker, src)
        finally:
            src.close()


@pytest.mark.parametrize("index_format", [ot.IDX_U8, ot.IDX_U16, ot.IDX_U32])
def test_profile_statistics_table(dll, hip, baker, index_format):
    """stats_util's table in the three index formats, with its areas as weights: invalid descriptors and the unselected block 7 give rows of zeros, 8
    primitives are skipped, block 0 is selected three times"""
    array_data, descs, index, areas = su.table_arrays()
    src = cu.Source(hip, array_data, descs, index, index_format, array_align=1)
    try:
        for weights in (None, areas):
            ref = profile_and_check(dll, hip, baker, src, weights)
            assert ref["info"]["skippedPrimitives"] == 8 and ref["info"]["referencedBlocks"] == 9 and ref["refs"][0] == 3 and ref["refs"][7] == 0
            dead = [d for d in range(len(descs)) if ref["shape"][d] is None]
            assert len(dead) == len(descs) - 9 and not ref["known"][dead].any() and not ref["weights"][dead].any()
    finally:
        src.close()


def test_profile_weights_at_their_edges(dll, hip, baker):
    """NaN, -1, +inf, 0, a subnormal and FLT_MAX among the weights; a block selected by several primitives; weights that are all refused; subnormals alone"""
    blocks = [(cu.planted_states(level, 2, seed=level), level, 2) for level in (2, 3, 1)]
    array_data, descs = cu.table_of_blocks(blocks)
    index = [0, 1, 0, 2, 0, 1, -2, 1, 2, 0, 7, 2]
    flt_max = np.float32(3.4028234663852886e38)
    src = cu.Source(hip, array_data, descs, index, ot.IDX_U8)
    try:
        w = np.array([np.nan, -1.0, np.inf, 0.0, 1e-45, flt_max, flt_max, 1e38, 3e38, 2.5e38, flt_max, 1.0], np.float32)
        ref = profile_and_check(dll, hip, baker, src, w)
        assert ref["info"]["weightExponent"] == 127 and ref["weights"][0] > 1 << 31 and ref["refs"].tolist() == [4, 3, 3]
        ref = profile_and_check(dll, hip, baker, src, np.array([np.nan, -1.0, np.inf, 0.0, -np.inf, -0.0] * 2, np.float32))
        assert ref["info"]["weightExponent"] == 0 and not ref["weights"].any()
        ref = profile_and_check(dll, hip, baker, src, np.array([1e-45, 2.5e-39, 1e-40, 0.0, 3e-41, 1e-45] * 2, np.float32))
        assert ref["info"]["weightExponent"] == -129 and ref["weights"].all()
        ref = profile_and_check(dll, hip, baker, src, np.full(12, 0.75, np.float32))
        assert ref["info"]["weightExponent"] == -1 and ref["weights"].tolist() == [4 * (3 << 30), 3 * (3 << 30), 3 * (3 << 30)]
    finally:
        src.close()


def test_profile_a_million_primitives(dll, hip, baker):
    """2^20 + 3 primitives over 1000 descriptors (32-bit entries) with weights handed over by a copy on the caller's stream that is not waited for: the
    references and the integer weight sums are exact, call after call"""
    rng = np.random.default_rng(20)
    protos = [(cu.planted_states(level, bits, seed), level, bits) for level in range(5) for bits in (1, 2) for seed in range(10)]
    table, pdescs = cu.table_of_blocks(protos)
    D, T = 1000, (1 << 20) + 3
    descs = pdescs[rng.integers(0, len(protos), D)]
    index = np.concatenate([np.arange(D), rng.integers(-5, D + 1, T - D)])
    rng.shuffle(index)
    weights = (rng.random(T) ** 8 * 1000.0).astype(np.float32)
    weights[rng.integers(0, T, 1000)] = np.nan
    src = cu.Source(hip, table, descs, index, ot.IDX_U32, array_align=16)
    stream = hip.stream_create(non_blocking=True)
    staged, dev = hip.upload(weights), hip.upload(np.zeros(T, np.float32))
    hip.rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    try:
        ref = fu.restate_profile(table, descs, index, weights)
        assert ref["info"]["referencedBlocks"] == D and ref["info"]["skippedPrimitives"] > 0 and int(ref["weights"].max()) > 1 << 36
        answers = []
        for call in range(2):
            assert hip.rt.hipMemcpyAsync(dev, staged, 4 * T, 3, stream) == 0          # (device to device, on the caller's stream, no wait)
            r, got, info = fu.profile(dll, hip, baker, src.rd, dev, stream)
            assert r == ot.SUCCESS and info == ref["info"]
            fu.assert_profile(got, ref)
            answers.append(b"".join(got[k].tobytes() for k in sorted(got)))
        assert answers[0] == answers[1]
    finally:
        hip.stream_sync(stream)
        hip.stream_destroy(stream)
        hip.free(staged)
        hip.free(dev)
        src.close()


# ---- the coarsening with a cap per block ----
def levels_and_check(dll, hip, baker, src, block_levels, cap=12, mixed=3, flags=0):
    a, d, i = src.host
    ref = fu.restate_coarsen_levels(a, d, i, src.rd.indexFormat, block_levels, cap, mixed, flags, unpacked=src.unpacked)
    for want_result in (False, True):
        r, info, handle = fu.coarsen_levels(dll, hip, baker, src.rd, block_levels, cap, mixed, flags, want_result=want_result)
        assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
    try:
        cu.assert_same(cu.download_result(dll, hip, handle), ref)
        assert src.unchanged()
    finally:
        assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
    return ref


@pytest.mark.parametrize("bits,mixed", [(1, 2), (2, 3)], ids=["2state_ut", "4state_uo"])
def test_levels_on_the_ten_block_table(dll, hip, baker, bits, mixed):
    """random per-block levels on one block per level 0..9, crossed with a global cap: each block goes to the minimum of the three; NULL levels are
    ommxCoarsenMicromap's bytes; entries of 12, 13 and 255 are no limit"""
    blocks = [(cu.planted_states(level, bits, seed=3), level, bits) for level in range(10)]
    array_data, descs = cu.table_of_blocks(blocks)
    src = cu.Source(hip, array_data, descs, list(range(10)), ot.IDX_U8, array_align=16)
    rng = np.random.default_rng(bits)
    try:
        for trial, cap in enumerate((12, 6, 3, 9, 0)):
            own = rng.integers(0, 11, 10)
            ref = levels_and_check(dll, hip, baker, src, own, cap, mixed, cu.NO_SPECIAL | cu.NO_DEDUP)
            assert sorted(ref["descs"][:, 1].tolist()) == sorted(min(l, cap, int(own[l])) for l in range(10))
            assert ref["info"]["coarsenedBlocks"] == sum(min(cap, int(own[l])) < l for l in range(10))
            levels_and_check(dll, hip, baker, src, own, cap, mixed)
        for cap in (12, 4):
            same = src.model(cap, mixed)
            for own in (None, [12] * 10, [13, 255, 12, 200, 14, 12, 255, 13, 12, 99]):
                ref = levels_and_check(dll, hip, baker, src, own, cap, mixed)
                cu.assert_same(ref, same)
                assert ref["info"] == same["info"]
            r, info, handle = cu.coarsen(dll, baker, src.rd, cap, mixed)
            assert r == ot.SUCCESS and info == same["info"]
            cu.assert_same(cu.download_result(dll, hip, handle), same)
            assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
    finally:
        src.close()


def test_levels_send_one_deep_block_down(dll, hip, baker):
    """the level-12 block sent to 3 while its level-10 neighbour stays (the deep list holds one of the two), the other way round, and both; levels set
    for descriptors that no primitive selects or that are invalid have no effect"""
    blocks = [(cu.planted_states(12, 2, seed=5), 12, 2), (cu.planted_states(10, 2, seed=6), 10, 2), (cu.planted_states(9, 2, seed=7), 9, 2)]
    array_data, descs = cu.table_of_blocks(blocks)
    descs = np.concatenate([descs, [[0, 13, 2], [1 << 30, 3, 2]]])          # 3, 4: invalid (level 13; past the array)
    src = cu.Source(hip, array_data, descs, [0, 1, 0, 3, 4], ot.IDX_U32, array_align=256)          # (block 2 is unreferenced)
    try:
        for own in ([3, 12, 0, 0, 0], [12, 2, 1, 1, 1], [3, 4, 5, 6, 7], [6, 255, 255, 0, 255]):
            ref = levels_and_check(dll, hip, baker, src, own, 12, 3, cu.NO_SPECIAL | cu.NO_DEDUP)
            assert sorted(ref["descs"][:, 1].tolist()) == sorted([min(12, own[0]), min(10, own[1])]) and ref["info"]["skippedPrimitives"] == 2
    finally:
        src.close()


# ---- the fit ----
def fit_table(seed=7, count=24):
    """10 to 40 mixed blocks: planted blocks of levels 0..5 in both formats, the designed pairs (quadrants and alternating states), equal blocks with
    equal weights (ties), an unreferenced block, a block selected by many primitives"""
    rng = np.random.default_rng(seed)
    blocks = []
    for k in range(count - 8):
        level, bits = int(rng.integers(0, 6)), int(rng.integers(1, 3))
        blocks.append((cu.planted_states(level, bits, seed * 100 + k), level, bits))
    blocks += fu.designed_blocks(3, 2, 2) + [blocks[3], blocks[3], blocks[5], (cu.planted_states(4, 2, 999), 4, 2)]
    array_data, descs = cu.table_of_blocks(blocks, first_offset=1, gap=1)
    n = len(blocks)
    index = np.concatenate([np.arange(n - 1), [3] * 5, [n - 3] * 5, [n - 2] * 5, rng.integers(-5, n - 1, 40)])          # (the last block is unreferenced)
    weights = np.ones(len(index), np.float32)
    weights[:n - 1] = (rng.integers(1, 6, n - 1) / 4).astype(np.float32)
    weights[[3, n - 3, n - 2]] = 0.5                                                                                     # (equal blocks, equal weights)
    return array_data, descs, index, weights


def fit_and_check(dll, hip, baker, src, budget, weights, dev_weights, prof, cap=12, mixed=3, flags=0):
    """the whole contract of one fit -> (plan, model result)"""
    a, d, i = src.host
    plan, ref = fu.restate_fit(a, d, i, src.rd.indexFormat, budget, weights, cap, mixed, flags, profile=prof, unpacked=src.unpacked)
    assert plan["feasible"]
    want = dict(unfittedArrayDataSize=plan["unfitted"], plannedArrayDataSize=plan["planned"], steps=plan["steps"], result=ref["info"])
    r0, info0, levels0, _ = fu.fit(dll, hip, baker, src.rd, budget, dev_weights, cap, mixed, flags, want_result=False)
    r, info, levels, handle = fu.fit(dll, hip, baker, src.rd, budget, dev_weights, cap, mixed, flags)
    assert (r0, info0) == (ot.SUCCESS, want) and (r, info) == (ot.SUCCESS, want), (budget, info0, info, want)
    try:
        assert levels.tolist() == plan["levels"] == levels0.tolist()
        got = cu.download_result(dll, hip, handle)
        cu.assert_same(got, ref)
        assert got["rdesc"].arrayDataSize == info["result"]["arrayDataSize"] <= info["plannedArrayDataSize"] <= budget
        r2, info2, h2 = fu.coarsen_levels(dll, hip, baker, src.rd, levels, 12, mixed, flags)
        assert (r2, info2) == (ot.SUCCESS, info["result"])
        try:
            cu.assert_same(cu.download_result(dll, hip, h2), got)
        finally:
            assert dll.ommxDestroyDeviceBakeResult(h2) == ot.SUCCESS
        assert src.unchanged()
    finally:
        assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
    return plan, ref


@pytest.mark.parametrize("mixed", [2, 3], ids=["ut", "uo"])
@pytest.mark.parametrize("flags", [cu.NONE, cu.NO_SPECIAL, cu.NO_DEDUP, cu.NO_SPECIAL | cu.NO_DEDUP], ids=["default", "no_special", "no_dedup", "neither"])
def test_fit_budget_sweep(dll, hip, baker, flags, mixed):
    """budgets from 0 (from the least feasible size without special indices) to the unfitted size on fit_table(): the output, the levels, the identity with
    ommxCoarsenMicromapLevels on the returned levels, the info-only call, arrayDataSize <= budget.  On the model: the sweep steps in more than three
    blocks and meets ties; the levels are monotone in the budget."""
    array_data, descs, index, weights = fit_table()
    src = cu.Source(hip, array_data, descs, index, ot.IDX_U16, array_align=1)
    dev = hip.upload(weights)
    try:
        prof = fu.restate_profile(array_data, descs, index, weights, unpacked=src.unpacked)
        special = not flags & cu.NO_SPECIAL
        floor = fu.restate_plan(prof["shape"], prof["known"], prof["opaque"], prof["weights"], 0, 12, special)
        assert floor["feasible"] == special and floor["ties"] > 0 and len(set(floor["stepped"])) > 3
        top, low = floor["unfitted"], floor["planned"]
        last = None
        for budget in sorted({low, low + 1, low + 7, (low + top) // 16, (low + top) // 5, (low + top) // 2, top - 40, top - 1}, reverse=True):
            plan, ref = fit_and_check(dll, hip, baker, src, budget, weights, dev, prof, 12, mixed, flags)
            assert plan["steps"] > 0 and (last is None or all(x <= y for x, y in zip(plan["levels"], last)))
            last = plan["levels"]
        fit_and_check(dll, hip, baker, src, (low + top) // 3, weights, dev, prof, 3, mixed, flags)          # with a global cap first
        # unweighted: every primitive counts 1
        prof1 = fu.restate_profile(array_data, descs, index, None, unpacked=src.unpacked)
        fit_and_check(dll, hip, baker, src, (low + top) // 4, None, None, prof1, 12, mixed, flags)
    finally:
        hip.free(dev)
        src.close()


def test_fit_infeasible_and_roomy_budgets(dll, hip, product):
    """without special indices no block goes below one byte: a budget under the number of blocks is FAILURE with a log line, the handle, the levels and
    the source untouched.  A budget at or above the unfitted size takes no step and equals ommxCoarsenMicromap at the cap."""
    msgs = []
    b = product.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    array_data, descs, index, weights = fit_table()
    src = cu.Source(hip, array_data, descs, index, ot.IDX_U16, array_align=1)
    try:
        prof = fu.restate_profile(array_data, descs, index, None, unpacked=src.unpacked)
        floor = fu.restate_plan(prof["shape"], prof["known"], prof["opaque"], prof["weights"], 0, 12, False)
        assert not floor["feasible"] and floor["planned"] == prof["info"]["referencedBlocks"]
        lv = hip.upload(np.full(64, 0xEE, np.uint8))
        for want_result in (True, False):
            out, info = C.c_void_p(0x5EED), fu.FitInfo()
            info.steps = 77
            r = dll.ommxFitMicromap(b, C.byref(src.rd), C.byref(fu.f_desc(floor["planned"] - 1, None, 12, 3, cu.NO_SPECIAL)), lv, C.byref(out) if want_result else None,
                                    C.byref(info), None)
            assert r == ot.FAILURE and out.value == 0x5EED and info.steps == 77 and "maxArrayDataSize" in msgs[-1][1] and len(msgs) == 1 + (not want_result)
            assert (hip.download(lv, 64) == 0xEE).all() and src.unchanged()
        hip.free(lv)
        for cap, flags in ((12, cu.NONE), (2, cu.NO_SPECIAL), (4, cu.NO_DEDUP)):
            same = src.model(cap, 2, flags)
            whole = fu.restate_plan(prof["shape"], prof["known"], prof["opaque"], prof["weights"], 1 << 40, cap, not flags & cu.NO_SPECIAL)
            for budget in (whole["unfitted"], whole["unfitted"] + 1, (1 << 64) - 1):
                plan, ref = fit_and_check(dll, hip, b, src, budget, None, None, prof, cap, 2, flags)
                assert plan["steps"] == 0 and ref["info"] == same["info"]
                cu.assert_same(ref, same)
    finally:
        src.close()
        product.destroy_baker(b)


def test_fit_designed_input(dll, hip, baker):
    """fit_util.designed_blocks (test_fit.py proves the claim on the model): at 4 * 64 + 4 bytes the fit keeps every known micro-triangle -- the quadrant
    blocks at level 1, the alternating ones untouched -- where the best global cap that fits (level 3) keeps a half.  Measured on the outputs with the
    statistics entry: no micro-triangle of the fitted result is unknown, half of the capped result's are."""
    blocks = fu.designed_blocks(4, 2, 4)
    array_data, descs = cu.table_of_blocks(blocks)
    src = cu.Source(hip, array_data, descs, list(range(8)), ot.IDX_U8)
    try:
        prof = fu.restate_profile(array_data, descs, list(range(8)), None, unpacked=src.unpacked)
        budget = 4 * 64 + 4
        plan, ref = fit_and_check(dll, hip, baker, src, budget, None, None, prof, 12, 3, cu.NO_DEDUP)
        assert plan["levels"] == [1] * 4 + [4] * 4 and ref["info"]["arrayDataSize"] == budget
        cap, cap_levels = fu.best_global_cap(prof, budget)
        assert cap == 3 and fu.known_share(prof, plan["levels"]) == 2 * fu.known_share(prof, cap_levels) == 8 * 4 ** 12
        r, info, levels, fitted = fu.fit(dll, hip, baker, src.rd, budget, None, 12, 3, cu.NO_DEDUP)
        r2, info2, capped = cu.coarsen(dll, baker, src.rd, cap, 3, cu.NO_DEDUP)
        assert r == r2 == ot.SUCCESS and info2["arrayDataSize"] <= budget
        try:
            f, c = (cu.device_stats(dll, baker, cu.result_desc_of(dll, h))[0] for h in (fitted, capped))
            # (stats_util.INT_FIELDS: opaque, transparent, unknown transparent, unknown opaque, then fully opaque, transparent, unknown opaque, unknown
            #  transparent; the alternating blocks are wholly unknown under the cap, hence promoted to FullyUnknownOpaque)
            assert f == (4 * 2 + 4 * 128, 4 * 2 + 4 * 128, 0, 0, 0, 0, 0, 0) and c == (4 * 32, 4 * 32, 0, 0, 0, 0, 4, 0)
        finally:
            assert dll.ommxDestroyDeviceBakeResult(fitted) == ot.SUCCESS and dll.ommxDestroyDeviceBakeResult(capped) == ot.SUCCESS
    finally:
        src.close()


def test_fit_a_real_bake(product, dll, hip):
    """ommxBakeDevice of a known-answer case (tests/kat_cases.py) with its own triangle areas as weights, fitted to a half and to a sixteenth of its
    size: the output equals the model from the downloaded source; for random hits through ommxLookupOpacity, wherever the fitted state is known it equals
    the source's state; the output is accepted by the statistics entry and by ommxFitMicromap again (at its own size: no step, the same bytes)."""
    c = next(k for k in kat_cases.CASES if k["name"] == "Mandelbrot")
    b = product.create_baker()
    tex = product.create_texture(b, [kat_runner.texture_array(c["tex"], c["size"], c["param"])])
    uv, ix = np.array(c["uv"], np.float32), np.array(c["ix"], np.uint32)
    rng = np.random.default_rng(7)
    try:
        d = ot.make_desc(tex, uv, ix, 7, fmt=ot.FMT_4STATE, promo=ot.PROMO_NEAREST)
        bake = lu.DeviceBake(product, hip, b, d, uv, ix)
        try:
            res = bake.host
            areas = C.c_void_p()
            assert dll.ommxGetDeviceBakeResultTriangleAreas(bake.out, C.byref(areas)) == ot.SUCCESS and areas.value
            weights = hip.download(areas, 4 * len(res.index), np.float32)
            prof = fu.restate_profile(res.array_data, res.descs, res.index, weights)
            plevel, _ = lu.prim_levels(res)
            prims = rng.integers(0, len(res.index), 20000)
            micro = (rng.random(20000) * (4.0 ** plevel[prims])).astype(np.int64)
            u, v = lu.interior_points(rng, lu.micro_vertices(micro, plevel[prims]))
            hits = np.empty(20000, lu.HIT)
            hits["prim"], hits["u"], hits["v"] = prims, u, v
            source_states = lu.lookup_device(dll, hip, bake.rdesc, hits)
            size = len(res.array_data)
            for budget in (size // 2, size // 16):
                plan, ref = fu.restate_fit(res.array_data, res.descs, res.index, res.index_format, budget, weights, profile=prof)
                r, info, levels, handle = fu.fit(dll, hip, b, bake.rdesc, budget, areas)
                assert r == ot.SUCCESS and plan["steps"] > 0 and levels.tolist() == plan["levels"]
                assert info == dict(unfittedArrayDataSize=plan["unfitted"], plannedArrayDataSize=plan["planned"], steps=plan["steps"], result=ref["info"])
                try:
                    got = cu.download_result(dll, hip, handle)
                    cu.assert_same(got, ref)
                    assert got["rdesc"].arrayDataSize <= budget
                    fitted_states = lu.lookup_device(dll, hip, got["rdesc"], hits)
                    known = fitted_states < 2
                    assert known.any() and np.array_equal(fitted_states[known], source_states[known])
                    want = su.reference_stats(ref["array"], ref["descs"], ref["index"])
                    assert cu.device_stats(dll, b, got["rdesc"]) == (want["fields"], 0)
                    r, again, _, h2 = fu.fit(dll, hip, b, got["rdesc"], got["rdesc"].arrayDataSize, None)
                    assert r == ot.SUCCESS and again["steps"] == 0 and again["result"]["arrayDataSize"] == got["rdesc"].arrayDataSize
                    try:
                        cu.assert_same(cu.download_result(dll, hip, h2), got)
                    finally:
                        assert dll.ommxDestroyDeviceBakeResult(h2) == ot.SUCCESS
                finally:
                    assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
        finally:
            bake.close()
    finally:
        product.destroy_texture(b, tex)
        product.destroy_baker(b)
