"""The restatement of the sharded block exchange (tests/shard_cases.py) held to code it did not come from, and the cases of tests/test_shard_gpu.py held
to what they claim, with the oracle alone.  No GPU.  Every test that bakes prints the oracle's time of its cases and bounds it at 3 s."""
import os
import subprocess
from math import gcd
import numpy as np
import pytest
import ommtest as ot
import tail_cases as tc
import shard_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_of(case):
    ref, raw, seconds = sc.reference(case)
    print("%s: oracle %.2f s" % (case["name"], seconds))
    assert seconds < 3.0, (case["name"], seconds)
    return ref, raw


# ---- ownership and interleave ----
def test_interleave_is_a_bijection_for_every_count():
    for cnt in range(1, 5001):
        p = sc.restate_interleave(cnt, 2)
        assert len(p) == cnt and np.array_equal(np.sort(p), np.arange(cnt)), cnt
        assert np.array_equal(sc.restate_interleave(cnt, 1), np.arange(cnt))
        if cnt >= 3:
            s = sc.interleave_stride(cnt)
            assert 1 <= s < cnt and gcd(s, cnt) == 1, (cnt, s)
            assert np.array_equal(p, (np.arange(cnt) * s) % cnt)
        else:
            assert np.array_equal(p, np.arange(cnt))


def test_interleave_stride_table():
    """by hand: 3 * 0.618 = 1.85 -> 1; 4 * 0.618 = 2.47 -> 2, gcd 2 -> 3; 6 * 0.618 = 3.7 -> 3, gcd 3 -> 4, gcd 2 -> 5; 10 * 0.618 = 6.18 -> 6, gcd 2 -> 7;
    257 * 0.618 = 158.8 -> 158, 257 is prime"""
    assert [sc.interleave_stride(c) for c in (3, 4, 6, 10, 257)] == [1, 3, 5, 7, 158]
    assert sc.restate_interleave(4).tolist() == [0, 3, 2, 1] and sc.restate_interleave(6).tolist() == [0, 5, 4, 3, 2, 1]
    assert sc.restate_interleave(10).tolist() == [0, 7, 4, 1, 8, 5, 2, 9, 6, 3]


@pytest.mark.parametrize("world", sc.WORLDS)
def test_bounds_partition_every_level(world):
    for kind in sc.O_KINDS:
        counts = sc.o_counts(kind, world)
        per_level = [counts.get(L, 0) for L in range(13)]
        own = sc.restate_bounds(per_level, world)
        assert len(own) == sum(per_level)
        a = 0
        for cnt in per_level:
            o = own[a:a + cnt]
            assert (np.diff(o) >= 0).all() and (not cnt or (0 <= o.min() and o.max() < world))
            share = np.bincount(o, minlength=world)
            assert share.sum() == cnt and share.max() - share.min() <= 1           # contiguous, complete, even to one item
            for r in range(world):
                assert share[r] == cnt * (r + 1) // world - cnt * r // world
            a += cnt
    union = set()
    for kind in sc.O_KINDS:
        c = sc.o_counts(kind, world)
        union |= {c.get(L, 0) for L in range(min(c), max(c) + 1)}
    assert {0, 1, 2, 3, 4, 6, 10, world - 1, world, world + 1, 255, 256, 257, 1025} <= union, union
    # by hand: 10 items over 3 ranks -> [0, 3), [3, 6), [6, 10); 2 items over 3 ranks -> rank 0 owns nothing
    assert sc.restate_bounds([10], 3).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2] and sc.restate_bounds([2], 3).tolist() == [1, 2]
    assert sc.restate_bounds([0, 2, 0, 1], 2).tolist() == [0, 1, 1]


@pytest.mark.parametrize("world", sc.WORLDS[1:])
def test_a_boundary_rounded_up_moves_an_owner_in_every_o_case(world):
    """the wrong variant `cnt * r / world` rounded up gives another owner to at least one list position of every O case from world 2 on"""
    for kind in sc.O_KINDS:
        counts = sc.o_counts(kind, world)
        per_level = [counts.get(L, 0) for L in range(13)]
        wrong = []
        for cnt in per_level:
            b = [-(-cnt * r // world) for r in range(world + 1)]
            own = np.zeros(cnt, np.int64)
            for r in range(world):
                own[b[r]:b[r + 1]] = r
            wrong.append(own)
        assert (np.concatenate(wrong) != sc.restate_bounds(per_level, world)).any(), (kind, world)


def test_list_order_and_owners_by_hand():
    """levels 1, 0, 1, 1, 0, 1 -> natural list: items 1, 4 (level 0) then 0, 2, 3, 5 (level 1); world 2 interleaves the four level-1 items with stride 3"""
    lst, own, counts = sc.list_items([1, 0, 1, 1, 0, 1], 2)
    assert lst.tolist() == [1, 4, 0, 5, 3, 2] and own.tolist() == [0, 1, 0, 0, 1, 1] and counts[:2].tolist() == [2, 4]
    assert sc.item_owners([1, 0, 1, 1, 0, 1], 2).tolist() == [0, 0, 1, 1, 1, 0]
    assert sc.list_items([1, 0, 1, 1, 0, 1], 1)[0].tolist() == [1, 4, 0, 2, 3, 5]


# ---- the codec ----
def adversarial_arrays():
    rng = np.random.default_rng(3)
    out = [np.zeros(0, np.uint8), np.zeros(256, np.uint8), np.full(256, 0x55, np.uint8), np.full(4096, 0xAA, np.uint8), np.full(4096 + 256, 0xFF, np.uint8),
           rng.integers(0, 256, 256).astype(np.uint8), rng.integers(0, 256, 4096).astype(np.uint8), rng.integers(0, 256, 3 * 4096 + 512).astype(np.uint8)]
    for n_units, raw_lanes in ((256, [0]), (256, [255]), (256, [63, 64]), (512, [255, 256]), (272, [271]), (4096 + 16, list(range(0, 4112, 2))), (4096 - 16, [4079])):
        a = np.repeat(np.array([0x00, 0x55, 0xAA, 0xFF], np.uint8)[rng.integers(0, 4, n_units)], 16)
        for u in raw_lanes:
            a[16 * u:16 * u + 16] = rng.integers(0, 256, 16)
            a[16 * u] ^= 1                                                            # (never a plateau by accident)
        out.append(a)
    near = np.full(512, 0x55, np.uint8)
    near[15] = 0x54                      # a unit that differs from its plateau in the last byte of its last word
    near[16 + 12] = 0x15                 # ... in the first byte of its last word
    near[32:48] = np.tile(np.array([0x55, 0x55, 0x55, 0x55, 0xAA, 0xAA, 0xAA, 0xAA], np.uint8), 2)      # words of two plateaus
    near[48:52] = 0                                                                  # first word of another plateau
    out.append(near)
    return out


def test_codec_round_trip_and_layout():
    for a in adversarial_arrays():
        s = sc.codec_encode(a)
        L = sc.codec_layout(a.size)
        assert np.array_equal(sc.codec_decode(s), a), a.size
        assert len(s) % 16 == 0 and L["offCodes"] % 16 == 0 and L["offRaw"] % 16 == 0 and L["offCodes"] >= 16 + 4 * (L["blocks"] + 1)
        assert len(s) == L["offRaw"] + 16 * int((sc.codec_unit_codes(a) == 4).sum() if a.size else 0)
    # by hand: 4096 bytes = 256 units = 1 block: offsets at 16 (2 words), codes at 32 (128 bytes), raw units at 160
    assert sc.codec_layout(4096) == dict(units=256, blocks=1, offOfs=16, offCodes=32, offRaw=160)
    assert sc.codec_layout(4096 + 256) == dict(units=272, blocks=2, offOfs=16, offCodes=32, offRaw=176)
    assert sc.codec_layout(65536) == dict(units=4096, blocks=16, offOfs=16, offCodes=96, offRaw=2144)
    near = adversarial_arrays()[-1]
    assert sc.codec_unit_codes(near)[:5].tolist() == [4, 4, 4, 4, 1]
    assert sc.comp_cap(65536) == 36864 and sc.comp_cap(256) == 4352 and sc.multi_device_cap(65536) == 2144 + 32768 + 16
    assert sc.chunk_bytes(22016, 256) == 2816 and len(sc.chunk_sizes(22016, 256)) == 8 and sum(sc.chunk_sizes(22016, 256)) == 22016
    assert sc.chunk_bytes(22016, 4352) == 3840 and sc.chunk_bytes(22016) == 22016 and sc.chunk_sizes(256, 256) == [256]


def test_numpy_streams_through_the_host_expansion(tmp_path):
    """a stand-alone program under AddressSanitizer and UBSan feeds numpy-encoded streams to host_expand.cpp's codec_expand_blocks and compares the
    output with the original bytes: the adversarial arrays, and the padded contributions of the C cases"""
    arrays = adversarial_arrays()
    for case in (sc.c_pattern_case(), sc.c_limit_case(0), sc.c_limit_case(1), sc.c_size_case(17), sc.c_size_case(257, ot.FMT_4STATE, ot.UT, ot.UO)):
        ref, _ = ref_of(case)
        arrays.append(sc.padded(ref.array_data, sc.pad256(ref.array_data.size)))
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for a in arrays:
            s = sc.codec_encode(a)
            f.write(np.array([a.size, s.size], "<u8").tobytes() + a.tobytes() + s.tobytes())
    exe = str(tmp_path / "codec_stream_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                        "-I" + os.path.join(ROOT, "omm_amd", "csrc"), os.path.join(ROOT, "tests", "native", "codec_stream_check.cpp"),
                        os.path.join(ROOT, "omm_amd", "csrc", "host_expand.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok %d streams" % len(arrays)), (r.stdout[-2000:], r.stderr[-4000:])


# ---- what the cases claim ----
def owners_of(case, raw, world):
    own, rs, inp = sc.block_owners(case, raw, world)
    return own, rs, inp


@pytest.mark.parametrize("world", sc.WORLDS)
@pytest.mark.parametrize("kind", sc.O_KINDS)
def test_o_cases(kind, world):
    case = sc.o_case(kind, world)
    ref, raw = ref_of(case)
    own, rs, inp = owners_of(case, raw, world)
    tc.check_result(case, ref, rs)                                        # the restated tail, hence `order`, is the oracle's
    got = {L: int(c) for L, c in enumerate(np.bincount(inp["level"], minlength=9)) if c}
    assert got == case["counts"] and len(inp["level"]) == len(case["uv"]) // 3
    if kind != "tiny":
        assert min(got) < 4 < max(got) or 4 in got                       # populated levels on both sides of an empty one
        empty = [L for L in range(min(got), max(got)) if L not in got]
        assert empty, got
    io = sc.item_owners(inp["level"], world)
    share = np.bincount(io, minlength=world)
    if kind == "tiny" and world >= 5:
        assert (share == 0).sum() >= world - 3                           # whole ranks own nothing
    masks = sc.item_masks(inp)
    assert (masks != 0).all()
    mixed = (masks & (masks - 1)) != 0
    dg = sc.item_digests(inp)
    assert len(set(dg[inp["level"] >= 5].tolist())) == int((inp["level"] >= 5).sum())       # blocks of 256 bytes and more: all digests distinct
    for L, cnt in got.items():                                                            # below: enough different items that a wrong order shows
        assert cnt < 3 or len(set(dg[inp["level"] == L].tolist())) >= 3, (L, cnt)


@pytest.mark.parametrize("fmt", tc.FORMATS)
@pytest.mark.parametrize("kind", sc.L_KINDS)
def test_l_cases(kind, fmt):
    case = sc.l_case(kind, fmt)
    ref, raw = ref_of(case)
    bits = 2 if fmt == ot.FMT_4STATE else 1
    sizes = tc.block_bytes(ref.descs[:, 1], bits)
    assert set(sizes.tolist()) == {int(tc.block_bytes(L, bits)) for L in range(9)} and sizes.max() == 8192 * bits and sizes.min() == 1
    assert (len(ref.descs) > 256) == (kind == "many") and len(ref.descs) == len(case["uv"]) // 3
    for world in (2, 3):
        own, rs, inp = owners_of(case, raw, world)
        tc.check_result(case, ref, rs)
        con, nbytes, stride = sc.restate_contributions(ref, own, world)
        assert sum(nbytes) == ref.array_data.size and stride % 256 == 0 and stride >= max(nbytes) > stride - 256
        if kind == "few":
            # the chunked scatter: 16 KiB (8 KiB) blocks in front, blocks under 16 bytes behind them; chunks cut blocks; a knob value that gives 8 chunks
            assert any(n % 16 for n in nbytes) and stride > 8 * 256
            knob8 = sc.pad256(stride // 8)
            assert len(sc.chunk_sizes(stride, knob8)) == 8 and len(sc.chunk_sizes(stride, 256)) == 8 and len(sc.chunk_sizes(stride, 4352)) >= 2
            assert sc.chunk_bytes(stride, 256) < sizes.max()
    if kind == "few":
        assert 0 in sc.restate_contributions(ref, owners_of(case, raw, 3)[0], 3)[1]          # two items per level over three ranks: rank 0 owns nothing


def test_l_duplicates_case():
    case = sc.l_duplicates_case()
    ref, raw = ref_of(case)
    for world in (2, 3):
        own, rs, inp = owners_of(case, raw, world)
        tc.check_result(case, ref, rs)
        io = sc.item_owners(inp["level"], world)
        copies = np.nonzero(rs["rep"] != np.arange(len(io)))[0]
        assert np.array_equal(rs["rep"][48:], rs["rep"][:48]) and len(ref.descs) >= 40        # every copy repeats its original, which keeps the block
        assert (io[copies] != io[rs["rep"][copies]]).sum() >= 10                              # ... on another rank than the copy's
        con, nbytes, stride = sc.restate_contributions(ref, own, world)
        assert sum(nbytes) == ref.array_data.size == len(ref.descs) * 16


@pytest.mark.parametrize("kind", sc.E_KINDS)
def test_e_cases(kind):
    case = sc.e_case(kind)
    ref, raw = ref_of(case)
    if kind == "nothing-valid":
        assert raw is None and len(ref.descs) == 0 and (ref.index == ot.SPECIAL_FUO).all()
    elif kind == "all-uniform":
        assert len(ref.descs) == 0 and ref.array_data.size == 0 and set(ref.index.tolist()) == {ot.SPECIAL_FT, ot.SPECIAL_FO}
        assert sc.restate_contributions(ref, np.zeros(0, np.int64), 8)[1:] == ([0] * 8, 256)
    else:
        assert len(ref.descs) == 1
        con, nbytes, stride = sc.restate_contributions(ref, owners_of(case, raw, 8)[0], 8)
        assert sorted(nbytes) == [0] * 7 + [16] and stride == 256


@pytest.mark.parametrize("fmt,le,gt", [(f, le, gt) for f in tc.FORMATS for le, gt in sc.U_STATES[f]])
def test_u_cases(fmt, le, gt):
    case = sc.u_case(fmt, le, gt)
    ref, raw = ref_of(case)
    inp = tc.tail_inputs(case, raw)
    rs = tc.restate_tail(inp, case["flags"])
    tc.check_result(case, ref, rs)
    side = case["side"]
    assert np.array_equal(rs["uniform"], side >= 0)                       # U's uniform items are uniform, the others are not
    masks = sc.item_masks(inp)
    uni_levels = sorted(set(inp["level"][side >= 0].tolist()))
    assert uni_levels == sc.U_LEVELS and sorted(set(inp["level"][side < 0].tolist())) == [1, 2, 3, 5]
    for L in sc.U_LEVELS:
        assert {int(m) for m in masks[(side >= 0) & (inp["level"] == L)]} == {1 << le, 1 << gt}, L      # both states of the mapping at every level
    assert len(ref.descs) == len(side) and np.abs(np.diff((side >= 0).astype(int))).sum() > 30          # every item a block; uniform and mixed interleaved


@pytest.mark.parametrize("n", sc.C_SIZES)
def test_c_size_cases(n):
    for fmt, le, gt in ((ot.FMT_4STATE, ot.T, ot.O), (ot.FMT_4STATE, ot.UT, ot.UO), (ot.FMT_2STATE, ot.T, ot.O)):
        case = sc.c_size_case(n, fmt, le, gt)
        ref, raw = ref_of(case)
        block = 256 if fmt == ot.FMT_4STATE else 512
        assert ref.array_data.size == n * block and len(ref.descs) == n                      # blocks of 256 bytes or more: the contribution is arrayData
        codes = sc.codec_unit_codes(ref.array_data)
        assert len(codes) == n * block // 16
        plateau = {(ot.FMT_4STATE, ot.T): {0, 1}, (ot.FMT_4STATE, ot.UT): {2, 3}, (ot.FMT_2STATE, ot.T): {0, 3}}[(fmt, le)]
        assert set(codes.tolist()) <= plateau | {4}
        if n >= 15:
            assert set(codes.tolist()) == plateau | {4}                                       # 16-byte runs of both plateau bytes, and raw units
        s = sc.codec_encode(ref.array_data)
        assert len(s) <= sc.comp_cap(ref.array_data.size)
        assert np.array_equal(sc.codec_decode(s), ref.array_data)
    if n in (255, 257):
        L = sc.codec_layout(n * 256)
        assert L["units"] == 4096 + (16 if n == 257 else -16) and L["blocks"] == (17 if n == 257 else 16)       # a last partial codec block / dead lanes


def test_c_pattern_case():
    case = sc.c_pattern_case()
    ref, raw = ref_of(case)
    assert ref.array_data.size == 2 * 16384
    counts = sc.pattern_holds(case, ref.array_data)
    print("raw units per codec block:", counts)
    _, rawu = sc.raw_units_per_block(ref.array_data)
    lanes = {int(u) % 256 for u in np.nonzero(rawu)[0]}
    assert {0, 63, 64, 255} <= lanes


@pytest.mark.parametrize("over", [0, 1])
def test_c_limit_case(over):
    case = sc.c_limit_case(over)
    ref, raw = ref_of(case)
    stride = ref.array_data.size
    assert stride == 65536 and len(ref.descs) == sc.LIMIT_ITEMS
    s = sc.codec_encode(ref.array_data)
    assert len(s) == sc.comp_cap(stride) + 16 * over == case["want_stream"], (len(s), sc.comp_cap(stride))
    if over:
        assert sc.chunk_sizes(stride, 256) == [8192] * 8 and sc.chunk_sizes(stride) == [65536]


def test_ragged_case():
    case = sc.ragged_case()
    ref, raw = ref_of(case)
    assert ref.array_data.size % 16 != 0 and ref.array_data.size > 6 * 256


@pytest.mark.parametrize("world", [2, 3, 8])
def test_m_cases(world):
    case = sc.mixed_case(world)
    ref, raw = ref_of(case)
    own, rs, inp = owners_of(case, raw, world)
    tc.check_result(case, ref, rs)
    con, nbytes, stride = sc.restate_contributions(ref, own, world)
    lens = [len(sc.codec_encode(sc.padded(c, stride))) for c in con]
    print(case["name"], nbytes, stride, lens, sc.comp_cap(stride), sc.multi_device_cap(stride))
    assert lens[0] > sc.comp_cap(stride) and max(lens[1:]) < 2048                             # one rank incompressible, the others far from it
    assert lens[0] > sc.multi_device_cap(stride) > max(lens[1:])                              # ... by the multi-device rule as well
    case = sc.lengths_case(world)
    ref, raw = ref_of(case)
    own, rs, inp = owners_of(case, raw, world)
    tc.check_result(case, ref, rs)
    con, nbytes, stride = sc.restate_contributions(ref, own, world)
    lens = [len(sc.codec_encode(sc.padded(c, stride))) for c in con]
    assert len(set(lens)) >= 2 and max(lens) <= sc.comp_cap(stride) and lens[0] == sc.codec_layout(stride)["offRaw"]      # rank 0: no raw unit
    for r, c in enumerate(con):                                                                # rank r's items carry r % 4 raw units each
        assert lens[r] == sc.codec_layout(stride)["offRaw"] + 16 * (r % 4) * int((own == r).sum())
