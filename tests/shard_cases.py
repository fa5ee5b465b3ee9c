"""The block exchange of a sharded bake (omm_amd/csrc/tail_kernels.hip: shard_interleave, owner_of_position, shard_pack_meta / shard_unpack_meta,
shard_masked_sizes / shard_take_offsets, shard_gather_contribution, shard_scatter_contributions, the device codec shard_codec_* and
shard_scatter_streams; bake_host.h: rank_ranges and interleave_stride; omm_host.cpp: sharded_tail's stride and cap, shard_chunk_bytes) restated in numpy / Python, and the
cases of tests/test_shard_reference.py (no GPU) and tests/test_shard_gpu.py.

What is restated, from the comments and the code named above:
  restate_bounds       active-list positions level by level, ascending; rank r owns [a + cnt * r // world, a + cnt * (r + 1) // world) of a level
  restate_interleave   list position j of a level of cnt >= 3 items holds natural position (j * stride) % cnt when world > 1; stride is
                       int(cnt * 0.6180339887498949), at least 1, incremented until coprime to cnt, then taken % cnt
  codec_encode / _decode   the stream of the "block exchange codec" comment: 16-byte header (stream bytes, units) | blocks + 1 uint32 first raw unit of
                       every 256-unit block | one nibble per 16-byte unit (0..3: sixteen bytes of 0x00 / 0x55 / 0xAA / 0xFF, 4: raw) | the raw units.
                       codec_layout's three offsets and codec_unit_code are written out here, not imported.  The bytes between the sections (up to 12
                       behind the offsets, up to 15 behind the codes) are written by nobody on the device: codec_encode leaves them zero and
                       stream_defined() masks them in a comparison with a recorded stream.
  restate_contributions    a rank's contribution: the active blocks it owns, dense, in final order; contributionBytes; strideBytes = pad256(max), 256 for
                       an all-empty exchange
  comp_cap, chunk_bytes, multi_device_cap   the host's pad256(stride / 2 + 4096), shard_chunk_bytes, and offRaw + padded / 2 + 16

Which work item sits where.  Work items are numbered in triangle order (first occurrences); setup lists them level by level, ascending inside a level,
and the compaction keeps that order for the active ones (classify_cases.py, "Order").  With the Nearest filter and no cut-off table query every valid
item is active (the GPU tests assert numWords / 4 and activeItems), so the natural position of an item is its rank among the items in (level, item)
order.  The digest words of the metadata are held to XXH64 (seed 42, UT folded into UO) of the item's states from the oracle's decode at exactly those
positions, which is the check that this order is the device's.

Result arrays always come from the oracle.  Textures and triangles are built so that the oracle's decode shows the wanted pattern; a case whose decode
does not show it raises."""
import functools
from math import gcd
import numpy as np
import ommtest as ot
import tail_cases as tc
import classify_cases as cc

F = np.float32
GOLDEN = 0.6180339887498949
CODEC_BLOCK = 256                # units per codec block (kCodecBlock)
WORLDS = [1, 2, 3, 5, 8, 16]
MAX_RANKS = 16
DEDUP_FLAGS = ot.FLAG_THREADS | ot.FLAG_NO_SPECIAL          # digests are computed, every distinct block is emitted
EVERY_FLAGS = tc.EVERY_FLAGS                                # every work item emits a block (no digests)


def pad256(n):
    return (int(n) + 255) & ~255


# ---------------------------------------------------------------------------------------------------------------------------------------------
# ownership and interleave
# ---------------------------------------------------------------------------------------------------------------------------------------------
def interleave_stride(cnt):
    """the stride handed to shard_interleave (bake_core): already reduced % cnt"""
    stride = max(1, int(cnt * GOLDEN))
    while gcd(stride, cnt) != 1:
        stride += 1
    return stride % cnt


def restate_interleave(cnt, world=2):
    """natural position held by every list position of a level with cnt active items"""
    j = np.arange(cnt, dtype=np.int64)
    if world <= 1 or cnt < 3:
        return j
    return (j * interleave_stride(cnt)) % cnt


def restate_bounds(level_counts, world):
    """owner of every active-list position; level_counts[l] = active items of level l"""
    out = []
    for cnt in level_counts:
        cnt = int(cnt)
        b = [cnt * r // world for r in range(world + 1)]
        own = np.zeros(cnt, np.int64)
        for r in range(world):
            own[b[r]:b[r + 1]] = r
        out.append(own)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def natural_items(level):
    """work items in natural active-list order (every item active): level by level, ascending inside a level -> (items, counts of levels 0..12)"""
    level = np.asarray(level, np.int64)
    items = np.lexsort((np.arange(len(level)), level))
    return items, np.bincount(level, minlength=13)[:13]


def list_items(level, world):
    """the work item at every list position after the interleave, and the owner of every list position"""
    items, counts = natural_items(level)
    out, a = [], 0
    for cnt in counts:
        out.append(items[a:a + cnt][restate_interleave(int(cnt), world)])
        a += cnt
    return np.concatenate(out), restate_bounds(counts, world), counts


def item_owners(level, world):
    """owner of every work item (every item active)"""
    lst, own, _ = list_items(level, world)
    o = np.full(len(level), -1, np.int64)
    o[lst] = own
    return o


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the codec
# ---------------------------------------------------------------------------------------------------------------------------------------------
def codec_layout(nbytes):
    units = int(nbytes) // 16
    blocks = (units + CODEC_BLOCK - 1) // CODEC_BLOCK
    off_ofs = 16
    off_codes = (off_ofs + 4 * (blocks + 1) + 15) & ~15
    off_raw = (off_codes + (units + 1) // 2 + 15) & ~15
    return dict(units=units, blocks=blocks, offOfs=off_ofs, offCodes=off_codes, offRaw=off_raw)


def codec_unit_codes(data):
    """code of every 16-byte unit: 0..3 = four equal words of 0, 0x55555555, 0xAAAAAAAA, 0xFFFFFFFF; 4 = raw"""
    w = np.frombuffer(np.ascontiguousarray(data, np.uint8).tobytes(), "<u4").reshape(-1, 4)
    same = (w == w[:, :1]).all(axis=1)
    code = np.full(len(w), 4, np.uint8)
    for k, v in enumerate((0, 0x55555555, 0xAAAAAAAA, 0xFFFFFFFF)):
        code[same & (w[:, 0] == v)] = k
    return code


def codec_encode(data):
    data = np.ascontiguousarray(data, np.uint8)
    assert data.size % 256 == 0, data.size                  # contributions travel padded to 256 bytes: the unit count is even
    L = codec_layout(data.size)
    code = codec_unit_codes(data) if data.size else np.zeros(0, np.uint8)
    raw = code == 4
    per_block = np.add.reduceat(raw.astype(np.int64), np.arange(0, L["units"], CODEC_BLOCK)) if L["units"] else np.zeros(0, np.int64)
    ofs = np.concatenate([[0], np.cumsum(per_block)]).astype("<u4")
    total = L["offRaw"] + 16 * int(raw.sum())
    s = np.zeros(total, np.uint8)
    s[0:16] = np.frombuffer(np.array([total, L["units"]], "<u8").tobytes(), np.uint8)
    s[L["offOfs"]:L["offOfs"] + 4 * len(ofs)] = np.frombuffer(ofs.tobytes(), np.uint8)
    s[L["offCodes"]:L["offCodes"] + L["units"] // 2] = code[0::2] | (code[1::2] << 4)
    s[L["offRaw"]:] = data.reshape(-1, 16)[raw].reshape(-1)
    return s


def stream_defined(nbytes, stream_len):
    """True for the bytes of a stream that the device writes: everything but the alignment gaps behind the offsets and behind the codes"""
    L = codec_layout(nbytes)
    m = np.ones(stream_len, bool)
    m[L["offOfs"] + 4 * (L["blocks"] + 1):L["offCodes"]] = False
    m[L["offCodes"] + L["units"] // 2:L["offRaw"]] = False
    return m


def codec_decode(stream):
    stream = np.ascontiguousarray(stream, np.uint8)
    total, units = (int(v) for v in np.frombuffer(stream[:16].tobytes(), "<u8"))
    L = codec_layout(units * 16)
    ofs = np.frombuffer(stream[L["offOfs"]:L["offOfs"] + 4 * (L["blocks"] + 1)].tobytes(), "<u4").astype(np.int64)
    packed = stream[L["offCodes"]:L["offCodes"] + (units + 1) // 2]
    code = np.stack([packed & 15, packed >> 4], axis=1).reshape(-1)[:units]
    out = np.zeros((units, 16), np.uint8)
    for k, v in enumerate((0x00, 0x55, 0xAA, 0xFF)):
        out[code == k] = v
    rawu = stream[L["offRaw"]:total].reshape(-1, 16)
    for b in range(L["blocks"]):
        u = np.nonzero(code[b * CODEC_BLOCK:(b + 1) * CODEC_BLOCK] == 4)[0] + b * CODEC_BLOCK
        assert len(u) == ofs[b + 1] - ofs[b], (b, len(u), ofs[b], ofs[b + 1])
        out[u] = rawu[ofs[b]:ofs[b] + len(u)]            # the rank of a raw unit inside its block counts the raw units in front of it
    return out.reshape(-1)


def raw_units_per_block(data):
    """raw units of every 256-unit codec block of a (padded) contribution, and the raw flag of every unit"""
    data = np.ascontiguousarray(data, np.uint8)
    pad = np.zeros(pad256(data.size), np.uint8)
    pad[:data.size] = data
    raw = codec_unit_codes(pad) == 4
    n = -(-len(raw) // CODEC_BLOCK)
    return [int(raw[b * CODEC_BLOCK:(b + 1) * CODEC_BLOCK].sum()) for b in range(n)], raw


def comp_cap(stride):
    """sharded_tail: the capacity of a rank's stream; a stream longer than this makes every rank send raw"""
    return pad256(stride // 2 + 4096)


def chunk_bytes(stride, knob=0):
    """shard_chunk_bytes"""
    want = knob if knob else 64 << 20
    chunks = min(8, max(1, (stride + want - 1) // want))
    return (((stride + chunks - 1) // chunks) + 255) & ~255


def chunk_sizes(stride, knob=0):
    c = chunk_bytes(stride, knob)
    return [min(lo + c, stride) - lo for lo in range(0, stride, c)]


def multi_device_cap(padded):
    """multi-device ommCpuBake: a rank's stream above this goes to the host as it is (the raw flag is per rank there)"""
    return codec_layout(padded)["offRaw"] + padded // 2 + 16


# ---------------------------------------------------------------------------------------------------------------------------------------------
# contributions
# ---------------------------------------------------------------------------------------------------------------------------------------------
def restate_contributions(result, owners, world):
    """result: a full result (descs (offset, level, format), array_data); owners[k]: the rank that owns emitted block k, -1 for a block no rank sends
    (a uniform item that never became active: every rank synthesises it).  -> (contribution bytes of every rank, contributionBytes, strideBytes)"""
    d = np.asarray(result.descs, np.int64).reshape(-1, 3)
    owners = np.asarray(owners, np.int64)
    assert len(owners) == len(d)
    sizes = tc.block_bytes(d[:, 1], np.where(d[:, 2] == ot.FMT_4STATE, 2, 1)) if len(d) else np.zeros(0, np.int64)
    out = []
    for r in range(world):
        parts = [result.array_data[int(o):int(o + n)] for o, n, w in zip(d[:, 0], sizes, owners) if w == r]
        out.append(np.concatenate(parts) if parts else np.zeros(0, np.uint8))
    nbytes = [int(c.size) for c in out]
    stride = pad256(max(nbytes)) if nbytes and max(nbytes) else 256
    return out, nbytes, stride


def padded(contribution, stride):
    p = np.zeros(stride, np.uint8)
    p[:contribution.size] = contribution
    return p


def block_owners(case, raw, world):
    """owner of every emitted block of a case whose valid items are all active: the block of final position k belongs to work item order[k] of the
    restated tail (the first item with its digest), whose list position decides.  -> (owners, restated tail, tail inputs)"""
    inp = tc.tail_inputs(case, raw)
    rs = tc.restate_tail(inp, case["flags"], case["rejection"])
    own = item_owners(inp["level"], world)
    return own[rs["order"]], rs, inp


def item_digests(inp):
    """XXH64 (seed 42, UT folded into UO) of the states of every work item"""
    dg = np.zeros(len(inp["level"]), np.uint64)
    for L, (ids, S) in inp["groups"].items():
        dg[ids] = tc.digests_of_rows(S)
    return dg


def item_masks(inp):
    m = np.zeros(len(inp["level"]), np.uint32)
    for L, (ids, S) in inp["groups"].items():
        for s in range(4):
            m[ids] |= ((S == s).any(axis=1).astype(np.uint32) << np.uint32(s))
    return m


# ---------------------------------------------------------------------------------------------------------------------------------------------
# textures and triangles
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise256():
    """noise in cells of 4 x 4 texels: with the Nearest filter triangles of a few texels are known where they lie inside a cell and unknown across
    cell edges, so the items of a level differ from each other from level 0 on"""
    cells = np.random.default_rng(77).integers(0, 2, (64, 64)).astype(np.uint8) * 255
    return np.ascontiguousarray(np.kron(cells, np.ones((4, 4), np.uint8)))


def noise_triangles(levels, seed, size=256):
    """one triangle per entry of `levels` over the noise: legs of 1.5 * 2^L + 3 texels at seeded places, every vertex of its own"""
    levels = np.asarray(levels, np.int64)
    rng = np.random.default_rng(seed)
    n = len(levels)
    o = rng.random((n, 2)) * 0.9
    leg = (1.5 * 2.0 ** levels + 3.0) / size
    j = rng.random((n, 3)) * 0.2 / size
    uv = np.stack([o[:, 0] + j[:, 0], o[:, 1], o[:, 0] + leg, o[:, 1] + j[:, 1], o[:, 0], o[:, 1] + leg + j[:, 2]], axis=1).astype(F)
    assert len(np.unique(uv.reshape(-1, 2), axis=0)) == 3 * n               # no duplicate UVs: work item = triangle
    return uv


def counts_case(name, counts, seed, fmt=ot.FMT_4STATE, flags=DEDUP_FLAGS):
    """counts: {level: active items}; the triangles of all levels shuffled, so that item numbers of a level are spread over the input"""
    lv = np.concatenate([np.full(c, L, np.int64) for L, c in sorted(counts.items())] + [np.zeros(0, np.int64)])
    lv = lv[np.random.default_rng(seed).permutation(len(lv))]
    c = tc.make_case(name, noise256(), noise_triangles(lv, seed + 1), 8, levels=lv.astype(np.uint8), fmt=fmt, flags=flags, filt=ot.NEAREST, addr=ot.WRAP)
    c["counts"] = {L: n for L, n in counts.items() if n}
    return c


# ---- O ----
O_KINDS = ["big", "world", "tiny"]


def o_counts(kind, world):
    if kind == "big":
        return {0: 1025, 1: 257, 2: 256, 3: 255, 5: 10, 6: 6, 8: 3}
    if kind == "world":
        return {1: 1, 2: 2, 3: 4, 4: world - 1, 5: world, 6: world + 1, 8: 1}
    return {2: 1, 5: 2}                                      # three active items: from world 5 on whole ranks own nothing


@functools.lru_cache(maxsize=None)
def o_case(kind, world):
    return counts_case("O-%s-w%d" % (kind, world if kind == "world" else 0), o_counts(kind, world), 100 + O_KINDS.index(kind) * 20 + (world if kind == "world" else 0))


# ---- L ----
L_KINDS = ["few", "many"]


@functools.lru_cache(maxsize=None)
def l_case(kind, fmt):
    """both formats at levels 0 - 8: blocks of 1, 1, 2, 8, 32 ... 8192 bytes (2-state) and 1, 1, 4, 16, 64 ... 16384 bytes (4-state) in one bake;
    `many`: more than 256 blocks (more than one round of the scatter's workgroup loop needs more than 262144: not built)"""
    counts = {L: 2 for L in range(9)} if kind == "few" else {0: 70, 1: 70, 2: 70, 3: 60, 4: 40, 5: 8, 6: 3, 7: 2, 8: 2}
    return counts_case("L-%s-fmt%d" % (kind, fmt), counts, 300 + 7 * fmt + L_KINDS.index(kind), fmt=fmt, flags=EVERY_FLAGS)


@functools.lru_cache(maxsize=None)
def l_duplicates_case():
    """48 level-3 triangles on the 1/4096 grid and their copies one texture period to the right (Wrap: the same texels): separate work items with equal
    digests; the block stays with the lowest work item, whose list position decides the owner"""
    rng = np.random.default_rng(5)
    o = rng.integers(0, 3600, (48, 2)) / 4096.0
    leg = 256 / 4096.0
    a = np.stack([o[:, 0], o[:, 1], o[:, 0] + leg, o[:, 1], o[:, 0], o[:, 1] + leg], axis=1)
    b = a.copy()
    b[:, 0::2] += 1.0
    uv = np.concatenate([a, b]).astype(F)
    assert np.array_equal(uv[48:, 0::2] - F(1), uv[:48, 0::2])
    return tc.make_case("L-duplicates", noise256(), uv, 3, fmt=ot.FMT_4STATE, flags=DEDUP_FLAGS, filt=ot.NEAREST, addr=ot.WRAP)


# ---- E ----
E_KINDS = ["nothing-valid", "all-uniform", "one-block"]


@functools.lru_cache(maxsize=None)
def e_case(kind):
    if kind == "nothing-valid":          # a NaN or an infinity in every triangle: no work item at all
        uv = np.array([[0.1, 0.1, np.nan, 0.2, 0.3, 0.4], [0.2, np.inf, 0.2, 0.2, 0.5, 0.2], [0.1, 0.1, 0.3, 0.3, -np.inf, 0.5], [np.inf, 0.0, 0.1, 0.2, 0.3, 0.1]], F)
        return tc.make_case("E-nothing-valid", noise256(), uv, 4, fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS, filt=ot.NEAREST, addr=ot.WRAP)
    if kind == "all-uniform":            # Nearest: every item is classified and turns out uniform -> special indices, metadata but no OMM
        k = np.arange(12)
        x, y = np.where(k % 2 == 0, 0.06, 0.62) + 0.01 * (k // 2), 0.1 + 0.05 * k
        uv = np.stack([x, y, x + 0.05, y + 0.01, x + 0.02, y + 0.04], axis=1).astype(F)
        return tc.make_case("E-all-uniform", tc.halves(), uv, 5, levels=(k % 6).astype(np.uint8), fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS, filt=ot.NEAREST, addr=ot.CLAMP)
    return counts_case("E-one-block", {3: 1}, 41, flags=ot.FLAG_THREADS)


# ---- U ----
U_STATES = {ot.FMT_2STATE: [(ot.T, ot.O)], ot.FMT_4STATE: [(ot.T, ot.O), (ot.UT, ot.UO)]}
U_LEVELS = [0, 1, 2, 3, 5, 7]


@functools.lru_cache(maxsize=None)
def u_case(fmt, le, gt):
    """tail_cases.r2_case without special indices (Linear with a table over the two halves: the uniform items settle in the triage and never become
    active, so every rank writes their blocks itself), uniform items of levels 0, 1, 2, 3, 5, 7 in both states of the mapping, between non-uniform items
    of levels 1, 2, 3 and 5 that straddle the halves"""
    c = dict(tc.r2_case(fmt, le, gt, 0, EVERY_FLAGS))
    side, lv = c["side"], np.array(c["levels"], np.int64)
    keep = (side < 0) | np.isin(lv, U_LEVELS)
    fill = np.nonzero(side[keep] < 0)[0]
    lv = lv[keep]
    lv[fill] = np.array([1, 2, 3, 5])[np.arange(len(fill)) % 4]
    uv = c["uv"].reshape(-1, 6)[keep]
    out = tc.make_case("U-fmt%d-le%d-gt%d" % (fmt, le, gt), c["tex"], uv, 8, levels=lv.astype(np.uint8), fmt=fmt, flags=EVERY_FLAGS, filt=ot.LINEAR, addr=ot.CLAMP, le=le, gt=gt)
    out["side"] = side[keep]
    return out


# ---- C: a grid of level-5 items whose 16-byte units are raw where the case wants them ----
GRID, CELL = 1024, 64             # texture edge, cell edge in texels: 16 x 16 cells, two triangles each


def _cell_triangles(cellno):
    x0, y0 = (cellno % 16) * CELL, (cellno // 16) * CELL
    lo = np.array([x0 + 2, y0 + 2, x0 + 58, y0 + 2, x0 + 2, y0 + 58], np.float64) / GRID
    hi = np.array([x0 + 62, y0 + 62, x0 + 6, y0 + 62, x0 + 62, y0 + 6], np.float64) / GRID
    return lo.astype(F), hi.astype(F)


def grid_case(name, kinds, fmt=ot.FMT_4STATE, le=ot.T, gt=ot.O, level=5):
    """one level-`level` item per entry of `kinds`, item k in cell k // 2 of a 1024^2 opaque texture: "clean" (every unit a plateau), "noise" (1-texel
    noise under the whole cell: both items of a cell are noise then), "clear" (a transparent cell), or a list of the 16-byte units to be raw -- a single
    transparent texel at the centroid of the first quarter of the unit's sub-triangle (a unit of a 4-state block is the level-(level - 3)
    sub-triangle of its item).  A negative entry -u - 1 puts the texel into the LAST quarter of unit u (its last word).  An item with a list is the
    first of its cell and the second is clean."""
    bits = 2 if fmt == ot.FMT_4STATE else 1
    per_unit = 128 // bits                                  # micro-triangles per 16-byte unit
    sub = {64: level - 3, 128: None}[per_unit]
    tex = np.full((GRID, GRID), 255, np.uint8)
    uv = []
    for k, kind in enumerate(kinds):
        cellno, half = k // 2, k % 2
        x0, y0 = (cellno % 16) * CELL, (cellno // 16) * CELL
        tri = _cell_triangles(cellno)[half]
        uv.append(tri)
        if isinstance(kind, str):
            if kind == "noise":
                tex[y0:y0 + CELL, x0:x0 + CELL] = np.random.default_rng(1000 + cellno).integers(0, 2, (CELL, CELL)) * 255
            elif kind == "clear":
                tex[y0:y0 + CELL, x0:x0 + CELL] = 0
            else:
                assert kind == "clean", kind
            continue
        assert half == 0 and (k + 1 >= len(kinds) or kinds[k + 1] == "clean"), k
        assert sub is not None, "defect lists are for 4-state cases"
        q = cc.sub_triangles(tri, sub + 1)                  # quarters of the units
        for u in kind:
            i = 4 * u if u >= 0 else 4 * (-u - 1) + 3
            cx, cy = q[i].astype(np.float64).mean(axis=0) * GRID
            tex[int(np.floor(cy)), int(np.floor(cx))] = 0
    c = tc.make_case(name, np.ascontiguousarray(tex), np.array(uv, F), level, fmt=fmt, flags=EVERY_FLAGS, filt=ot.NEAREST, addr=ot.WRAP, le=le, gt=gt)
    c["kinds"] = list(kinds)
    return c


def only_first_halves(case):
    """drops the triangles of the second halves: a case built from 2 n kinds keeps the n items of the first halves, every one alone in its cell"""
    uv = case["uv"].reshape(-1, 6)[0::2]
    c = tc.make_case(case["name"], case["tex"], uv, case["gmax"], fmt=case["fmt"], flags=case["flags"], filt=case["filt"], addr=case["addr"], le=case["le"], gt=case["gt"])
    c["kinds"] = case["kinds"][0::2]
    return c


def alone(name, kinds, **kw):
    """grid_case with every item alone in its cell"""
    doubled = []
    for k in kinds:
        doubled += [k, "clean"]
    return only_first_halves(grid_case(name, doubled, **kw))


C_SIZES = [1, 15, 16, 17, 255, 257]                         # level-5 items of 16 units: contributions of 16, 240, 256, 272, 4096 -+ 16 units


@functools.lru_cache(maxsize=None)
def c_size_case(n, fmt=ot.FMT_4STATE, le=ot.T, gt=ot.O):
    """n level-5 items (level 6 in 2-state: 512-byte blocks): every third cell noise, every fifth transparent, the rest opaque -- plateaus of both states
    of the mapping next to raw units"""
    kinds = []
    for k in range(n):
        cellno = k // 2
        kinds.append("noise" if cellno % 3 == 1 else ("clear" if cellno % 5 == 2 else "clean"))
    return grid_case("C-size-%d-fmt%d-le%d" % (n, fmt, le), kinds, fmt=fmt, le=le, gt=gt, level=5 if fmt == ot.FMT_4STATE else 6)


@functools.lru_cache(maxsize=None)
def c_pattern_case():
    """two level-8 items (4-state: 16 KiB = 4 codec blocks of 256 units each) over a 1024^2 opaque texture with single transparent texels: codec blocks
    with 0, 1 (lane 0), 63 (lanes 1 - 63), 64 (lanes 64 - 127), 65 (lanes 0 - 64), 255 (lanes 1 - 255), 256 and 1 (lane 255) raw units.  A texel sits at the
    centroid of the first quarter of its unit's sub-triangle; in lanes 0 and 1 of the 65-unit block it sits in the LAST quarter, so those two units differ
    from their plateau in their last word only (pattern_holds asserts both through the oracle's decode)"""
    tris = [np.array([8, 8, 776, 8, 8, 776], np.float64) / GRID, np.array([1016, 1016, 248, 1016, 1016, 248], np.float64) / GRID]
    plans = [[[], [0], list(range(1, 64)), list(range(64, 128))],
             [[-1, -2] + list(range(2, 65)), list(range(1, 256)), list(range(256)), [255]]]
    tex = np.full((GRID, GRID), 255, np.uint8)
    for tri, plan in zip(tris, plans):
        q = cc.sub_triangles(tri.astype(F), 6)              # level-6 sub-triangles: quarters of the 1024 units of a level-8 item
        for b, lanes in enumerate(plan):
            for lane in lanes:
                u = b * CODEC_BLOCK + (lane if lane >= 0 else -lane - 1)
                i = 4 * u + (3 if lane < 0 else 0)
                cx, cy = q[i].astype(np.float64).mean(axis=0) * GRID
                tex[int(np.floor(cy)), int(np.floor(cx))] = 0
    c = tc.make_case("C-pattern", np.ascontiguousarray(tex), np.array(tris, F), 8, fmt=ot.FMT_4STATE, flags=EVERY_FLAGS, filt=ot.NEAREST, addr=ot.WRAP)
    c["plans"] = plans
    return c


def pattern_holds(case, array_data):
    """the oracle's decode shows the planned raw units of c_pattern_case, whichever item the sort puts first; raises otherwise"""
    counts, raw = raw_units_per_block(array_data)
    want = []
    for plan in case["plans"]:
        r = np.zeros(4 * CODEC_BLOCK, bool)
        for b, lanes in enumerate(plan):
            r[b * CODEC_BLOCK + np.array([l if l >= 0 else -l - 1 for l in lanes], np.int64)] = True
        want.append(r)
    a, b = raw[:1024], raw[1024:]
    if not ((np.array_equal(a, want[0]) and np.array_equal(b, want[1])) or (np.array_equal(a, want[1]) and np.array_equal(b, want[0]))):
        raise AssertionError("C-pattern: raw units per codec block %r are not the planned ones" % (counts,))
    assert sorted(counts) == [0, 1, 1, 63, 64, 65, 255, 256]
    # the two last-word units: words 0 - 2 of the unit are the plateau, word 3 is not
    w = np.frombuffer(np.ascontiguousarray(array_data).tobytes(), "<u4").reshape(-1, 4)
    last_only = (w[:, 0] == 0x55555555) & (w[:, 1] == 0x55555555) & (w[:, 2] == 0x55555555) & (w[:, 3] != 0x55555555)
    assert last_only.sum() >= 2, int(last_only.sum())
    return counts


LIMIT_ITEMS = 256                 # 64 KiB of contribution: 4096 units, 16 codec blocks


@functools.lru_cache(maxsize=None)
def c_limit_case(over):
    """256 level-5 items, every one alone in its cell: noise items (16 raw units each), one item with single defects, the rest clean, so that the restated
    stream is exactly comp_cap(stride) bytes long (over = 0) or 16 bytes longer (over = 1)"""
    stride = LIMIT_ITEMS * 256
    need = (comp_cap(stride) - codec_layout(stride)["offRaw"]) // 16 + over
    full, part = divmod(need, 16)
    kinds = ["noise"] * full + [list(range(part))] + ["clean"] * (LIMIT_ITEMS - full - 1)
    c = alone("C-limit-%d" % over, kinds)
    c["want_stream"] = comp_cap(stride) + 16 * over
    return c


def ragged_case():
    """totals that are no multiple of 256 or 16: blocks of 1 - 64 bytes behind level-5 ones, with duplicates merged"""
    return counts_case("C-ragged", {0: 5, 1: 7, 2: 9, 3: 5, 4: 3, 5: 6}, 77)


# ---- M / D: one rank's share incompressible, the others' not ----
@functools.lru_cache(maxsize=None)
def mixed_case(world, n=96):
    """n level-6 items (1 KiB) alone in their cells: noise where rank 0 owns the item, clean elsewhere -- rank 0's stream is longer than the cap (the
    4096 bytes the cap adds to half the stride need a stride above 8 KiB for that), the others' are a few hundred bytes"""
    own = item_owners(np.full(n, 6), world)
    c = alone("mixed-w%d" % world, ["noise" if o == 0 else "clean" for o in own], level=6)
    c["owners"] = own
    return c


@functools.lru_cache(maxsize=None)
def lengths_case(world, n=48):
    """n level-5 items alone in their cells, rank r's items with r % 4 raw units each (rank 0: none): streams of different lengths, all compressible"""
    own = item_owners(np.full(n, 5), world)
    c = alone("lengths-w%d" % world, [list(range(int(o) % 4)) if o % 4 else "clean" for o in own])
    c["owners"] = own
    return c


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the oracle's side, once per case
# ---------------------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(case):
    """(oracle's result of the case, oracle's result under RAW_FLAGS or None for cases with invalid triangles, seconds of oracle time)"""
    import time
    key = case["name"]
    if key not in _REF:
        t0 = time.perf_counter()
        orc = cc.own_oracle()
        ref = tc.bake(orc, case)
        raw = None if np.isnan(case["uv"]).any() or np.isinf(case["uv"]).any() else tc.bake(orc, case, flags=tc.RAW_FLAGS, rejection=0.0)
        _REF[key] = (ref, raw, time.perf_counter() - t0)
    return _REF[key]
