"""The serial host tail of the two lossy reducers (omm_amd/csrc/host_tail.cpp: near-duplicate merging by LSH or brute force, the maxArrayDataSize budget)
at its level, format and threshold edges: the case builders of tests/test_host_tail_reference.py (oracle + the stand-alone program
tests/native/host_tail_check.cpp, no GPU) and tests/test_host_tail_gpu.py (HIP library against the oracle).

The oracle (oracle/omm_oracle.c: dedup_lsh, dedup_brute, compress_items) is the reference of every result.  What is restated here serves the proofs that
a case does what it claims, never an expected array: the states a painted triangle must classify to, the folded Hamming distance of two blocks, and the
budget walk's keys (compute_info: float32, one rounding per operation): a result is compared only where the walk is pinned (budget_walk), because the
reference's std::sort leaves the order of tied and NaN keys open.

Painted triangles.  A case of this file is a texture painted per triangle: right triangles with legs of sx * 2^level by sy * 2^level texels (sx, sy >= 6) on
a shelf layout, every one over texels of its own, Nearest filter.  The base of a tile decides the known state of its micro-triangles -- "O": all opaque,
"T": all transparent, "cols": opaque with a transparent column every 12 texels (legs of 6: the micro-triangles over columns 0 - 5 (mod 12) are opaque, the
others unknown) -- and a defect, one texel of the other value strictly inside a micro-triangle, makes exactly that micro-triangle unknown.  Two tiles of one
level and base whose defect sets differ in d micro-triangles are blocks at folded Hamming distance d; the oracle's decode confirms every tile."""
import functools
import struct
import numpy as np
import ommtest as ot
import tail_cases as tc
import setup_cases as sc
import lookup_util as lu

F = np.float32
BRUTE = 1 << 10                      # the internal brute-force bit of the near-duplicate search (bake_cpu_impl.cpp:43-48)
NO_BUDGET = 0xFFFFFFFF
NO_REDUCTION = 0xFFFFFFFE            # a budget nothing reaches: the host tail runs and reduces nothing
NEAR = ot.FLAG_THREADS | ot.FLAG_NEAR_DUP
MAGIC = 0x4c544f48


# ---------------------------------------------------------------------------------------------------------------------------------------------
# baking, decoding, the stand-alone program's files
# ---------------------------------------------------------------------------------------------------------------------------------------------
def knobs_of(case, flags=None, budget=None, factor=None, rejection=None):
    """(flags, budget, factor, rejection) of a bake of the case: the case's own unless given"""
    return (case["flags"] if flags is None else flags, case.get("budget", NO_BUDGET) if budget is None else budget,
            case.get("factor", 0.15) if factor is None else factor, case["rejection"] if rejection is None else rejection)


def make_desc(tex, case, flags=None, budget=None, factor=None, rejection=None):
    flags, budget, factor, rejection = knobs_of(case, flags, budget, factor, rejection)
    d = ot.make_desc(tex, case["uv"], case["ix"], case["gmax"], **tc.desc_kw(case, flags, rejection))
    d.maxArrayDataSize = budget
    d.nearDuplicateDeduplicationFactor = factor
    return d


def bake(lib, case, flags=None, budget=None, factor=None, rejection=None, expect=ot.SUCCESS, want_stats=False):
    """one bake of the case (the oracle keeps its texture for the next bake over the same array, as tail_cases.bake does)"""
    if lib.which == "oracle":
        b, t = tc._oracle_texture(lib, case["tex"])
    else:
        b = lib.create_baker()
        t = lib.create_texture(b, [case["tex"]], alpha_cutoff=0.5)
    r = lib.bake(b, make_desc(t, case, flags, budget, factor, rejection), expect=expect, want_stats=want_stats)
    if lib.which != "oracle":
        lib.destroy_texture(b, t)
        lib.destroy_baker(b)
    return r


def work_items(case, raw, flags=None):
    """the work items of the case as the host tail receives them, from `raw`, the oracle's result under tail_cases.RAW_FLAGS: triangles grouped by equal
    (coordinates, level) -- every triangle its own with duplicate detection disabled --, invalid triangles in no item.  -> list of dict(level, uv, prims,
    states) and the triangle-to-item map"""
    flags = case["flags"] if flags is None else flags
    bits = 2 if case["fmt"] == ot.FMT_4STATE else 1
    p = np.ascontiguousarray(case["uv"], F).reshape(-1, 6)
    T = len(p)
    level = tc.triangle_levels(case)
    inv = sc.invalid(p)
    assert raw.index_format == ot.IDX_U32 and len(raw.index) == T and ((raw.index >= 0) == ~inv).all(), case["name"]
    first = sc.first_occurrence(p, level, inv, dedup=not flags & ot.FLAG_NO_DEDUP)
    owners = np.nonzero((first == np.arange(T)) & ~inv)[0]
    number = np.full(T, -1, np.int64)
    number[owners] = np.arange(len(owners))
    tri_item = np.where(inv, -1, number[first])
    items = []
    for i, t in enumerate(owners):
        off, L, f = raw.descs[raw.index[t]]
        assert L == level[t] and f == case["fmt"]
        blk = raw.array_data[off:off + int(tc.block_bytes(L, bits))]
        items.append(dict(level=int(L), uv=p[t], prims=np.nonzero(tri_item == i)[0].astype(np.uint32), states=tc.unpack_block(blk[None, :], 4 ** int(L), bits)[0]))
    return items, tri_item


def decode(oracle, case):
    return work_items(case, bake(oracle, case, flags=tc.RAW_FLAGS, budget=NO_BUDGET, rejection=0.0))


def pack2(states):
    """2 bits per micro-triangle, least significant first, a level-0 block as one field of one byte: HostItem::packed"""
    return tc.pack_states(np.asarray(states, np.uint8)[None, :], 2)[0]


def encode_case(case, items, numTris, flags=None, budget=None, factor=None, rejection=None, uniform_form=True, unresolved=ot.SPECIAL_FUO):
    """one case of the stand-alone program's input.  uniform_form: items whose states are all equal go as (state, level), as the device hands them over;
    otherwise every item carries its packed states"""
    flags, budget, factor, rejection = knobs_of(case, flags, budget, factor, rejection)
    out = [struct.pack("<Ii4iffIIiI", MAGIC, case["fmt"], int(bool(flags & ot.FLAG_NO_SPECIAL)), int(bool(flags & ot.FLAG_NO_DEDUP)), int(bool(flags & ot.FLAG_NEAR_DUP)),
                       int(bool(flags & BRUTE)), rejection, factor, budget, numTris, unresolved, len(items))]
    for it in items:
        s = np.asarray(it["states"], np.uint8)
        uniform = int(s[0]) if uniform_form and (s == s[0]).all() else -1
        out.append(struct.pack("<Ii6fI", it["level"], case["fmt"], *[float(v) for v in it["uv"]], len(it["prims"])))
        out.append(np.asarray(it["prims"], np.uint32).tobytes())
        out.append(struct.pack("<i", uniform))
        if uniform < 0:
            out.append(pack2(s).tobytes())
    return b"".join(out)


class TailResult:
    """what the stand-alone program wrote for one case"""

    def __init__(self, buf, pos):
        def take(n, dtype):
            nonlocal pos
            a = np.frombuffer(buf, dtype, n, pos).copy()
            pos += a.nbytes
            return a
        self.rc = int(take(1, np.int32)[0])
        self.array_data = take(int(take(1, np.uint32)[0]), np.uint8)
        rec = np.dtype([("a", "<u4"), ("l", "<u2"), ("f", "<u2")])
        d = take(int(take(1, np.uint32)[0]), rec)
        self.descs = np.stack([d["a"], d["l"], d["f"]], axis=1).astype(np.int64).reshape(-1, 3)
        self.array_hist = [tuple(int(v) for v in h) for h in take(int(take(1, np.uint32)[0]), rec)]
        self.index_hist = [tuple(int(v) for v in h) for h in take(int(take(1, np.uint32)[0]), rec)]
        self.index = take(int(take(1, np.uint32)[0]), np.int32)
        self.end = pos


def read_results(buf, count):
    out, pos = [], 0
    for _ in range(count):
        out.append(TailResult(buf, pos))
        pos = out[-1].end
    assert pos == len(buf), (pos, len(buf))
    return out


def same(name, got, ref):
    """a result of the program or of the HIP library equals the oracle's (32-bit indices), byte for byte"""
    assert len(got.descs) == len(ref.descs), (name, len(got.descs), len(ref.descs))
    assert np.array_equal(np.asarray(got.descs).reshape(-1, 3), np.asarray(ref.descs).reshape(-1, 3)), (name, "descriptors")
    assert np.array_equal(got.array_data, ref.array_data), (name, "arrayData", got.array_data.size, ref.array_data.size)
    assert np.array_equal(np.asarray(got.index, np.int64), np.asarray(ref.index, np.int64)), (name, "index", np.nonzero(np.asarray(got.index, np.int64) != np.asarray(ref.index, np.int64))[0][:8])
    assert [tuple(int(v) for v in h) for h in got.array_hist] == [tuple(int(v) for v in h) for h in ref.array_hist], (name, got.array_hist, ref.array_hist)
    assert [tuple(int(v) for v in h) for h in got.index_hist] == [tuple(int(v) for v in h) for h in ref.index_hist], (name, got.index_hist, ref.index_hist)


def invariants_hold(name, res, fmt, numTris, unresolved=ot.SPECIAL_FUO):
    """what holds of every successful result, whatever the order of tied keys: offsets are the running sum of the block sizes, every triangle points at a
    descriptor or a special index, the histograms sum to the descriptors and to the triangles that point at one"""
    bits = 2 if fmt == ot.FMT_4STATE else 1
    assert res.rc == 0, (name, res.rc)
    d = res.descs
    sizes = tc.block_bytes(d[:, 1], bits) if len(d) else np.zeros(0, np.int64)
    assert np.array_equal(d[:, 0], np.concatenate([[0], np.cumsum(sizes)[:-1]]) if len(d) else d[:, 0]), name
    assert res.array_data.size == int(sizes.sum()) and (d[:, 2] == fmt).all(), name
    assert len(res.index) == max(numTris, 1) and ((res.index >= -4) & (res.index < (len(d) if len(d) else 0))).all(), name
    for L in range(13):
        assert sum(c for c, l, f in res.array_hist if l == L) == int((d[:, 1] == L).sum()), (name, L)
        pointing = res.index[:numTris][res.index[:numTris] >= 0]
        assert sum(c for c, l, f in res.index_hist if l == L) == int((d[pointing, 1] == L).sum()), (name, L)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# restated for the proofs: folded Hamming distance, compute_info and the budget walk
# ---------------------------------------------------------------------------------------------------------------------------------------------
def fold(states):
    s = np.asarray(states, np.uint8)
    return np.where(s == ot.UT, ot.UO, s)


def distance(a, b):
    """hamming3 (bake_cpu_impl.cpp:1068-1083): micro-triangles whose 3-state values differ"""
    return int((fold(a) != fold(b)).sum())


def parent_states(states):
    """one level down (:1499-1529): the children's common state where all four are the same known state, UnknownOpaque otherwise"""
    q = fold(states).reshape(-1, 4)
    known = (q[:, 0] <= ot.O) & (q == q[:, :1]).all(axis=1)
    return np.where(known, q[:, 0], ot.UO).astype(np.uint8)


def area_of(uv):
    """util/geometry.h:141-145 on a 2-D triangle: half the length of (0, 0, v0 x v1), float32"""
    p = np.asarray(uv, F)
    v0x, v0y, v1x, v1y = p[4] - p[0], p[5] - p[1], p[2] - p[0], p[3] - p[1]
    nz = F(v0x * v1y) - F(v1x * v0y)
    return F(0.5) * np.sqrt(F(nz * nz), dtype=F)


def info_of(states, level, area, nprims):
    """compute_info (:1572-1595) -> (coveragePerByte, mem, memDown)"""
    s = fold(states)
    n = 4 ** level
    nd = 4 ** (level - 1)
    known = F(int((s <= ot.O).sum())) / F(n)
    down = F(int((parent_states(s) != ot.UO).sum())) / F(nd)
    total = F(0)
    for _ in range(nprims):
        total = F(total + area)
    mem, mem_down = max(1, n * 2 // 8), max(1, nd * 2 // 8)
    with np.errstate(all="ignore"):
        key = F(F(total * F(known - down)) / F(mem - mem_down))
    return key, mem, mem_down


def budget_walk(active, budget, need_pinned=True):
    """compress (:1597-1688) over `active`, the items that enter it (dict(states, level, area, nprims), none special, none of level 0).  -> dict(S: the
    total before, levels and states: where every item ends, rounds, revisits: how often the walk steps back onto an item (the `i--`), pinned: the order
    the walk visits the items in does not depend on how a sort places equal or unordered keys).  Pinned means: no key is NaN or -inf at a sort or at the
    comparison of the step back; no item is visited while another item of the last sort shares its key, finite or +inf (level-1 items: memDelta == 0) --
    items that tie and are never reached lie behind the place where the walk stops, in whatever order; and the step back never compares equal finite
    keys.  need_pinned: raise where the walk is not"""
    st = [dict(s=fold(a["states"]), L=a["level"], area=a["area"], np=a["nprims"], id=i) for i, a in enumerate(active)]
    for a in st:
        a["key"], a["mem"], a["down"] = info_of(a["s"], a["L"], a["area"], a["np"])
    S = total = sum(a["mem"] for a in st)
    out = dict(S=S, rounds=0, revisits=0, pinned=True, failed=False)

    def unpinned(why):
        out["pinned"] = False
        assert not need_pinned, why

    def tied(act):
        """the items whose key another item of the sort shares; a NaN or -inf key leaves the whole order open"""
        k = np.array([a["key"] for a in act], F)
        if np.isnan(k).any() or (k == -np.inf).any():
            unpinned("unordered keys: %r" % k.tolist()[:8])
        vals, counts = np.unique(k[~np.isnan(k)], return_counts=True)
        shared = set(vals[counts > 1].tolist())
        return {a["id"] for a in act if float(a["key"]) in shared}

    levels = [a["L"] for a in st]
    if total >= budget:
        ties = tied(st)
        act = sorted(st, key=lambda a: a["key"]) if out["pinned"] else list(st)
        while total >= budget and act:
            out["rounds"] += 1
            i, N = 0, len(act)
            while i < N:
                a = act[i]
                if a["id"] in ties:
                    unpinned("item %d is visited while another shares its key %r" % (a["id"], float(a["key"])))
                ties.discard(a["id"])
                total -= a["mem"]
                if a["L"] == 0:
                    out["failed"] = True
                    return out
                a["s"], a["L"] = parent_states(a["s"]), a["L"] - 1
                levels[a["id"]] = a["L"]
                total += a["down"]
                if a["L"] == 0:
                    a["gone"] = True
                    i += 1
                    continue
                a["key"], a["mem"], a["down"] = info_of(a["s"], a["L"], a["area"], a["np"])
                if total < budget:
                    break
                if i + 1 != N:
                    if np.isnan(a["key"]) or a["key"] == act[i + 1]["key"] and a["key"] != np.inf:
                        unpinned("the step back compares %r with %r" % (float(a["key"]), float(act[i + 1]["key"])))
                    if a["key"] < act[i + 1]["key"]:
                        out["revisits"] += 1
                        i -= 1
                i += 1
            act = [a for a in act if not a.get("gone")]
            ties = tied(act)
            act = sorted(act, key=lambda a: a["key"]) if out["pinned"] else act
    out["levels"] = levels
    out["states"] = [a["s"] for a in st]
    out["total"] = total
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# painted triangles
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def micro_table(level):
    """per micro-triangle of the bird curve: the cell of its right-angle corner in micro-triangle legs, and whether it is upright"""
    n = 4 ** level
    v = lu.micro_vertices(np.arange(n), np.full(n, level))
    return np.rint(v[:, 0] * 2 ** level).astype(np.int64), v[:, 1, 0] > v[:, 0, 0]


@functools.lru_cache(maxsize=None)
def clear_micro(level):
    """the micro-triangles a "cols" tile leaves opaque: those over columns 0 - 5 (mod 12)"""
    cell, up = micro_table(level)
    return (np.where(up, cell[:, 0], cell[:, 0] - 1) * 6) % 12 == 0


def tile(level, defects=(), base="cols", sx=6, sy=6, tris=1):
    defects = tuple(sorted(int(j) for j in defects))
    assert base in ("cols", "O", "T") and (base != "cols" or (sx, sy) == (6, 6)) and sx >= 6 and sy >= 6 and len(set(defects)) == len(defects)
    assert all(0 <= j < 4 ** level for j in defects) and (base != "cols" or all(clear_micro(level)[j] for j in defects)), (level, base, defects)
    return dict(level=level, defects=defects, base=base, sx=sx, sy=sy, tris=tris)


def expected_states(t, fmt, promo=ot.PROMO_FORCE_TRANSPARENT):
    """what the tile must classify to (le = T, gt = O)"""
    n = 4 ** t["level"]
    unknown = {ot.PROMO_FORCE_TRANSPARENT: ot.UT, ot.PROMO_FORCE_OPAQUE: ot.UO}[promo] if fmt == ot.FMT_4STATE else {ot.PROMO_FORCE_TRANSPARENT: ot.T, ot.PROMO_FORCE_OPAQUE: ot.O}[promo]
    s = np.full(n, ot.T if t["base"] == "T" else ot.O, np.uint8)
    if t["base"] == "cols":
        s[~clear_micro(t["level"])] = unknown
    s[list(t["defects"])] = unknown
    return s


def painted(name, tiles, fmt=ot.FMT_4STATE, flags=ot.FLAG_THREADS, shuffle=None, promo=ot.PROMO_FORCE_TRANSPARENT, **knobs):
    """the case of the tiles: one triangle (or t["tris"] with the same coordinates: one work item) per tile, in tile order or shuffled by the seed.
    c["tile_of"]: the tile of every triangle; c["tiles"]; further keywords (budget, factor, rejection) are the bake's"""
    ex = [t["sx"] << t["level"] for t in tiles]
    ey = [t["sy"] << t["level"] for t in tiles]
    W = 256
    while W < max(ex) + 40:
        W *= 2
    while True:                                                    # shelves; a wider texture while the shelves are taller than wide
        x, y, rowh, places = 12, 2, 0, []
        for Ex, Ey in zip(ex, ey):
            if x + Ex + 2 > W:
                x, y, rowh = 12, y + rowh + 3, 0
            places.append((x, y))
            x += -(-(Ex + 3) // 12) * 12
            rowh = max(rowh, Ey)
        need = y + rowh + 3
        if need <= W:
            break
        W *= 2
    H = 64
    while H < need:
        H *= 2
    tex = np.full((H, W), 255, np.uint8)
    tex[:, np.arange(W) % 12 == 9] = 0
    rows = []
    for t, (x, y), Ex, Ey in zip(tiles, places, ex, ey):
        if t["base"] != "cols":
            tex[y - 1:y + Ey + 2, x - 1:x + Ex + 2] = 255 if t["base"] == "O" else 0
        cell, up = micro_table(t["level"])
        for j in t["defects"]:
            o = 1 if up[j] else -2
            tex[y + cell[j, 1] * t["sy"] + o, x + cell[j, 0] * t["sx"] + o] = 255 if t["base"] == "T" else 0
        rows.append([x / W, y / H, (x + Ex) / W, y / H, x / W, (y + Ey) / H])
    tile_of = np.concatenate([np.full(t["tris"], i, np.int64) for i, t in enumerate(tiles)])
    if shuffle is not None:
        tile_of = tile_of[np.random.default_rng(shuffle).permutation(len(tile_of))]
    uv = np.array(rows, F)[tile_of]
    lv = np.array([tiles[i]["level"] for i in tile_of], np.uint8)
    one = len(set(lv.tolist())) == 1
    c = tc.make_case(name, np.ascontiguousarray(tex), uv, int(lv.max()), levels=None if one else lv, fmt=fmt, flags=flags, filt=ot.NEAREST, addr=ot.WRAP, promo=promo,
                     rejection=knobs.pop("rejection", 0.0))
    c.update(tile_of=tile_of, tiles=list(tiles), **knobs)
    return c


def tiles_decode_as_painted(case, items, tri_item):
    """the oracle's decode of every work item is what its tile was painted to give; items follow the first triangles of their tiles"""
    for i, it in enumerate(items):
        t = case["tiles"][case["tile_of"][it["prims"][0]]]
        want = expected_states(t, case["fmt"], case["promo"])
        assert it["level"] == t["level"] and np.array_equal(it["states"], want), (case["name"], i, t, it["states"], want)
        assert (case["tile_of"][it["prims"]] == case["tile_of"][it["prims"][0]]).all()


def item_of_tile(case, tri_item, k):
    """the work item of tile k"""
    return int(tri_item[np.nonzero(case["tile_of"] == k)[0][0]])


def pick(rng, level, count, base="cols", avoid=()):
    """`count` micro-triangles a defect may sit in, none of `avoid`"""
    pool = np.nonzero(clear_micro(level))[0] if base == "cols" else np.arange(4 ** level)
    pool = np.setdiff1d(pool, np.asarray(list(avoid), np.int64))
    assert len(pool) >= count, (level, count, len(pool))
    return tuple(sorted(int(j) for j in rng.choice(pool, count, replace=False)))


def radius(level, factor):
    """r of the LSH (:1190): factor * 4^level, float32"""
    return F(F(factor) * F(4 ** level))


def around(r):
    """(the largest whole distance below r, r itself where it is whole else None, the smallest above)"""
    r = float(r)
    whole = r == int(r)
    below = int(r) - 1 if whole else int(np.floor(r))
    return below, (int(r) if whole else None), int(np.floor(r)) + 1


def lsh_k(n, level, factor):
    """the number of sampled micro-triangles per table for a batch of n (:1196), float32 as the reference computes it; 0: the batch is skipped"""
    with np.errstate(all="ignore"):
        r = radius(level, factor)
        v = np.ceil(F(F(np.log(F(n), dtype=F)) * F(4 ** level)) / F(F(4.0) * r))
    return int(sc.cvt_i32(np.array([v], F))[0]) & 0xFFFFFFFF if np.isfinite(v) else 0


def lsh_tables(n):
    with np.errstate(all="ignore"):
        return int(np.ceil(np.power(F(n), F(0.25), dtype=F)))


def fillers(rng, level, count, used, far, base="cols"):
    """`count` non-uniform tiles of the level whose defect sets lie at least `far` apart from each other and from the sets of `used`"""
    out, sets = [], [set(u) for u in used]
    room = int(clear_micro(level).sum()) if base == "cols" else 4 ** level
    for k in range(count):
        for attempt in range(400):
            d = set(pick(rng, level, int(rng.integers(0 if base == "cols" else 1, room)), base))
            if all(len(d ^ s) >= far for s in sets):
                break
        else:
            raise AssertionError("no room for %d fillers at level %d" % (count, level))
        sets.append(d)
        out.append(tile(level, d, base, 6 + (k % 5 if base != "cols" else 0), 6))
    return out


def merged_with(res, case, tri_item, a, b):
    """tiles a and b share a descriptor in the result"""
    ta, tb = np.nonzero(case["tile_of"] == a)[0][0], np.nonzero(case["tile_of"] == b)[0][0]
    return res.index[ta] >= 0 and res.index[ta] == res.index[tb]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the families' tile sets
# ---------------------------------------------------------------------------------------------------------------------------------------------
def pair_case(name, level, d, seed, nfill, far, base="cols", **knobs):
    """tile 0 and tile 1 at distance d (tile 1 has d defects more), then nfill fillers at least `far` from everything"""
    rng = np.random.default_rng(seed)
    room = int(clear_micro(level).sum()) if base == "cols" else 4 ** level
    a = pick(rng, level, int(rng.integers(1, max(2, room - d))), base)
    b = tuple(sorted(a + pick(rng, level, d, base, avoid=a)))
    first, second = (a, b) if seed % 2 == 0 else (b, a)                 # the fuller block as merge target and as merge source
    tiles = [tile(level, first, base), tile(level, second, base)]
    tiles += fillers(rng, level, nfill, [a, b], far, base)
    return painted(name, tiles, flags=knobs.pop("flags", NEAR), **knobs)


def mixed_levels_tiles(seed, lone=1):
    """levels 1, 3, 5, 6 with many items in loose clusters (members 4 - 9 defects from a centre at level 3, fewer below, more above: merges that depend on
    the buckets), level 2 with `lone` non-special items (and two uniform ones, special), level 4 with none"""
    rng = np.random.default_rng(seed)
    tiles = [tile(1, d, "O") for d in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 3))]
    for k in range(lone):
        tiles.append(tile(2, pick(rng, 2, 5 + k, "O"), "O"))
    tiles += [tile(2, (), "O"), tile(2, (), "T")]
    for L, clusters, members, spread in ((3, 6, 5, (4, 10)), (5, 3, 4, (60, 150)), (6, 2, 3, (300, 600))):
        for _ in range(clusters):
            centre = pick(rng, L, 4 ** L // 3, "O")
            tiles.append(tile(L, centre, "O"))
            for _ in range(members):
                extra = pick(rng, L, int(rng.integers(*spread)), "O", avoid=centre)
                tiles.append(tile(L, centre + extra, "O", tris=int(rng.integers(1, 3))))
    return tiles


def budget_tiles(seed, levels, count, uniform=False):
    """`count` tiles of the levels in turn, each with legs of its own (pairwise different areas within a level), opaque or transparent base, defects in whole
    groups of four siblings and in single micro-triangles (so that parents stay known here and turn unknown there), some of two or three triangles; at
    most one of level 1; uniform: some tiles without a defect or all defect"""
    rng = np.random.default_rng(seed)
    tiles, shapes, ones = [], set(), 0
    while len(tiles) < count:
        L = levels[len(tiles) % len(levels)]
        if L == 1:
            ones += 1
            if ones > 1:
                L = 3
        for attempt in range(1000):
            top = {5: 12, 6: 10}.get(L, 20)                            # (short legs at the high levels: the texture stays small)
            shape = (L, int(rng.integers(6, top)), int(rng.integers(6, top)))
            if 4 ** L * shape[1] * shape[2] not in shapes:              # (pairwise different areas: 4^L * sx * sy / 2 texels)
                shapes.add(4 ** L * shape[1] * shape[2])
                break
        else:
            raise AssertionError("no leg lengths left at level %d" % L)
        n = 4 ** L
        groups = rng.random(max(1, n // 4)) < rng.uniform(0.05, 0.5)
        d = (np.repeat(groups, 4)[:n] & (rng.random(n) < rng.uniform(0.2, 1.0))) | (rng.random(n) < 0.02)
        if uniform and len(tiles) % 5 == 0:
            d[:] = len(tiles) % 10 == 0
        else:                                                          # one unknown micro-triangle alone among its siblings: dropping a level costs coverage, the key is not 0
            g = int(rng.integers(0, max(1, n // 4)))
            d[4 * g:4 * g + 4] = False
            d[min(n - 1, 4 * g + int(rng.integers(0, 4)))] = True
            if d.all():
                d[(4 * g + 4) % n] = False
        tiles.append(tile(L, np.nonzero(d)[0], "OT"[int(rng.integers(0, 2))], shape[1], shape[2], tris=1 + (len(tiles) % 7 == 3) + (len(tiles) % 11 == 5)))
    return tiles
