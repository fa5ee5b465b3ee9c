"""The classification's work distribution (omm_amd/csrc/bake_kernels.hip: triage_items, triage_tiles, triage_groups, classify_tiles, classify_generic)
restated as a SCHEDULE, and the directed cases of tests/test_classify_reference.py (no GPU) and tests/test_classify_gpu.py.

What is restated.  `region_rect` / `region_state_impl` (classify_device.h) and nothing else of the arithmetic: the box of a bird-curve sub-triangle grown
by maxAbs * 2^-17 + 1e-30, the texel rectangle floor(lo * size - 0.5) .. floor(hi * size - 0.5) + 1, the translation under Wrap and the interior rule of
the other modes, a uniform sum of the table of `alpha > cutoff` = settled, a mixed 2 x 2 rectangle = all open.  The vertices of every sub-triangle come
from the oracle (`orc_micro_triangle`): a tile is the level-(N - 6) sub-triangle of its item (N - 5 in the 1024-tile queue), a group the level-(N - 3)
one.  The restatement is float64, not bit-exact: `restate_schedule` asserts that no rectangle edge it reasons about lies within 1e-3 texel of a rounding
step (and no box edge within 1e-6 of a UV-tile edge), so the fp32 of the kernels, fused or not, gives the same integers.

What it predicts.  Which work items are active, which tiles are settled or open, the verdict and rectangle of every group of an open tile, the record
order of the 4096-tile queue, the chunks triage_groups forms from it (head, followers, first slots, union rectangle, whether classify_tiles loads the LDS
window) and the counters of ommxBakeTimings.  It never predicts a result array: those always come from the oracle's bake of the same input.

Order.  Work items are numbered in triangle order (first occurrences; the cases here have no duplicates, no invalid and no degenerate triangle unless
they say so), `setup_split_scatter` lists them level by level, ascending inside a level, `prep_compact` keeps that order for the active ones.
`classify_plan` enumerates the 4096-tiles with the HIGHEST level first, inside a level by position on the active list, inside an item by tile index;
triage_tiles appends the open ones wave by wave, in lane order inside a wave.  With 64 tiles or fewer that is ONE wave and the queue order is the
enumeration order; beyond that waves append through an atomic and no order is asserted (`deterministic` is False).  An unstreamed bake has one section;
triage_groups walks it in windows of kChunkWindow = 8 records from record 0 (1 when level 6 is the top level of the bake).

Exactness.  The table is asked only where the reference runs its coarse pass: Linear filter, one mip, a table (`P.useCoarse`, omm_host.cpp; the
reference's ResampleCoarse has the same condition).  With the Nearest filter or a mip chain nothing is triaged: every item is active, every tile open,
every group unknown, every micro-triangle queued, no record joins another (64 + 64 > 64) -- `restate_schedule` says so and the counters are exact.  With
Linear and one mip the curve-free-region test (region_curve.h) can settle what the table leaves open, so the restatement gives bounds there: a tile
whose rectangle is uniform is certainly settled (upper bound of openTiles), a tile that holds two states in the oracle's decode is certainly open
(lower bound, `linear_bounds`).  The mode in which the schedule is EXACTLY the table's is Linear with DisableLevelLineIntersection (bake flag bit 8:
`region_curve_applies` is false, the coarse pass stays on): activeItems, openTiles and openTileMicroTriangles are the restatement's, and
fineMicroTriangles is what phase 1 queues -- every micro-triangle of an all-open group and, of an unknown group, those the per-micro-triangle coarse test
leaves unresolved (`unresolved_micro_triangles`: exact under Wrap, else between 64 * all-open groups and 64 * open groups).  The three
modes of a case are `variant(case, mode=...)`: "table", "linear", "nearest"."""
import ctypes as C
import functools
import numpy as np
import ommtest as ot
import sat_util as su
import tail_cases as tc

F = np.float32
UNKNOWN, ALL_OPEN = -1, -2           # kRegionUnknown, kRegionAllOpen
CHUNK_WINDOW, WIN = 8, 32            # kChunkWindow, the LDS window edge
CUTOFF = 0.5
MARGIN = 1e-3
FORMATS = tc.FORMATS
RAW_FLAGS = tc.RAW_FLAGS
FLAG_NO_LEVELLINE = 1 << 8           # DisableLevelLineIntersection
MODES = ["table", "linear", "nearest"]
LINEAR_TRIES = 12
MAX_CANDIDATES = 40000


@functools.lru_cache(maxsize=None)
def own_oracle():
    return ot.Lib("oracle")


@functools.lru_cache(maxsize=None)
def orc():
    dll = C.CDLL(ot.oracle_path())
    dll.orc_micro_triangle.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    return dll


def sub_triangles(uv6, sub_level):
    """(4^sub_level, 3, 2) float32: the oracle's vertices of every level-`sub_level` bird-curve sub-triangle of the triangle uv6"""
    tri = np.ascontiguousarray(uv6, F).reshape(6)
    tp = tri.ctypes.data_as(C.POINTER(C.c_float))
    n = 4 ** sub_level
    out = np.empty((n, 6), F)
    buf = (C.c_float * 6)()
    f = orc().orc_micro_triangle
    for i in range(n):
        f(tp, i, sub_level, buf)
        out[i] = buf[:]
    return out.reshape(n, 3, 2)


def region_rects(subs, max_abs, w, h, addr):
    """region_rect of n sub-triangles, float64 -> dict of int arrays X0, Y0, X1, Y1 (unaddressed), sx, sy, ex, ey (addressed), ok, and the smallest
    distance of a rectangle edge to a rounding step"""
    p = np.asarray(subs, np.float64)
    lo, hi = p.min(axis=1), p.max(axis=1)
    grow = float(max_abs) * 2.0 ** -17 + 1e-30
    lx, ly, hx, hy = lo[:, 0] - grow, lo[:, 1] - grow, hi[:, 0] + grow, hi[:, 1] + grow
    edges = np.stack([lx * w - 0.5, ly * h - 0.5, hx * w - 0.5, hy * h - 0.5], axis=1)
    margin = float(np.abs(edges - np.round(edges)).min())
    boxes = np.stack([lx, ly, hx, hy], axis=1)
    tile_margin = float(np.abs(boxes - np.round(boxes)).min())
    fl = np.floor(edges).astype(np.int64)
    X0, Y0, X1, Y1 = fl[:, 0], fl[:, 1], fl[:, 2] + 1, fl[:, 3] + 1
    ok = (np.trunc(lx) == np.trunc(hx)) & (np.trunc(ly) == np.trunc(hy)) & (max_abs <= 16384.0)
    ok &= (X1 - X0 < w) & (Y1 - Y0 < h)
    if addr == ot.WRAP:
        sx, ex, sy, ey = X0 % w, X1 % w, Y0 % h, Y1 % h
        ok &= (ex - sx == X1 - X0) & (ey - sy == Y1 - Y0)
    else:
        sx, ex, sy, ey = X0, X1, Y0, Y1
        ok &= (X0 >= 0) & (Y0 >= 0) & (X1 < w) & (Y1 < h)
    z = lambda a: np.where(ok, a, 0)
    return dict(X0=X0, Y0=Y0, X1=X1, Y1=Y1, sx=z(sx), sy=z(sy), ex=z(ex), ey=z(ey), ok=ok, margin=margin, tile_margin=tile_margin)


def padded_table(tex, cutoff=CUTOFF):
    """(h + 1, w + 1) int64: exclusive sums of the indicator (row and column 0 are zero), from sat_util's numpy table"""
    s = su.sat_reference(tex, cutoff).astype(np.int64)
    out = np.zeros((s.shape[0] + 1, s.shape[1] + 1), np.int64)
    out[1:, 1:] = s
    return out


def verdicts(R, S, le, gt, want_open):
    """region_state_impl over the rectangles R: state (>= 0), UNKNOWN or, with want_open, ALL_OPEN"""
    sx, sy, ex, ey = R["sx"], R["sy"], R["ex"], R["ey"]
    area = (ex - sx + 1) * (ey - sy + 1)
    sa = S[ey + 1, ex + 1] - S[sy, ex + 1] - S[ey + 1, sx] + S[sy, sx]
    v = np.full(len(sx), UNKNOWN, np.int64)
    v[sa == 0] = le
    v[sa == area] = gt
    if want_open:
        v[(sa != 0) & (sa != area) & (area == 4)] = ALL_OPEN
    v[v == 3] = UNKNOWN
    v[~R["ok"]] = UNKNOWN
    return v


@functools.lru_cache(maxsize=None)
def _geometry(uv_bytes, level, w, h, addr):
    """the rectangles of an item, its tiles and its groups: they depend on the triangle alone, not on the texels"""
    uv6 = np.frombuffer(uv_bytes, F)
    max_abs = float(np.abs(uv6).max())
    g = dict(max_abs=max_abs, whole=region_rects(uv6.reshape(1, 3, 2), max_abs, w, h, addr))
    if level >= 5:
        tlog = 6 if level >= 6 else 5
        g["tiles"] = region_rects(sub_triangles(uv6, level - tlog), max_abs, w, h, addr)
        g["groups"] = region_rects(sub_triangles(uv6, level - 3), max_abs, w, h, addr)
        g["gpt"] = 64 if level >= 6 else 16
    return g


def case_levels(case):
    T = len(case["uv"]) // 3
    return tc.triangle_levels(case) if case["levels"] is not None else np.full(T, case["gmax"], np.int64)


def restate_schedule(case, table=None, exact_fine=False):
    """the schedule of a case (module docstring).  Returns a dict:
    active[i] per work item; items[i] = None (inactive or below level 5) or dict(level, tile_open[t], tile_state[t], tile_rect, group_verdict[t, g],
    group_rect); records = the 4096-tile queue in order, each (item, tile, open groups, rect, ok); small = the same for the 1024-tile queue; chunks = what
    triage_groups forms; deterministic; window; activeItems, openTiles, openTileMicroTriangles, fineMicroTriangles (exact with Nearest)."""
    tex = case["tex"]
    h, w = tex.shape
    S = padded_table(tex) if table is None else table
    le, gt = case["le"], case["gt"]
    p = np.ascontiguousarray(case["uv"], F).reshape(-1, 6)
    levels = case_levels(case)
    n = len(p)
    coarse = case["filt"] == ot.LINEAR and len(case.get("mips") or [0]) == 1       # P.useCoarse: otherwise nobody asks the table
    active = np.zeros(n, bool)
    items = [None] * n
    margin, tile_margin = np.inf, np.inf
    for i in range(n):
        L = int(levels[i])
        g = _geometry(p[i].tobytes(), L, w, h, case["addr"])
        margin, tile_margin = min(margin, g["whole"]["margin"]), min(tile_margin, g["whole"]["tile_margin"])
        active[i] = verdicts(g["whole"], S, le, gt, False)[0] < 0 or not coarse
        if not active[i] or L < 5:
            continue
        margin = min(margin, g["tiles"]["margin"], g["groups"]["margin"])
        tile_margin = min(tile_margin, g["tiles"]["tile_margin"], g["groups"]["tile_margin"])
        tv = verdicts(g["tiles"], S, le, gt, False)
        if L <= 6 or not coarse:
            tv[:] = UNKNOWN     # a tile that IS its item is not asked again: it is on the active list because the answer was no
        gv = verdicts(g["groups"], S, le, gt, True).reshape(-1, g["gpt"])
        if not coarse:
            gv[:] = UNKNOWN
        items[i] = dict(level=L, tile_open=tv < 0, tile_state=tv, tile_rect=g["tiles"], group_verdict=gv, group_rect=g["groups"], gpt=g["gpt"])
    assert margin > MARGIN, (case["name"], "a rectangle edge lies within 1e-3 texel of a rounding step", margin)
    assert tile_margin > 1e-6, (case["name"], "a box edge lies on a UV-tile edge", tile_margin)
    records, small = [], []
    for L in sorted({int(x) for x in levels if x >= 5}, reverse=True):
        for i in np.nonzero((levels == L) & active)[0]:
            it = items[i]
            for t in np.nonzero(it["tile_open"])[0]:
                R = it["tile_rect"]
                rec = dict(item=int(i), tile=int(t), level=L, open=int((it["group_verdict"][t] < 0).sum()), ok=bool(R["ok"][t]),
                           rect=(int(R["sx"][t]), int(R["sy"][t]), int(R["ex"][t]), int(R["ey"][t])))
                (records if L >= 6 else small).append(rec)
    big_tiles = int(sum(4 ** (int(levels[i]) - 6) for i in range(n) if active[i] and levels[i] >= 6))
    top = max([int(levels[i]) for i in range(n) if active[i] and levels[i] >= 6], default=0)
    window = 1 if top == 6 else CHUNK_WINDOW
    open_groups = sum(r["open"] for r in records) + sum(r["open"] for r in small)
    all_open = sum(int((items[r["item"]]["group_verdict"][r["tile"]] == ALL_OPEN).sum()) for r in records + small)
    out = dict(active=active, items=items, records=records, small=small, window=window, deterministic=big_tiles <= 64,
                chunks=form_chunks(records, window), margin=margin,
                activeItems=int(active.sum()), openTiles=len(records) + len(small), openTileMicroTriangles=4096 * len(records) + 1024 * len(small),
                fineMicroTriangles=64 * open_groups, fineLower=64 * all_open, fineExact=None)
    if coarse and exact_fine and case["addr"] == ot.WRAP and case["le"] < 2 and case["gt"] < 2:
        n_fine, m = unresolved_micro_triangles(case, out, S)
        out["fineExact"] = n_fine if m > MARGIN else None
    return out


def unresolved_micro_triangles(case, sched, S):
    """fineMicroTriangles of the "table" mode under Wrap: what classify_tiles phase 1 queues.  Every micro-triangle of an all-open group; of an unknown
    group, those the per-micro-triangle coarse test (coarse_state, classify_device.h -- the reference's ResampleCoarse) leaves unresolved: the same
    rectangle rule on the micro-triangle's own box, not grown.  -> (count, smallest distance of a micro-triangle's rectangle edge to a rounding step)"""
    h, w = case["tex"].shape
    p = np.ascontiguousarray(case["uv"], F).reshape(-1, 6)
    total, margin = 0, np.inf
    f, buf = orc().orc_micro_triangle, (C.c_float * 6)()
    for r in sched["records"] + sched["small"]:
        it = sched["items"][r["item"]]
        gv = it["group_verdict"][r["tile"]]
        total += 64 * int((gv == ALL_OPEN).sum())
        tp = np.ascontiguousarray(p[r["item"]]).ctypes.data_as(C.POINTER(C.c_float))
        idx = [(r["tile"] * it["gpt"] + int(g)) * 64 + i for g in np.nonzero(gv == UNKNOWN)[0] for i in range(64)]
        if not idx:
            continue
        tri = np.empty((len(idx), 6), np.float64)
        for k, i in enumerate(idx):
            f(tp, i, r["level"], buf)
            tri[k] = buf[:]
        tri = tri.reshape(-1, 3, 2)
        lo, hi = tri.min(axis=1), tri.max(axis=1)
        edges = np.stack([lo[:, 0] * w - 0.5, lo[:, 1] * h - 0.5, hi[:, 0] * w - 0.5, hi[:, 1] * h - 0.5], axis=1)
        margin = min(margin, float(np.abs(edges - np.round(edges)).min()))
        fl = np.floor(edges).astype(np.int64)
        X0, Y0, X1, Y1 = fl[:, 0], fl[:, 1], fl[:, 2] + 1, fl[:, 3] + 1
        sx, sy, ex, ey = X0 % w, Y0 % h, X1 % w, Y1 % h
        ok = (np.trunc(lo) == np.trunc(hi)).all(axis=1) & (ex >= sx) & (ey >= sy)
        sx, sy, ex, ey = (np.where(ok, a, 0) for a in (sx, sy, ex, ey))
        sa = S[ey + 1, ex + 1] - S[sy, ex + 1] - S[ey + 1, sx] + S[sy, sx]
        resolved = ok & ((sa == 0) | (sa == (ex - sx + 1) * (ey - sy + 1)))
        total += int((~resolved).sum())
    return total, margin


def form_chunks(records, window):
    """triage_groups' join over the one section of an unstreamed bake's queue: windows of `window` records from the section's first; a record with open groups follows the
    head before it in its window when it is of the same item and hOpen + open <= 64.  -> list of chunks: head (record number), members (record numbers,
    head first), slots (first slot of each member), total (open groups), rect (union), ok, lds (classify_tiles loads the LDS window), mask (follower
    bits), dead (records of the head's window passed over between head and last member)"""
    chunks = []
    for w0 in range(0, len(records), window):
        cur = None
        for r in range(w0, min(w0 + window, len(records))):
            rec = records[r]
            if rec["open"] == 0:
                continue
            if cur is not None and rec["item"] == records[cur["head"]]["item"] and cur["total"] + rec["open"] <= 64:
                cur["members"].append(r)
                cur["slots"].append(cur["total"])
                cur["mask"] |= 1 << (r - cur["head"] - 1)
                cur["total"] += rec["open"]
                cur["ok"] = cur["ok"] and rec["ok"]
                a, b = cur["rect"], rec["rect"]
                cur["rect"] = (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))
            else:
                cur = dict(head=r, members=[r], slots=[0], mask=0, total=rec["open"], ok=rec["ok"], rect=rec["rect"], window_start=w0)
                chunks.append(cur)
    for c in chunks:
        sx, sy, ex, ey = c["rect"]
        c["lds"] = c["ok"] and ex - sx + 1 <= WIN and ey - sy + 1 <= WIN
        c["dead"] = [r for r in range(c["members"][0], c["members"][-1]) if r not in c["members"]]
        assert c["mask"] < 128 and c["total"] <= 64 and all(s < 64 for s in c["slots"])
    return chunks


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the oracle's decode and what it says about the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------
def oracle_states(oracle, case):
    """per triangle (every triangle its own work item under RAW_FLAGS): (4^level,) uint8 states from the oracle's bake"""
    raw = tc.bake(oracle, case, flags=RAW_FLAGS, rejection=0.0)
    bits = 2 if case["fmt"] == ot.FMT_4STATE else 1
    levels = case_levels(case)
    out = []
    for i, L in enumerate(levels):
        d = raw.descs[int(raw.index[i])]
        assert d[1] == L
        nb = int(tc.block_bytes(int(L), bits))
        out.append(tc.unpack_block(raw.array_data[None, int(d[0]):int(d[0]) + nb], 4 ** int(L), bits)[0])
    return out


def check_against_decode(case, sched, states):
    """every sub-triangle the restatement calls settled has exactly that state, on all its micro-triangles, in the oracle's decode"""
    levels = case_levels(case)
    for i, it in enumerate(sched["items"]):
        s, L = states[i], int(levels[i])
        if not sched["active"][i]:
            assert len(set(s.tolist())) == 1, (case["name"], i)
            continue
        if it is None:
            continue
        per_tile = s.reshape(len(it["tile_open"]), -1)
        for t in np.nonzero(~it["tile_open"])[0]:
            assert (per_tile[t] == it["tile_state"][t]).all(), (case["name"], i, t)
        per_group = s.reshape(-1, 64)
        gv = it["group_verdict"].reshape(-1)
        open_tile = np.repeat(it["tile_open"], it["gpt"])
        for g in np.nonzero((gv >= 0) & open_tile)[0]:
            assert (per_group[g] == gv[g]).all(), (case["name"], i, g)


def linear_bounds(case, sched, states):
    """(lower, upper) of openTiles in a Linear, one-mip bake: tiles with two states in the oracle's decode are certainly open, tiles the table settles
    certainly are not.  Level-5 and level-6 items are one tile, open whenever the item is active: the item may be culled by the curve test, so an active
    item of one state counts for the upper bound only."""
    lo = hi = 0
    for i, it in enumerate(sched["items"]):
        if it is None:
            continue
        per_tile = states[i].reshape(len(it["tile_open"]), -1)
        mixed = np.array([len(set(r.tolist())) > 1 for r in per_tile])
        assert not (mixed & ~it["tile_open"]).any()
        lo += int(mixed.sum())
        hi += int(it["tile_open"].sum())
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------------------------------------
# textures with isolated defects, and the seeded search that places them
# ---------------------------------------------------------------------------------------------------------------------------------------------
def base_texture(size, fp32, opaque=True):
    if fp32:
        return np.full((size, size), 0.9 if opaque else 0.1, F)
    return np.full((size, size), 230 if opaque else 25, np.uint8)


def put_defects(tex, texels):
    """texels on the other side of the cut-off"""
    out = tex.copy()
    for (x, y) in texels:
        out[y, x] = (F(0.1) if tex[y, x] > 0.5 else F(0.9)) if tex.dtype == np.float32 else (25 if tex[y, x] > 127 else 230)
    return out


def right_triangle(x0, y0, ex, ey, size, shift=(0, 0)):
    """right angle at texel coordinates (x0, y0), legs ex along u and ey along v, moved by whole periods"""
    return np.array([[x0 / size + shift[0], y0 / size + shift[1]], [(x0 + ex) / size + shift[0], y0 / size + shift[1]],
                     [x0 / size + shift[0], (y0 + ey) / size + shift[1]]], F)


TABLE_FLAGS = tc.EVERY_FLAGS | FLAG_NO_LEVELLINE


def make_case(name, tex, tris, levels, *, fmt=ot.FMT_4STATE, filt=ot.LINEAR, addr=ot.WRAP, flags=TABLE_FLAGS, rejection=0.0, family="J"):
    """a case in its "table" mode (module docstring) unless told otherwise"""
    levels = [int(x) for x in levels]
    c = tc.make_case(name, tex, np.concatenate([np.asarray(t, F).reshape(3, 2) for t in tris]), max(levels), levels=levels, fmt=fmt, flags=flags, filt=filt,
                     addr=addr, rejection=rejection)
    c["family"] = family
    return c


class DefectTable:
    """padded_table of an all-above texture with single-texel defects, evaluated entry by entry (the search asks for a few thousand entries of a table
    of up to 1024 x 1024 after every move)"""

    def __init__(self, defects):
        self.d = np.array(sorted(defects), np.int64).reshape(-1, 2)

    def __getitem__(self, key):
        Y, X = (np.asarray(k, np.int64) for k in key)
        out = X * Y
        if len(self.d):
            out = out - ((self.d[None, :, 0] < X[:, None]) & (self.d[None, :, 1] < Y[:, None])).sum(axis=1)
        return out


def open_counts(sched):
    """{(item, tile): open groups} of every record of the 4096-tile queue"""
    return {(r["item"], r["tile"]): r["open"] for r in sched["records"]}


def search(name, size, fp32, tris, levels, want, *, seed=1, addr=ot.WRAP, iters=60000, fmt=ot.FMT_4STATE):
    """Places single-texel defects on an opaque texture until the restated schedule has a record exactly for the tiles of `want` = {(item, tile): open
    groups}, with exactly that many open groups (0: a dead record).  A seeded walk over the texels that lie in the rectangle of a wanted tile and of no
    other tile: add a defect where a tile has too few open groups, take one away where it has too many, keep the move when the distance to `want` does
    not grow.  The walk counts with the rectangles alone; the placement is kept only if `restate_schedule` of the finished texture gives `want`.
    Raises when nothing is found: a case that cannot be built is a failure."""
    rng = np.random.default_rng(seed)
    base = base_texture(size, fp32)
    proto = make_case(name, base, tris, levels, addr=addr, fmt=fmt)
    p = np.ascontiguousarray(proto["uv"], F).reshape(-1, 6)
    allowed = np.zeros((size, size), bool)
    geo = [_geometry(p[i].tobytes(), int(levels[i]), size, size, addr) for i in range(len(p))]
    keys = sorted(want)
    for (i, t) in keys:
        R = geo[i]["tiles"]
        assert R["ok"][t] and levels[i] >= 6, (name, "wanted tile without a rectangle")
        allowed[R["sy"][t]:R["ey"][t] + 1, R["sx"][t]:R["ex"][t] + 1] = True
    for i, g in enumerate(geo):
        R = g["tiles"]
        for t in range(len(R["ok"])):
            if (i, t) not in want:
                assert R["ok"][t]
                allowed[R["sy"][t]:R["ey"][t] + 1, R["sx"][t]:R["ex"][t] + 1] = False
    cy, cx = np.nonzero(allowed)
    if len(cx) > MAX_CANDIDATES:            # (B's tiles are 385 texels wide: a seeded sample of their texels is plenty)
        keep = np.sort(rng.choice(len(cx), MAX_CANDIDATES, replace=False))
        cy, cx = cy[keep], cx[keep]
    K = len(cx)
    tinc, ginc = [], []
    for (i, t) in keys:
        R, G = geo[i]["tiles"], geo[i]["groups"]
        tinc.append((cx >= R["sx"][t]) & (cx <= R["ex"][t]) & (cy >= R["sy"][t]) & (cy <= R["ey"][t]))
        gs = slice(t * 64, t * 64 + 64)
        assert G["ok"][gs].all()
        ginc.append((cx[None, :] >= G["sx"][gs, None]) & (cx[None, :] <= G["ex"][gs, None]) & (cy[None, :] >= G["sy"][gs, None]) & (cy[None, :] <= G["ey"][gs, None]))
    tinc, ginc = np.array(tinc), np.array(ginc).astype(np.int32)            # (tiles, K), (tiles, 64, K)
    target = np.array([want[k] for k in keys])
    cand = [np.nonzero(r)[0] for r in tinc]
    assert all(len(c) for c in cand), (name, "a wanted tile has no texel of its own")
    state = {}

    def distance():
        return np.abs((state["g"] > 0).sum(axis=1) - target) + 8 * (state["t"] == 0)

    def walk():
        """one walk of at most `iters` moves -> the chosen texels, or None"""
        for it in range(iters):
            if it % 6000 == 0:          # a fresh start every 6000 moves
                sel = np.zeros(K, bool)
                state["g"], state["t"] = np.zeros(ginc.shape[:2], np.int32), np.zeros(len(keys), np.int32)
                d = distance()
            if d.sum() == 0:
                return sel
            bad = np.nonzero(d)[0]
            ti = int(bad[rng.integers(len(bad))]) if rng.random() < 0.9 else int(rng.integers(len(keys)))
            surplus = (state["g"][ti] > 0).sum() > target[ti]
            mine = cand[ti]
            if surplus or (rng.random() < 0.15 and sel[mine].any()):
                on = mine[sel[mine]]
                if not len(on):
                    continue
                k, sign = int(on[rng.integers(len(on))]), -1
            else:
                k, sign = int(mine[rng.integers(len(mine))]), 1
                if sel[k]:
                    continue
            state["g"] += sign * ginc[:, :, k]
            state["t"] += sign * tinc[:, k]
            nd = distance()
            if nd.sum() <= d.sum() or (nd.sum() <= d.sum() + 2 and rng.random() < 0.02):
                d, sel[k] = nd, sign > 0
            else:
                state["g"] -= sign * ginc[:, :, k]
                state["t"] -= sign * tinc[:, k]
        raise AssertionError("%s: no placement found (distance %d left)" % (name, int(d.sum())))

    # The Linear form of the case: the curve-free-region test may settle a tile the table leaves open.  A placement is kept when every wanted tile that
    # has an open group holds two states in the oracle's Linear decode -- such a tile is open on the device whatever the curve test says, so the bounds of
    # linear_bounds coincide on it.  `loose` lists the wanted tiles for which the last of LINEAR_TRIES placements still did not manage.
    for attempt in range(LINEAR_TRIES):
        sel = walk()
        defects = sorted((int(x), int(y)) for x, y in zip(cx[sel], cy[sel]))
        c = make_case(name, put_defects(base, defects), tris, levels, addr=addr, fmt=fmt)
        c["defects"] = defects
        assert open_counts(restate_schedule(c)) == want, name     # (kept only if the restatement of the real texture says so)
        st = oracle_states(own_oracle(), variant(c, mode="linear"))
        c["loose"] = [k for k in keys if want[k] > 0 and len(set(st[k[0]].reshape(-1, 4096)[k[1]].tolist())) < 2]
        if not c["loose"]:
            return c
    raise AssertionError("%s: no placement whose wanted tiles are all mixed in the Linear decode (left: %r)" % (name, c["loose"]))


def variant(case, mode=None, fmt=None, fp32=None, name=None):
    """the same placement in another mode ("table": Linear with DisableLevelLineIntersection, "linear", "nearest") / format / texel type"""
    c = dict(case)
    if mode is not None:
        c["filt"] = ot.NEAREST if mode == "nearest" else ot.LINEAR
        c["flags"] = (case["flags"] | FLAG_NO_LEVELLINE) if mode == "table" else (case["flags"] & ~FLAG_NO_LEVELLINE)
    if fmt is not None:
        c["fmt"] = fmt
    if fp32 is not None and (case["tex"].dtype == np.float32) != fp32:
        above = su.indicator(case["tex"], CUTOFF)
        c["tex"] = np.where(above, F(0.9), F(0.1)).astype(F) if fp32 else np.where(above, 230, 25).astype(np.uint8)
    c["mode"] = "nearest" if c["filt"] == ot.NEAREST else ("table" if c["flags"] & FLAG_NO_LEVELLINE else "linear")
    c["name"] = name or "%s-%s-f%d-%s" % (case["name"], c["mode"], c["fmt"], "fp32" if c["tex"].dtype == np.float32 else "u8")
    return c


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family J: the chunk join.  One level-9 item with a tile leg of 24 texels (group leg 3, micro-triangle leg 3 / 8) on a 256^2 texture
# ---------------------------------------------------------------------------------------------------------------------------------------------
SIZE = 256
J_TRI = right_triangle(5.3, 6.3, 192, 192, SIZE)
J_PAIRS = [(0, 1), (3, 4), (5, 6), (8, 9)]      # tiles that share a box (the two halves of a square): a defect in it opens both; they are adjacent records
J_LONE = 42                                     # a tile on the item's hypotenuse: nobody shares its box
J_SUMS = [62, 63, 64, 65, 66]
J_NEXT = 43                                     # ... and the next tile is another: adjacent records of unrelated boxes
# (the two halves of a square hold the same group boxes along their shared hypotenuse, and every other group box twice: the open groups of the two
#  sum to an even number, and a half next to a dead half has an even number itself.  Odd sums need tiles that share no box: 42 and 43.)
J_MEMBERS = {1: {J_LONE: 7}, 2: {0: 5, 1: 7}, 4: dict(zip([0, 1, 3, 4, 5, 6, 8, 9], [0, 6, 4, 0, 0, 4, 8, 0])),
             5: dict(zip([0, 1, 3, 4, 5, 6, 8, 9], [6, 0, 4, 6, 0, 4, 8, 0])), 8: dict(zip([0, 1, 3, 4, 5, 6, 8, 9], [8] * 8))}
J_TAILS = {7: [0, 1, 3, 4, 5, 6, J_LONE], 8: [0, 1, 3, 4, 5, 6, 8, 9], 9: [0, 1, 3, 4, 5, 6, 8, 9, J_LONE]}
J_LEVEL6 = [4, 10, 2, 20, 7]


def _one(want):
    return {(0, t): k for t, k in want.items()}


@functools.lru_cache(maxsize=None)
def j_case(name):
    """the "table", 4-state, UNORM8 form of a J case (variant() gives the others)"""
    kind, _, arg = name.partition("-")
    if kind == "sum":
        s = int(arg)
        return search("J-" + name, SIZE, False, [J_TRI], [9], _one({J_LONE: 30, J_NEXT: s - 30}), seed=s)
    if kind == "pair":           # the two halves of one square: one rectangle, the LDS window holds the chunk
        s = int(arg)
        return search("J-" + name, SIZE, False, [J_TRI], [9], _one({0: 30, 1: s - 30}), seed=s)
    if kind == "head64":
        return search("J-" + name, SIZE, False, [J_TRI], [9], _one({J_LONE: 64}), seed=3)
    if kind == "follower1":
        return search("J-" + name, SIZE, False, [J_TRI], [9], _one({0: 10, 1: 10, J_LONE: 1}), seed=4)
    if kind == "members":
        return search("J-" + name, SIZE, False, [J_TRI], [9], _one(J_MEMBERS[int(arg)]), seed=10 + int(arg))
    if kind == "tail":
        return search("J-" + name, SIZE, False, [J_TRI], [9], _one({t: 5 for t in J_TAILS[int(arg)]}), seed=20 + int(arg))
    if kind == "items":          # a level-8 and a level-7 item side by side: the record behind the level-8 item's last belongs to the other item
        tris = [right_triangle(5.3, 6.3, 96, 96, SIZE), right_triangle(120.3, 6.3, 48, 48, SIZE)]
        return search("J-" + name, SIZE, False, tris, [8, 7], {(0, 0): 10, (0, 1): 8, (1, 0): 8, (1, 1): 6}, seed=30)
    if kind == "four":           # four level-8 items (64 tiles: one wave), two open records each: a streamed bake cuts the queue between them
        tris = [right_triangle(5.3 + 105 * (k % 2), 6.3 + 105 * (k // 2), 96, 96, SIZE) for k in range(4)]
        want = {(k, t): n for k in range(4) for t, n in ((0, 6 + 2 * k), (1, 8 + 2 * k))}
        return search("J-" + name, SIZE, False, tris, [8] * 4, want, seed=31)
    if kind == "level6":         # level-6 items only (window 1); "level6-plus7": the same and a level-7 item, LAST in the input, first in the queue
        tris = [right_triangle(5.3 + 40 * k, 6.3, 24, 24, SIZE) for k in range(len(J_LEVEL6))]
        want = {(k, 0): n for k, n in enumerate(J_LEVEL6)}
        levels = [6] * len(J_LEVEL6)
        if arg == "plus7":
            tris.append(right_triangle(5.3, 60.3, 48, 48, SIZE))
            levels.append(7)
            want.update({(len(J_LEVEL6), 0): 12, (len(J_LEVEL6), 1): 14})
        return search("J-" + name, SIZE, False, tris, levels, want, seed=40)
    raise KeyError(name)


J_PAIR_SUMS = [62, 64, 66]
J_NAMES = ["sum-%d" % s for s in J_SUMS] + ["pair-%d" % s for s in J_PAIR_SUMS] + ["head64", "follower1"] + ["members-%d" % m for m in J_MEMBERS] + ["tail-%d" % n for n in J_TAILS] + \
          ["items", "four", "level6", "level6-plus7"]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family W: the LDS window
# ---------------------------------------------------------------------------------------------------------------------------------------------
W_SPOTS = [0, 1, 3, 4, 5, 6, J_LONE, 63]


@functools.lru_cache(maxsize=None)
def w_case(name):
    if name in ("sizes-a", "sizes-b"):     # tile legs of 29.5 and 30.5 texels: rectangles of 31 / 32 and of 32 / 33 texels, by the sub-texel offset of the tile
        ex, ey = (236, 244) if name == "sizes-a" else (244, 236)
        return search("W-" + name, SIZE, False, [right_triangle(5.3, 6.3, ex, ey, SIZE)], [9], _one({t: 4 for t in W_SPOTS}), seed=50)
    if name == "union":                    # tiles 4 and 5 are adjacent records with different boxes: each fits the window, their union (50 texels) does not
        return search("W-" + name, SIZE, False, [J_TRI], [9], _one({3: 0, 4: 6, 5: 6, 6: 0}), seed=51)
    if name == "origin":                   # rectangles from texel 0 on both axes: the zero row and column of the table's window
        return search("W-" + name, SIZE, False, [right_triangle(0.7, 0.7, 192, 192, SIZE)], [9], _one({0: 5, 1: 5}), seed=52)
    if name == "end":                      # rectangles that end at texel 255: tile 42 on u, tile 63 on v
        return search("W-" + name, SIZE, False, [right_triangle(62.8, 62.8, 192, 192, SIZE)], [9], _one({J_LONE: 5, 63: 5}), seed=53)
    if name in ("wrap+1", "wrap-2"):       # the J item a whole period away: region_rect translates the rectangle
        k = 1 if name == "wrap+1" else -2
        return search("W-" + name, SIZE, False, [right_triangle(5.3, 6.3, 192, 192, SIZE, shift=(k, k))], [9], _one({0: 12, 1: 10, 3: 4, 4: 6}), seed=54)
    if name in ("clamp-over", "border-over"):   # no defect: an item reaching over the left edge; the rectangles that leave [0, w) have no `ok`
        addr = ot.CLAMP if name == "clamp-over" else ot.BORDER
        return make_case("W-" + name, base_texture(SIZE, False), [right_triangle(-20.3, 6.3, 192, 192, SIZE)], [9], addr=addr, family="W")
    raise KeyError(name)


W_NAMES = ["sizes-a", "sizes-b", "union", "origin", "end", "wrap+1", "wrap-2", "clamp-over", "border-over"]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family M: the sums (stateMask, knownCount) through what reads them
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def m_dead_case():
    """a defect inside the box of hypotenuse tile 44 but outside the item: the tile is open, every group is settled, the item is uniform"""
    c = search("M-dead", SIZE, False, [J_TRI], [9], _one({44: 0}), seed=60)
    c["flags"] = ot.FLAG_THREADS
    c["family"] = "M"
    return c


def m_sources(sched, states, item=0):
    """known (T / O) micro-triangles of an item by where the kernels count them: settled tiles (triage_tiles, + 4096 each), settled groups of open tiles
    (triage_groups, + 64 each), the rest (classify_tiles phase 3) -- the last from the oracle's decode"""
    it = sched["items"][item]
    known = states[item] < 2
    tiles = int((~it["tile_open"] & (it["tile_state"] < 2)).sum()) * (4096 if it["gpt"] == 64 else 1024)
    gv = it["group_verdict"]
    groups = int(((gv >= 0) & (gv < 2) & it["tile_open"][:, None]).sum()) * 64
    return tiles, groups, int(known.sum()) - tiles - groups, int(known.sum())


def m_thresholds(known, total):
    """float32(known / total), the float below and the float above: kept, kept, rejected"""
    t = F(known) / F(total)
    return [(float(t), True), (float(np.nextafter(t, F(0))), True), (float(np.nextafter(t, F(2))), False)]


def m_threshold_case(fmt_fp32, rejection):
    c = variant(j_case("sum-64"), mode="linear", fmt=ot.FMT_4STATE, fp32=fmt_fp32)
    c["flags"] = ot.FLAG_THREADS
    c["rejection"] = float(rejection)
    c["family"] = "M"
    return c


# ---- M at level 5: the 1024-tile queue (16 groups per tile, four tiles per wave of triage_groups, 16 per workgroup) ----
# A level-5 item is one tile, never asked again by triage_tiles: its known count has two sources, settled groups and classified groups.  The items are
# skew (the two halves of a parallelogram have different boxes: a right triangle's group 0 shares its box with group 1), one per 40-texel cell; the
# cells are above and below the cut-off in turn and the patterns rotate, so the four items of a wave differ in state and in pattern.
M5_SIZE, M5_CELL, M5_PER_ROW = 512, 40, 12
M5_COUNTS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65]
M5_PATTERNS = [("none", 0x0000), ("all", 0xFFFF), ("group0", 0x0001), ("group15", 0x8000), ("alternating", 0x5555)]
M5_SHAPE = np.array([[5.3, 6.3], [29.3, 12.3], [11.3, 30.3]])


def m5_threshold_item(n):
    """the item whose known fraction is the threshold: the first "alternating" one (8 settled groups, 8 classified), or the "all" one of a small bake"""
    return 4 if n >= 5 else 1


def m5_triangle(k):
    return ((M5_SHAPE + np.array([M5_CELL * (k % M5_PER_ROW), M5_CELL * (k // M5_PER_ROW)])) / M5_SIZE).astype(F)


@functools.lru_cache(maxsize=None)
def m5_placement(k):
    """the defects of item k, placed directly: single texels in rectangles of groups of the pattern and of no other group, one per group still left out (for "none": one
    texel of the item's rectangle that no group's rectangle holds)"""
    g = _geometry(m5_triangle(k).tobytes(), 5, M5_SIZE, M5_SIZE, ot.WRAP)
    G, Wh = g["groups"], g["whole"]
    pattern = M5_PATTERNS[k % len(M5_PATTERNS)][1]
    ys, xs = np.mgrid[int(Wh["sy"][0]):int(Wh["ey"][0]) + 1, int(Wh["sx"][0]):int(Wh["ex"][0]) + 1]
    xs, ys = xs.ravel(), ys.ravel()
    assert xs.min() >= M5_CELL * (k % M5_PER_ROW) and xs.max() < M5_CELL * (k % M5_PER_ROW + 1) and ys.min() >= M5_CELL * (k // M5_PER_ROW) and ys.max() < M5_CELL * (k // M5_PER_ROW + 1)
    inside = (xs[None, :] >= G["sx"][:, None]) & (xs[None, :] <= G["ex"][:, None]) & (ys[None, :] >= G["sy"][:, None]) & (ys[None, :] <= G["ey"][:, None])
    mask = (inside.astype(np.int64) << np.arange(16)[:, None]).sum(axis=0)
    pick = (mask == 0) if pattern == 0 else ((mask != 0) & ((mask & ~pattern) == 0))
    chosen, covered = (list(np.nonzero(pick)[0][:1]) if pattern == 0 else []), 0
    for g in range(16):                    # a single texel for every group of the pattern that the texels before it leave out
        if (pattern >> g) & 1 and not (covered >> g) & 1:
            mine = np.nonzero(pick & (((mask >> g) & 1) == 1))[0]
            assert len(mine), (k, g, "pattern cannot be placed")
            chosen.append(int(mine[len(mine) // 2]))
            covered |= int(mask[chosen[-1]])
    assert len(chosen) and covered == pattern, (k, "pattern cannot be placed")
    return [(int(xs[i]), int(ys[i])) for i in chosen]


def m5_case(n, fp32=False, mode="table", fmt=ot.FMT_4STATE, rejection=0.0):
    y, x = np.mgrid[0:M5_SIZE, 0:M5_SIZE]
    above = ((x // M5_CELL + (y // M5_CELL) * M5_PER_ROW) % 2 == 0)
    tex = np.where(above, F(0.9), F(0.1)).astype(F) if fp32 else np.where(above, 230, 25).astype(np.uint8)
    tex = put_defects(tex, [d for k in range(n) for d in m5_placement(k)])
    c = make_case("M5-n%d" % n, tex, [m5_triangle(k) for k in range(n)], [5] * n, fmt=fmt, family="M", rejection=rejection,
                  flags=ot.FLAG_THREADS | ot.FLAG_NO_DEDUP | FLAG_NO_LEVELLINE)
    return variant(c, mode=mode)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family S: the unsliced launches of levels 0 - 4
# ---------------------------------------------------------------------------------------------------------------------------------------------
S_SIZE, S_CELL, S_CHECKER_ROWS = 512, 8, 300


def s_counts(level):
    per = 1024 // 4 ** level
    return [1] + [k * per + d for k in (1, 2) for d in (-1, 0, 1) if k * per + d > 1]


S_CASES = [(L, n) for L in range(5) for n in s_counts(L)]


@functools.lru_cache(maxsize=None)
def s_texture(fp32):
    """a 1-texel checker over the first 300 rows, above the cut-off below them"""
    y, x = np.mgrid[0:S_SIZE, 0:S_SIZE]
    above = ((x + y) & 1).astype(bool) | (y >= S_CHECKER_ROWS)
    return np.where(above, F(0.9), F(0.1)).astype(F) if fp32 else np.where(above, 230, 25).astype(np.uint8)


def s_case(level, count, fmt, fp32, mode="table"):
    """`count` triangles of 5 texels over the checker (active), one over the uniform rows behind every second of them (culled by triage_items)"""
    tris, per_row = [], S_SIZE // S_CELL
    for k in range(count):
        tris.append(right_triangle(S_CELL * (k % per_row) + 1.3, S_CELL * (k // per_row) + 1.3, 5, 5, S_SIZE))
        if k % 2 == 1:
            u = k // 2
            tris.append(right_triangle(S_CELL * (u % per_row) + 1.3, S_CHECKER_ROWS + 8 + S_CELL * (u // per_row) + 1.3, 5, 5, S_SIZE))
    assert S_CELL * ((count - 1) // per_row) + 8 < S_CHECKER_ROWS and S_CHECKER_ROWS + 16 + S_CELL * (count // 2 // per_row) + 8 <= S_SIZE
    c = make_case("S-L%d-n%d-f%d-%s" % (level, count, fmt, "fp32" if fp32 else "u8"), s_texture(fp32), tris, [level] * len(tris), fmt=fmt, family="S",
                  flags=ot.FLAG_THREADS | ot.FLAG_NO_DEDUP | FLAG_NO_LEVELLINE)
    c["count"] = count
    return variant(c, mode=mode, name=c["name"] + "-" + mode)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# family B: micro-triangles of several texels.  J's join at level 7 on a 1024^2 texture: micro-triangle leg 6 texels, group leg 48, tile leg 384
# ---------------------------------------------------------------------------------------------------------------------------------------------
B_SIZE = 1024
B_TRI = right_triangle(20.3, 21.3, 768, 768, B_SIZE)
B_SUMS = [62, 64, 65]
B_WANTS = {"sum-62": {2: 30, 3: 32}, "sum-64": {2: 30, 3: 34}, "sum-65": {2: 30, 3: 35},       # tiles 2 and 3 share no box
           "members-4": {0: 6, 1: 8, 2: 5, 3: 7}, "dead": {0: 0, 1: 6, 2: 0, 3: 5}, "tail-3": {0: 4, 1: 4, 2: 3}}
B_NAMES = list(B_WANTS)


@functools.lru_cache(maxsize=None)
def b_case(name, mode="linear"):
    c = search("B-" + name, B_SIZE, False, [B_TRI], [7], _one(B_WANTS[name]), seed=70 + len(name) + sum(B_WANTS[name].values()))
    c["family"] = "B"
    return variant(c, mode=mode)


def b_mips_case():
    """a degenerate item and a two-mip chain: the serial fine_state inside the deferred pass"""
    c = dict(b_case("sum-64"))
    mip1 = np.ascontiguousarray(c["tex"][::2, ::2])
    deg = np.array([[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]], F)
    c2 = make_case("B-mips", c["tex"], [B_TRI, deg], [7, 7], flags=tc.EVERY_FLAGS, family="B")
    c2["mips"] = [c["tex"], mip1]
    return c2


# ---------------------------------------------------------------------------------------------------------------------------------------------
# above the deterministic size: one level-10 item, 256 tiles = four waves of triage_tiles
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def t_case(mode="table"):
    size = 512
    rng = np.random.default_rng(80)
    tri = right_triangle(5.3, 6.3, 384, 384, size)
    defects = [(int(x), int(y)) for x, y in rng.integers(8, 390, (160, 2)) if x + y < 380]
    return variant(make_case("T-level10", put_defects(base_texture(size, False), defects), [tri], [10], family="T"), mode=mode)
