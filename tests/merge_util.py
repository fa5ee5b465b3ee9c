"""Shared by tests/test_merge.py, tests/test_merge_gpu.py and tests/scripts/merge_throughput.py: ctypes bindings of ommxMergeSimilarMicromaps, two
statements of the definition in include/omm_mi355x_ext.h that owe nothing to the kernels -- restate_merge (numpy: the live candidates of a level as one
(n, 4^L) array, the signatures by fancy indexing, leaders by np.unique, distances by a row-wise comparison, joins by minimum.at / maximum.at, then the
tail of rebuild_util) and brute_merge (Python loops over single fields read bit by bit and over single items) -- planted near-copies, and the call on
device copies of hand-built sources."""
import ctypes as C
import numpy as np
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import compare_util as pu
import rebuild_util as ru
from rebuild_util import NO_SPECIAL  # noqa: F401  (the callers' name for it)

UNIT = 4 ** 12
MAX_ROUNDS, MAX_SAMPLES = 32, 28
NONE = 0xFFFFFFFF
COUNT_FIELDS = ("arrayDataSize", "descArrayCount", "referencedBlocks", "candidateBlocks", "absorbedBlocks", "uniformBlocks", "duplicateBlocks",
                "skippedPrimitives")


class MergeDesc(C.Structure):
    _fields_ = [("maxDistance", C.c_uint32), ("rounds", C.c_uint32), ("samples", C.c_uint32), ("seed", C.c_uint32), ("mixedState", C.c_uint8),
                ("reserved", C.c_uint8 * 3), ("flags", C.c_uint32)]


class MergeInfo(C.Structure):
    _fields_ = [("arrayDataSize", C.c_uint64)] + [(f, C.c_uint32) for f in COUNT_FIELDS[1:]] + [("absorbedPerRound", C.c_uint32 * MAX_ROUNDS)]


def bind(dll):
    pu.bind(dll)
    lu.bind(dll)
    dll.ommxMergeSimilarMicromaps.argtypes = [C.c_void_p, C.POINTER(ot.BakeResultDesc), C.POINTER(MergeDesc), C.c_void_p, C.POINTER(C.c_void_p),
                                              C.POINTER(MergeInfo), C.c_void_p]
    return dll


def c_desc(max_distance=0, rounds=0, samples=0, seed=0, mixed=3, flags=0, reserved=(0, 0, 0)):
    d = MergeDesc()
    d.maxDistance, d.rounds, d.samples, d.seed, d.mixedState, d.flags = max_distance, rounds, samples, seed, mixed, flags
    d.reserved[:] = list(reserved)
    return d


def info_dict(info):
    d = {f: int(getattr(info, f)) for f in COUNT_FIELDS}
    d["absorbedPerRound"] = [int(x) for x in info.absorbedPerRound]
    return d


# ---- the definition, twice ----
def lowbias32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def pos(seed, L, r, j):
    return lowbias32(seed + 0x9E3779B9 * ((L << 16) | (r << 8) | j)) & (4 ** L - 1)


def join_states(rows, mixed):
    """the join of ommxCombineMicromaps across the rows of a (k, n) array of 4-state states"""
    rows = np.asarray(rows, np.uint8)
    side, unknown = rows & 1, rows >> 1
    return np.where(side.min(axis=0) != side.max(axis=0), mixed, side[0] | (2 * unknown.any(axis=0))).astype(np.uint8)


def _defaults(rounds, samples):
    return rounds or 8, samples or 16


def restate_merge(array_data, descs, index, index_format, max_distance, rounds=0, samples=0, seed=0, mixed=3, flags=0, array_data_size=None, unpacked=None):
    """What ommxMergeSimilarMicromaps answers, from host copies as for coarsen_util.restate_coarsen -> dict: array, descs, index, array_hist,
    index_hist, info, roots (uint32 per source descriptor), states ({surviving item: its final states}), source ({item: its source states})"""
    rounds, samples = _defaults(rounds, samples)
    size = len(array_data) if array_data_size is None else array_data_size
    descs = np.asarray(descs, np.int64).reshape(-1, 3)
    e = np.asarray(index).astype(np.int64)
    D = len(descs)
    valid = np.array([cu._valid(d, size) for d in descs], bool)
    selects = (e >= 0) & (e < D)
    selects[selects] = valid[e[selects]]
    special_in = (e < 0) & (e >= -4)
    out_e = np.where(special_in, e, -4)
    items = np.unique(e[selects]).tolist()
    states, kind = {}, {}
    for d in items:
        o, l, f = (int(x) for x in descs[d])
        s = unpacked.get((o, l, f)) if unpacked is not None else None
        if s is None:
            s = cu.block_states(array_data, o, l, f)
            if unpacked is not None:
                unpacked[(o, l, f)] = s
        states[d], kind[d] = s, (l, f)
    source = dict(states)
    candidates = [d for d in items if kind[d][1] == 2 and kind[d][0] >= 1]
    lead, per_round = {}, [0] * MAX_ROUNDS
    live_by_level = {}
    for d in candidates:
        live_by_level.setdefault(kind[d][0], []).append(d)          # (ascending: items is sorted)
    for r in range(rounds):
        for L in sorted(live_by_level):
            live = live_by_level[L]
            if len(live) < 2:
                continue
            S = np.stack([states[d] for d in live])
            at = np.array([pos(seed, L, r, j) for j in range(samples)])
            sig = S[:, at].astype(np.uint64)
            key = (sig << (2 * np.arange(samples, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
            _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
            leader = first[inverse.reshape(-1)]                                     # (the first row under a key is its lowest rank)
            dist = (S != S[leader]).sum(axis=1)
            absorbed = (leader != np.arange(len(live))) & (dist * 4 ** (12 - L) <= max_distance)
            if not absorbed.any():
                continue
            side, unknown = S & 1, S >> 1
            lo, hi, un = side.copy(), side.copy(), unknown.copy()
            np.minimum.at(lo, leader[absorbed], side[absorbed])
            np.maximum.at(hi, leader[absorbed], side[absorbed])
            np.maximum.at(un, leader[absorbed], unknown[absorbed])
            joined = np.where(lo != hi, mixed, lo | (2 * un)).astype(np.uint8)
            for k in np.unique(leader[absorbed]).tolist():
                states[live[k]] = joined[k]
            for k in np.nonzero(absorbed)[0].tolist():
                lead[live[k]] = live[int(leader[k])]
                del states[live[k]]
            per_round[r] += int(absorbed.sum())
            live_by_level[L] = [d for k, d in enumerate(live) if not absorbed[k]]

    def root(d):
        while d in lead:
            d = lead[d]
        return d

    roots = np.full(D, NONE, np.uint32)
    for d in items:
        roots[d] = root(d)
    info = dict.fromkeys(COUNT_FIELDS, 0)
    info.update(skippedPrimitives=int(len(e) - selects.sum() - special_in.sum()), referencedBlocks=len(items), candidateBlocks=len(candidates),
                absorbedBlocks=len(lead), absorbedPerRound=per_round)
    blocks, entry, kept = {}, {}, {}
    for d, s in states.items():
        uniform = bool((s == s[0]).all())
        info["uniformBlocks"] += uniform
        kept[d] = kind[d]
        if uniform and not flags & NO_SPECIAL:
            entry[d] = -(int(s[0]) + 1)
        else:
            blocks[d] = lu.pack(s, kind[d][1])
    tail = ru.restate_tail(kept, blocks, entry, flags)
    rooted = roots[e[selects]].astype(np.int64)
    new_entry = np.zeros(D, np.int64)
    for d, v in tail["entry"].items():
        new_entry[d] = v
    out_e[selects] = new_entry[rooted]
    uses = np.bincount(rooted, minlength=D) if D else np.zeros(0, np.int64)
    info["duplicateBlocks"], info["arrayDataSize"], info["descArrayCount"] = tail["duplicates"], len(tail["array"]), len(tail["emitted"])
    return dict(array=tail["array"], descs=tail["descs"], index=out_e.astype(su.INDEX_DTYPE[index_format]), array_hist=tail["array_hist"],
                index_hist=ru.index_histogram(kept, blocks, uses), info=info, roots=roots, states=states, source=source)


def brute_merge(array_data, descs, index, max_distance, rounds=0, samples=0, seed=0, mixed=3, flags=0, array_data_size=None):
    """The same answer by Python loops over single fields and single items (levels <= 4); every entry is judged by the sentences of the header ->
    dict: blocks [(states list, level, bits)] in output order, index (entries), roots, info"""
    rounds, samples = _defaults(rounds, samples)
    size = len(array_data) if array_data_size is None else array_data_size
    D = len(descs)

    def judge(e):
        if e < 0:
            return "special" if e >= -4 else None
        if e >= D:
            return None
        o, l, f = (int(x) for x in descs[e])
        if l > 12 or f not in (1, 2) or o + max(1, (4 ** l * f) // 8) > size:
            return None
        return "block"

    judged = [judge(int(e)) for e in index]
    items = sorted({int(e) for e, what in zip(index, judged) if what == "block"})
    bits = {}
    for d in items:
        o, l, f = (int(x) for x in descs[d])
        assert l <= 4
        bits[d] = [pu._field(array_data, o, f, j) for j in range(4 ** l)]
    level = {d: int(descs[d][1]) for d in items}
    fmt = {d: int(descs[d][2]) for d in items}
    candidates = [d for d in items if fmt[d] == 2 and level[d] >= 1]
    live, lead, per_round = list(candidates), {}, [0] * MAX_ROUNDS
    for r in range(rounds):
        keys = {}
        for d in live:
            k = level[d] << 56
            for j in range(samples):
                k |= bits[d][pos(seed, level[d], r, j)] << (2 * j)
            keys[d] = k
        decided = []
        for d in live:
            leader = min(c for c in live if keys[c] == keys[d])
            if leader == d:
                continue
            dist = sum(1 for x, y in zip(bits[d], bits[leader]) if x != y)
            if dist * 4 ** (12 - level[d]) <= max_distance:
                decided.append((d, leader))
        joined = {}
        for d, leader in decided:                                     # (both blocks as they were at the start of the round)
            acc = joined.setdefault(leader, list(bits[leader]))
            for j, (x, y) in enumerate(zip(acc, bits[d])):
                acc[j] = mixed if (x & 1) != (y & 1) else (x & 1) | (2 if (x | y) & 2 else 0)
        assert not set(joined) & {d for d, _ in decided}              # a leader is never absorbed in its own round
        for leader, acc in joined.items():
            bits[leader] = acc
        for d, leader in decided:
            lead[d] = leader
            live.remove(d)
        per_round[r] = len(decided)

    def root(d):
        while d in lead:
            d = lead[d]
        return d

    left = [d for d in items if d not in lead]
    uniform = [d for d in left if all(s == bits[d][0] for s in bits[d])]
    special = {d: -(bits[d][0] + 1) for d in uniform} if not flags & NO_SPECIAL else {}
    keep = [d for d in left if d not in special]
    rep = {}
    for d in keep:
        rep[d] = d
        for c in keep:
            if c < d and (bits[c], level[c], fmt[c]) == (bits[d], level[d], fmt[d]):
                rep[d] = c
                break
    emitted = sorted((d for d in keep if rep[d] == d), key=lambda d: (-max(1, 4 ** level[d] * fmt[d] // 8), d))
    entries = []
    for e, what in zip(index, judged):
        if what == "special":
            entries.append(int(e))
        elif what is None:
            entries.append(-4)
        else:
            at = root(int(e))
            entries.append(special[at] if at in special else emitted.index(rep[at]))
    info = dict(arrayDataSize=sum(max(1, 4 ** level[d] * fmt[d] // 8) for d in emitted), descArrayCount=len(emitted), referencedBlocks=len(items),
                candidateBlocks=len(candidates), absorbedBlocks=len(lead), uniformBlocks=len(uniform), duplicateBlocks=sum(1 for d in keep if rep[d] != d),
                skippedPrimitives=sum(1 for what in judged if what is None), absorbedPerRound=per_round)
    roots = [root(d) if d in bits else NONE for d in range(D)]
    return dict(blocks=[(bits[d], level[d], fmt[d]) for d in emitted], index=entries, roots=roots, info=info)


def output_states(ref):
    """the blocks of a restated result, unpacked -> [(states list, level, bits)] in output order"""
    return [(cu.block_states(ref["array"], int(o), int(l), int(f)).tolist(), int(l), int(f)) for o, l, f in ref["descs"]]


def lost_known_fields(ref, descs, index):
    """per primitive weight 4^(12 - L): the source fields that were known and are unknown in the output, summed over the primitives of valid blocks
    -> (lost, kept known) in units of 4^-12 of a primitive; asserts the safety statement field by field on the way"""
    descs = np.asarray(descs, np.int64).reshape(-1, 3)
    lost = kept = 0
    uses = {}
    for e in np.asarray(index).astype(np.int64).tolist():
        if 0 <= e < len(descs) and ref["roots"][e] != NONE:
            uses[e] = uses.get(e, 0) + 1
    for d, n in uses.items():
        src, out = ref["source"][d], ref["states"][int(ref["roots"][d])]
        assert ((out == src) | (out >= 2)).all(), d                    # the source state or an unknown state
        w = 4 ** (12 - int(descs[d][1])) * n
        lost += int(((src < 2) & (out >= 2)).sum()) * w
        kept += int(((src < 2) & (out < 2)).sum()) * w
    return lost, kept


# ---- planted near-copies ----
def near_copies(level, count, share, seed, bits=2):
    """`count` blocks of `level`: one base of planted states (coarsen_util.planted_states) and copies of it with about `share` of their fields set to
    another state (at least one field) -> [(states, level, bits)], the base first"""
    rng = np.random.default_rng(seed * 977 + level)
    base = cu.planted_states(level, bits, seed)
    out = [(base, level, bits)]
    n, top = 4 ** level, 2 * bits
    for _ in range(count - 1):
        s = base.copy()
        flips = rng.choice(n, max(1, int(round(n * share * rng.uniform(0.4, 1.0)))), replace=False)
        s[flips] = (s[flips] + rng.integers(1, top, len(flips))) % top
        out.append((s, level, bits))
    return out


# ---- a call on the device ----
def host_of(src):
    """the host arrays of a coarsen_util.Source as it declares them -> (array, descs, index, size or None)"""
    a, d, i = src.host
    if src.declared:
        size, D, T = src.declared
        return a, d[:D], i[:T], size
    return a, d, i, None


def model(src, max_distance, **kw):
    a, d, i, size = host_of(src)
    return restate_merge(a, d, i, src.rd.indexFormat, max_distance, array_data_size=size, unpacked=src.unpacked, **kw)


def merge(dll, hip, baker, rd, max_distance, rounds=0, samples=0, seed=0, mixed=3, flags=0, want_result=True, want_roots=True, want_info=True, stream=None):
    """-> (result code, info dict or None, handle or None, roots (uint32 array) or None); the roots buffer is pre-filled with 0xEE"""
    out, info = C.c_void_p(), MergeInfo()
    n = int(rd.descArrayCount)
    buf = hip.upload(np.full(max(n, 1) * 4, 0xEE, np.uint8)) if want_roots else None
    try:
        r = dll.ommxMergeSimilarMicromaps(baker, C.byref(rd), C.byref(c_desc(max_distance, rounds, samples, seed, mixed, flags)), buf,
                                          C.byref(out) if want_result else None, C.byref(info) if want_info else None, stream)
        roots = hip.download(buf, 4 * n).view(np.uint32) if want_roots and n else (np.zeros(0, np.uint32) if want_roots else None)
    finally:
        if buf is not None:
            hip.free(buf)
    ok = r == ot.SUCCESS
    return r, (info_dict(info) if want_info and ok else None), (out if want_result and ok else None), roots


def merge_and_check(dll, hip, baker, src, max_distance, stream=None, ref=None, **kw):
    """the whole contract on one input: the info-only call, the roots-only call and the full call against the model; the output has no areas; the
    source is untouched -> the model's answer"""
    ref = ref or model(src, max_distance, **kw)
    r, info, _, _ = merge(dll, hip, baker, src.rd, max_distance, want_result=False, want_roots=False, stream=stream, **kw)
    assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
    r, _, _, roots = merge(dll, hip, baker, src.rd, max_distance, want_result=False, want_info=False, stream=stream, **kw)
    assert r == ot.SUCCESS and np.array_equal(roots, ref["roots"]), "roots alone"
    r, info, handle, roots = merge(dll, hip, baker, src.rd, max_distance, stream=stream, **kw)
    assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
    try:
        cu.assert_same(cu.download_result(dll, hip, handle), ref)
        bad = np.nonzero(roots != ref["roots"])[0]
        assert bad.size == 0, "roots: %d differ, first at %d: %d != %d" % (bad.size, bad[0], roots[bad[0]], ref["roots"][bad[0]])
        if not kw.get("flags", 0):
            assert info["referencedBlocks"] == info["descArrayCount"] + info["absorbedBlocks"] + info["uniformBlocks"] + info["duplicateBlocks"]
        assert sum(info["absorbedPerRound"]) == info["absorbedBlocks"] and not any(info["absorbedPerRound"][kw.get("rounds", 0) or 8:])
        areas = C.c_void_p(1)
        assert dll.ommxGetDeviceBakeResultTriangleAreas(handle, C.byref(areas)) == ot.SUCCESS and not areas.value
        assert src.unchanged()
    finally:
        assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
    return ref
