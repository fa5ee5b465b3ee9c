"""Shared by tests/test_combine.py, tests/test_combine_gpu.py and tests/scripts/combine_throughput.py: ctypes bindings of ommxCombineMicromaps, two
statements of the definition in include/omm_mi355x_ext.h that owe nothing to the kernels -- restate_combine (numpy: unpack with
coarsen_util.block_states, np.repeat down to the tuple's level, the set rule over the K rows, then promotion, duplicates, order, offsets, index buffer,
histograms, info) and brute_combine (Python loops over single states, levels <= 4) -- and the call on device copies of hand-built sources."""
import ctypes as C
import numpy as np
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import rebuild_util as ru

MAX_SOURCES = 16
INFO_FIELDS = ("arrayDataSize", "descArrayCount", "combinedTuples", "refinedTuples", "uniformBlocks", "duplicateBlocks", "skippedPrimitives")


class CombineDesc(C.Structure):
    _fields_ = [("format", C.c_uint32), ("mixedState", C.c_uint8), ("reserved", C.c_uint8 * 3), ("flags", C.c_uint32)]


class CombineInfo(C.Structure):
    _fields_ = [("arrayDataSize", C.c_uint64), ("descArrayCount", C.c_uint32), ("combinedTuples", C.c_uint32), ("refinedTuples", C.c_uint32),
                ("uniformBlocks", C.c_uint32), ("duplicateBlocks", C.c_uint32), ("skippedPrimitives", C.c_uint32)]


def bind(dll):
    cu.bind(dll)
    dll.ommxCombineMicromaps.argtypes = [C.c_void_p, C.POINTER(C.POINTER(ot.BakeResultDesc)), C.c_uint32, C.POINTER(CombineDesc), C.POINTER(C.c_void_p),
                                         C.POINTER(CombineInfo), C.c_void_p]
    return dll


def c_desc(fmt, mixed=3, flags=0, reserved=(0, 0, 0)):
    d = CombineDesc()
    d.format, d.mixedState, d.flags = fmt, mixed, flags
    d.reserved[:] = list(reserved)
    return d


def pointer_array(rds):
    """the deviceResults argument over ctypes result descs (None: a null element)"""
    arr = (C.POINTER(ot.BakeResultDesc) * max(len(rds), 1))()
    for k, rd in enumerate(rds):
        arr[k] = C.pointer(rd) if rd is not None else None
    return arr


def info_dict(info):
    return {f: int(getattr(info, f)) for f in INFO_FIELDS}


# ---- the definition, twice ----
def join_states(rows, fmt, mixed):
    """the rule over the K rows of a (K, n) array of states 0..3 -> n states in the output format"""
    rows = np.asarray(rows, np.uint8)
    side, unknown = rows & 1, rows >> 1
    both = side.min(axis=0) != side.max(axis=0)
    r = np.where(both, mixed, side[0] | (2 * unknown.any(axis=0))).astype(np.uint8)
    return r & 1 if fmt == 1 else r


def brute_join(states, fmt, mixed):
    """the same for one micro-triangle by a loop over its K states"""
    sides = {int(s) & 1 for s in states}
    r = mixed if len(sides) == 2 else sides.pop() | (2 if any(int(s) >> 1 for s in states) else 0)
    return r & 1 if fmt == 1 else r


def _valid_rows(descs, size):
    d = np.asarray(descs, np.int64).reshape(-1, 3)
    ok = (d[:, 1] <= 12) & ((d[:, 2] == 1) | (d[:, 2] == 2))
    bytes_ = np.maximum(1, (np.where(ok, d[:, 2], 1) << (2 * np.where(ok, d[:, 1], 0))) >> 3)
    return ok & (d[:, 0] + bytes_ <= size)


def restate_combine(sources, fmt, mixed=3, unpacked=None, merge=None):
    """What ommxCombineMicromaps answers.  sources: [(array_data uint8, descs (D, 3) rows of (offset, level, format), index, arrayDataSize or None)] ->
    dict: array (uint8), descs (E, 3) int64, index (int32), array_hist / index_hist ({(level, format): count}), info ({field: int}).
    unpacked: a dict that keeps the unpacked states of source blocks between calls on the same sources (keyed by id of the array); merge: see
    rebuild_util.representatives()"""
    K = len(sources)
    T = len(sources[0][2])
    entries = np.stack([np.asarray(s[2]).astype(np.int64) for s in sources], 1) if T else np.zeros((0, K), np.int64)
    fails, is_block = np.zeros(T, bool), np.zeros((T, K), bool)
    tables = []
    for k, (a, d, _, size) in enumerate(sources):
        d = np.asarray(d, np.int64).reshape(-1, 3)
        valid = _valid_rows(d, len(a) if size is None else size)
        e = entries[:, k]
        inside = (e >= 0) & (e < len(d))
        good = inside.copy()
        good[inside] = valid[e[inside]]
        fails |= (e < -4) | ((e >= 0) & ~good)
        is_block[:, k] = good
        tables.append(d)
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["skippedPrimitives"] = int(fails.sum())
    out_e = np.full(T, -4, np.int64)
    only_special = ~fails & ~is_block.any(axis=1)
    if only_special.any():
        out_e[only_special] = -(join_states((-(entries[only_special] + 1)).T, fmt, mixed).astype(np.int64) + 1)
    joined = ~fails & is_block.any(axis=1)
    prims = np.nonzero(joined)[0]
    none = np.zeros(0, np.int64)
    tuples, first, inverse = np.unique(entries[prims], axis=0, return_index=True, return_inverse=True) if len(prims) else (none.reshape(0, K), none, none)
    order = np.argsort(first, kind="stable")                 # tuples by their lowest primitive
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    info["combinedTuples"] = len(order)
    blocks, entry, kind = {}, {}, {}                         # tuple (by rank) -> output bytes; -> special entry; -> (level, format)
    for t, u in enumerate(order.tolist()):
        tup = tuples[u]
        levels = [int(tables[k][e, 1]) for k, e in enumerate(tup) if e >= 0]
        top = max(levels)
        info["refinedTuples"] += min(levels) < top
        rows = []
        for k, e in enumerate(tup.tolist()):
            if e < 0:
                rows.append(np.full(4 ** top, -(e + 1), np.uint8))
                continue
            o, l, f = (int(x) for x in tables[k][e])
            key = (id(sources[k][0]), o, l, f)
            states = unpacked.get(key) if unpacked is not None else None
            if states is None:
                states = cu.block_states(sources[k][0], o, l, f)
                if unpacked is not None:
                    unpacked[key] = states
            rows.append(np.repeat(states, 4 ** (top - l)))
        out = join_states(np.stack(rows), fmt, mixed)
        kind[t] = (top, fmt)
        if (out == out[0]).all():
            info["uniformBlocks"] += 1
            entry[t] = -(int(out[0]) + 1)
        else:
            blocks[t] = lu.pack(out, fmt)
    tail = ru.restate_tail(kind, blocks, entry, 0, merge)
    uses = {}
    if len(order):
        of_prim = rank[inverse.reshape(-1)]
        out_e[prims] = np.array([tail["entry"][t] for t in range(len(order))], np.int64)[of_prim]
        uses = np.bincount(of_prim, minlength=len(order))
    info["duplicateBlocks"], info["arrayDataSize"], info["descArrayCount"] = tail["duplicates"], len(tail["array"]), len(tail["emitted"])
    return dict(array=tail["array"], descs=tail["descs"], index=out_e.astype(np.int32), array_hist=tail["array_hist"],
                index_hist=ru.index_histogram(kind, blocks, uses), info=info)


def brute_combine(sources, fmt, mixed=3):
    """The same answer for well-formed inputs by Python loops.  sources: [(blocks as [(states, level, bits)], index entries)] -> (blocks out as [(states
    list, level)] in output order, index entries, info counts (tuples, refined, uniform, duplicate))"""
    K, T = len(sources), len(sources[0][1])
    tuples, outs = [], {}
    for i in range(T):
        tup = tuple(int(s[1][i]) for s in sources)
        if any(e >= 0 for e in tup) and tup not in tuples:
            tuples.append(tup)
    refined = 0
    for tup in tuples:
        levels = [sources[k][0][e][1] for k, e in enumerate(tup) if e >= 0]
        top = max(levels)
        assert top <= 4
        refined += min(levels) < top
        states = []
        for j in range(4 ** top):
            seen = []
            for k, e in enumerate(tup):
                if e < 0:
                    seen.append(-(e + 1))
                else:
                    block, level, _ = sources[k][0][e]
                    seen.append(int(block[j >> (2 * (top - level))]))
            states.append(brute_join(seen, fmt, mixed))
        outs[tup] = (states, top)
    special = {tup: -(o[0][0] + 1) for tup, o in outs.items() if all(s == o[0][0] for s in o[0])}
    keep = [tup for tup in tuples if tup not in special]
    rep = {}
    for n, tup in enumerate(keep):
        rep[tup] = next((c for c in keep[:n] if outs[c] == outs[tup]), tup)
    emitted = sorted((tup for tup in keep if rep[tup] == tup), key=lambda tup: (-max(1, 4 ** outs[tup][1] * fmt // 8), tuples.index(tup)))
    entries = []
    for i in range(T):
        tup = tuple(int(s[1][i]) for s in sources)
        if all(e < 0 for e in tup):
            entries.append(-(brute_join([-(e + 1) for e in tup], fmt, mixed) + 1))
        else:
            entries.append(special[tup] if tup in special else emitted.index(rep[tup]))
    counts = (len(tuples), refined, len(special), len(keep) - len(emitted))
    return [outs[tup] for tup in emitted], entries, counts


# ---- a call on the device ----
def host_sources(srcs):
    """coarsen_util.Source objects -> restate_combine's sources (what each source DECLARES)"""
    out = []
    for s in srcs:
        a, d, i = s.host
        if s.declared:
            size, D, T = s.declared
            out.append((a, d[:D], i[:T], size))
        else:
            out.append((a, d, i, None))
    return out


def combine(dll, baker, rds, fmt, mixed=3, want_result=True, stream=None):
    """-> (result code, info dict, handle or None)"""
    out, info = C.c_void_p(), CombineInfo()
    r = dll.ommxCombineMicromaps(baker, pointer_array(rds), len(rds), C.byref(c_desc(fmt, mixed)), C.byref(out) if want_result else None, C.byref(info), stream)
    return r, info_dict(info), (out if want_result and r == ot.SUCCESS else None)


def check_result(dll, hip, baker, handle, info, ref):
    """every output byte, both histograms, the info and the invariant against the model; 32-bit entries, no triangle areas, accepted by the statistics"""
    got = cu.download_result(dll, hip, handle)
    assert info == ref["info"], (info, ref["info"])
    assert got["index_format"] == ot.IDX_U32
    cu.assert_same(got, ref)
    assert info["combinedTuples"] == info["descArrayCount"] + info["uniformBlocks"] + info["duplicateBlocks"]
    areas = C.c_void_p(1)
    assert dll.ommxGetDeviceBakeResultTriangleAreas(handle, C.byref(areas)) == ot.SUCCESS and not areas.value
    want = su.reference_stats(ref["array"], ref["descs"], ref["index"])
    assert cu.device_stats(dll, baker, got["rdesc"]) == (want["fields"], 0)
    return got


def combine_and_check(dll, hip, baker, srcs, fmt, mixed=3, stream=None, unpacked=None):
    """the whole contract on one input: the info-only call, the full call, both against the model; the sources are untouched -> the model's answer"""
    ref = restate_combine(host_sources(srcs), fmt, mixed, unpacked)
    rds = [s.rd for s in srcs]
    r, info, _ = combine(dll, baker, rds, fmt, mixed, want_result=False, stream=stream)
    assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
    r, info, handle = combine(dll, baker, rds, fmt, mixed, stream=stream)
    assert r == ot.SUCCESS, r
    try:
        check_result(dll, hip, baker, handle, info, ref)
        assert all(s.unchanged() for s in {id(s): s for s in srcs}.values())
    finally:
        assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
    return ref
