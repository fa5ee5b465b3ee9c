"""Shared by tests/test_gather.py, tests/test_gather_gpu.py and tests/scripts/gather_throughput.py: ctypes bindings of ommxGatherMicromaps, two
statements of the definition in include/omm_mi355x_ext.h that owe nothing to the kernels -- restate_gather (numpy: resolve the selection, the bounds
rule, unpack with coarsen_util.block_states, repack with lookup_util.pack, then promotion, duplicates, order, offsets, index buffer, histograms, info)
and brute_gather (Python loops over single states, levels <= 4) -- and the call on device copies of hand-built sources."""
import ctypes as C
import numpy as np
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import combine_util as mu
import rebuild_util as ru
from rebuild_util import NONE, NO_SPECIAL, NO_DEDUP  # noqa: F401  (the callers' names for them)

MAX_SOURCES = 4096
INFO_FIELDS = ("arrayDataSize", "descArrayCount", "primitiveCount", "referencedBlocks", "uniformBlocks", "duplicateBlocks", "skippedPrimitives")
REF = np.dtype([("source", "<u4"), ("primitive", "<u4")])


class GatherDesc(C.Structure):
    _fields_ = [("selection", C.c_void_p), ("selectionCount", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class GatherInfo(C.Structure):
    _fields_ = [("arrayDataSize", C.c_uint64), ("descArrayCount", C.c_uint32), ("primitiveCount", C.c_uint32), ("referencedBlocks", C.c_uint32),
                ("uniformBlocks", C.c_uint32), ("duplicateBlocks", C.c_uint32), ("skippedPrimitives", C.c_uint32)]


def bind(dll):
    mu.bind(dll)
    dll.ommxGatherMicromaps.argtypes = [C.c_void_p, C.POINTER(C.POINTER(ot.BakeResultDesc)), C.c_uint32, C.POINTER(GatherDesc), C.POINTER(C.c_void_p),
                                        C.POINTER(GatherInfo), C.c_void_p]
    return dll


def c_desc(selection=None, count=0, flags=0, reserved=0):
    d = GatherDesc()
    d.selection, d.selectionCount, d.flags, d.reserved = selection, count, flags, reserved
    return d


def info_dict(info):
    return {f: int(getattr(info, f)) for f in INFO_FIELDS}


def refs(pairs):
    """[(source, primitive)] -> the selection as the header's array of ommxPrimitiveRef"""
    out = np.zeros(len(pairs), REF)
    if len(pairs):
        p = np.asarray(pairs, np.int64).reshape(-1, 2)
        out["source"], out["primitive"] = p[:, 0], p[:, 1]
    return out


# ---- the definition, twice ----
def restate_gather(sources, selection=None, flags=0, unpacked=None, merge=None):
    """What ommxGatherMicromaps answers.  sources: [(array_data uint8, descs (D, 3) rows of (offset, level, format), index, arrayDataSize or None)];
    selection: None or (N, 2) rows of (source, primitive) -> dict: array (uint8), descs (E, 3) int64, index (int32), array_hist / index_hist
    ({(level, format): count}), info ({field: int}).  unpacked: a dict that keeps the packed bytes of source blocks between calls on the same sources;
    merge: see rebuild_util.representatives()"""
    K = len(sources)
    counts = np.array([len(s[2]) for s in sources], np.int64)
    tables = [np.asarray(s[1], np.int64).reshape(-1, 3) for s in sources]
    desc_end = np.cumsum([len(t) for t in tables])
    desc_base = desc_end - [len(t) for t in tables]
    if selection is None:
        ks = np.repeat(np.arange(K, dtype=np.int64), counts)
        ps = np.concatenate([np.arange(n, dtype=np.int64) for n in counts]) if K else np.zeros(0, np.int64)
    else:
        sel = np.asarray(selection, np.int64).reshape(-1, 2)
        ks, ps = sel[:, 0], sel[:, 1]
    N = len(ks)
    out_e = np.full(N, -4, np.int64)
    item_of = np.full(N, -1, np.int64)                    # the (source, descriptor) pair as a rank in the concatenated descriptor arrays
    passes = np.zeros(N, bool)                            # a special entry passes through
    named = ks < K
    named[named] = ps[named] < counts[ks[named]]
    order = np.nonzero(named)[0]
    order = order[np.argsort(ks[order], kind="stable")]
    cuts = np.searchsorted(ks[order], np.arange(K + 1))
    for k in np.unique(ks[order]).tolist():
        prims = order[cuts[k]:cuts[k + 1]]
        a, d, index, size = sources[k]
        e = np.asarray(index).astype(np.int64)[ps[prims]]
        special = (e < 0) & (e >= -4)
        out_e[prims[special]] = e[special]
        passes[prims[special]] = True
        valid = mu._valid_rows(tables[k], len(a) if size is None else size)
        selects = (e >= 0) & (e < len(tables[k]))
        selects[selects] = valid[e[selects]]
        item_of[prims[selects]] = desc_base[k] + e[selects]
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["primitiveCount"] = N
    info["skippedPrimitives"] = int(N - passes.sum() - (item_of >= 0).sum())
    blocks, entry, kind = {}, {}, {}                       # item -> output bytes; -> special entry; -> (level, format)
    for it in np.unique(item_of[item_of >= 0]).tolist():
        k = int(np.searchsorted(desc_end, it, side="right"))
        o, l, f = (int(x) for x in tables[k][it - desc_base[k]])
        key = (id(sources[k][0]), o, l, f)
        packed = unpacked.get(key) if unpacked is not None else None
        if packed is None:
            packed = lu.pack(cu.block_states(sources[k][0], o, l, f), f)
            if unpacked is not None:
                unpacked[key] = packed
        info["referencedBlocks"] += 1
        kind[it] = (l, f)
        uniform_state = _uniform_state(packed, l, f)
        info["uniformBlocks"] += uniform_state is not None
        if uniform_state is not None and not flags & NO_SPECIAL:
            entry[it] = -(uniform_state + 1)
        else:
            blocks[it] = packed
    tail = ru.restate_tail(kind, blocks, entry, flags, merge)
    chosen, items, uses = item_of >= 0, sorted(kind), {}
    if chosen.any():
        at_item = np.searchsorted(items, item_of[chosen])
        out_e[chosen] = np.array([tail["entry"][it] for it in items], np.int64)[at_item]
        uses = dict(zip(items, np.bincount(at_item, minlength=len(items))))
    info["duplicateBlocks"], info["arrayDataSize"], info["descArrayCount"] = tail["duplicates"], len(tail["array"]), len(tail["emitted"])
    return dict(array=tail["array"], descs=tail["descs"], index=out_e.astype(np.int32), array_hist=tail["array_hist"],
                index_hist=ru.index_histogram(kind, blocks, uses), info=info)


def _uniform_state(packed, level, bits):
    """the one state of a packed block whose states are all equal, or None (from the bytes: 4^level fields of `bits` bits)"""
    fields = 4 ** level
    b = np.unpackbits(packed, bitorder="little")[:fields * bits]
    s = b if bits == 1 else b[0::2] + 2 * b[1::2]
    return int(s[0]) if (s == s[0]).all() else None


def brute_gather(sources, selection=None, flags=0):
    """The same answer for well-formed sources by Python loops.  sources: [(blocks as [(states, level, bits)], index entries)]; selection: None or
    [(source, primitive)] -> (blocks out as [(states list, level, bits)] in output order, index entries, counts (referenced, uniform, duplicate,
    skipped))"""
    if selection is None:
        selection = [(k, p) for k, (_, index) in enumerate(sources) for p in range(len(index))]
    entries_in, skipped = [], 0
    for k, p in selection:
        if k >= len(sources) or p >= len(sources[k][1]):
            entries_in.append(None)
            skipped += 1
        else:
            entries_in.append((k, int(sources[k][1][p])))
    items = sorted({ke for ke in entries_in if ke is not None and ke[1] >= 0})
    body = {}
    for k, e in items:
        states, level, bits = sources[k][0][e]
        assert level <= 4
        body[(k, e)] = ([int(s) for s in states], level, bits)
    uniform = [it for it in items if all(s == body[it][0][0] for s in body[it][0])]
    special = {} if flags & NO_SPECIAL else {it: -(body[it][0][0] + 1) for it in uniform}
    keep = [it for it in items if it not in special]
    rep = {}
    for n, it in enumerate(keep):
        rep[it] = it if flags & NO_DEDUP else next((c for c in keep[:n] if body[c] == body[it]), it)
    emitted = sorted((it for it in keep if rep[it] == it), key=lambda it: (-max(1, 4 ** body[it][1] * body[it][2] // 8), it))
    entries = []
    for ke in entries_in:
        if ke is None:
            entries.append(-4)
        elif ke[1] < 0:
            entries.append(ke[1])
        else:
            entries.append(special[ke] if ke in special else emitted.index(rep[ke]))
    return [body[it] for it in emitted], entries, (len(items), len(uniform), len(keep) - len(emitted), skipped)


# ---- a call on the device ----
def gather(dll, baker, rds, selection=None, count=0, flags=0, want_result=True, stream=None):
    """selection: a device pointer (or None) -> (result code, info dict, handle or None)"""
    out, info = C.c_void_p(), GatherInfo()
    r = dll.ommxGatherMicromaps(baker, mu.pointer_array(rds), len(rds), C.byref(c_desc(selection, count, flags)), C.byref(out) if want_result else None,
                                C.byref(info), stream)
    return r, info_dict(info), (out if want_result and r == ot.SUCCESS else None)


def check_result(dll, hip, baker, handle, info, ref, flags=0):
    """every output byte, both histograms, the info and the invariant against the model; 32-bit entries, no triangle areas, accepted by the statistics"""
    got = cu.download_result(dll, hip, handle)
    assert info == ref["info"], (info, ref["info"])
    assert got["index_format"] == ot.IDX_U32
    cu.assert_same(got, ref)
    if not flags:
        assert info["referencedBlocks"] == info["descArrayCount"] + info["uniformBlocks"] + info["duplicateBlocks"]
    areas = C.c_void_p(1)
    assert dll.ommxGetDeviceBakeResultTriangleAreas(handle, C.byref(areas)) == ot.SUCCESS and not areas.value
    want = su.reference_stats(ref["array"], ref["descs"], ref["index"])
    assert cu.device_stats(dll, baker, got["rdesc"]) == (want["fields"], 0)
    return got


def gather_and_check(dll, hip, baker, srcs, selection=None, flags=0, stream=None, unpacked=None, keep=False):
    """the whole contract on one input: the info-only call, the full call, both against the model; the sources are untouched.  selection: None or
    [(source, primitive)] / an array of REF -> the model's answer (keep: and the handle, which the caller destroys)"""
    sel = None if selection is None else (selection if isinstance(selection, np.ndarray) and selection.dtype == REF else refs(selection))
    pairs = None if sel is None else np.stack([sel["source"], sel["primitive"]], 1).astype(np.int64)
    ref = restate_gather(mu.host_sources(srcs), pairs, flags, unpacked)
    rds = [s.rd for s in srcs]
    d_sel = None if sel is None else hip.upload(sel if len(sel) else np.zeros(1, REF))
    n = 0 if sel is None else len(sel)
    handle = None
    try:
        r, info, _ = gather(dll, baker, rds, d_sel, n, flags, want_result=False, stream=stream)
        assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
        r, info, handle = gather(dll, baker, rds, d_sel, n, flags, stream=stream)
        assert r == ot.SUCCESS, r
        check_result(dll, hip, baker, handle, info, ref, flags)
        assert all(s.unchanged() for s in {id(s): s for s in srcs}.values())
    finally:
        if d_sel is not None:
            hip.free(d_sel)
        if handle is not None and not keep:
            assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
    return (ref, handle) if keep else ref
