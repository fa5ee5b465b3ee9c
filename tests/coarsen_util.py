"""Shared by tests/test_coarsen.py, tests/test_coarsen_gpu.py and tests/scripts/coarsen_throughput.py: ctypes bindings of ommxCoarsenMicromap, two
statements of the definition in include/omm_mi355x_ext.h that owe nothing to the kernels -- restate_coarsen (numpy: unpack, reshape(4^T, -1), the set
rule, then uniform blocks, duplicates, order, offsets, index buffer, histograms) and brute_coarsen (Python loops over single states, levels <= 4) --
the block patterns of the tier edges, and the upload / download of a call's arrays."""
import ctypes as C
import numpy as np
import ommtest as ot
import lookup_util as lu
import stats_util as su
import rebuild_util as ru
from rebuild_util import NONE, NO_SPECIAL, NO_DEDUP, representatives  # noqa: F401  (the callers' names for them)

INFO_FIELDS = ("arrayDataSize", "descArrayCount", "referencedBlocks", "coarsenedBlocks", "uniformBlocks", "duplicateBlocks", "skippedPrimitives")
RAW_DESC = np.dtype([("o", "<u4"), ("l", "<u2"), ("f", "<u2")])


class CoarsenDesc(C.Structure):
    _fields_ = [("maxSubdivisionLevel", C.c_uint32), ("mixedState", C.c_uint8), ("reserved", C.c_uint8 * 3), ("flags", C.c_uint32)]


class CoarsenInfo(C.Structure):
    _fields_ = [("arrayDataSize", C.c_uint64), ("descArrayCount", C.c_uint32), ("referencedBlocks", C.c_uint32), ("coarsenedBlocks", C.c_uint32),
                ("uniformBlocks", C.c_uint32), ("duplicateBlocks", C.c_uint32), ("skippedPrimitives", C.c_uint32)]


def bind(dll):
    su.bind(dll)
    dll.ommxCoarsenMicromap.argtypes = [C.c_void_p, C.POINTER(ot.BakeResultDesc), C.POINTER(CoarsenDesc), C.POINTER(C.c_void_p), C.POINTER(CoarsenInfo),
                                        C.c_void_p]
    return dll


def c_desc(max_level, mixed=3, flags=0, reserved=(0, 0, 0)):
    d = CoarsenDesc()
    d.maxSubdivisionLevel, d.mixedState, d.flags = max_level, mixed, flags
    d.reserved[:] = list(reserved)
    return d


def info_dict(info):
    return {f: int(getattr(info, f)) for f in INFO_FIELDS}


# ---- the definition, twice ----
def block_states(array_data, offset, level, bits):
    n = 4 ** level
    b = np.unpackbits(np.asarray(array_data[offset:offset + su.block_bytes(level, bits)], np.uint8), bitorder="little")[:n * bits]
    return b if bits == 1 else b[0::2] + 2 * b[1::2]


def coarsen_states(states, level, target, bits, mixed):
    """the 4^target states of a block of `level` coarsened to `target` <= level: the set rule of the header on reshape(4^target, -1)"""
    g = np.asarray(states, np.uint8).reshape(4 ** target, -1)
    side, unknown = g & 1, g >> 1
    both = side.min(axis=1) != side.max(axis=1)
    if bits == 1:
        return np.where(both, mixed & 1, side[:, 0]).astype(np.uint8)
    return np.where(both, mixed, side[:, 0] | (2 * unknown.any(axis=1))).astype(np.uint8)


def brute_states(states, level, target, bits, mixed):
    """the same by loops over single states (levels <= 4)"""
    assert level <= 4 and len(states) == 4 ** level
    span, out = 4 ** (level - target), []
    for j in range(4 ** target):
        covered = [int(s) for s in states[j * span:(j + 1) * span]]
        sides = {s & 1 for s in covered}
        if len(sides) == 2:
            out.append(mixed if bits == 2 else mixed & 1)
        else:
            out.append(sides.pop() | (2 if any(s >> 1 for s in covered) else 0))
    return out


def _valid(desc, size):
    o, l, f = (int(x) for x in desc)
    return l <= 12 and f in (1, 2) and o + su.block_bytes(l, f) <= size


def restate_coarsen(array_data, descs, index, index_format, max_level, mixed=3, flags=0, array_data_size=None, unpacked=None, merge=None):
    """What ommxCoarsenMicromap answers, from host copies (array_data uint8, descs (D, 3) rows of (offset, level, format), index signed) -> dict:
    array (uint8), descs (E, 3) int64, index (in the format's dtype), array_hist / index_hist ({(level, format): count}), info ({field: int}).
    unpacked: a dict that keeps the unpacked states of the source blocks between calls on the same arrays; merge: see rebuild_util.representatives()"""
    size = len(array_data) if array_data_size is None else array_data_size
    descs = np.asarray(descs, np.int64).reshape(-1, 3)
    e = np.asarray(index).astype(np.int64)
    D = len(descs)
    cap = min(max_level, 12)
    valid = np.array([_valid(d, size) for d in descs], bool)
    selects = (e >= 0) & (e < D)
    selects[selects] = valid[e[selects]]
    special_in = (e < 0) & (e >= -4)
    out_e = np.where(special_in, e, -4)
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["skippedPrimitives"] = int(len(e) - selects.sum() - special_in.sum())
    blocks, entry, target_of = {}, {}, {}          # source index -> output bytes; -> special entry; -> (level, format)
    for d in np.unique(e[selects]).tolist():
        o, l, f = (int(x) for x in descs[d])
        t = min(l, cap)
        states = unpacked.get((o, l, f)) if unpacked is not None else None
        if states is None:
            states = block_states(array_data, o, l, f)
            if unpacked is not None:
                unpacked[(o, l, f)] = states
        out = coarsen_states(states, l, t, f, mixed)
        info["referencedBlocks"] += 1
        info["coarsenedBlocks"] += l > cap
        uniform = bool((out == out[0]).all())
        info["uniformBlocks"] += uniform
        target_of[d] = (t, f)
        if uniform and not flags & NO_SPECIAL:
            entry[d] = -(int(out[0]) + 1)
        else:
            blocks[d] = lu.pack(out, f)
    tail = ru.restate_tail(target_of, blocks, entry, flags, merge)
    new_entry = np.zeros(D, np.int64)
    for d, v in tail["entry"].items():
        new_entry[d] = v
    out_e[selects] = new_entry[e[selects]]
    uses = np.bincount(e[selects], minlength=D) if D else np.zeros(0, np.int64)
    info["duplicateBlocks"], info["arrayDataSize"], info["descArrayCount"] = tail["duplicates"], len(tail["array"]), len(tail["emitted"])
    return dict(array=tail["array"], descs=tail["descs"], index=out_e.astype(su.INDEX_DTYPE[index_format]), array_hist=tail["array_hist"],
                index_hist=ru.index_histogram(target_of, blocks, uses), info=info)


def brute_coarsen(blocks, index, max_level, mixed=3, flags=0):
    """The same answer for well-formed inputs by Python loops.  blocks: [(states, level, bits)], index: entries -> (blocks out as [(states list, level,
    bits)] in output order, index entries)"""
    outs, used = {}, sorted({i for i in index if i >= 0})
    for d in used:
        states, level, bits = blocks[d]
        t = min(level, max_level)
        outs[d] = (brute_states(list(states), level, t, bits, mixed), t, bits)
    special = {d: -(o[0][0] + 1) for d, o in outs.items() if not flags & NO_SPECIAL and all(s == o[0][0] for s in o[0])}
    keep = [d for d in used if d not in special]
    rep = {}
    for d in keep:
        rep[d] = d
        if not flags & NO_DEDUP:
            for c in keep:
                if c < d and outs[c] == outs[d]:
                    rep[d] = c
                    break
    emitted = sorted((d for d in keep if rep[d] == d), key=lambda d: (-max(1, 4 ** outs[d][1] * outs[d][2] // 8), d))
    entries = [i if i < 0 else special[i] if i in special else emitted.index(rep[i]) for i in index]
    return [outs[d] for d in emitted], entries


# ---- block patterns: known, leaning and mixed outcomes at every scale of the combine ----
def planted_states(level, bits, seed):
    """random states of a block of `level` with planted regions at EVERY scale 4^0 .. 4^level: each aligned region of each scale is, with some probability,
    made uniform in one state, one-sided known/unknown, or left alone -- so that reductions by any number of levels meet groups that stay known, groups
    that lean to unknown and groups that are mixed"""
    rng = np.random.default_rng(seed * 131 + level * 7 + bits)
    n = 4 ** level
    top = 2 if bits == 1 else 4
    s = rng.integers(0, top, n).astype(np.uint8)
    for scale in range(level + 1):
        span, groups = 4 ** scale, 4 ** (level - scale)
        pick = rng.random(groups)
        g = s.reshape(groups, span)
        state = rng.integers(0, top, groups).astype(np.uint8)
        uniform = pick < 0.30
        g[uniform] = state[uniform, None]
        if bits == 2:
            lean = (pick >= 0.30) & (pick < 0.55)          # one side, known and unknown of it
            side = (state & 1)[:, None]
            g[lean] = (side | (2 * (rng.random((groups, span)) < 0.3)).astype(np.uint8))[lean]
    return s


def table_of_blocks(blocks, first_offset=0, gap=0, filler=0xA5):
    """blocks: [(states, level, bits)] -> (array_data, descs (D, 3)), each block `gap` bytes behind the last"""
    parts, descs, at = [np.full(first_offset, filler, np.uint8)], [], first_offset
    for states, level, bits in blocks:
        b = lu.pack(states, bits)
        descs.append((at, level, bits))
        parts += [b, np.full(gap, filler, np.uint8)]
        at += len(b) + gap
    return np.concatenate(parts), np.array(descs, np.int64).reshape(-1, 3)


def raw_descs(descs):
    descs = np.asarray(descs, np.int64).reshape(-1, 3)
    raw = np.zeros(len(descs), RAW_DESC)
    raw["o"], raw["l"], raw["f"] = descs[:, 0], descs[:, 1], descs[:, 2]
    return raw


# ---- a call on the device ----
class Source:
    """device copies of a hand-built result: the array data LAST in its allocation, at `array_align` modulo 2 * array_align, so that a read past the
    array leaves the allocation's payload; descs and index in allocations of their own.  declared: (arrayDataSize, descArrayCount, indexCount) where
    the desc declares less than the arrays hold."""

    def __init__(self, hip, array_data, descs, index, index_format, array_align=16, declared=None):
        self.hip = hip
        idx = np.asarray(index).astype(su.INDEX_DTYPE[index_format])
        raw = raw_descs(descs)
        lead = array_align if array_align < 256 else 0          # hipMalloc returns 256-byte aligned memory
        self.bufs = [hip.upload(np.concatenate([np.full(lead, 0x5A, np.uint8), np.asarray(array_data, np.uint8)])),
                     hip.upload(raw if len(raw) else np.zeros(1, RAW_DESC)), hip.upload(idx if len(idx) else np.zeros(4, np.int8))]
        size, D, T = declared if declared else (len(array_data), len(raw), len(idx))
        rd = ot.BakeResultDesc()
        rd.arrayData, rd.arrayDataSize = self.bufs[0].value + lead, size
        rd.descArray, rd.descArrayCount = C.cast(self.bufs[1], C.POINTER(ot.MicromapDesc)), D
        rd.indexBuffer, rd.indexCount, rd.indexFormat = self.bufs[2], T, index_format
        self.rd = rd
        self.host = (np.asarray(array_data, np.uint8), np.asarray(descs, np.int64).reshape(-1, 3), np.asarray(index).astype(np.int64))
        self.declared, self.unpacked = declared, {}

    def model(self, max_level, mixed=3, flags=0):
        a, d, i = self.host
        if self.declared:
            size, D, T = self.declared
            return restate_coarsen(a, d[:D], i[:T], self.rd.indexFormat, max_level, mixed, flags, size, self.unpacked)
        return restate_coarsen(a, d, i, self.rd.indexFormat, max_level, mixed, flags, unpacked=self.unpacked)

    def unchanged(self):
        """the source arrays still hold what was uploaded"""
        a, d, i = self.host
        lead = self.rd.arrayData - self.bufs[0].value
        return (np.array_equal(self.hip.download(self.bufs[0], lead + len(a))[lead:], a)
                and (not len(d) or np.array_equal(self.hip.download(self.bufs[1], 8 * len(d)).view(RAW_DESC), raw_descs(d)))
                and np.array_equal(self.hip.download(self.bufs[2], i.size * np.dtype(su.INDEX_DTYPE[self.rd.indexFormat]).itemsize)
                                   .view(su.INDEX_DTYPE[self.rd.indexFormat]), i.astype(su.INDEX_DTYPE[self.rd.indexFormat])))

    def close(self):
        for p in self.bufs:
            self.hip.free(p)
        self.bufs = []


def coarsen(dll, baker, rd, max_level, mixed=3, flags=0, want_result=True, stream=None):
    """-> (result code, info dict, handle or None)"""
    out, info = C.c_void_p(), CoarsenInfo()
    r = dll.ommxCoarsenMicromap(baker, C.byref(rd), C.byref(c_desc(max_level, mixed, flags)), C.byref(out) if want_result else None, C.byref(info), stream)
    return r, info_dict(info), (out if want_result and r == ot.SUCCESS else None)


def result_desc_of(dll, handle):
    pd = C.POINTER(ot.BakeResultDesc)()
    assert dll.ommxGetDeviceBakeResultDesc(handle, C.byref(pd)) == ot.SUCCESS
    return pd.contents


def hist_dict(ptr, count):
    out = {}
    for k in range(count):
        key = (int(ptr[k].subdivisionLevel), int(ptr[k].format))
        assert key not in out and ptr[k].count > 0, "a histogram entry twice, or a zero count"
        out[key] = int(ptr[k].count)
    return out


def download_result(dll, hip, handle):
    """host copies of a device result -> dict like restate_coarsen's (without info), plus rdesc (the device desc)"""
    rd = result_desc_of(dll, handle)
    dt = su.INDEX_DTYPE[rd.indexFormat]
    descs = hip.download(rd.descArray, 8 * rd.descArrayCount).view(RAW_DESC) if rd.descArrayCount else np.zeros(0, RAW_DESC)
    return dict(array=hip.download(rd.arrayData, rd.arrayDataSize) if rd.arrayDataSize else np.zeros(0, np.uint8),
                descs=np.stack([descs["o"], descs["l"], descs["f"]], 1).astype(np.int64).reshape(-1, 3),
                index=hip.download(rd.indexBuffer, rd.indexCount * np.dtype(dt).itemsize).view(dt),
                array_hist=hist_dict(rd.descArrayHistogram, rd.descArrayHistogramCount), index_hist=hist_dict(rd.indexHistogram, rd.indexHistogramCount),
                rdesc=rd, index_format=rd.indexFormat)


def assert_same(got, ref):
    """byte for byte: arrayData, descArray, index buffer; the histograms as mappings"""
    assert len(got["array"]) == len(ref["array"]), (len(got["array"]), len(ref["array"]))
    assert np.array_equal(got["descs"], ref["descs"]), "descArray"
    bad = np.nonzero(got["array"] != ref["array"])[0]
    assert bad.size == 0, "arrayData: %d bytes differ, first at %d of %d" % (bad.size, bad[0], len(ref["array"]))
    assert got["index"].dtype == ref["index"].dtype and np.array_equal(got["index"], ref["index"]), "index buffer"
    assert got["array_hist"] == ref["array_hist"] and got["index_hist"] == ref["index_hist"], (got["array_hist"], ref["array_hist"], got["index_hist"], ref["index_hist"])


def coarsen_and_check(dll, hip, baker, src, max_level, mixed=3, flags=0, stream=None):
    """the whole contract on one input: the info-only call, the full call, both against the model; the output is accepted by the statistics entry;
    the source is untouched -> the model's answer"""
    ref = src.model(max_level, mixed, flags)
    r, info, _ = coarsen(dll, baker, src.rd, max_level, mixed, flags, want_result=False, stream=stream)
    assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
    r, info, handle = coarsen(dll, baker, src.rd, max_level, mixed, flags, stream=stream)
    assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
    try:
        got = download_result(dll, hip, handle)
        assert_same(got, ref)
        if not flags & (NO_SPECIAL | NO_DEDUP):
            assert info["referencedBlocks"] == info["descArrayCount"] + info["uniformBlocks"] + info["duplicateBlocks"]
        areas = C.c_void_p(1)
        assert dll.ommxGetDeviceBakeResultTriangleAreas(handle, C.byref(areas)) == ot.SUCCESS and not areas.value
        assert src.unchanged()
    finally:
        assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
    return ref


def device_stats(dll, baker, rd):
    st, skipped = ot.DebugStats(), C.c_uint32(77)
    assert dll.ommxDebugGetStatsDevice(baker, C.byref(rd), None, None, C.byref(st), C.byref(skipped), None) == ot.SUCCESS
    return su.int_fields(st), skipped.value
