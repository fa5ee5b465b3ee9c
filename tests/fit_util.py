"""Shared by tests/test_fit.py, tests/test_fit_gpu.py and tests/scripts/fit_throughput.py: ctypes bindings of ommxProfileMicromapLevels,
ommxCoarsenMicromapLevels and ommxFitMicromap, and statements of their definitions in include/omm_mi355x_ext.h that owe nothing to the kernels or to
fit_plan.h -- the profile in numpy (reshape(4^t, -1) with the set rule, on coarsen_util.block_states) and in Python loops over single states, the
weights as Python integers through math.frexp, the plan as Python integers with a rescan of every candidate at every step, and restate_coarsen_levels
(coarsen_util.coarsen_states per block with its own target, then rebuild_util.restate_tail)."""
import ctypes as C
import math
import numpy as np
import ommtest as ot
import lookup_util as lu
import stats_util as su
import rebuild_util as ru
import coarsen_util as cu
from rebuild_util import NONE, NO_SPECIAL, NO_DEDUP  # noqa: F401  (the callers' names for them)

LEVELS = 13          # OMMX_PROFILE_LEVELS
NO_LEVEL = 0xFF
PROFILE_INFO_FIELDS = ("referencedBlocks", "skippedPrimitives", "weightExponent", "reserved")
FIT_INFO_FIELDS = ("unfittedArrayDataSize", "plannedArrayDataSize", "steps")


class LevelProfileOutputs(C.Structure):
    _fields_ = [("knownCounts", C.c_void_p), ("knownOpaqueCounts", C.c_void_p), ("referenceCounts", C.c_void_p), ("blockWeights", C.c_void_p)]


class LevelProfileInfo(C.Structure):
    _fields_ = [("referencedBlocks", C.c_uint32), ("skippedPrimitives", C.c_uint32), ("weightExponent", C.c_int32), ("reserved", C.c_uint32)]


class FitDesc(C.Structure):
    _fields_ = [("maxArrayDataSize", C.c_uint64), ("devicePrimitiveWeights", C.c_void_p), ("maxSubdivisionLevel", C.c_uint32), ("mixedState", C.c_uint8),
                ("reserved", C.c_uint8 * 3), ("flags", C.c_uint32)]


class FitInfo(C.Structure):
    _fields_ = [("result", cu.CoarsenInfo), ("unfittedArrayDataSize", C.c_uint64), ("plannedArrayDataSize", C.c_uint64), ("steps", C.c_uint64)]


def bind(dll):
    cu.bind(dll)
    dll.ommxProfileMicromapLevels.argtypes = [C.c_void_p, C.POINTER(ot.BakeResultDesc), C.c_void_p, C.POINTER(LevelProfileOutputs), C.POINTER(LevelProfileInfo),
                                              C.c_void_p]
    dll.ommxCoarsenMicromapLevels.argtypes = [C.c_void_p, C.POINTER(ot.BakeResultDesc), C.c_void_p, C.POINTER(cu.CoarsenDesc), C.POINTER(C.c_void_p),
                                              C.POINTER(cu.CoarsenInfo), C.c_void_p]
    dll.ommxFitMicromap.argtypes = [C.c_void_p, C.POINTER(ot.BakeResultDesc), C.POINTER(FitDesc), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(FitInfo), C.c_void_p]
    return dll


def f_desc(budget, weights=None, max_level=12, mixed=3, flags=0, reserved=(0, 0, 0)):
    d = FitDesc()
    d.maxArrayDataSize, d.devicePrimitiveWeights, d.maxSubdivisionLevel, d.mixedState, d.flags = budget, weights, max_level, mixed, flags
    d.reserved[:] = list(reserved)
    return d


def fit_info_dict(info):
    out = {f: int(getattr(info, f)) for f in FIT_INFO_FIELDS}
    out["result"] = cu.info_dict(info.result)
    return out


# ---- the profile, twice ----
def known_counts(states, level):
    """(known[13], opaque[13]) of one block from its states: a group is known when every state is < 2 and they are all of one side"""
    known, opaque = [0] * LEVELS, [0] * LEVELS
    s = np.asarray(states, np.uint8)
    for t in range(level + 1):
        g = s.reshape(4 ** t, -1)
        ok = (g < 2).all(axis=1) & (g.min(axis=1) == g.max(axis=1))
        known[t], opaque[t] = int(ok.sum()), int((ok & (g[:, 0] == 1)).sum())
    return known, opaque


def brute_known_counts(states, level):
    """the same by loops over single states (levels <= 4)"""
    assert level <= 4 and len(states) == 4 ** level
    known, opaque = [0] * LEVELS, [0] * LEVELS
    for t in range(level + 1):
        span = 4 ** (level - t)
        for j in range(4 ** t):
            covered = [int(x) for x in states[j * span:(j + 1) * span]]
            if all(x == covered[0] for x in covered) and covered[0] < 2:
                known[t] += 1
                opaque[t] += covered[0]
    return known, opaque


def weight_units(weights):
    """-> (q as a list of Python integers, weightExponent): a weight that is not finite and positive counts 0; M = m * 2^e, 1 <= m < 2;
    q = floor(w * 2^(31 - e)) exactly"""
    w = [float(np.float32(x)) for x in weights]
    w = [x if math.isfinite(x) and x > 0.0 else 0.0 for x in w]
    top = max(w, default=0.0)
    if top == 0.0:
        return [0] * len(w), 0
    e = math.frexp(top)[1] - 1          # frexp: top = m * 2^x with 0.5 <= m < 1
    out = []
    for x in w:
        num, den = x.as_integer_ratio()
        shift = 31 - e
        out.append((num << shift) // den if shift >= 0 else num // (den << -shift))
    return out, e


def weight_units_numpy(weights):
    """the same in numpy for a million weights (float64 holds every step exactly: a float32 times a power of two, then the floor) -> (uint64 array, e)"""
    with np.errstate(invalid="ignore"):      # (signalling NaNs among the weights)
        w = np.asarray(weights, np.float32).astype(np.float64)
        w = np.where(np.isfinite(w) & (w > 0.0), w, 0.0)
    top = float(w.max()) if w.size else 0.0
    if top == 0.0:
        return np.zeros(w.shape, np.uint64), 0
    e = math.frexp(top)[1] - 1
    return np.floor(np.ldexp(w, 31 - e)).astype(np.uint64), e


def _selection(descs, index, size):
    descs = np.asarray(descs, np.int64).reshape(-1, 3)
    e = np.asarray(index).astype(np.int64)
    D = len(descs)
    valid = np.array([cu._valid(d, size) for d in descs], bool)
    selects = (e >= 0) & (e < D)
    selects[selects] = valid[e[selects]]
    special = (e < 0) & (e >= -4)
    return descs, e, selects, int(len(e) - selects.sum() - special.sum())


def restate_profile(array_data, descs, index, weights=None, array_data_size=None, unpacked=None):
    """What ommxProfileMicromapLevels answers, from host copies -> dict: known, opaque ((D, 13) uint32), refs ((D,) uint32), weights ((D,) uint64),
    shape ([(level, bits) or None]), info"""
    size = len(array_data) if array_data_size is None else array_data_size
    descs, e, selects, skipped = _selection(descs, index, size)
    D = len(descs)
    known, opaque = np.zeros((D, LEVELS), np.uint32), np.zeros((D, LEVELS), np.uint32)
    refs = np.bincount(e[selects], minlength=D).astype(np.uint32) if D else np.zeros(0, np.uint32)
    if weights is not None and len(e) > 100000:      # (test_fit.py holds the two statements of the weights together)
        q, exponent = weight_units_numpy(weights)
        sums = np.zeros(D, np.uint64)
        np.add.at(sums, e[selects], q[selects])      # (64-bit integer sums: indexCount * 2^32 < 2^64)
        sums = [int(x) for x in sums]
    else:
        q, exponent = weight_units(weights) if weights is not None else ([1] * len(e), 0)
        sums = [0] * D
        for i in np.nonzero(selects)[0].tolist():
            sums[int(e[i])] += q[i]
    shape = [None] * D
    for d in np.unique(e[selects]).tolist():
        o, l, f = (int(x) for x in descs[d])
        states = unpacked.get((o, l, f)) if unpacked is not None else None
        if states is None:
            states = cu.block_states(array_data, o, l, f)
            if unpacked is not None:
                unpacked[(o, l, f)] = states
        known[d], opaque[d] = known_counts(states, l)
        shape[d] = (l, f)
    assert all(s < 1 << 64 for s in sums)
    info = dict(referencedBlocks=int((refs > 0).sum()), skippedPrimitives=skipped, weightExponent=exponent, reserved=0)
    return dict(known=known, opaque=opaque, refs=refs, weights=np.array(sums, np.uint64), shape=shape, info=info)


# ---- the plan, in Python integers ----
def plan_size(shape, known, opaque, t, special):
    fields = 4 ** t
    if special and (t == 0 or (known[t] == fields and opaque[t] in (0, fields))):
        return 0
    return max(1, fields * shape[1] // 8)


def plan_value(weight, known, t):
    return int(weight) * int(known[t]) * 4 ** (12 - t)


def restate_plan(shape, known, opaque, weights, budget, max_level=12, special=True):
    """the rule of the header with a rescan of every candidate at every step -> dict: levels ([D], NO_LEVEL for unselected), unfitted, planned, steps,
    feasible, stepped (the descriptor of every step, in order), ties (steps whose ratio another candidate shared)"""
    D = len(shape)
    known, opaque = [[int(x) for x in row] for row in known], [[int(x) for x in row] for row in opaque]
    levels = [NO_LEVEL if shape[d] is None else min(shape[d][0], max_level) for d in range(D)]
    live = [d for d in range(D) if shape[d] is not None]
    size = lambda d, t: plan_size(shape[d], known[d], opaque[d], t, special)
    total = sum(size(d, levels[d]) for d in live)
    out = dict(unfitted=total, steps=0, stepped=[], ties=0)
    while total > budget:
        best = None
        tie = False
        for d in live:
            t = levels[d]
            if t == 0:
                continue
            ds = size(d, t) - size(d, t - 1)
            if ds <= 0:
                continue
            dv = plan_value(weights[d], known[d], t) - plan_value(weights[d], known[d], t - 1)
            assert dv >= 0 and dv * (1 << 22) < 1 << 114
            if best is None or dv * best[1] < best[0] * ds:
                best, tie = (dv, ds, d), False
            elif dv * best[1] == best[0] * ds:
                tie = True
        if best is None:
            break
        levels[best[2]] -= 1
        total -= best[1]
        out["steps"] += 1
        out["stepped"].append(best[2])
        out["ties"] += tie
    out.update(levels=levels, planned=total, feasible=total <= budget)
    return out


def known_share(profile, levels):
    """the weighted known share of a choice of levels, as an integer in units of 4^-12 of a block"""
    return sum(plan_value(profile["weights"][d], profile["known"][d], levels[d]) for d in range(len(levels)) if profile["shape"][d] is not None)


# ---- the coarsening with a cap per block ----
def restate_coarsen_levels(array_data, descs, index, index_format, block_levels, max_level=12, mixed=3, flags=0, array_data_size=None, unpacked=None):
    """What ommxCoarsenMicromapLevels answers (block_levels: [D] or None), as coarsen_util.restate_coarsen does for one cap"""
    size = len(array_data) if array_data_size is None else array_data_size
    descs, e, selects, skipped = _selection(descs, index, size)
    D = len(descs)
    special_in = (e < 0) & (e >= -4)
    out_e = np.where(special_in, e, -4)
    info = dict.fromkeys(cu.INFO_FIELDS, 0)
    info["skippedPrimitives"] = skipped
    blocks, entry, target_of = {}, {}, {}
    for d in np.unique(e[selects]).tolist():
        o, l, f = (int(x) for x in descs[d])
        t = min(l, min(max_level, 12), 12 if block_levels is None else int(block_levels[d]))
        states = unpacked.get((o, l, f)) if unpacked is not None else None
        if states is None:
            states = cu.block_states(array_data, o, l, f)
            if unpacked is not None:
                unpacked[(o, l, f)] = states
        out = cu.coarsen_states(states, l, t, f, mixed)
        info["referencedBlocks"] += 1
        info["coarsenedBlocks"] += l > t
        uniform = bool((out == out[0]).all())
        info["uniformBlocks"] += uniform
        target_of[d] = (t, f)
        if uniform and not flags & NO_SPECIAL:
            entry[d] = -(int(out[0]) + 1)
        else:
            blocks[d] = lu.pack(out, f)
    tail = ru.restate_tail(target_of, blocks, entry, flags, None)
    new_entry = np.zeros(D, np.int64)
    for d, v in tail["entry"].items():
        new_entry[d] = v
    out_e[selects] = new_entry[e[selects]]
    uses = np.bincount(e[selects], minlength=D) if D else np.zeros(0, np.int64)
    info["duplicateBlocks"], info["arrayDataSize"], info["descArrayCount"] = tail["duplicates"], len(tail["array"]), len(tail["emitted"])
    return dict(array=tail["array"], descs=tail["descs"], index=out_e.astype(su.INDEX_DTYPE[index_format]), array_hist=tail["array_hist"],
                index_hist=ru.index_histogram(target_of, blocks, uses), info=info)


def restate_fit(array_data, descs, index, index_format, budget, weights=None, max_level=12, mixed=3, flags=0, profile=None, unpacked=None):
    """What ommxFitMicromap answers -> (plan dict, result dict or None when infeasible)"""
    p = profile if profile is not None else restate_profile(array_data, descs, index, weights, unpacked=unpacked)
    plan = restate_plan(p["shape"], p["known"], p["opaque"], p["weights"], budget, max_level, not flags & NO_SPECIAL)
    if not plan["feasible"]:
        return plan, None
    return plan, restate_coarsen_levels(array_data, descs, index, index_format, plan["levels"], 12, mixed, flags, unpacked=unpacked)


# ---- the designed input: blocks that lose nothing for several levels beside blocks that lose everything at the first step ----
def designed_blocks(level=4, bits=2, pairs=4):
    """`pairs` blocks of four uniform quadrants (T, O, T, O: known at every level >= 1, a block down to level 1) and `pairs` blocks of alternating T / O
    (known only at their own level).  Every coarser level of a quadrant block keeps its whole known share; the first step of an alternating block loses all
    of it.  A global cap treats both alike."""
    n = 4 ** level
    quad = np.repeat(np.array([0, 1, 0, 1], np.uint8), n // 4)
    alt = (np.arange(n) % 2).astype(np.uint8)
    return [(quad.copy(), level, bits) for _ in range(pairs)] + [(alt.copy(), level, bits) for _ in range(pairs)]


def best_global_cap(profile, budget, special=True):
    """the finest global cap whose planned size fits the budget -> (cap, levels) or None"""
    shape = profile["shape"]
    for cap in range(12, -1, -1):
        levels = [NO_LEVEL if s is None else min(s[0], cap) for s in shape]
        total = sum(plan_size(shape[d], profile["known"][d], profile["opaque"][d], levels[d], special) for d in range(len(shape)) if shape[d] is not None)
        if total <= budget:
            return cap, levels
    return None


# ---- calls on the device ----
class ProfileBuffers:
    def __init__(self, hip, D, poison=0xCD):
        self.hip, self.D = hip, D
        fill = lambda n: hip.upload(np.full(max(n, 16), poison, np.uint8))
        self.bufs = [fill(4 * LEVELS * D), fill(4 * LEVELS * D), fill(4 * D), fill(8 * D)]
        self.out = LevelProfileOutputs(*[b.value for b in self.bufs])

    def download(self):
        D, h = self.D, self.hip
        return dict(known=h.download(self.bufs[0], 4 * LEVELS * D, np.uint32).reshape(D, LEVELS), opaque=h.download(self.bufs[1], 4 * LEVELS * D, np.uint32).reshape(D, LEVELS),
                    refs=h.download(self.bufs[2], 4 * D, np.uint32), weights=h.download(self.bufs[3], 8 * D, np.uint64))

    def close(self):
        for b in self.bufs:
            self.hip.free(b)
        self.bufs = []


def profile(dll, hip, baker, rd, weights=None, stream=None):
    """-> (result code, arrays dict, info dict); weights: a device pointer or None"""
    bufs = ProfileBuffers(hip, rd.descArrayCount)
    try:
        info = LevelProfileInfo()
        info.reserved = 7
        r = dll.ommxProfileMicromapLevels(baker, C.byref(rd), weights, C.byref(bufs.out), C.byref(info), stream)
        return r, bufs.download(), {f: int(getattr(info, f)) for f in PROFILE_INFO_FIELDS}
    finally:
        bufs.close()


def assert_profile(got, ref):
    for k in ("known", "opaque", "refs", "weights"):
        bad = np.argwhere(got[k] != ref[k])
        assert bad.size == 0, "%s: %d entries differ, first at %s: %s, want %s" % (k, len(bad), bad[0], got[k][tuple(bad[0])], ref[k][tuple(bad[0])])


def coarsen_levels(dll, hip, baker, rd, block_levels, max_level=12, mixed=3, flags=0, want_result=True, stream=None):
    """block_levels: a host sequence (uploaded here), a device pointer, or None -> (result code, info dict, handle or None)"""
    own = None
    if block_levels is not None and not isinstance(block_levels, C.c_void_p):
        own = hip.upload(np.asarray(block_levels, np.uint8))
    try:
        out, info = C.c_void_p(), cu.CoarsenInfo()
        r = dll.ommxCoarsenMicromapLevels(baker, C.byref(rd), own if own is not None else block_levels, C.byref(cu.c_desc(max_level, mixed, flags)),
                                          C.byref(out) if want_result else None, C.byref(info), stream)
        return r, cu.info_dict(info), (out if want_result and r == ot.SUCCESS else None)
    finally:
        if own is not None:
            hip.free(own)


def fit(dll, hip, baker, rd, budget, weights=None, max_level=12, mixed=3, flags=0, want_result=True, want_levels=True, stream=None):
    """-> (result code, info dict, levels (uint8 array) or None, handle or None)"""
    D = rd.descArrayCount
    lv = hip.upload(np.full(max(D, 16), 0xEE, np.uint8)) if want_levels else None
    try:
        out, info = C.c_void_p(), FitInfo()
        r = dll.ommxFitMicromap(baker, C.byref(rd), C.byref(f_desc(budget, weights, max_level, mixed, flags)), lv, C.byref(out) if want_result else None, C.byref(info), stream)
        levels = hip.download(lv, D) if want_levels else None
        return r, fit_info_dict(info), levels, (out if want_result and r == ot.SUCCESS else None)
    finally:
        if lv is not None:
            hip.free(lv)
