"""Shared by tests/test_compare.py, tests/test_compare_gpu.py and tests/scripts/compare_throughput.py: ctypes bindings of ommxCompareMicromaps, two
statements of the definition in include/omm_mi355x_ext.h that owe nothing to the kernels -- restate_compare (numpy: unpack with
coarsen_util.block_states, np.repeat down to the pair's level, bincount of 4 * sa + sb) and brute_compare (Python loops over single fields read bit by
bit, levels <= 4) -- and the call on device copies of hand-built sources."""
import ctypes as C
import numpy as np
import ommtest as ot
import coarsen_util as cu
import combine_util as mu

CONFLICT, A_WEAKER, B_WEAKER, HINT, SKIPPED = 0x01, 0x02, 0x04, 0x08, 0x80
FORCE_2STATE = 1
NO_CONFLICT = 0xFFFFFFFF
UNIT = 4 ** 12          # the totals are in units of 4^-12 of a primitive
COUNT_FIELDS = ("identicalPrimitives", "conflictPrimitives", "aWeakerPrimitives", "bWeakerPrimitives", "hintPrimitives", "skippedPrimitives",
                "comparedPairs", "refinedPairs", "firstConflictPrimitive", "reserved")


class CompareDesc(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32)]


class CompareOutputs(C.Structure):
    _fields_ = [("relations", C.c_void_p), ("levels", C.c_void_p), ("confusion", C.c_void_p)]


class CompareInfo(C.Structure):
    _fields_ = [("totals", (C.c_uint64 * 4) * 4)] + [(f, C.c_uint32) for f in COUNT_FIELDS]


def bind(dll):
    mu.bind(dll)
    dll.ommxCompareMicromaps.argtypes = [C.c_void_p, C.POINTER(ot.BakeResultDesc), C.POINTER(ot.BakeResultDesc), C.POINTER(CompareDesc),
                                         C.POINTER(CompareOutputs), C.POINTER(CompareInfo), C.c_void_p]
    return dll


def c_desc(flags=0, reserved=0):
    d = CompareDesc()
    d.flags, d.reserved = flags, reserved
    return d


def info_dict(info):
    d = {f: int(getattr(info, f)) for f in COUNT_FIELDS}
    d["totals"] = [[int(info.totals[sa][sb]) for sb in range(4)] for sa in range(4)]
    return d


# ---- the definition, twice ----
def cell_relation(sa, sb):
    if sa == sb:
        return 0
    if sa < 2:
        return CONFLICT if sb < 2 else B_WEAKER
    return A_WEAKER if sb < 2 else HINT


def relation_of(matrix):
    r = 0
    for sa in range(4):
        for sb in range(4):
            if matrix[sa][sb]:
                r |= cell_relation(sa, sb)
    return r


def info_of(relations, levels, confusion, pairs, refined):
    """the info from the per-primitive answers: Python integers, no float anywhere"""
    kept = [i for i, r in enumerate(relations) if r != SKIPPED]
    totals = [[0] * 4 for _ in range(4)]
    for i in kept:
        w = 4 ** (12 - int(levels[i]))
        for sa in range(4):
            for sb in range(4):
                totals[sa][sb] += int(confusion[i][sa][sb]) * w
    count = lambda bit: sum(1 for i in kept if relations[i] & bit)
    conflicts = [i for i in kept if relations[i] & CONFLICT]
    return dict(totals=totals, identicalPrimitives=sum(1 for i in kept if relations[i] == 0), conflictPrimitives=count(CONFLICT),
                aWeakerPrimitives=count(A_WEAKER), bWeakerPrimitives=count(B_WEAKER), hintPrimitives=count(HINT),
                skippedPrimitives=len(relations) - len(kept), comparedPairs=pairs, refinedPairs=refined,
                firstConflictPrimitive=conflicts[0] if conflicts else NO_CONFLICT, reserved=0)


def _kinds(source):
    """per primitive of (array, descs (D, 3), index, size or None): the entry, whether it selects a block, whether it fails the rule"""
    a, d, index, size = source
    d = np.asarray(d, np.int64).reshape(-1, 3)
    e = np.asarray(index).astype(np.int64)
    valid = mu._valid_rows(d, len(a) if size is None else size) if len(d) else np.zeros(0, bool)
    inside = (e >= 0) & (e < len(d))
    block = inside.copy()
    block[inside] = valid[e[inside]]
    return e, d, block, (e < -4) | ((e >= 0) & ~block)


def restate_compare(src_a, src_b, force2=False, unpacked=None):
    """What ommxCompareMicromaps answers.  src: (array_data uint8, descs (D, 3) rows of (offset, level, format), index, arrayDataSize or None) ->
    dict: relations (uint8), levels (uint8), confusion ((N, 4, 4) uint32), info ({field: int, totals: 4 x 4 ints}).  unpacked: a dict that keeps the
    unpacked states of source blocks between calls on the same sources"""
    ea, da, block_a, bad_a = _kinds(src_a)
    eb, db, block_b, bad_b = _kinds(src_b)
    N = len(ea)
    assert len(eb) == N
    relations, levels = np.full(N, SKIPPED, np.uint8), np.full(N, 0xFF, np.uint8)
    confusion = np.zeros((N, 4, 4), np.uint32)
    answers, pairs, refined = {}, 0, 0

    def side(src, d, e, is_block):
        if not is_block:
            return np.array([-(e + 1)], np.uint8), 0
        o, l, f = (int(x) for x in d[e])
        key = (id(src[0]), o, l, f)
        states = unpacked.get(key) if unpacked is not None else None
        if states is None:
            states = cu.block_states(src[0], o, l, f)
            if unpacked is not None:
                unpacked[key] = states
        return states, l

    for i in np.nonzero(~(bad_a | bad_b))[0].tolist():
        key = (int(ea[i]), int(eb[i]))
        if key not in answers:
            sa, la = side(src_a, da, key[0], block_a[i])
            sb, lb = side(src_b, db, key[1], block_b[i])
            T = max(la, lb)
            sa, sb = np.repeat(sa.astype(np.uint8), 4 ** (T - la)), np.repeat(sb.astype(np.uint8), 4 ** (T - lb))
            if force2:
                sa, sb = sa & 1, sb & 1
            m = np.bincount(4 * sa + sb, minlength=16).reshape(4, 4)                          # (uint8 throughout: 4 * sa + sb <= 15)
            assert int(m.sum()) == 4 ** T
            answers[key] = (relation_of(m), T, m.astype(np.uint32))
            if block_a[i] or block_b[i]:
                pairs += 1
                refined += (la != lb) or not (block_a[i] and block_b[i])
        relations[i], levels[i], confusion[i] = answers[key]
    return dict(relations=relations, levels=levels, confusion=confusion, info=info_of(relations, levels, confusion, pairs, refined))


def _field(array_data, offset, bits, j):
    """field j of the block at `offset`, bit by bit"""
    at = j * bits
    v = 0
    for k in range(bits):
        v |= ((int(array_data[offset + ((at + k) >> 3)]) >> ((at + k) & 7)) & 1) << k
    return v


def brute_compare(src_a, src_b, force2=False):
    """The same answer by Python loops over single fields (levels <= 4); every entry is judged by the sentences of the header -> (relations, levels,
    confusion as nested lists, info)"""
    def judge(src, e):
        a, d, _, size = src
        size = len(a) if size is None else size
        if e < 0:
            return ("special", -(e + 1)) if e >= -4 else None
        if e >= len(d):
            return None
        o, l, f = (int(x) for x in d[e])
        if l > 12 or f not in (1, 2):
            return None
        if o + max(1, (4 ** l * f) // 8) > size:
            return None
        return ("block", o, l, f)

    def state(src, what, j, T):
        if what[0] == "special":
            return what[1]
        _, o, l, f = what
        return _field(src[0], o, f, j >> (2 * (T - l)))

    N = len(src_a[2])
    relations, levels, confusion, seen, refined = [], [], [], set(), 0
    for i in range(N):
        wa, wb = judge(src_a, int(src_a[2][i])), judge(src_b, int(src_b[2][i]))
        if wa is None or wb is None:
            relations.append(SKIPPED)
            levels.append(0xFF)
            confusion.append([[0] * 4 for _ in range(4)])
            continue
        T = max(wa[2] if wa[0] == "block" else 0, wb[2] if wb[0] == "block" else 0)
        assert T <= 4
        m = [[0] * 4 for _ in range(4)]
        for j in range(4 ** T):
            sa, sb = state(src_a, wa, j, T), state(src_b, wb, j, T)
            if force2:
                sa, sb = sa & 1, sb & 1
            m[sa][sb] += 1
        relations.append(relation_of(m))
        levels.append(T)
        confusion.append(m)
        key = (int(src_a[2][i]), int(src_b[2][i]))
        if (wa[0] == "block" or wb[0] == "block") and key not in seen:
            seen.add(key)
            refined += not (wa[0] == wb[0] == "block" and wa[2] == wb[2])
    return relations, levels, confusion, info_of(relations, levels, confusion, len(seen), refined)


# ---- a call on the device ----
class Outputs:
    """device arrays for the three outputs, pre-filled with 0xEE; `want` chooses the members that are handed in"""

    def __init__(self, hip, count, want=("relations", "levels", "confusion")):
        self.hip, self.count, self.want = hip, count, want
        self.bufs = {"relations": hip.upload(np.full(max(count, 1), 0xEE, np.uint8)), "levels": hip.upload(np.full(max(count, 1), 0xEE, np.uint8)),
                     "confusion": hip.upload(np.full(max(count, 1) * 64, 0xEE, np.uint8))}
        self.c = CompareOutputs(*[self.bufs[k].value if k in want else None for k in ("relations", "levels", "confusion")])

    def download(self):
        n = self.count
        return dict(relations=self.hip.download(self.bufs["relations"], n), levels=self.hip.download(self.bufs["levels"], n),
                    confusion=self.hip.download(self.bufs["confusion"], 64 * n).view(np.uint32).reshape(n, 4, 4))

    def close(self):
        for p in self.bufs.values():
            self.hip.free(p)


def compare(dll, baker, rd_a, rd_b, flags=0, outputs=None, want_info=True, stream=None):
    """-> (result code, info dict or None)"""
    info = CompareInfo()
    r = dll.ommxCompareMicromaps(baker, C.byref(rd_a), C.byref(rd_b), C.byref(c_desc(flags)), C.byref(outputs.c) if outputs else None,
                                 C.byref(info) if want_info else None, stream)
    return r, (info_dict(info) if want_info and r == ot.SUCCESS else None)


def assert_outputs(got, ref, want=("relations", "levels", "confusion")):
    """byte for byte; a member that was not handed in still holds its 0xEE"""
    for k in ("relations", "levels", "confusion"):
        if k in want:
            bad = np.nonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(axis=1))[0]
            assert bad.size == 0, "%s: %d primitives differ, first %d: %s != %s" % (k, bad.size, bad[0], got[k][bad[0]].tolist(), ref[k][bad[0]].tolist())
        else:
            assert (got[k].view(np.uint8) == 0xEE).all(), k


def host_pair(sa, sb):
    return tuple(mu.host_sources([sa, sb]))


def compare_and_check(dll, hip, baker, sa, sb, force2=False, stream=None, unpacked=None):
    """the whole contract on one input: the info-only call, the outputs-only call and the full call against the model; one output alone; the sources
    are untouched -> the model's answer"""
    ha, hb = host_pair(sa, sb)
    ref = restate_compare(ha, hb, force2, unpacked)
    flags = FORCE_2STATE if force2 else 0
    n = len(ref["relations"])
    r, info = compare(dll, baker, sa.rd, sb.rd, flags, stream=stream)
    assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
    for want, want_info in ((("relations", "levels", "confusion"), False), (("relations", "levels", "confusion"), True), (("confusion",), True), (("relations",), False)):
        out = Outputs(hip, n, want)
        try:
            r, info = compare(dll, baker, sa.rd, sb.rd, flags, out, want_info, stream)
            assert r == ot.SUCCESS and (info == ref["info"] if want_info else info is None), (r, info, ref["info"])
            assert_outputs(out.download(), ref, want)
        finally:
            out.close()
    assert sa.unchanged() and sb.unchanged()
    return ref
