"""Shared by tests/test_geometry.py, tests/test_geometry_gpu.py and tests/scripts/geometry_throughput.py: ctypes bindings of ommxExtractMicroGeometry /
ommxExpandMicroNodes, two statements of the cut's definition in include/omm_mi355x_ext.h that owe nothing to the kernels -- restate_cut (numpy, level by
level from the bottom) and brute_cut (a recursive walk over Python lists, levels <= 4) -- the block patterns of the tier edges, a numpy restatement of
the expansion, and the arena that holds every array of a call in one device allocation."""
import collections
import ctypes as C
import numpy as np
import ommtest as ot
import lookup_util as lu
import stats_util as su

DROP = 0xFF
NODE = np.dtype([("prim", "<u4"), ("node", "<u4")])
NAN_BITS = 0x7FC00000
INSUFFICIENT = 3   # ommResult_INSUFFICIENT_SCRATCH_MEMORY

GDesc = collections.namedtuple("GDesc", "list_of_state mixed max_emit")
PRESET = GDesc((DROP, 0, 1, 1), 1, 0xFFFFFFFF)            # opaque -> list 0, alpha-tested -> list 1, transparent gone
PRESET_WHOLE = GDesc((DROP, 0, 1, 1), 1, 0)               # the same partition on whole primitives
IDENTITY = GDesc((0, 1, 2, 3), 0, 0xFFFFFFFF)


class MicroGeometryDesc(C.Structure):
    _fields_ = [("listOfState", C.c_uint8 * 4), ("mixedList", C.c_uint8), ("reserved", C.c_uint8 * 3), ("maxEmitLevel", C.c_uint32)]


class MicroGeometryOutputs(C.Structure):
    _fields_ = [("nodes", C.c_void_p * 4), ("capacity", C.c_uint64 * 4), ("primitiveOffsets", C.c_void_p * 4)]


class MicroMeshDesc(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("positionStrideInBytes", C.c_uint32), ("indexBuffer", C.c_void_p), ("indexFormat", C.c_int),
                ("triangleCount", C.c_uint32)]


def bind(dll):
    su.bind(dll)
    dll.ommxExtractMicroGeometry.argtypes = [C.c_void_p, C.POINTER(ot.BakeResultDesc), C.POINTER(MicroGeometryDesc), C.POINTER(MicroGeometryOutputs),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_void_p]
    dll.ommxExpandMicroNodes.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(MicroMeshDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    return dll


def c_desc(g, reserved=(0, 0, 0)):
    d = MicroGeometryDesc()
    d.listOfState[:] = list(g.list_of_state)
    d.mixedList, d.maxEmitLevel = g.mixed, g.max_emit
    d.reserved[:] = list(reserved)
    return d


# ---- the definition, twice ----
def _cls(v):
    return 4 if v == DROP else v


def block_cut(states, level, g):
    """the records of ONE block (states: its 4^level micro-triangle states) per list, in order -> four uint32 arrays of node words.  Built from the text
    of the header: classes at level E, classes above by 'all four children agree', emission where the parent has no class."""
    states = np.asarray(states, np.uint8)
    assert len(states) == 4 ** level
    E = min(level, g.max_emit, 12)
    c = np.array([_cls(v) for v in g.list_of_state], np.int8)[states].reshape(4 ** E, -1)
    cls = {E: np.where((c == c[:, :1]).all(axis=1), c[:, 0], _cls(g.mixed)).astype(np.int8)}
    for l in range(E - 1, -1, -1):
        ch = cls[l + 1].reshape(-1, 4)
        cls[l] = np.where((ch == ch[:, :1]).all(axis=1) & (ch[:, 0] >= 0), ch[:, 0], -1).astype(np.int8)
    first, node, lst = [], [], []
    for l in range(E + 1):
        has = cls[l] >= 0
        if l:
            has &= np.repeat(cls[l - 1], 4) < 0
        j = np.nonzero(has)[0].astype(np.int64)
        first.append(j << (2 * (level - l)))
        node.append((l << 24) | j)
        lst.append(cls[l][j])
    first, node, lst = np.concatenate(first), np.concatenate(node).astype(np.uint32), np.concatenate(lst)
    order = np.argsort(first, kind="stable")
    node, lst = node[order], lst[order]
    return [node[lst == k] for k in range(4)]


def brute_cut(states, level, g):
    """the same records by a plain recursive walk (levels <= 4): -> four Python lists of node words"""
    states = [int(s) for s in states]
    assert level <= 4 and len(states) == 4 ** level
    E = min(level, g.max_emit)
    out = [[], [], [], []]

    def class_of(l, j):
        if l == E:
            span = 4 ** (level - E)
            seen = {_cls(g.list_of_state[s]) for s in states[j * span:(j + 1) * span]}
            return seen.pop() if len(seen) == 1 else _cls(g.mixed)
        kids = [class_of(l + 1, 4 * j + q) for q in range(4)]
        return kids[0] if kids[0] is not None and kids.count(kids[0]) == 4 else None

    def walk(l, j):
        c = class_of(l, j)
        if c is not None:          # the parent had none (or this is the root): emitted; every descendant has a parent with a class
            if c < 4:
                out[c].append((l << 24) | j)
        else:
            for q in range(4):
                walk(l + 1, 4 * j + q)
    walk(0, 0)
    return out


def block_states(array_data, offset, level, bits):
    n = 4 ** level
    b = np.unpackbits(np.asarray(array_data[offset:offset + su.block_bytes(level, bits)], np.uint8), bitorder="little")[:n * bits]
    return b if bits == 1 else b[0::2] + 2 * b[1::2]


def restate_cut(array_data, descs, index, g, array_data_size=None):
    """What ommxExtractMicroGeometry answers, from host copies (arguments as stats_util.reference_stats) -> dict: nodes (four NODE arrays), offsets (four
    uint64 arrays of T + 1), counts (four ints), skipped"""
    size = len(array_data) if array_data_size is None else array_data_size
    descs = np.asarray(descs, np.int64).reshape(-1, 3)
    e = np.asarray(index).astype(np.int64)
    D, T = len(descs), len(e)
    cnt = np.zeros((4, T), np.uint64)
    for s in range(4):
        if g.list_of_state[s] != DROP:
            cnt[g.list_of_state[s], e == -1 - s] = 1
    blocks = {}
    for d in np.unique(e[(e >= 0) & (e < D)]):
        o, l, f = (int(x) for x in descs[d])
        if l <= 12 and f in (1, 2) and o + su.block_bytes(l, f) <= size:
            blocks[int(d)] = (np.nonzero(e == d)[0], block_cut(block_states(array_data, o, l, f), l, g))
            for k in range(4):
                cnt[k, blocks[int(d)][0]] = len(blocks[int(d)][1][k])
    answered = sum(len(p) for p, _ in blocks.values()) + int(((e < 0) & (e >= -4)).sum())
    offsets = [np.concatenate([[0], np.cumsum(cnt[k])]).astype(np.uint64) for k in range(4)]
    nodes = []
    for k in range(4):
        rec = np.zeros(int(offsets[k][-1]), NODE)
        sp = np.nonzero((e < 0) & (e >= -4) & (cnt[k] == 1))[0]
        rec["prim"][offsets[k][sp].astype(np.int64)] = sp
        for prims, cut in blocks.values():
            n = len(cut[k])
            if n:
                at = (offsets[k][prims].astype(np.int64)[:, None] + np.arange(n)[None, :]).reshape(-1)
                rec["prim"][at], rec["node"][at] = np.repeat(prims, n), np.tile(cut[k], len(prims))
        nodes.append(rec)
    return dict(nodes=nodes, offsets=offsets, counts=[int(o[-1]) for o in offsets], skipped=T - answered)


def covering(level, cut):
    """how often each micro-triangle of a block of `level` is covered by the nodes of `cut` (four arrays of node words) -> int array of 4^level"""
    cover = np.zeros(4 ** level + 1, np.int64)
    for nodes in cut:
        nodes = np.asarray(nodes, np.int64)
        l, j = nodes >> 24, nodes & 0xFFFFFF
        span = 4 ** (level - l)
        np.add.at(cover, j * span, 1)
        np.add.at(cover, (j + 1) * span, -1)
    return np.cumsum(cover)[:-1]


# ---- block patterns of the tier edges ----
def pattern(name, level, bits, seed=1):
    """the 4^level states of a named pattern (2-state blocks use states 0 / 1 only)"""
    n = 4 ** level
    top = 2 if bits == 1 else 4
    i = np.arange(n, dtype=np.int64)
    kind, _, arg = name.partition(":")
    if kind == "uniform":
        return np.full(n, int(arg) % top, np.uint8)
    if kind == "except":        # uniform 1 except one micro-triangle (arg: its index, negative from the end)
        s = np.ones(n, np.uint8)
        s[int(arg) % n if int(arg) < 0 else min(int(arg), n - 1)] = 0
        return s
    if kind == "alternate":     # states change every `arg` micro-triangles
        return ((i // int(arg)) % top).astype(np.uint8)
    if kind == "random":        # arg: minority share in percent
        rng = np.random.default_rng(seed + 17 * level + bits)
        s = np.ones(n, np.uint8)
        minority = rng.random(n) < int(arg) / 100.0
        s[minority] = rng.integers(0, top, int(minority.sum())).astype(np.uint8)
        return s
    if kind == "quarters":
        return ((i * 4 // n) % top).astype(np.uint8) if n >= 4 else np.zeros(n, np.uint8)
    raise ValueError(name)


ALL_PATTERNS = ["uniform:0", "uniform:1", "uniform:2", "uniform:3", "except:0", "except:63", "except:64", "except:4095", "except:4096", "except:-1",
                "alternate:1", "alternate:4", "alternate:64", "alternate:4096", "random:1", "random:50", "quarters"]
# the largest blocks: everything but the patterns whose record count is of the order of the micro-triangle count
BIG_PATTERNS = ["uniform:1", "uniform:3", "except:0", "except:4095", "except:4096", "except:-1", "alternate:64", "alternate:4096", "random:1", "quarters"]


def table_of_blocks(blocks, first_offset=0, gap=0):
    """blocks: [(states, level, bits)] -> (array_data, descs (D, 3)), each block `gap` bytes behind the last"""
    parts, descs, at = [np.zeros(first_offset, np.uint8)], [], first_offset
    for states, level, bits in blocks:
        b = lu.pack(states, bits)
        descs.append((at, level, bits))
        parts += [b, np.full(gap, 0xA5, np.uint8)]
        at += len(b) + gap
    return np.concatenate(parts), np.array(descs, np.int64).reshape(-1, 3)


# ---- the arena ----
class Image:
    """One device allocation that holds every array of a call, inputs and outputs, each at the alignment its C type asks for and no more, the gaps and
    the outputs pre-filled with random bytes.  After the call every byte outside the outputs must be what it was."""

    def __init__(self, hip, seed=3):
        self.hip, self.parts, self.size, self.rng = hip, {}, 0, np.random.default_rng(seed)

    def add(self, name, nbytes, align, data=None, output=False):
        """place `nbytes` at an address that is `align` modulo 2 * align (aligned for the type, not for anything wider), behind a gap"""
        at = self.size + 24
        at += (align - at) % (2 * align)
        self.parts[name] = (at, nbytes, data, output)
        self.size = at + nbytes

    def upload(self):
        self.size += 40
        self.before = self.rng.integers(0, 256, self.size, dtype=np.uint8)
        for at, n, data, _ in self.parts.values():
            if data is not None:
                self.before[at:at + n] = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.base = self.hip.upload(self.before)
        assert self.base.value % 256 == 0
        return self

    def ptr(self, name):
        return C.c_void_p(self.base.value + self.parts[name][0])

    def download(self):
        self.after = self.hip.download(self.base, self.size)
        return self

    def out(self, name, dtype):
        at, n, _, _ = self.parts[name]
        return self.after[at:at + n].copy().view(dtype)

    def assert_only_outputs_changed(self, written=None):
        keep = np.ones(self.size, bool)
        for name, (at, n, _, output) in self.parts.items():
            if output and (written is None or name in written):
                keep[at:at + n] = False
        bad = np.nonzero((self.before != self.after) & keep)[0]
        assert bad.size == 0, "bytes outside the outputs changed, first at %d of %d" % (bad[0], self.size)

    def free(self):
        self.hip.free(self.base)


def raw_descs(descs):
    descs = np.asarray(descs, np.int64).reshape(-1, 3)
    raw = np.zeros(len(descs), dtype=[("o", "<u4"), ("l", "<u2"), ("f", "<u2")])
    raw["o"], raw["l"], raw["f"] = descs[:, 0], descs[:, 1], descs[:, 2]
    return raw


class Call:
    """the arrays of one ommxExtractMicroGeometry call in an Image: array data at an odd address, descs, index, and per list a record array of
    `capacity[k]` (None: the list's pointer stays NULL) and an offsets array (where `offsets[k]`)"""

    def __init__(self, hip, array_data, descs, index, index_format, capacity, offsets=(True,) * 4, declared=None, array_align=1):
        """declared: (arrayDataSize, descArrayCount, indexCount) where the desc declares less than the arrays hold (what follows is padding)"""
        idx = np.asarray(index).astype(su.INDEX_DTYPE[index_format])
        raw = raw_descs(descs)
        size, D, self.T = declared if declared else (len(array_data), len(raw), len(idx))
        self.capacity, self.offsets = list(capacity), list(offsets)
        im = Image(hip)
        im.add("array", len(array_data), array_align, array_data)
        im.add("descs", max(8 * len(raw), 8), 4, raw if len(raw) else None)
        im.add("index", idx.nbytes, idx.itemsize, idx)
        for k in range(4):
            if capacity[k] is not None:
                im.add("nodes%d" % k, 8 * capacity[k], 4, output=True)
            if offsets[k]:
                im.add("offsets%d" % k, 8 * (self.T + 1), 8, output=True)
        self.im = im.upload()
        rd = ot.BakeResultDesc()
        rd.arrayData, rd.arrayDataSize = im.ptr("array"), size
        rd.descArray, rd.descArrayCount = C.cast(im.ptr("descs"), C.POINTER(ot.MicromapDesc)), D
        rd.indexBuffer, rd.indexCount, rd.indexFormat = im.ptr("index"), self.T, index_format
        self.rd = rd
        o = MicroGeometryOutputs()
        for k in range(4):
            o.nodes[k] = im.ptr("nodes%d" % k).value if capacity[k] is not None else None
            o.capacity[k] = capacity[k] if capacity[k] is not None else 0
            o.primitiveOffsets[k] = im.ptr("offsets%d" % k).value if offsets[k] else None
        self.o = o

    def run(self, dll, baker, g, stream=None, count_only=False):
        counts, skipped = (C.c_uint64 * 4)(7, 7, 7, 7), C.c_uint32(12345)
        r = dll.ommxExtractMicroGeometry(baker, C.byref(self.rd), C.byref(c_desc(g)), None if count_only else C.byref(self.o), counts, C.byref(skipped), stream)
        self.im.download()
        return r, list(counts), skipped.value

    def check(self, ref, written=True):
        """every output against restate_cut's answer, byte for byte; written = False: the call must not have written any output byte"""
        if not written:
            self.im.assert_only_outputs_changed(written=())
            return
        for k in range(4):
            if self.capacity[k] is not None:
                got = self.im.out("nodes%d" % k, NODE)
                n = ref["counts"][k]
                assert np.array_equal(got[:n], ref["nodes"][k]), "list %d: first difference at record %d of %d" % (
                    k, int(np.nonzero(got[:n] != ref["nodes"][k])[0][0]), n)
                at = self.im.parts["nodes%d" % k][0]     # the records behind the list's count stay untouched
                assert np.array_equal(self.im.after[at + 8 * n:at + 8 * self.capacity[k]], self.im.before[at + 8 * n:at + 8 * self.capacity[k]])
            if self.offsets[k]:
                assert np.array_equal(self.im.out("offsets%d" % k, np.uint64), ref["offsets"][k]), "offsets of list %d" % k
        self.im.assert_only_outputs_changed()

    def free(self):
        self.im.free()


def restate_declared(array_data, descs, index, g, declared=None):
    if not declared:
        return restate_cut(array_data, descs, index, g)
    size, D, T = declared
    return restate_cut(array_data, np.asarray(descs, np.int64).reshape(-1, 3)[:D], np.asarray(index)[:T], g, size)


def extract_and_check(dll, hip, baker, array_data, descs, index, index_format, g, slack=3, declared=None, array_align=1, stream=None):
    """the whole contract on one input: count-only, then the full call into arrays of capacity count + slack; everything equals restate_cut"""
    ref = restate_declared(array_data, descs, index, g, declared)
    call = Call(hip, array_data, descs, index, index_format, [c + slack for c in ref["counts"]], declared=declared, array_align=array_align)
    try:
        r, counts, skipped = call.run(dll, baker, g, stream, count_only=True)
        assert (r, counts, skipped) == (ot.SUCCESS, ref["counts"], ref["skipped"]), (r, counts, skipped, ref["counts"], ref["skipped"])
        call.check(ref, written=False)
        r, counts, skipped = call.run(dll, baker, g, stream)
        assert (r, counts, skipped) == (ot.SUCCESS, ref["counts"], ref["skipped"]), (r, counts, skipped, ref["counts"], ref["skipped"])
        call.check(ref)
    finally:
        call.free()
    return ref


def pattern_table(level, bits, names, first_offset=0, gap=0):
    """one block per named pattern, every block selected once, the four specials, and the first block again -> (array_data, descs, index)"""
    array_data, descs = table_of_blocks([(pattern(n, level, bits), level, bits) for n in names], first_offset, gap)
    return array_data, descs, list(range(len(names))) + [-1, -2, -3, -4, 0]


def extract_device(dll, hip, baker, rdesc, g, ref, stream=None):
    """ommxExtractMicroGeometry on a result that already lives on the device: count, allocate (records and offsets between canaries), extract; every
    output equals `ref` (restate_cut of the downloaded arrays) -> the bytes of the four record arrays"""
    counts, skipped = (C.c_uint64 * 4)(), C.c_uint32(99)
    gd = c_desc(g)
    assert dll.ommxExtractMicroGeometry(baker, C.byref(rdesc), C.byref(gd), None, counts, C.byref(skipped), stream) == ot.SUCCESS
    assert list(counts) == ref["counts"] and skipped.value == ref["skipped"], (list(counts), ref["counts"], skipped.value, ref["skipped"])
    T, canary = rdesc.indexCount, 64
    o, bufs = MicroGeometryOutputs(), []
    for k in range(4):
        for nbytes, field in ((8 * counts[k], o.nodes), (8 * (T + 1), o.primitiveOffsets)):
            p = hip.upload(np.full(nbytes + 2 * canary, 0xAB, np.uint8))
            bufs.append((p, nbytes))
            field[k] = p.value + canary
        o.capacity[k] = counts[k]
    try:
        assert dll.ommxExtractMicroGeometry(baker, C.byref(rdesc), C.byref(gd), C.byref(o), counts, None, stream) == ot.SUCCESS
        got = []
        for i, (p, nbytes) in enumerate(bufs):
            raw = hip.download(p, nbytes + 2 * canary)
            assert (raw[:canary] == 0xAB).all() and (raw[canary + nbytes:] == 0xAB).all(), "bytes outside an output were written"
            got.append(raw[canary:canary + nbytes].copy())
        for k in range(4):
            assert np.array_equal(got[2 * k].view(NODE), ref["nodes"][k]), "list %d" % k
            assert np.array_equal(got[2 * k + 1].view(np.uint64), ref["offsets"][k]), "offsets of list %d" % k
        return [got[2 * k] for k in range(4)]
    finally:
        for p, _ in bufs:
            hip.free(p)


def list_of_hits(nodes_by_list, prim_levels, prims, micro):
    """the list of the one node that contains micro-triangle `micro` (at its primitive's level) of primitive `prims`, DROP where no emitted node does.
    prim_levels: the level of every primitive's block (0 for a special index).  Nodes of one primitive are disjoint, so the node is the last one
    that starts at or before the micro-triangle, if it reaches that far."""
    keys, lists, ends = [], [], []
    for k, rec in enumerate(nodes_by_list):
        p, node = rec["prim"].astype(np.int64), rec["node"].astype(np.int64)
        l, j, L = node >> 24, node & 0xFFFFFF, np.asarray(prim_levels, np.int64)[p]
        first = j << (2 * (L - l))
        keys.append((p << 24) + first)
        ends.append((p << 24) + first + (1 << (2 * (L - l))))
        lists.append(np.full(len(rec), k, np.int64))
    keys, ends, lists = np.concatenate(keys), np.concatenate(ends), np.concatenate(lists)
    order = np.argsort(keys, kind="stable")
    keys, ends, lists = keys[order], ends[order], lists[order]
    want = (np.asarray(prims, np.int64) << 24) + np.asarray(micro, np.int64)
    at = np.maximum(np.searchsorted(keys, want, side="right") - 1, 0)
    found = (keys[at] <= want) & (want < ends[at]) if len(keys) else np.zeros(len(want), bool)
    return np.where(found, lists[at], DROP) if len(keys) else np.full(len(want), DROP)


# ---- ommxExpandMicroNodes ----
def expand_reference(nodes, positions=None, tri_indices=None, triangle_count=None):
    """numpy fp32 restatement: -> (barycentrics (n, 3, 2) float32, positions (n, 3, 3) float32 or None); malformed records are NaN_BITS throughout"""
    node = nodes["node"].astype(np.int64)
    level, index = node >> 24, node & 0xFFFFFF
    ok = (level <= 12) & (index < (1 << (2 * np.minimum(level, 12))))
    if triangle_count is not None:
        ok &= nodes["prim"].astype(np.int64) < triangle_count
    bary = np.full((len(nodes), 3, 2), np.uint32(NAN_BITS).view(np.float32), np.float32)
    bary[ok] = lu.micro_vertices(index[ok], level[ok]).astype(np.float32)
    if positions is None:
        return bary, None
    pos = np.full((len(nodes), 3, 3), np.uint32(NAN_BITS).view(np.float32), np.float32)
    tri = np.asarray(tri_indices).reshape(-1, 3)[nodes["prim"][ok].astype(np.int64)].astype(np.int64)
    V = np.asarray(positions, np.float32)[tri]                     # (m, 3 corners, 3 components)
    u, v = bary[ok][:, :, 0:1], bary[ok][:, :, 1:2]                # (m, 3 vertices, 1)
    w = ((np.float32(1.0) - u).astype(np.float32) - v).astype(np.float32)
    V0, V1, V2 = V[:, None, 0, :], V[:, None, 1, :], V[:, None, 2, :]
    pos[ok] = (((V0 * w).astype(np.float32) + (V1 * u).astype(np.float32)).astype(np.float32) + (V2 * v).astype(np.float32)).astype(np.float32)
    return bary, pos
