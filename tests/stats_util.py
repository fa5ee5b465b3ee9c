"""Shared by tests/test_stats_reference.py, tests/test_stats_gpu.py and tests/scripts/stats_throughput.py: ctypes bindings of the device statistics
(ommxDebugGetStatsDevice, ommxGetDeviceBakeResultTriangleAreas, ommxDebugGetStatsDevice2), a numpy restatement of what they answer, the hand-built
result table of the bounds rule, and the bound that separates the host's fp32 knownAreaMetric from the fp64 one."""
import ctypes as C
import numpy as np
import ommtest as ot
import lookup_util as lu

SEGMENT_BYTES = 16384   # kStatsSegmentBytes (omm_amd/csrc/stats_count.h)
INT_FIELDS = ("totalOpaque", "totalTransparent", "totalUnknownTransparent", "totalUnknownOpaque", "totalFullyOpaque", "totalFullyTransparent",
              "totalFullyUnknownOpaque", "totalFullyUnknownTransparent")
INDEX_DTYPE = {ot.IDX_U8: np.int8, ot.IDX_U16: np.int16, ot.IDX_U32: np.int32}


class DeviceStatsOutputs(C.Structure):
    _fields_ = [("stateCounts", C.c_void_p), ("referenceCounts", C.c_void_p), ("knownFraction", C.c_void_p)]


def bind(dll):
    lu.bind(dll)
    dll.ommxDebugGetStatsDevice.argtypes = [C.c_void_p, C.POINTER(ot.BakeResultDesc), C.c_void_p, C.POINTER(DeviceStatsOutputs), C.POINTER(ot.DebugStats),
                                            C.POINTER(C.c_uint32), C.c_void_p]
    dll.ommxGetDeviceBakeResultTriangleAreas.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    dll.ommxDebugGetStatsDevice2.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ot.DebugStats)]
    return dll


def int_fields(st):
    return tuple(int(getattr(st, f)) for f in INT_FIELDS)


def metric_bits(st):
    return np.float32(st.knownAreaMetric).view(np.uint32).item()


def host_metric_bound(num_triangles):
    """|host fp32 knownAreaMetric - exact| <= 4 * (T + 4) * 2^-24 (derived in tests/test_stats_reference.py); the device's fp64 value adds half an ulp
    of its one rounding to fp32, which the bound's slack of two covers"""
    return 4.0 * (num_triangles + 4) * 2.0 ** -24


def block_bytes(level, bits):
    return ((bits << (2 * level)) + 7) >> 3


def block_counts(array_data, offset, level, bits):
    """the four state counts of one block by a decode per field"""
    n = 1 << (2 * level)
    b = np.unpackbits(array_data[offset:offset + block_bytes(level, bits)], bitorder="little")[:n * bits].astype(np.uint8)
    states = b if bits == 1 else b[0::2] + 2 * b[1::2]
    return np.bincount(states, minlength=4).astype(np.uint32)


def reference_stats(array_data, descs, index, areas=None, array_data_size=None):
    """What ommxDebugGetStatsDevice answers, from host copies: array_data uint8, descs (D, 3) rows of (offset, level, format), index a signed numpy
    array, areas float32 or None.  Returns a dict: state_counts (D, 4) uint32, refs (D,) uint32, known_fraction (T,) float32, skipped, fields (the eight
    integers in INT_FIELDS order, 32-bit products as the host forms them), metric (float32 of the float64 quotient, 0 without areas)."""
    size = len(array_data) if array_data_size is None else array_data_size
    descs = np.asarray(descs, np.int64).reshape(-1, 3)
    D, T = len(descs), len(index)
    counts = np.zeros((D, 4), np.uint32)
    valid = np.zeros(D, bool)
    for d, (o, l, f) in enumerate(descs):
        if l <= 12 and f in (1, 2) and o + block_bytes(int(l), int(f)) <= size:
            valid[d] = True
            counts[d] = block_counts(array_data, int(o), int(l), int(f))
    e = np.asarray(index).astype(np.int64)
    selects = (e >= 0) & (e < D)
    selects[selects] = valid[e[selects]]
    refs = np.bincount(e[selects], minlength=D).astype(np.uint32)[:D] if D else np.zeros(0, np.uint32)
    special = [int((e == -1 - k).sum()) for k in range(4)]
    skipped = int(T - selects.sum() - sum(special))
    kf = np.zeros(T, np.float32)
    kf[(e == -1) | (e == -2)] = 1.0
    known, total = counts[:, 0] + counts[:, 1], counts.sum(axis=1, dtype=np.uint32)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_block = known.astype(np.float32) / total.astype(np.float32)
    kf[selects] = per_block[e[selects]]
    prod = (refs.astype(np.uint64)[:, None] * counts.astype(np.uint64)) & np.uint64(0xFFFFFFFF)   # (uint32_t)(references * count)
    tot = prod.sum(axis=0, dtype=np.uint64) if D else np.zeros(4, np.uint64)
    fields = (int(tot[1]), int(tot[0]), int(tot[2]), int(tot[3]), special[1], special[0], special[3], special[2])
    metric = np.float32(0.0)
    if areas is not None:
        a = np.asarray(areas, np.float32).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            metric = np.float32(np.float64((a * kf.astype(np.float64)).sum()) / np.float64(a.sum()))
    return dict(state_counts=counts, refs=refs, known_fraction=kf, skipped=skipped, fields=fields, metric=metric)


def host_stats(lib, baker, array_data, descs, index, index_format):
    """the library's host ommDebugGetStats (needs no GPU) over host arrays"""
    d = np.asarray(descs, np.int64).reshape(-1, 3)
    raw = np.zeros(max(len(d), 1), dtype=[("o", "<u4"), ("l", "<u2"), ("f", "<u2")])
    raw["o"][:len(d)], raw["l"][:len(d)], raw["f"][:len(d)] = d[:, 0], d[:, 1], d[:, 2]
    rd = lu.result_desc_over((np.ascontiguousarray(array_data), raw.view(np.uint8)[:8 * len(d)] if len(d) else np.zeros(0, np.uint8),
                              np.ascontiguousarray(index)), index_format)
    st = ot.DebugStats()
    assert lib.fn("ommDebugGetStats")(baker, C.byref(rd), C.byref(st)) == ot.SUCCESS
    return st


def ulp_distance(a, b):
    """distance of two finite float32 values in units of the last place"""
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    ia, ib = (x if x >= 0 else -(x & 0x7FFFFFFF) for x in (ia, ib))
    return abs(ia - ib)


# ---- the hand-built table (tests/test_stats_gpu.py: the bounds rule; tests/test_stats_reference.py: its well-formed rows on the host) ----
TABLE_ARRAY_BYTES = 100001
# (offset, level, format): levels 0 - 3 in both formats at odd offsets; a level-7 4-state block (4 KiB) across the array's byte 16384; a level-9 4-state
# block (64 KiB = four segments and, at an odd address, five 16-byte-aligned pieces); then the malformed rows: level 13, formats 0 and 3, and a block that
# ends one byte past arrayDataSize
TABLE_DESCS = [(1, 0, 1), (3, 0, 2), (43, 1, 1), (45, 1, 2), (5, 2, 1), (9, 2, 2), (15, 3, 1), (25, 3, 2),
               (15385, 7, 2), (19483, 9, 2),
               (101, 13, 2), (103, 3, 0), (105, 3, 3), (TABLE_ARRAY_BYTES - 15, 3, 2)]
TABLE_WELL_FORMED = 10
# index entries: the four specials, -5 and descArrayCount (ignored by the host too), the malformed rows (ignored by the device), block 0 three times,
# block 8 once, block 7 never
TABLE_INDEX = [-1, 0, -2, 8, -3, 1, -4, 2, -5, 14, 0, 3, 10, 4, 11, 5, 12, 6, 13, 9, 0, -1, 9, -100, 100, -2]


def table_arrays(seed=5):
    rng = np.random.default_rng(seed)
    array_data = rng.integers(0, 256, TABLE_ARRAY_BYTES, dtype=np.uint8)
    areas = rng.random(len(TABLE_INDEX), dtype=np.float32) + np.float32(0.01)
    return array_data, np.array(TABLE_DESCS, np.int64), np.array(TABLE_INDEX, np.int64), areas
