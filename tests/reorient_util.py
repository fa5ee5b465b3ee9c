"""Shared by tests/test_reorient.py, tests/test_reorient_gpu.py and tests/scripts/reorient_throughput.py: ctypes bindings of ommxReorientMicromap,
two statements of the definition in include/omm_mi355x_ext.h that owe nothing to the kernels or to the transducer of omm_amd/csrc/reorient_map.h --
restate_reorient (numpy: the map from the discrete barycentrics of the forward decode, coarsen_util.block_states, lookup_util.pack, then
rebuild_util.restate_tail) and brute_reorient (Python loops over ommx_micro_vertices centroids and ommx_micro_index, levels <= 4) -- and the call on
device copies of hand-built sources."""
import ctypes as C
import functools
import os
import subprocess
import numpy as np
import ommtest as ot
import lookup_util as lu
import stats_util as su
import coarsen_util as cu
import combine_util as mu
import rebuild_util as ru
from rebuild_util import NONE, NO_SPECIAL, NO_DEDUP  # noqa: F401  (the callers' names for them)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERMS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))   # perm_o[k]: new vertex k is old vertex perm_o[k]
INVERSE = (0, 2, 1, 3, 4, 5)
INFO_FIELDS = ("arrayDataSize", "descArrayCount", "referencedBlocks", "reorientedBlocks", "uniformBlocks", "duplicateBlocks", "skippedPrimitives")


class ReorientDesc(C.Structure):
    _fields_ = [("deviceOrientations", C.c_void_p), ("orientation", C.c_uint8), ("reserved", C.c_uint8 * 3), ("flags", C.c_uint32)]


class ReorientInfo(C.Structure):
    _fields_ = [("arrayDataSize", C.c_uint64), ("descArrayCount", C.c_uint32), ("referencedBlocks", C.c_uint32), ("reorientedBlocks", C.c_uint32),
                ("uniformBlocks", C.c_uint32), ("duplicateBlocks", C.c_uint32), ("skippedPrimitives", C.c_uint32)]


def bind(dll):
    mu.bind(dll)
    dll.ommxReorientMicromap.argtypes = [C.c_void_p, C.POINTER(ot.BakeResultDesc), C.POINTER(ReorientDesc), C.POINTER(C.c_void_p), C.POINTER(ReorientInfo),
                                         C.c_void_p]
    return dll


def c_desc(orientations=None, orientation=0, flags=0, reserved=(0, 0, 0)):
    d = ReorientDesc()
    d.deviceOrientations, d.orientation, d.flags = orientations, orientation, flags
    d.reserved[:] = list(reserved)
    return d


def info_dict(info):
    return {f: int(getattr(info, f)) for f in INFO_FIELDS}


# ---- the rule, from the discrete barycentrics of the forward decode ----
def _weights(index, level):
    """(iw, iu, iv) of the forward decode: the weights of vertices 0, 1, 2 (lookup_util.micro_cells, with the third kept)"""
    index = np.asarray(index, np.uint32)
    b0, b1 = lu._even_bits(index), lu._even_bits(index >> np.uint32(1))
    fx, fy = lu._pxor(b0), lu._pxor(b0 & ~b1)
    t = fy ^ b1
    m = np.uint32((1 << level) - 1)
    iu = ((fx & ~t) | (b0 & ~t) | (~b0 & ~fx & t)) & m
    iv = (fy ^ b0) & m
    iw = ((~fx & ~t) | (b0 & ~t) | (~b0 & fx & t)) & m
    return iw.astype(np.int64), iu.astype(np.int64), iv.astype(np.int64)


def _cell_key(w, level):
    """a micro-triangle's place from its weights (w0, w1, w2) = (iw, iu, iv): the grid cell (iu, iv) and which half of it -- the three sum to
    2^level - 1 in the upright half and to 2^level - 2 in the inverted one"""
    n = 1 << level
    total = w[0] + w[1] + w[2]
    assert ((total == n - 1) | (total == n - 2)).all()
    return (((w[1] << level) | w[2]) << 1) | (total == n - 1)


@functools.lru_cache(maxsize=16)
def _decode_inverse(level):
    """table[key] = the index whose forward decode has that key, -1 where there is none.  The decode visits every half cell once, so this table IS
    its inverse -- no digit table, no transducer"""
    idx = np.arange(4 ** level, dtype=np.uint32)
    table = np.full(2 << (2 * level), -1, np.int64)
    table[_cell_key(_weights(idx, level), level)] = idx
    assert (table >= 0).sum() == len(idx)
    return table


@functools.lru_cache(maxsize=64)
def source_map(level, o):
    """source index of every output index 0 .. 4^level - 1 under orientation o (int64)"""
    if level == 0:
        return np.zeros(1, np.int64)
    new = _weights(np.arange(4 ** level, dtype=np.uint32), level)       # t'[k]: the weight of new vertex k
    old = [None, None, None]
    for k in range(3):
        old[PERMS[o][k]] = new[k]                                       # t[perm_o[k]] = t'[k]
    source = _decode_inverse(level)[_cell_key(old, level)]
    assert (source >= 0).all()
    return source


def reorient_states(states, level, o):
    return np.asarray(states)[source_map(level, o)]


# ---- the definition, twice ----
def restate_reorient(source, orientations, flags=0, unpacked=None):
    """What ommxReorientMicromap answers.  source: (array_data uint8, descs (D, 3) rows of (offset, level, format), index, arrayDataSize or None);
    orientations: one code for every primitive or an array of bytes -> dict like restate_gather's.  unpacked: a dict that keeps the unpacked states
    of source blocks between calls on the same source"""
    a, descs, index, size = source
    descs = np.asarray(descs, np.int64).reshape(-1, 3)
    e = np.asarray(index).astype(np.int64)
    N, D = len(e), len(descs)
    o = np.full(N, orientations, np.int64) if np.isscalar(orientations) else np.asarray(orientations).astype(np.int64)
    assert len(o) == N
    oriented = o <= 5
    valid = mu._valid_rows(descs, len(a) if size is None else size)
    special = oriented & (e < 0) & (e >= -4)
    selects = oriented & (e >= 0) & (e < D)
    selects[selects] = valid[e[selects]]
    out_e = np.full(N, -4, np.int64)
    out_e[special] = e[special]
    item_of = np.full(N, -1, np.int64)
    item_of[selects] = 6 * e[selects] + o[selects]                       # rank (e, o), lexicographic
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["skippedPrimitives"] = int(N - special.sum() - selects.sum())
    blocks, entry, kind = {}, {}, {}
    for it in np.unique(item_of[selects]).tolist():
        d, oo = divmod(it, 6)
        off, l, f = (int(x) for x in descs[d])
        states = unpacked.get((off, l, f)) if unpacked is not None else None
        if states is None:
            states = cu.block_states(a, off, l, f)
            if unpacked is not None:
                unpacked[(off, l, f)] = states
        out = states[source_map(l, oo)]
        info["referencedBlocks"] += 1
        info["reorientedBlocks"] += oo != 0
        kind[it] = (l, f)
        uniform = bool((out == out[0]).all())
        info["uniformBlocks"] += uniform
        if uniform and not flags & NO_SPECIAL:
            entry[it] = -(int(out[0]) + 1)
        else:
            blocks[it] = lu.pack(out, f)
    tail = ru.restate_tail(kind, blocks, entry, flags)
    items, uses = sorted(kind), {}
    if selects.any():
        at_item = np.searchsorted(items, item_of[selects])
        out_e[selects] = np.array([tail["entry"][it] for it in items], np.int64)[at_item]
        uses = dict(zip(items, np.bincount(at_item, minlength=len(items))))
    info["duplicateBlocks"], info["arrayDataSize"], info["descArrayCount"] = tail["duplicates"], len(tail["array"]), len(tail["emitted"])
    return dict(array=tail["array"], descs=tail["descs"], index=out_e.astype(np.int32), array_hist=tail["array_hist"],
                index_hist=ru.index_histogram(kind, blocks, uses), info=info)


SHIM = r"""
#include "omm_mi355x_lookup.h"
extern "C" {
uint32_t shim_micro_index(float u, float v, uint32_t level) { return ommx_micro_index(u, v, level); }
void shim_micro_vertices(uint32_t index, uint32_t level, float* uv) { ommx_micro_vertices(index, level, uv); }
uint32_t shim_reorient_index(uint32_t index, uint32_t level, uint32_t o) { return ommx_reorient_index(index, level, o); }
void shim_reorient_map(uint32_t level, uint32_t o, uint32_t* out) { for (uint32_t i = 0; i < (1u << (2u * level)); ++i) out[i] = ommx_reorient_index(i, level, o); }
}
"""


def host_header(tmp_path):
    """include/omm_mi355x_lookup.h compiled as plain host C++ behind four C functions"""
    src, so = os.path.join(str(tmp_path), "reorient_shim.cpp"), os.path.join(str(tmp_path), "reorient_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src, "-o", so], check=True)
    dll = C.CDLL(so)
    dll.shim_micro_index.argtypes, dll.shim_micro_index.restype = [C.c_float, C.c_float, C.c_uint32], C.c_uint32
    dll.shim_micro_vertices.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    dll.shim_reorient_index.argtypes, dll.shim_reorient_index.restype = [C.c_uint32] * 3, C.c_uint32
    dll.shim_reorient_map.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    return dll


def header_map(shim, level, o):
    out = np.zeros(4 ** level, np.uint32)
    shim.shim_reorient_map(level, o, out.ctypes.data)
    return out.astype(np.int64)


def brute_map(shim, level, o):
    """the same map through hits: the centroid of output micro-triangle j' in the new order, its barycentrics handed to the old vertices
    (b[perm_o[k]] = b'[k]), ommx_micro_index of (b[1], b[2]).  Python loops, levels <= 4"""
    assert level <= 4
    out, uv = [], (C.c_float * 6)()
    for j in range(4 ** level):
        shim.shim_micro_vertices(j, level, uv)
        u, v = (uv[0] + uv[2] + uv[4]) / 3.0, (uv[1] + uv[3] + uv[5]) / 3.0
        new, old = (1.0 - u - v, u, v), [0.0, 0.0, 0.0]
        for k in range(3):
            old[PERMS[o][k]] = new[k]
        out.append(int(shim.shim_micro_index(old[1], old[2], level)))
    return out


def brute_reorient(shim, blocks, index, orientations, flags=0):
    """The same answer for a well-formed source by Python loops.  blocks: [(states, level, bits)]; index: entries; orientations: one byte per
    primitive -> (blocks out as [(states list, level, bits)] in output order, index entries, counts (referenced, reoriented, uniform, duplicate,
    skipped))"""
    pairs, skipped = [], 0
    for e, o in zip(index, orientations):
        if o > 5 or e < -4 or e >= len(blocks):
            pairs.append(None)
            skipped += 1
        else:
            pairs.append((int(e), int(o)))
    items = sorted({p for p in pairs if p is not None and p[0] >= 0})
    body = {}
    for e, o in items:
        states, level, bits = blocks[e]
        m = brute_map(shim, level, o)
        body[(e, o)] = ([int(states[j]) for j in m], level, bits)
    uniform = [it for it in items if all(s == body[it][0][0] for s in body[it][0])]
    special = {} if flags & NO_SPECIAL else {it: -(body[it][0][0] + 1) for it in uniform}
    keep = [it for it in items if it not in special]
    rep = {}
    for n, it in enumerate(keep):
        rep[it] = it if flags & NO_DEDUP else next((c for c in keep[:n] if body[c] == body[it]), it)
    emitted = sorted((it for it in keep if rep[it] == it), key=lambda it: (-max(1, 4 ** body[it][1] * body[it][2] // 8), it))
    entries = []
    for p in pairs:
        if p is None:
            entries.append(-4)
        elif p[0] < 0:
            entries.append(p[0])
        else:
            entries.append(special[p] if p in special else emitted.index(rep[p]))
    return ([body[it] for it in emitted], entries,
            (len(items), sum(1 for it in items if it[1]), len(uniform), len(keep) - len(emitted), skipped))


# ---- a call on the device ----
def reorient(dll, baker, rd, orientations=None, orientation=0, flags=0, want_result=True, stream=None):
    """orientations: a device pointer or None -> (result code, info dict, handle or None)"""
    out, info = C.c_void_p(), ReorientInfo()
    r = dll.ommxReorientMicromap(baker, C.byref(rd), C.byref(c_desc(orientations, orientation, flags)), C.byref(out) if want_result else None, C.byref(info), stream)
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


def reorient_and_check(dll, hip, baker, src, orientations, flags=0, stream=None, keep=False):
    """the whole contract on one input: the info-only call, the full call, both against the model; the source is untouched.  src: a
    coarsen_util.Source; orientations: one code (given through the desc) or an array of bytes (uploaded) -> the model's answer (keep: and the
    handle, which the caller destroys)"""
    a, d, i = src.host
    if src.declared:
        size, D, T = src.declared
        host = (a, d[:D], i[:T], size)
    else:
        host = (a, d, i, None)
    per_primitive = not np.isscalar(orientations)
    ref = restate_reorient(host, orientations, flags, src.unpacked)
    d_o = hip.upload(np.ascontiguousarray(orientations, np.uint8) if len(orientations) else np.zeros(1, np.uint8)) if per_primitive else None
    uniform = 0 if per_primitive else int(orientations)
    handle = None
    try:
        r, info, _ = reorient(dll, baker, src.rd, d_o, uniform, flags, want_result=False, stream=stream)
        assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
        r, info, handle = reorient(dll, baker, src.rd, d_o, uniform, flags, stream=stream)
        assert r == ot.SUCCESS, r
        check_result(dll, hip, baker, handle, info, ref, flags)
        assert src.unchanged()
    finally:
        if d_o is not None:
            hip.free(d_o)
        if handle is not None and not keep:
            assert dll.ommxDestroyDeviceBakeResult(handle) == ot.SUCCESS
    return (ref, handle) if keep else ref
