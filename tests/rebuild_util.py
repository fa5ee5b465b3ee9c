"""Shared by tests/coarsen_util.py, tests/combine_util.py and tests/gather_util.py: the tail of a derived result (omm_amd/csrc/rebuild_kernels.hip),
restated once in Python for restate_coarsen, restate_combine and restate_gather.  Each of them produces its items in its own way -- a source descriptor,
a tuple, a (source, descriptor) pair, numbered in the order in which the definition ranks them -- and hands them here: representatives, the order of
the output blocks, offsets, arrayData, the array histogram and every item's new index entry.  It owes nothing to the kernels."""
import numpy as np

NONE, NO_SPECIAL, NO_DEDUP = 0, 1, 2


def representatives(merge, order, items):
    """a merge rule other than "equal level, format and bytes" (tests/rebuild_cases.py): merge([(level, format, bytes)] in item order) answers each
    item's representative as a position in that list -> {item: representative item}"""
    return {d: order[int(c)] for d, c in zip(order, merge(items))}


def restate_tail(kind, blocks, special, flags=0, merge=None):
    """kind: {item: (level, format)} of every item the operation produced; an item has either its packed bytes in `blocks` (uint8 array) or its special
    entry in `special`.  flags: NO_DEDUP counts here (NO_SPECIAL is the producer's: it decides which items keep a block); merge: see representatives()
    -> dict: rep {item: item}, emitted [item] in output order, place {item: output descriptor}, descs (E, 3) int64, array (uint8), array_hist
    {(level, format): count}, entry {item: new index entry}, duplicates"""
    order = sorted(blocks)
    rep, seen, duplicates = {}, {}, 0
    for d in order:
        key = (kind[d], blocks[d].tobytes())
        if not flags & NO_DEDUP and key in seen:
            rep[d] = seen[key]
            duplicates += 1
        else:
            rep[d] = seen[key] = d
    if merge is not None and not flags & NO_DEDUP:
        rep = representatives(merge, order, [kind[d] + (blocks[d],) for d in order])
        duplicates = sum(d != r for d, r in rep.items())
    emitted = sorted((d for d in blocks if rep[d] == d), key=lambda d: (-len(blocks[d]), d))
    place = {d: j for j, d in enumerate(emitted)}
    descs, at, array_hist = [], 0, {}
    for d in emitted:
        descs.append((at,) + kind[d])
        at += len(blocks[d])
        array_hist[kind[d]] = array_hist.get(kind[d], 0) + 1
    array = np.concatenate([blocks[d] for d in emitted]) if emitted else np.zeros(0, np.uint8)
    entry = {d: special[d] if d in special else place[rep[d]] for d in kind}
    return dict(rep=rep, emitted=emitted, place=place, descs=np.array(descs, np.int64).reshape(-1, 3), array=array, array_hist=array_hist, entry=entry,
                duplicates=duplicates)


def index_histogram(kind, blocks, uses):
    """the index histogram of an operation: uses[item] primitives end at item, and those of an item that keeps a block count under its (level, format)"""
    hist = {}
    for d in blocks:
        hist[kind[d]] = hist.get(kind[d], 0) + int(uses[d])
    return hist
