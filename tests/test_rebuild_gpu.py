"""The shared tail of ommxCoarsenMicromap, ommxCombineMicromaps and ommxGatherMicromaps (omm_amd/csrc/rebuild_kernels.hip, hash_build.h,
result_words.h) where digests, keys and slots collide.  Random data never collides in 64 bits, so every other test of the three entries only ever
shows the confirmation of rebuild_resolve blocks that ARE equal; the blocks here are constructed (tests/rebuild_cases.py) to share a digest while
differing in two chosen words, to share a key across (level, format), to have the all-ones key, and to have keys with one home slot.

Every case goes through the C ABI, every result is compared in full -- arrayData, descriptors, index values, both histograms, the info counts -- with
the three restatements under the rule of rebuild_cases.merge_under_keys (the candidate of a block is the LOWEST item under its key; a block that
differs from its candidate is kept, and so is a later copy of it), without a tolerance, and every call is made twice with equal bytes.  The copy B'
of a rejected block B is the witness: only a tail that reached the rejecting branch keeps three blocks for A, B, B'.

Blocks pass through the entries verbatim -- the gather copies bytes, a coarsening at cap 12 keeps every level, a combine of ONE source into its own
format is a join that changes nothing -- so one table collides in all three although each has its own digest writer.  The combine has one output
format, so it gets the 4-state and the 2-state blocks of a table in two calls, and no cross-key pair of two formats.

What cannot be built, and is not chased: blocks of 1, 2 and 4 bytes, and two 8-byte blocks of one format, cannot collide -- mix64 is injective on
the one word -- so the byte loop and (for equal formats) the 8-byte case of same_bytes cannot be made to reject.  An 8-byte block can only share the
key of a block of another (level, format).  Collisions of the combine's TUPLE hash are out of scope: entries are 32-bit, with one source the hash is
injective, and with more a collision costs about 2^32 work to find (meet in the middle over valid entries), which no seconds-sized test can spend."""
import numpy as np
import pytest
import ommtest as ot
import coarsen_util as cu
import combine_util as mu
import gather_util as gt
import rebuild_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return ot.Hip()


@pytest.fixture(scope="module")
def dll(product):
    return gt.bind(product.dll)


@pytest.fixture(scope="module")
def baker(product):
    b = product.create_baker()
    yield b
    product.destroy_baker(b)


def source_of(hip, items, unreferenced=0, index_format=ot.IDX_U16):
    """one source over the items' bytes: two primitives per block (ascending, then descending), `unreferenced` more descriptors that no primitive
    selects (they count for the size of the tail's hash table and stage nothing)"""
    array, descs = rc.table_of_bytes(items)
    index = np.concatenate([np.arange(len(items)), np.arange(len(items))[::-1]])
    return cu.Source(hip, array, np.concatenate([descs, np.repeat(descs[:1], unreferenced, axis=0)]), index, index_format, array_align=16)


def destroy(dll, handles):
    for h in handles:
        assert dll.ommxDestroyDeviceBakeResult(h) == ot.SUCCESS


def run_gather(dll, hip, baker, src, flags=0, stream=None):
    ref = gt.restate_gather(mu.host_sources([src]), None, flags, merge=rc.merge_under_keys)
    made = []
    try:
        r, info, _ = gt.gather(dll, baker, [src.rd], flags=flags, want_result=False, stream=stream)
        assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
        for _ in range(2):
            r, info, h = gt.gather(dll, baker, [src.rd], flags=flags, stream=stream)
            assert r == ot.SUCCESS
            made.append(h)
        got = gt.check_result(dll, hip, baker, made[0], info, ref, flags)
        cu.assert_same(cu.download_result(dll, hip, made[1]), got)
        assert src.unchanged()
    finally:
        destroy(dll, made)
    return ref


def run_coarsen(dll, hip, baker, src, flags=0):
    a, d, i = src.host
    ref = cu.restate_coarsen(a, d, i, src.rd.indexFormat, 12, 3, flags, merge=rc.merge_under_keys)
    made = []
    try:
        r, info, _ = cu.coarsen(dll, baker, src.rd, 12, 3, flags, want_result=False)
        assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
        for _ in range(2):
            r, info, h = cu.coarsen(dll, baker, src.rd, 12, 3, flags)
            assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
            made.append(h)
        got = cu.download_result(dll, hip, made[0])
        cu.assert_same(got, ref)
        cu.assert_same(cu.download_result(dll, hip, made[1]), got)
        assert info["coarsenedBlocks"] == 0 and src.unchanged()
    finally:
        destroy(dll, made)
    return ref


def run_combine(dll, hip, baker, src, fmt):
    ref = mu.restate_combine(mu.host_sources([src]), fmt, 3, merge=rc.merge_under_keys)
    made = []
    try:
        r, info, _ = mu.combine(dll, baker, [src.rd], fmt, want_result=False)
        assert (r, info) == (ot.SUCCESS, ref["info"]), (r, info, ref["info"])
        for _ in range(2):
            r, info, h = mu.combine(dll, baker, [src.rd], fmt)
            assert r == ot.SUCCESS
            made.append(h)
        got = mu.check_result(dll, hip, baker, made[0], info, ref)
        cu.assert_same(cu.download_result(dll, hip, made[1]), got)
        assert info["refinedTuples"] == 0 and src.unchanged()
    finally:
        destroy(dll, made)
    return ref


def blocks_of(ref):
    """the bytes of every output block of a model's answer"""
    return [ref["array"][int(o):int(o) + rc.block_bytes(int(l), int(f))].tobytes() for o, l, f in ref["descs"]]


# ---- C: the core table ----
@pytest.fixture(scope="module")
def core(hip):
    items, merges = rc.core_table()
    src = source_of(hip, items)
    yield items, merges, src
    src.close()


@pytest.mark.parametrize("entry", ["gather", "coarsen"])
@pytest.mark.parametrize("flags", [0, cu.NO_DEDUP, cu.NO_SPECIAL], ids=["default", "no-dedup", "no-special"])
def test_core_table(dll, hip, baker, core, entry, flags):
    """twins A, B of 16, 32, 64, 256 and 1024 bytes, each followed by A' == A and B' == B, in the orders A B A' B' and B A A' B': the copy of the
    first merges, the other and ITS copy are kept, duplicateBlocks counts the ten merged copies, and the primitives of the kept copy read its bytes
    from a block of their own.  A level-4 4-state A with a level-3 4-state B (16 bytes) and with a level-3 2-state B (8 bytes) under A's key, and
    B' == B behind each: three blocks each -- B's bytes are the first bytes of A, so only the comparison of level and format keeps them apart.  With DisableDuplicateDetection nothing merges and no table is built; with DisableSpecialIndices the
    uniform pair enters the table too and its copy merges"""
    items, merges, src = core
    ref = (run_gather if entry == "gather" else run_coarsen)(dll, hip, baker, src, flags)
    live = len(items) - (0 if flags & cu.NO_SPECIAL else 2)
    want = 0 if flags & cu.NO_DEDUP else merges + (1 if flags & cu.NO_SPECIAL else 0)
    assert ref["info"]["duplicateBlocks"] == want and ref["info"]["descArrayCount"] == live - want and ref["info"]["uniformBlocks"] == 2
    if not flags:
        emitted = blocks_of(ref)                                            # a rejected block is there twice: for itself and for its copy
        assert sorted(emitted.count(b) for b in set(emitted)).count(2) == 12 and max(emitted.count(b) for b in emitted) == 2


@pytest.mark.parametrize("fmt", [2, 1])
def test_core_table_through_the_combine(dll, hip, baker, core, fmt):
    """the blocks of one format of the core table as one source whose primitives each select their own descriptor, so the tuples are the descriptors
    in order: the combine's own digest writer (combine_units) collides on the same bytes"""
    items = [it for it in core[0] if it[1] == fmt]
    live = [it for it in items if not rc.is_uniform(it[2], fmt)]
    merges = int((rc.merge_under_keys(live) != np.arange(len(live))).sum())
    assert merges == (8 if fmt == 2 else 3)                                # (2-state: the two 32-byte quads, and the 8-byte B' into B, whose A is not here)
    src = source_of(hip, items, index_format=ot.IDX_U8)
    try:
        ref = run_combine(dll, hip, baker, src, fmt)
        assert ref["info"]["duplicateBlocks"] == merges and ref["info"]["combinedTuples"] == len(items)
        assert ref["info"]["descArrayCount"] == len(items) - merges - ref["info"]["uniformBlocks"]
    finally:
        src.close()


# ---- E: the all-ones key ----
@pytest.mark.parametrize("nbytes", [8, 64])
def test_the_all_ones_key(dll, hip, baker, nbytes):
    """a block whose key is kEmptyKey between ordinary blocks, with an exact copy (merged) and, at 64 bytes, a twin and the twin's copy (both kept),
    through all three entries; in front of it and behind it a block whose key has the home slot that the slot arithmetic would give the all-ones
    key, with copies of both at the end (merged).  Such a key never probes: hash_put_min and hash_get go straight to the slot of index `slots`,
    one past the probed ones.  Its value vals[slots] is inside the table's bytes: hash_table_at puts vals at byte 8 * slots, so vals[slots] ends at 8 * slots + 4 * (slots + 1),
    which is hash_table_bytes(slots) -- the size that carve() takes from the scratch and that rebuild_count fills with 0xFF, the dedicated value
    included (tests/native/rebuild_hash_check.cpp places it in real memory of that size under ASan)"""
    items, merges, places = rc.empty_key_table(nbytes)
    bits = rc.KIND_OF_BYTES[nbytes][1]
    src = source_of(hip, items)
    try:
        for ref in (run_gather(dll, hip, baker, src), run_coarsen(dll, hip, baker, src), run_combine(dll, hip, baker, src, bits)):
            assert ref["info"]["duplicateBlocks"] == merges == 3 and ref["info"]["descArrayCount"] == len(items) - 3
            entries = [int(ref["index"][t]) for t in places]
            assert entries[0] == entries[1] and (nbytes == 8 or (entries[2] != entries[3] and entries[0] not in entries[2:]))
    finally:
        src.close()


# ---- S: where same_bytes looks ----
@pytest.mark.parametrize("nbytes", [16, 32, 64, 128, 256, 1024, 16384])
def test_position_sweep(dll, hip, baker, nbytes):
    """quads A, B, A', B' whose twins differ in exactly the words (i, j) of rebuild_cases.sweep_pairs: every word pair of 16, 32 and 64 bytes (the
    8-byte loop; one 64-byte turn); for the larger sizes both words in each of the four vectors of the first and of the last turn, each position of a
    turn, both in the lower and both in the upper halves of vectors, the last two words, the first and the last.  A same_bytes that skips a vector, a
    half or a turn merges at least one B into its A; one that says no too early keeps an A'.  The 256-byte table also goes through the coarsening"""
    items, merges = rc.sweep_table(nbytes)
    src = source_of(hip, items)
    try:
        ref = run_gather(dll, hip, baker, src)
        assert ref["info"]["duplicateBlocks"] == merges == len(items) // 4 and ref["info"]["descArrayCount"] == 3 * merges
        if nbytes == 256:
            assert run_coarsen(dll, hip, baker, src)["info"]["duplicateBlocks"] == merges
    finally:
        src.close()


# ---- H: chains ----
@pytest.mark.parametrize("entry", ["gather", "coarsen"])
@pytest.mark.parametrize("home,descriptors", [(1023, 309), (0, 309), (2047, 513)], ids=["wraps-1024", "home-0", "wraps-2048"])
def test_probe_chains(dll, hip, baker, entry, home, descriptors):
    """300 distinct 16-byte blocks whose keys all have one home slot: from the last slot of 1024 the chain wraps to slot 298, from slot 0 it runs to
    299; with 513 descriptors (204 of them unreferenced) the table has 2048 slots, the first size above the floor.  Behind the chain an exact copy of
    its 1st, 150th and 300th block (merged: the look-up walks the whole chain, wherever the puts of that block landed) and a twin of each with the
    twin's copy (kept).  N is the concatenated descriptor count for the gather and descArrayCount for the coarsening"""
    slots = rc.hash_table_slots(descriptors)
    assert slots == (2048 if descriptors == 513 else 1024) and home in (0, slots - 1)
    items, merges = rc.chain_table(home, slots)
    assert len(items) == 309
    src = source_of(hip, items, unreferenced=descriptors - len(items))
    try:
        ref = (run_gather if entry == "gather" else run_coarsen)(dll, hip, baker, src)
        assert ref["info"]["duplicateBlocks"] == merges == 3 and ref["info"]["descArrayCount"] == 306 and ref["info"]["referencedBlocks"] == 309
        assert ref["index"][[300, 303, 306]].tolist() == ref["index"][[0, 149, 299]].tolist()
        assert len({int(e) for e in ref["index"][[301, 302, 304, 305, 307, 308]]} | {int(e) for e in ref["index"][:300]}) == 306
    finally:
        src.close()


# ---- D: lanes that leave the comparison at different turns, in many workgroups ----
def test_divergence_at_scale(dll, hip, baker):
    """70 001 descriptors of 256-byte blocks in one source (262 144 slots, 274 workgroups of the per-item kernels) through the gather on a caller's
    non-blocking stream, info-only and full: 17 500 quads A, B, A', B' whose twins differ first in word k, k stepping through the four turns from
    quad to quad, every item at a seeded place -- so the lanes of a wave are candidates (no comparison), copies (the loop to its end) and rejected
    blocks that leave at turn 0, 1, 2 or 3, and their candidates lie in other workgroups.  duplicateBlocks is the number of quads, and every index
    entry and every byte is the model's (rebuild_cases.expected_verbatim, which tests/test_rebuild_reference.py holds to restate_gather)"""
    items, merges = rc.divergence_table(17500)
    assert len(items) == 70001 and rc.hash_table_slots(len(items)) == 262144
    array, descs = rc.table_of_bytes(items)
    index = np.arange(len(items))
    ref = rc.expected_verbatim(items, index)
    assert ref["info"]["duplicateBlocks"] == merges == 17500 and ref["info"]["descArrayCount"] == 52501
    src = cu.Source(hip, array, descs, index, ot.IDX_U32, array_align=16)
    stream = hip.stream_create(non_blocking=True)
    made = []
    try:
        for _ in range(2):
            r, info, _ = gt.gather(dll, baker, [src.rd], want_result=False, stream=stream)
            assert r == ot.SUCCESS and {k: info[k] for k in ref["info"]} == ref["info"] and info["primitiveCount"] == len(items), info
            r, info, h = gt.gather(dll, baker, [src.rd], stream=stream)
            assert r == ot.SUCCESS
            made.append(h)
            assert {k: info[k] for k in ref["info"]} == ref["info"], info
        got = cu.download_result(dll, hip, made[0])
        cu.assert_same(got, ref)
        cu.assert_same(cu.download_result(dll, hip, made[1]), got)
    finally:
        destroy(dll, made)
        hip.stream_destroy(stream)
        src.close()
