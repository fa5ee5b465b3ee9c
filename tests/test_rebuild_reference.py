"""The model behind tests/test_rebuild_gpu.py without a GPU: the restated digest / key / slot arithmetic of tests/rebuild_cases.py against the
headers' own functions (tests/native/rebuild_hash_check.cpp, host code under the sanitizers), the inverses and the constructors' claims, and the merge
rule "the candidate is the lowest item under the key" against the merge by bytes of the three restatements: equal where nothing collides, different
exactly in the copies of rejected blocks where something does."""
import os
import struct
import subprocess
import numpy as np
import pytest
import ommtest as ot
import lookup_util as lu
import coarsen_util as cu
import combine_util as mu
import gather_util as gt
import rebuild_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- the restatement against the headers ----
def _record(level, bits, block, items, slots=None, slot=None, digest=None, key=None):
    """a record of rebuild_hash_check's file; what is not given is what the restatement computes"""
    block = np.asarray(block, np.uint8)
    digest = int(rc.block_digest(block)) if digest is None else digest
    key = int(rc.block_key(digest, level, bits)) if key is None else key
    slots = rc.hash_table_slots(items) if slots is None else slots
    slot = (slots if key == rc.EMPTY_KEY else int(rc.hash_slot_of(key, slots))) if slot is None else slot
    return struct.pack("<IIQQIIQQ", level, bits, len(block), items, slots, slot, digest, key) + rc.bytes_of(rc.words_of(block)).tobytes()


def _case_records():
    rng = np.random.default_rng(11)
    out = []
    sizes = sorted(rc.KIND_OF_BYTES)                                      # 8 B .. 16 KiB
    counts = {1024: 300, 2048: 513, 262144: 70001}
    for nbytes in sizes:
        level, bits = rc.KIND_OF_BYTES[nbytes]
        n = nbytes // 8
        for slots, items in counts.items():
            assert rc.hash_table_slots(items) == slots
            a = rc.random_block(rng, nbytes)
            out.append(_record(*a, items))
            # a chosen digest; a chosen key, the all-ones key among them; keys for the first, a middle and the last home slot
            d = int(rng.integers(0, 1 << 64, dtype=np.uint64))
            out.append(_record(level, bits, rc.bytes_of(rc.with_digest(rc.random_words(rng, n), d)), items, digest=d))
            for key in (rc.EMPTY_KEY, 0, 1, rc.M64 - 1, int(rng.integers(0, 1 << 64, dtype=np.uint64))):
                out.append(_record(level, bits, rc.with_key(key, level, bits, rng), items, key=key, slot=slots if key == rc.EMPTY_KEY else None))
            for home in (0, slots // 2 - 1, slots - 1):
                key = rc.key_in_slot(home, slots, rng)
                out.append(_record(level, bits, rc.with_key(key, level, bits, rng), items, key=key, slot=home))
            if n >= 2:
                for i, j in ((0, n - 1), (n - 1, 0), (n // 2, n // 2 - 1)):
                    t = rc.twin_block(a, i, j, int(rng.integers(1, 1 << 64, dtype=np.uint64)))
                    out.append(_record(*t, items, digest=int(rc.block_digest(a[2]))))
            for level_b, bits_b in ((3, 1), (3, 2), (8, 2)):
                if (level_b, bits_b) != (level, bits):
                    key = int(rc.block_key(rc.block_digest(a[2]), level, bits))
                    out.append(_record(level_b, bits_b, rc.cross_key(a[2], level, bits, level_b, bits_b, rng), items, key=key))
    for items, want in ((0, 1024), (1, 1024), (512, 1024), (513, 2048), (1024, 2048), (1025, 4096), (65536, 131072), (65537, 262144), (1 << 30, 1 << 31),
                        (1 << 31, 1 << 31), ((1 << 32) - 1, 1 << 31)):
        assert rc.hash_table_slots(items) == want
        out.append(_record(3, 2, rc.random_block(rng, 16)[2], items) if want <= 262144 else b"")
    for nbytes in rng.choice(sizes[:8], 10000):                            # 10 000 random blocks of 8 B .. 1 KiB
        out.append(_record(*rc.random_block(rng, int(nbytes)), int(rng.integers(0, 3000))))
    # blocks below a word, padded with zeros: the restated digest is the writers' digest there too
    for nbytes, (level, bits) in ((1, (0, 2)), (1, (1, 2)), (2, (2, 2)), (4, (2, 2)), (2, (2, 1))):
        out.append(_record(level, bits, rng.integers(1, 255, nbytes).astype(np.uint8), 10))
    return [r for r in out if r]


def test_restatement_against_the_headers(tmp_path):
    """every constructor's output for block sizes 8 B .. 16 KiB and tables of 1024, 2048 and 262 144 slots, the all-ones key, the slot counts at
    their steps and 10 000 random blocks, written as data; a stand-alone program recomputes digest, key, slot count and slot with the functions of
    result_words.h and hash_build.h themselves and places the slot's value inside hash_table_bytes() -- host code only, under ASan and UBSan"""
    records = _case_records()
    assert len(records) > 10500
    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"RBHASH01" + struct.pack("<Q", len(records)) + b"".join(records))
    exe = str(tmp_path / "rebuild_hash_check")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "omm_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "rebuild_hash_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "rebuild_hash_check: %d records, 0 mismatches" % len(records) in r.stdout, r.stdout
    # the program is not deaf: one flipped bit of a block is four mismatches (digest, key, and with them the slot -- or not, by chance)
    broken = bytearray(b"".join(records[:1]))
    broken[-1] ^= 0x10
    cases.write_bytes(b"RBHASH01" + struct.pack("<Q", 1) + bytes(broken))
    r = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 1 and "the digest is" in r.stdout and "the key is" in r.stdout, r.stdout


# ---- inverses and constructors ----
def test_inverses_round_trip():
    rng = np.random.default_rng(12)
    x = np.concatenate([rc.random_words(rng, 100000), rc.u64([0, 1, rc.M64, rc.M64 - 1, 1 << 63])])
    i = rng.integers(0, 2048, len(x)).astype(np.uint64)
    assert np.array_equal(rc.unmix64(rc.mix64(x)), x) and np.array_equal(rc.mix64(rc.unmix64(x)), x)
    assert np.array_equal(rc.word_of_digest(rc.word_digest(x, i), i), x) and np.array_equal(rc.word_digest(rc.word_of_digest(x, i), i), x)
    for level, bits in ((0, 1), (3, 1), (3, 2), (12, 2)):
        assert np.array_equal(rc.block_key(rc.digest_of_key(x, level, bits), level, bits), x)
    assert [rc.py_mix64(int(v)) for v in x[:2000]] == rc.mix64(x[:2000]).tolist()
    blocks = [rc.random_block(rng, n) for n in (8, 16, 64, 1024)] + [(1, 2, np.array([0x0D], np.uint8)), (2, 1, np.array([7, 9], np.uint8))]
    assert [rc.py_block_key(b, l, f) for l, f, b in blocks] == rc.keys_of(blocks).tolist()


def test_constructor_claims():
    """twins differ in exactly two words and share the digest; keys land in the slot asked for; cross-key blocks are of the other (level, format)
    under the same key; the all-ones key can be had at 8 bytes and above -- checked here from outside the constructors' own assertions"""
    rng = np.random.default_rng(13)
    for nbytes in (16, 32, 64, 256, 16384):
        n = nbytes // 8
        a = rc.random_block(rng, nbytes)
        for p, q in rc.sweep_pairs(n)[:40]:
            for i, j in ((p, q), (q, p)):
                b = rc.twin_block(a, i, j, 1 << int(rng.integers(0, 64)))
                diff = np.nonzero(rc.words_of(a[2]) != rc.words_of(b[2]))[0].tolist()
                assert diff == sorted((i, j)) and rc.keys_of([a])[0] == rc.keys_of([b])[0] and b[:2] == a[:2]
    for slots in (1024, 2048, 262144):
        for home in (0, 511, slots - 1):
            key = rc.key_in_slot(home, slots, rng)
            b = rc.with_key(key, 3, 2, rng)
            assert int(rc.hash_slot_of(rc.keys_of([(3, 2, b)])[0], slots)) == home
    a = rc.random_block(rng, 64)
    for level, bits in ((3, 2), (3, 1), (5, 2)):
        b = rc.cross_key(a[2], 4, 2, level, bits, rng)
        assert len(b) == rc.block_bytes(level, bits) and rc.keys_of([(level, bits, b)])[0] == rc.keys_of([a])[0]
    for small in (rc.random_block(rng, 8), rc.random_block(rng, 16)):     # the larger block begins with the smaller one's bytes
        big = rc.cross_key(small[2], small[0], small[1], 4, 2, rng, share_prefix=True)
        assert bytes(big[:len(small[2])]) == bytes(small[2]) and rc.keys_of([(4, 2, big)])[0] == rc.keys_of([small])[0]
    for nbytes in (8, 64):
        level, bits = rc.KIND_OF_BYTES[nbytes]
        assert int(rc.keys_of([(level, bits, rc.with_key(rc.EMPTY_KEY, level, bits, rng))])[0]) == rc.EMPTY_KEY
    with pytest.raises(AssertionError):
        rc.with_key(5, 2, 2, rng)                                          # 4 bytes: no 64 free bits
    sizes = {n: len(rc.sweep_pairs(n // 8)) for n in (16, 32, 64, 128, 16384)}
    assert sizes[16] == 1 and sizes[32] == 6 and sizes[64] == 28 and sizes[128] >= 24 and sizes[16384] >= 24
    for n in (16, 2048):                                                   # every vector and half of a turn, the first turn and the last, alone
        pairs = rc.sweep_pairs(n)
        for v in range(4):
            assert (2 * v, 2 * v + 1) in pairs and (n - 8 + 2 * v, n - 7 + 2 * v) in pairs
        assert any(i % 2 == j % 2 == 1 for i, j in pairs) and any(i % 2 == j % 2 == 0 for i, j in pairs) and (0, n - 1) in pairs
        assert all(any(i % 8 == w == j % 8 for i, j in pairs) for w in range(8))


# ---- the merge rule against the merge by bytes ----
def _items_of(blocks):
    return [(level, bits, lu.pack(states, bits)) for states, level, bits in blocks]


def _collision_free_tables():
    """tables of the kind the coarsen, combine and gather tests use: planted states, copies, uniform blocks, the tables of their duplicate tests"""
    rng = np.random.default_rng(14)
    a, b, c = cu.planted_states(4, 2, 21), cu.planted_states(4, 2, 25), cu.planted_states(6, 2, 23)
    one, same = np.array([1, 0, 1, 1], np.uint8), np.array([1, 3, 0, 0], np.uint8)
    tables = [
        [(b, 4, 2), (a, 4, 2), (a, 4, 2), (np.repeat(a, 4), 5, 2), (one, 1, 1), (np.full(256, 3, np.uint8), 4, 2),
         (c, 6, 2), (a, 4, 2), (same, 1, 2), (b, 4, 2), (np.full(256, 3, np.uint8), 4, 2), (one, 1, 1)],                          # test_gather_gpu
        [(a, 4, 2), (a, 4, 2), (np.repeat(a, 4), 5, 2), (c, 6, 2), (same, 1, 2), (np.repeat(same, 4), 2, 2), (b, 4, 2), (b, 4, 2), (c, 6, 2)],   # test_combine_gpu
        [(cu.planted_states(6, 2, 1), 6, 2), (a, 4, 2), (a, 4, 2), (a, 4, 2), (one, 1, 1), (same, 1, 2), (same, 1, 2)],            # test_coarsen_gpu, at cap 4
    ]
    pool = [(cu.planted_states(level, bits, seed), level, bits) for level in range(6) for bits in (1, 2) for seed in range(6)]
    for _ in range(6):
        tables.append([pool[int(k)] for k in rng.integers(0, len(pool), 200)])
    return tables


def test_the_rule_is_the_byte_merge_where_nothing_collides():
    for blocks in _collision_free_tables():
        items = _items_of(blocks)
        by_key = rc.merge_under_keys(items).tolist()
        assert by_key == rc.merge_by_bytes(items) == rc.merge_under_keys_loop(items)
        assert len(set(by_key)) < len(items)                               # (every table has duplicates)
        table = cu.table_of_blocks(blocks, first_offset=3, gap=1)
        index = np.concatenate([np.arange(len(blocks)), np.arange(len(blocks))[::-1], [-1, -4]])
        for flags in (0, 1, 2):
            want = cu.restate_coarsen(*table, index, ot.IDX_U32, 12, 3, flags)
            got = cu.restate_coarsen(*table, index, ot.IDX_U32, 12, 3, flags, merge=rc.merge_under_keys)
            assert want["info"] == got["info"]
            cu.assert_same(got, want)
            want = gt.restate_gather([table + (index, None)] * 2, None, flags)
            got = gt.restate_gather([table + (index, None)] * 2, None, flags, merge=rc.merge_under_keys)
            assert want["info"] == got["info"]
            cu.assert_same(got, want)
        want = mu.restate_combine([table + (index, None), table + (index[::-1], None)], 2, 3)
        got = mu.restate_combine([table + (index, None), table + (index[::-1], None)], 2, 3, merge=rc.merge_under_keys)
        assert want["info"] == got["info"]
        cu.assert_same(got, want)


COLLISION_TABLES = [("core", rc.core_table), ("empty8", lambda: rc.empty_key_table(8)), ("empty64", lambda: rc.empty_key_table(64)),
                    ("sweep16", lambda: rc.sweep_table(16)), ("sweep64", lambda: rc.sweep_table(64)), ("sweep1024", lambda: rc.sweep_table(1024)),
                    ("chain", lambda: rc.chain_table(1023, 1024)), ("divergence", lambda: rc.divergence_table(500))]


@pytest.mark.parametrize("name,make", COLLISION_TABLES, ids=[n for n, _ in COLLISION_TABLES])
def test_the_rule_differs_exactly_in_the_copies_of_rejected_blocks(name, make):
    """on the tables of the GPU tests: the byte merge finds a representative for every copy; under the rule the copy of a block that was itself
    rejected by its candidate stands alone.  The items where the two differ are counted, and each is the later copy of an item that shares its key
    with a lower, different item; a loop over Python integers states the rule a second time"""
    items, merges = make()[:2]
    items = [it for it in items if not rc.is_uniform(it[2], it[1])]        # (what enters the table with default flags)
    by_key, by_bytes = rc.merge_under_keys(items), np.array(rc.merge_by_bytes(items))
    assert by_key.tolist() == rc.merge_under_keys_loop(items)
    differ = np.nonzero(by_key != by_bytes)[0]
    keys = rc.keys_of(items)
    for t in differ.tolist():
        first = int(np.nonzero(keys == keys[t])[0][0])
        assert by_key[t] == t and first < by_bytes[t] < t and bytes(items[first][2]) != bytes(items[t][2])
    stands_alone = len(set(by_key.tolist()))
    assert int((by_key != np.arange(len(items))).sum()) == merges == len(items) - stands_alone
    expected_witnesses = {"core": 10 + 2, "empty8": 0, "empty64": 1, "chain": 3}.get(name, merges)   # (one B' per quad; the chain's three twins)
    assert len(differ) == expected_witnesses, (name, len(differ))


@pytest.mark.parametrize("name,make", COLLISION_TABLES, ids=[n for n, _ in COLLISION_TABLES])
def test_the_vectorised_answer_is_the_restatements_answer(name, make):
    """rebuild_cases.expected_verbatim, which answers the 70 001-block table of the GPU tests in a fraction of a second, equals restate_gather and
    restate_coarsen (cap 12) under the same rule on smaller tables of the same make, with every flag"""
    items = make()[0]
    table = rc.table_of_bytes(items)
    index = np.concatenate([np.arange(len(items)), np.arange(len(items))[::-7]])
    for flags in (0, 1, 2, 3):
        want = rc.expected_verbatim(items, index, flags)
        got = gt.restate_gather([table + (index, None)], None, flags, merge=rc.merge_under_keys)
        cu.assert_same(got, want)
        assert {k: got["info"][k] for k in want["info"]} == want["info"]
        got = cu.restate_coarsen(*table, index, ot.IDX_U32, 12, 3, flags, merge=rc.merge_under_keys)
        got["index"] = got["index"].astype(np.int32)
        cu.assert_same(got, want)
        assert {k: got["info"][k] for k in want["info"]} == want["info"]
