"""Shared by tests/test_rebuild_reference.py and tests/test_rebuild_gpu.py: the digest, key and slot arithmetic of the derived-result tail restated
from the text of omm_amd/csrc/result_words.h and hash_build.h (numpy uint64, vectorised; nothing is imported from the product, and
tests/native/rebuild_hash_check.cpp holds the restatement to the headers' own functions), the inverses of that arithmetic, constructors of blocks
that collide where random data never does -- in the digest, in the key across (level, format), in the key with the all-ones value, in the home slot --
and the merge rule of rebuild_resolve as a model: the candidate of a block is the LOWEST item under its key, and nothing else is ever compared.

A block here is its bytes (uint8); every size is a power of two of 8 bytes and more, so a block is whole 64-bit words.  Any bytes are a valid block of
either format.  Every constructor asserts what it claims through the restated functions, and that its block is not uniform: a uniform block becomes a
special index and never enters the table."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15            # word_digest's index constant and hash_slot_of's multiplier
MIX_A, MIX_B = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
KIND = 0xD6E8FEB86659FD93              # block_key's (level, format) constant
EMPTY_KEY = M64                        # kEmptyKey
GOLDEN_INV, MIX_A_INV, MIX_B_INV = (pow(c, -1, 1 << 64) for c in (GOLDEN, MIX_A, MIX_B))
KIND_OF_BYTES = {8: (3, 1), 16: (3, 2), 32: (4, 1), 64: (4, 2), 128: (5, 1), 256: (5, 2), 512: (6, 1), 1024: (6, 2), 2048: (7, 1), 4096: (7, 2),
                 8192: (8, 1), 16384: (8, 2)}


def u64(x):
    return np.asarray(x, dtype=np.uint64)


def _c(x):
    return np.uint64(x)


def block_bytes(level, bits):
    return max(1, 4 ** level * bits // 8)


# ---- the arithmetic of the two headers, and its inverses ----
def mix64(x):
    with np.errstate(over="ignore"):
        x = u64(x)
        x = x ^ (x >> _c(30))
        x = x * _c(MIX_A)
        x = x ^ (x >> _c(27))
        x = x * _c(MIX_B)
        return x ^ (x >> _c(31))


def unmix64(y):
    """mix64 is a bijection: y = x ^ (x >> s) is undone by x = y ^ (y >> s) ^ (y >> 2s) for 3s >= 64, an odd multiplier by its inverse mod 2^64"""
    with np.errstate(over="ignore"):
        y = u64(y)
        y = y ^ (y >> _c(31)) ^ (y >> _c(62))
        y = y * _c(MIX_B_INV)
        y = y ^ (y >> _c(27)) ^ (y >> _c(54))
        y = y * _c(MIX_A_INV)
        return y ^ (y >> _c(30)) ^ (y >> _c(60))


def _index_salt(index):
    with np.errstate(over="ignore"):
        return (u64(index) + _c(1)) * _c(GOLDEN)


def word_digest(w, index):
    return mix64(u64(w) ^ _index_salt(index))


def word_of_digest(d, index):
    """the word w with word_digest(w, index) == d"""
    return unmix64(d) ^ _index_salt(index)


def words_of(blocks):
    """(m, bytes) or (bytes,) uint8 -> (m, words) or (words,) uint64, the last word padded with zeros"""
    b = np.asarray(blocks, np.uint8)
    pad = (-b.shape[-1]) % 8
    if pad:
        b = np.concatenate([b, np.zeros(b.shape[:-1] + (pad,), np.uint8)], axis=-1)
    return np.ascontiguousarray(b).view("<u8").astype(np.uint64)


def bytes_of(words):
    return np.ascontiguousarray(u64(words).astype("<u8")).view(np.uint8)


def digest_of_words(words):
    words = u64(words)
    return word_digest(words, np.arange(words.shape[-1], dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def block_digest(blocks):
    """the sum of word_digest over the block's 64-bit words"""
    return digest_of_words(words_of(blocks))


def _kind_salt(level, bits):
    with np.errstate(over="ignore"):
        return ((u64(level) << _c(2)) | u64(bits)) * _c(KIND)


def block_key(digest, level, bits):
    with np.errstate(over="ignore"):
        return mix64(u64(digest) + _kind_salt(level, bits))


def digest_of_key(key, level, bits):
    """the digest d with block_key(d, level, bits) == key"""
    with np.errstate(over="ignore"):
        return unmix64(key) - _kind_salt(level, bits)


def hash_table_slots(n):
    s = 1024
    while s < 2 * n and s < 0x80000000:
        s <<= 1
    return s


def hash_slot_of(key, slots):
    """the home slot of a key other than the all-ones key (that one lives in the dedicated slot `slots`)"""
    with np.errstate(over="ignore"):
        return ((u64(key) * _c(GOLDEN)) >> _c(64 - (slots.bit_length() - 1))).astype(np.int64)


# the same arithmetic once more on Python integers, for the second statement of the merge rule
def py_mix64(x):
    x ^= x >> 30
    x = x * MIX_A & M64
    x ^= x >> 27
    x = x * MIX_B & M64
    return x ^ (x >> 31)


def py_block_key(block, level, bits):
    b = bytes(np.asarray(block, np.uint8).tobytes())
    b += b"\0" * (-len(b) % 8)
    digest = 0
    for i in range(len(b) // 8):
        digest = (digest + py_mix64(int.from_bytes(b[8 * i:8 * i + 8], "little") ^ ((i + 1) * GOLDEN & M64))) & M64
    return py_mix64((digest + ((level << 2) | bits) * KIND) & M64)


# ---- constructors ----
def is_uniform(block, bits):
    b = np.asarray(block, np.uint8)
    return bool((b == b[0]).all()) and int(b[0]) in ((0x00, 0xFF) if bits == 1 else (0x00, 0x55, 0xAA, 0xFF))


def _not_uniform(words, bits):
    for row in np.atleast_2d(bytes_of(words)):
        assert not is_uniform(row, bits), "a uniform block never enters the table"


def random_words(rng, nwords, count=None):
    return rng.integers(0, 1 << 64, nwords if count is None else (count, nwords), dtype=np.uint64)


def with_digest(words, digest):
    """words (n,) or (m, n) with the LAST word solved so that the block's digest is `digest` (one value, or one per row)"""
    with np.errstate(over="ignore"):
        out = u64(words).copy()
        n = out.shape[-1]
        rest = digest_of_words(out[..., :n - 1]) if n > 1 else _c(0)
        out[..., n - 1] = word_of_digest(u64(digest) - rest, n - 1)
    assert np.array_equal(digest_of_words(out), np.broadcast_to(u64(digest), out.shape[:-1]))
    return out


def twin(words, i, j, flip, bits=2):
    """a block with the digest of `words` that differs from it in word i (by xor with `flip`, not zero) and in word j (solved) and nowhere else.
    words (n,) with integers i, j, flip, or (m, n) with one i, j, flip per row"""
    with np.errstate(over="ignore"):
        a = np.atleast_2d(u64(words))
        rows = np.arange(len(a))
        i, j, flip = (np.broadcast_to(np.asarray(v, t), (len(a),)) for v, t in ((i, np.int64), (j, np.int64), (flip, np.uint64)))
        assert (i != j).all() and (flip != 0).all()
        b = a.copy()
        b[rows, i] ^= flip
        owed = word_digest(a[rows, i], i) - word_digest(b[rows, i], i)
        b[rows, j] = word_of_digest(word_digest(a[rows, j], j) + owed, j)
    differs = a != b
    assert np.array_equal(digest_of_words(a), digest_of_words(b)) and (differs.sum(axis=1) == 2).all() and differs[rows, i].all() and differs[rows, j].all()
    _not_uniform(b, bits)
    return b.reshape(np.shape(words))


def with_key(key, level, bits, rng, prefix=None):
    """the bytes of a block of (level, format) whose key is `key`: random words (behind the bytes of `prefix`, if given), the last one solved"""
    nbytes = block_bytes(level, bits)
    assert nbytes >= 8 and nbytes % 8 == 0, "a block below 8 bytes has no 64 free bits"
    words = random_words(rng, nbytes // 8)
    if prefix is not None:
        assert len(prefix) % 8 == 0 and len(prefix) < nbytes
        words[:len(prefix) // 8] = words_of(prefix)
    words = with_digest(words, digest_of_key(key, level, bits))
    assert prefix is None or bytes_of(words)[:len(prefix)].tobytes() == bytes(prefix)
    assert int(block_key(digest_of_words(words), level, bits)) == int(key)
    _not_uniform(words, bits)
    return bytes_of(words)


def key_in_slot(slot, slots, rng):
    """a key whose home slot in a table of `slots` is `slot`: the slot in the top bits of key * GOLDEN, random bits below, times GOLDEN's inverse"""
    shift = 64 - (slots.bit_length() - 1)
    key = ((slot << shift) | int(rng.integers(0, 1 << shift, dtype=np.uint64))) * GOLDEN_INV & M64
    assert key != EMPTY_KEY and int(hash_slot_of(key, slots)) == slot
    return key


def cross_key(block_a, level_a, bits_a, level_b, bits_b, rng, share_prefix=False):
    """a block of (level_b, bits_b) under the key of block_a, which is of another (level, format).  share_prefix: the larger block_b begins with
    the bytes of block_a, so that a comparison over block_a's size alone would call them equal"""
    assert (level_a, bits_a) != (level_b, bits_b)
    key = block_key(block_digest(block_a), level_a, bits_a)
    b = with_key(key, level_b, bits_b, rng, prefix=np.asarray(block_a, np.uint8) if share_prefix else None)
    assert int(block_key(block_digest(b), level_b, bits_b)) == int(key) and len(b) == block_bytes(level_b, bits_b)
    return b


def random_block(rng, nbytes):
    """-> (level, bits, bytes): an ordinary block, not uniform"""
    level, bits = KIND_OF_BYTES[nbytes]
    b = bytes_of(random_words(rng, nbytes // 8))
    assert not is_uniform(b, bits)
    return level, bits, b


def twin_block(item, i, j, flip=1):
    level, bits, b = item
    return level, bits, bytes_of(twin(words_of(b), i, j, flip, bits))


# ---- the merge rule ----
def keys_of(items):
    """the restated key of every item of [(level, bits, bytes)]"""
    keys = np.zeros(len(items), np.uint64)
    kinds = {}
    for t, (level, bits, b) in enumerate(items):
        kinds.setdefault((level, bits, len(b)), []).append(t)
    for (level, bits, _), ts in kinds.items():
        keys[ts] = block_key(block_digest(np.stack([items[t][2] for t in ts])), level, bits)
    return keys


def merge_under_keys(items):
    """items: [(level, bits, bytes)] in item order -> the representative of each (an item number).  An item's candidate is the lowest item with
    the same key; the item merges into it iff the candidate is lower and equal in level, format and bytes, otherwise it stands for itself"""
    n = len(items)
    leader = np.arange(n)
    if not n:
        return leader
    _, first, inverse = np.unique(keys_of(items), return_index=True, return_inverse=True)
    cand = first[inverse.reshape(-1)]
    kind = np.array([(level, bits) for level, bits, _ in items], np.int64)
    maybe = np.nonzero((cand < leader) & (kind[cand] == kind).all(axis=1))[0]
    for key in {tuple(k) for k in kind[maybe].tolist()}:
        ts = maybe[(kind[maybe] == key).all(axis=1)]
        equal = (np.stack([items[t][2] for t in ts]) == np.stack([items[c][2] for c in cand[ts]])).all(axis=1)
        leader[ts[equal]] = cand[ts[equal]]
    return leader


def merge_under_keys_loop(items):
    """the same rule as a plain loop over Python integers"""
    lowest, leader = {}, []
    for t, (level, bits, b) in enumerate(items):
        lowest.setdefault(py_block_key(b, level, bits), t)
    for t, (level, bits, b) in enumerate(items):
        c = lowest[py_block_key(b, level, bits)]
        same = c < t and (items[c][0], items[c][1]) == (level, bits) and bytes(items[c][2]) == bytes(b)
        leader.append(c if same else t)
    return leader


def merge_by_bytes(items):
    """what the restatements of the three entries do by default: the first item equal in level, format and bytes"""
    seen, leader = {}, []
    for t, (level, bits, b) in enumerate(items):
        leader.append(seen.setdefault((level, bits, bytes(b)), t))
    return leader


# ---- tables ----
def table_of_bytes(items, first_offset=0, filler=0xA5):
    """[(level, bits, bytes)] -> (array_data, descs (D, 3)), packed without gaps behind first_offset bytes"""
    offsets = first_offset + np.concatenate([[0], np.cumsum([len(b) for _, _, b in items])[:-1]]).astype(np.int64)
    array = np.concatenate([np.full(first_offset, filler, np.uint8)] + [np.asarray(b, np.uint8) for _, _, b in items])
    return array, np.stack([offsets, [l for l, _, _ in items], [f for _, f, _ in items]], 1).astype(np.int64)


def expected_verbatim(items, index, flags=0):
    """What the tail answers for one source whose blocks pass through verbatim (a gather, a coarsening at cap 12): the model of this module without
    the unpacking and repacking of the three restatements, vectorised for tables of 10^5 blocks.  items: [(level, bits, bytes)] of 8 bytes and more;
    index: entries 0 .. len(items) - 1 -> dict like restate_gather's, info without the fields that only one entry has"""
    index = np.asarray(index, np.int64)
    used = np.unique(index)
    level, bits = (np.array([it[k] for it in items], np.int64) for k in (0, 1))
    size = np.array([len(it[2]) for it in items], np.int64)
    uniform = np.array([is_uniform(items[t][2], items[t][1]) for t in used], bool)
    promoted = uniform & (not flags & 1)
    kept = used[~promoted]
    leader = np.arange(len(kept)) if flags & 2 else merge_under_keys([items[t] for t in kept])
    rep = kept[leader]
    emitted = kept[rep == kept]
    emitted = emitted[np.lexsort((emitted, -size[emitted]))]
    place = np.full(len(items), -1, np.int64)
    place[emitted] = np.arange(len(emitted))
    entry = np.full(len(items), -4, np.int64)
    entry[kept] = place[rep]
    for t in used[promoted]:
        b0 = int(items[t][2][0])
        entry[t] = -((b0 & (1 if items[t][1] == 1 else 3)) + 1)
    offsets = np.concatenate([[0], np.cumsum(size[emitted])[:-1]]).astype(np.int64) if len(emitted) else np.zeros(0, np.int64)
    array = np.concatenate([items[t][2] for t in emitted]) if len(emitted) else np.zeros(0, np.uint8)
    array_hist, index_hist = {}, {}
    uses = np.bincount(index, minlength=len(items))
    for t in emitted:
        array_hist[(int(level[t]), int(bits[t]))] = array_hist.get((int(level[t]), int(bits[t])), 0) + 1
    for t in kept:
        index_hist[(int(level[t]), int(bits[t]))] = index_hist.get((int(level[t]), int(bits[t])), 0) + int(uses[t])
    info = dict(arrayDataSize=len(array), descArrayCount=len(emitted), referencedBlocks=len(used), uniformBlocks=int(uniform.sum()),
                duplicateBlocks=int((rep != kept).sum()), skippedPrimitives=0)
    return dict(array=array, descs=np.stack([offsets, level[emitted], bits[emitted]], 1).astype(np.int64).reshape(-1, 3), index=entry[index].astype(np.int32),
                array_hist=array_hist, index_hist=index_hist, info=info)


# ---- the cases of the GPU tests (built here so that the non-GPU tests hold the model to the restatements on the same tables) ----
def quad(rng, nbytes, i, j, b_first=False):
    """A, B = twin(A) in words i and j, A' == A, B' == B -- or B, A, A', B'.  One of the four merges: the copy of whichever comes first"""
    a = random_block(rng, nbytes)
    b = twin_block(a, i, j, int(rng.integers(1, 1 << 64, dtype=np.uint64)))
    return [b, a, a, b] if b_first else [a, b, a, b]


def core_table(seed=1):
    """the table of the core test: twin quads of 16, 32, 64, 256 and 1024 bytes in both orders, the two cross-key triples, a uniform pair and a few
    ordinary blocks between them -> (items, number of items that merge)"""
    rng = np.random.default_rng(seed)
    items, merges = [], 0
    for nbytes in (16, 32, 64, 256, 1024):
        n = nbytes // 8
        items += quad(rng, nbytes, 0, n - 1) + [random_block(rng, nbytes)] + quad(rng, nbytes, n // 2, n // 2 - 1, b_first=True)
        merges += 2
    for nbytes in (16, 8):                                        # a level-4 4-state A, and B of 16 / of 8 bytes under A's key, B' == B behind it;
        b = random_block(rng, nbytes)                             # B's bytes are the first bytes of A: only level and format tell them apart
        a = (4, 2, cross_key(b[2], b[0], b[1], 4, 2, rng, share_prefix=True))
        items += [a, b, b]
    uniform = (4, 2, np.full(64, 0x55, np.uint8))
    items += [uniform, random_block(rng, 8), uniform]
    return items, merges


def empty_key_table(nbytes, seed=2):
    """ordinary blocks around a block E whose key is the all-ones key, its exact copy and, for 64 bytes, its twin and the twin's copy; a block X in
    front of E and a block Y behind it whose keys have the home slot that the slot arithmetic would give the all-ones key if it were ever asked (a
    tail that probed for that key would take an empty slot for it and lose it to X or Y), with copies of X and Y at the end
    -> (items, number of items that merge, the places of E and its kin)"""
    rng = np.random.default_rng(seed + nbytes)
    level, bits = KIND_OF_BYTES[nbytes]
    home = int(hash_slot_of(EMPTY_KEY, 1024))
    x, y = ((level, bits, with_key(key_in_slot(home, 1024, rng), level, bits, rng)) for _ in range(2))
    e = (level, bits, with_key(EMPTY_KEY, level, bits, rng))
    items = [x, random_block(rng, nbytes), e, random_block(rng, nbytes), e]
    places = [2, 4]
    if nbytes >= 16:
        t = twin_block(e, 1, nbytes // 8 - 1, 1 << 40)
        items += [random_block(rng, nbytes), t, t]
        places += [6, 7]
    items += [y, x, y, random_block(rng, nbytes)]
    assert hash_table_slots(len(items)) == 1024 and [int(k) == EMPTY_KEY for k in keys_of(items)] == [t in places for t in range(len(items))]
    return items, 3, places


def sweep_pairs(nwords):
    """the word pairs (i, j) of the position sweep: every pair up to eight words; beyond, both words in each vector of the first and of the last
    turn, each position of a turn in two turns, both in the lower / in the upper halves of vectors, the last two words, the first and the last"""
    if nwords <= 8:
        return [(i, j) for i in range(nwords) for j in range(i + 1, nwords)]
    last = nwords - 8
    pairs = [(2 * v, 2 * v + 1) for v in range(4)] + [(last + 2 * v, last + 2 * v + 1) for v in range(4)] + [(w, last + w) for w in range(8)]
    pairs += [(0, 2), (4, 6), (1, 3), (5, 7), (last, last + 2), (last + 5, last + 7), (0, nwords - 1), (7, 8), (last - 1, last)]
    return sorted(set(pairs))


def sweep_table(nbytes, seed=3):
    rng = np.random.default_rng(seed + nbytes)
    items = []
    for i, j in sweep_pairs(nbytes // 8):
        items += quad(rng, nbytes, i, j)
    return items, len(items) // 4


def chain_table(home, slots, seed=4):
    """300 distinct 16-byte blocks whose keys all have the home slot `home` of `slots`; behind them an exact copy of the 1st, the 150th and the 300th,
    each followed by a twin of it and the twin's copy -> (items, number of items that merge)"""
    rng = np.random.default_rng(seed + home)
    keys = []
    while len(keys) < 300:
        k = key_in_slot(home, slots, rng)
        if k not in keys:
            keys.append(k)
    items = [(3, 2, with_key(k, 3, 2, rng)) for k in keys]
    assert (hash_slot_of(keys_of(items), slots) == home).all() and len(set(keys_of(items).tolist())) == 300
    for n in (0, 149, 299):
        t = twin_block(items[n], 0, 1, 1 << (n % 64))
        items += [items[n], t, t]
    return items, 3


def divergence_table(groups, seed=5):
    """`groups` quads of 256-byte blocks (A, B = twin(A) differing first in word k, A', B'), k from group to group over the four turns, then every
    item at a seeded place: whichever member of a quad comes first is the candidate of the other three, its copy merges and the other two are kept
    -> (items, number of items that merge)"""
    rng = np.random.default_rng(seed)
    a = random_words(rng, 32, groups)
    k = (np.arange(groups) * 11) % 31
    j = k + 1 + (rng.integers(0, 32, groups) % (31 - k))
    b = twin(a, k, j, rng.integers(1, 1 << 64, groups, dtype=np.uint64))
    rows = bytes_of(np.stack([a, b, a, b], 1).reshape(-1, 32))
    extra = random_block(rng, 256)
    order = rng.permutation(4 * groups)
    return [(5, 2, rows[t]) for t in order] + [extra], groups
