// rebuild_hash_check.cpp -- holds the restatement in tests/rebuild_cases.py to the tail's own arithmetic, without a device: it reads blocks with the
// digest, key, slot count and home slot that the Python side expects and recomputes each with mix64 / word_digest / block_key (result_words.h) and
// hash_table_slots / hash_table_at / hash_slot_of (hash_build.h).  Host code only (hipcc -x hip --offload-host-only), under ASan and UBSan.
//
//   file:    "RBHASH01", u64 count, then per record
//            u32 level, u32 bits, u64 bytes, u64 items, u32 slots, u32 slot, u64 digest, u64 key, the block's bytes padded with zeros to whole words
//   slot:    the home slot of the key in a table of hash_table_slots(items); for the all-ones key the dedicated slot, whose index is `slots`
//   output:  "rebuild_hash_check: <records> records, <mismatches> mismatches"; exit status 1 with any mismatch or a malformed file
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "result_words.h"
#include "hash_build.h"

using namespace ommx;

struct Record { uint32_t level, bits; uint64_t bytes, items; uint32_t slots, slot; uint64_t digest, key; };

static unsigned long long g_bad = 0;
static void expect(bool ok, unsigned long long record, const char* what, unsigned long long got, unsigned long long want)
{
    if (ok) return;
    if (g_bad++ < 20) fprintf(stderr, "record %llu: %s is %#llx, the file says %#llx\n", record, what, got, want);
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: rebuild_hash_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[8]; uint64_t count = 0;
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "RBHASH01", 8) != 0 || fread(&count, 8, 1, f) != 1) { fprintf(stderr, "not a case file\n"); return 2; }
    std::vector<uint64_t> words;
    std::vector<uint8_t> memory;
    for (uint64_t r = 0; r < count; ++r) {
        Record rec;
        if (fread(&rec, sizeof rec, 1, f) != 1 || rec.bytes == 0 || rec.bytes > (1u << 22)) { fprintf(stderr, "record %llu is cut short\n", (unsigned long long)r); return 2; }
        words.assign((size_t)((rec.bytes + 7) / 8), 0);
        if (fread(words.data(), 8, words.size(), f) != words.size()) { fprintf(stderr, "record %llu is cut short\n", (unsigned long long)r); return 2; }
        uint64_t digest = 0;
        for (size_t i = 0; i < words.size(); ++i) digest += word_digest(words[i], i);
        expect(digest == rec.digest, r, "the digest", digest, rec.digest);
        const uint64_t key = block_key(digest, rec.level, rec.bits);
        expect(key == rec.key, r, "the key", key, rec.key);
        const uint32_t slots = hash_table_slots(rec.items);
        expect(slots == rec.slots, r, "the slot count", slots, rec.slots);
        // the table over real memory of hash_table_bytes(): the slot that the key starts at must hold a value inside it
        if (memory.size() != hash_table_bytes(slots)) memory.assign(hash_table_bytes(slots), 0);
        const HashTable t = hash_table_at(memory.data(), slots);
        expect(t.mask == slots - 1u, r, "the mask", t.mask, slots - 1u);
        const uint32_t slot = key == kEmptyKey ? t.mask + 1u : hash_slot_of(t, key);
        expect(slot == rec.slot, r, "the slot", slot, rec.slot);
        expect(slot <= slots && (key == kEmptyKey) == (slot == slots), r, "the slot's range", slot, slots);
        const uint8_t* value = (const uint8_t*)(t.vals + slot);
        expect(value >= memory.data() + (size_t)slots * 8 && value + 4 <= memory.data() + memory.size(), r, "the value's place", (unsigned long long)(value - memory.data()), memory.size());
        memory[(size_t)(value - memory.data()) + 3] = 1;   // (a write that ASan sees if the place is outside)
    }
    uint8_t extra;
    if (fread(&extra, 1, 1, f) == 1) { fprintf(stderr, "bytes behind the last record\n"); return 2; }
    fclose(f);
    printf("rebuild_hash_check: %llu records, %llu mismatches\n", (unsigned long long)count, g_bad);
    return g_bad ? 1 : 0;
}
