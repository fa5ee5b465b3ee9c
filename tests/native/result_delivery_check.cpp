// The integer rules of ommCpuBake's result delivery (omm_amd/csrc/host_expand.h: carve_codec_block, plan_codec_slices, last_slice_needed, the expansion's
// tasks) at the smallest cases at which each can go wrong, against the arithmetic they replaced -- restated here, not taken from the header.  Built with
// AddressSanitizer and UBSan by tests/test_result_delivery_host.py.  Prints "ok <number of checks>".
#include "codec_model.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ommx;

static long g_checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } ++g_checks; } while (0)

static uint64_t s = 0x9E3779B97F4A7C15ull;   // (fixed seed)
static uint64_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static size_t p256(size_t b) { return (b + 255) / 256 * 256; }   // (written differently from the header's on purpose)

// the layout of a codec stream as the device computes it (tail_kernels.hip: codec_layout), restated
struct Lay { uint64_t padded, units, blocks, offOfs, offCodes, offRaw, cap; };
static Lay lay_of(uint64_t arrayBytes)
{
    Lay l; l.padded = (arrayBytes + 255) / 256 * 256; l.units = l.padded / 16; l.blocks = (l.units + 255) / 256; l.offOfs = 16;
    l.offCodes = (l.offOfs + 4 * (l.blocks + 1) + 15) / 16 * 16; l.offRaw = (l.offCodes + (l.units + 1) / 2 + 15) / 16 * 16;
    l.cap = l.offRaw + l.padded / 2 + 16;
    return l;
}

// ---- the device block of a codec stream: size word (256 B) | scan scratch | [unit codes | block raw counts] | the stream ----
static void codec_block_carve()
{
    const uint64_t M = 1ull << 20;
    const uint64_t sizes[6] = { 16, 4096, 4096 + 16, 32 * M, 32 * M + 16, 1024 * M };
    const size_t scratches[3] = { 0, 256, 4352 };
    for (uint64_t bytes : sizes) for (size_t scratch : scratches) for (int withCodes = 0; withCodes < 2; ++withCodes) {
        // what ommCpuBake summed by hand before the carve existed
        const Lay l = lay_of(bytes);
        const size_t codeBytes = withCodes ? p256((size_t)(l.padded / 16)) : 0, countBytes = withCodes ? p256(((size_t)l.blocks + 1) * 4) : 0;
        const size_t offScratch = 256, offCodes = 256 + scratch, offCounts = offCodes + codeBytes, offStream = 256 + scratch + codeBytes + countBytes;
        const size_t total = offStream + (size_t)l.cap;
        // the sizing pass: pointers are offsets
        const CodecBlockCarve z = carve_codec_block(0, bytes, scratch, withCodes != 0);
        CHECK(z.bytes == total, "bytes %zu, the hand sum gives %zu (array %llu scratch %zu codes %d)", z.bytes, total, (unsigned long long)bytes, scratch, withCodes);
        CHECK((uintptr_t)z.sizeWord == 0 && (uintptr_t)z.scratch == offScratch && (uintptr_t)z.stream == offStream, "size word / scratch / stream offsets");
        if (withCodes) CHECK((uintptr_t)z.unitCodes == offCodes && (uintptr_t)z.blockRawCounts == offCounts, "codes / counts offsets");
        else CHECK(z.unitCodes == nullptr && z.blockRawCounts == nullptr, "no code slots without codes");
        CHECK(((uintptr_t)z.scratch | (uintptr_t)z.unitCodes | (uintptr_t)z.blockRawCounts | (uintptr_t)z.stream) % 256 == 0, "slots start at 256-byte boundaries");
        // in the stated order, none reaching into the next
        bool apart = (uintptr_t)z.sizeWord + 4 <= (uintptr_t)z.scratch && (uintptr_t)z.scratch + scratch <= (withCodes ? (uintptr_t)z.unitCodes : (uintptr_t)z.stream);
        if (withCodes) apart = apart && (uintptr_t)z.unitCodes + l.padded / 16 <= (uintptr_t)z.blockRawCounts && (uintptr_t)z.blockRawCounts + (l.blocks + 1) * 4 <= (uintptr_t)z.stream;
        CHECK(apart, "slots are disjoint and in order");
        CHECK((uintptr_t)z.stream + l.cap == z.bytes, "the reservation ends with the stream slot");
        if (bytes > 32 * M + 16) continue;   // (sizing only: a heap block of half a gigabyte per shape is out of proportion)
        // over an exact-size heap block: every slot is filled in full -- a byte past the reservation stops the program -- and keeps its own bytes
        uint8_t* block = (uint8_t*)malloc(z.bytes);
        const CodecBlockCarve c = carve_codec_block((uintptr_t)block, bytes, scratch, withCodes != 0);
        CHECK((uint8_t*)c.sizeWord == block && c.scratch == block + offScratch && c.stream == block + offStream && c.bytes == z.bytes &&
              (!withCodes || (c.unitCodes == block + offCodes && (uint8_t*)c.blockRawCounts == block + offCounts)), "pointers are the base plus the offsets");
        memset(c.sizeWord, 1, 256); memset(c.scratch, 2, scratch); memset(c.stream, 5, (size_t)l.cap);
        if (withCodes) { memset(c.unitCodes, 3, (size_t)(l.padded / 16)); memset(c.blockRawCounts, 4, ((size_t)l.blocks + 1) * 4); }
        bool kept = block[0] == 1 && block[255] == 1 && (!scratch || (c.scratch[0] == 2 && c.scratch[scratch - 1] == 2)) && c.stream[0] == 5 && c.stream[l.cap - 1] == 5;
        if (withCodes) kept = kept && c.unitCodes[0] == 3 && c.unitCodes[l.padded / 16 - 1] == 3 && ((uint8_t*)c.blockRawCounts)[0] == 4 && ((uint8_t*)c.blockRawCounts)[(l.blocks + 1) * 4 - 1] == 4;
        CHECK(kept, "every slot keeps what was written into it");
        free(block);
    }
}

// ---- the cut of a codec stream into slices, and the expansion's tasks ----
static const uint64_t kBlockCounts[8] = { 1, 11, 12, 13, 511, 512, 513, 6145 };
static HostCodecLayout layout_of_blocks(uint64_t blocks) { return host_codec_layout(blocks * 4096); }
// table 0: every unit raw, 1: none, 2: random monotone
static std::vector<uint32_t> offset_table(uint64_t blocks, int kind)
{
    std::vector<uint32_t> ofs(blocks + 1, 0u);
    for (uint64_t b = 0; b < blocks; ++b) ofs[b + 1] = ofs[b] + (kind == 0 ? 256u : (kind == 1 ? 0u : (uint32_t)(rnd() % 257)));
    return ofs;
}
static uint64_t stream_bytes(const Lay& l, const std::vector<uint32_t>& ofs) { return l.offRaw + 16ull * ofs.back(); }

static void slice_plans()
{
    for (uint64_t blocks : kBlockCounts) {
        const HostCodecLayout L = layout_of_blocks(blocks); const Lay l = lay_of(blocks * 4096);
        for (int kind = 0; kind < 3; ++kind) {
            const std::vector<uint32_t> ofs = offset_table(blocks, kind);
            const uint64_t streamBytes = stream_bytes(l, ofs);
            const CodecSlicePlan P = plan_codec_slices(L, ofs.data(), streamBytes);
            CHECK(P.ok, "a monotone table that ends at the stream's length is accepted (blocks %llu table %d)", (unsigned long long)blocks, kind);
            bool blocksTile = P.blockCut[0] == 0 && P.blockCut[12] == blocks, codesTile = P.slice[0].c0 == l.offCodes && P.slice[11].c1 == l.offRaw;
            bool rawTile = P.slice[0].r0 == l.offRaw && P.slice[11].r1 == l.offRaw + 16ull * ofs[blocks];
            for (int k = 0; k < 12; ++k) {   // (empty slices are legal: a range may have no bytes, but never a negative number of them)
                blocksTile = blocksTile && P.blockCut[k] <= P.blockCut[k + 1];
                codesTile = codesTile && P.slice[k].c0 <= P.slice[k].c1 && (k == 11 || P.slice[k].c1 == P.slice[k + 1].c0);
                rawTile = rawTile && P.slice[k].r0 <= P.slice[k].r1 && (k == 11 || P.slice[k].r1 == P.slice[k + 1].r0);
            }
            CHECK(blocksTile, "block ranges tile [0, blocks)");
            CHECK(codesTile, "code ranges tile [offCodes, offRaw)");
            CHECK(rawTile, "raw ranges tile [offRaw, offRaw + 16 ofs[blocks])");
            // the loop ommCpuBake ran inline before the plan existed
            bool same = true, okOld = true;
            uint64_t blockCut[13];
            for (uint32_t k = 0; k <= 12; ++k) blockCut[k] = l.blocks * k / 12;
            for (uint32_t k = 0; okOld && k < 12; ++k) {
                const uint64_t b0 = blockCut[k], b1 = blockCut[k + 1];
                const uint64_t c0b = l.offCodes + b0 * 128u, c1b = b1 == l.blocks ? l.offRaw : l.offCodes + b1 * 128u;
                const uint64_t r0b = l.offRaw + 16ull * ofs[b0], r1b = l.offRaw + 16ull * ofs[b1];
                okOld = r0b <= r1b && r1b <= streamBytes;
                same = same && P.blockCut[k] == b0 && P.blockCut[k + 1] == b1 && P.slice[k].c0 == c0b && P.slice[k].c1 == c1b && P.slice[k].r0 == r0b && P.slice[k].r1 == r1b;
            }
            CHECK(same && okOld, "the plan equals the inline arithmetic it replaced");
        }
        // a corrupt table must not turn into a wild copy: an entry AT a slice cut that decreases, a last entry beyond the stream
        std::vector<uint32_t> bad = offset_table(blocks, 0);
        bad[blocks * 11 / 12] = bad[blocks] + 1;   // (the first block of the last slice)
        CHECK(!plan_codec_slices(L, bad.data(), ~0ull).ok, "a decreasing entry at a cut is rejected (blocks %llu)", (unsigned long long)blocks);
        const std::vector<uint32_t> raw = offset_table(blocks, 0);
        CHECK(!plan_codec_slices(L, raw.data(), stream_bytes(l, raw) - 16).ok, "a last entry beyond the stream is rejected (blocks %llu)", (unsigned long long)blocks);
        // A decreasing entry strictly INSIDE a slice is accepted, as it always was: the plan reads the table at the cuts only, and the copies it describes stay
        // inside the stream whatever the entries between two cuts say (the expansion then reads raw units from the wrong place inside the staging block, not
        // outside it).  Block counts below 13 have no such entry: every block starts a slice.
        const CodecSlicePlan P = plan_codec_slices(L, raw.data(), stream_bytes(l, raw));
        for (int k = 1; k < 12; ++k) if (P.blockCut[k + 1] - P.blockCut[k] >= 2) {   // (from slice 1: the entry in front of the dip is then above zero)
            std::vector<uint32_t> dip = raw;
            dip[P.blockCut[k] + 1] = dip[P.blockCut[k]] - 1;
            CHECK(plan_codec_slices(L, dip.data(), stream_bytes(l, dip)).ok, "a decreasing entry inside a slice is accepted (blocks %llu)", (unsigned long long)blocks);
            break;
        }
    }
}

static void tasks_and_slices()
{
    for (uint64_t blocks : kBlockCounts) {
        const HostCodecLayout L = layout_of_blocks(blocks);
        const std::vector<uint32_t> ofs = offset_table(blocks, 1);
        const CodecSlicePlan P = plan_codec_slices(L, ofs.data(), L.offRaw);
        const uint64_t tasks = codec_task_count(L);
        bool tile = tasks == (blocks + 511) / 512;
        uint64_t next = 0;
        for (uint64_t t = 0; t < tasks; ++t) {
            uint64_t s0, s1; codec_task_range(L, t, &s0, &s1);
            tile = tile && s0 == next && s0 < s1 && s1 - s0 <= 512; next = s1;
            // the slice a block lies in: the one k with blockCut[k] <= b < blockCut[k + 1]
            const uint32_t need = last_slice_needed(P, s1);
            bool covered = need < 12; uint32_t last = 0;
            for (uint64_t b = s0; b < s1; ++b) {
                uint32_t k = 0; while (!(P.blockCut[k] <= b && b < P.blockCut[k + 1])) ++k;
                covered = covered && k <= need; last = k;
            }
            CHECK(covered && last == need, "task %llu of %llu blocks waits for slice %u, its last block lies in slice %u", (unsigned long long)t, (unsigned long long)blocks, need, last);
        }
        CHECK(tile && next == blocks, "tasks tile [0, blocks) in steps of 512 (blocks %llu)", (unsigned long long)blocks);
    }
}

// a stream of the scalar codec model, delivered the way ommCpuBake delivers it: the head first, then a task's slices only when the task asks for them
static void round_trip()
{
    static const uint8_t pat[4] = { 0x00, 0x55, 0xAA, 0xFF };
    for (uint64_t blocks : { (uint64_t)13, (uint64_t)513 }) {
        const size_t padded = (size_t)blocks * 4096, bytes = padded - 48;   // (the array ends inside the last 256-byte pad)
        std::vector<uint8_t> src(padded, 0);
        for (size_t o = 0; o < bytes; ) {   // runs of a repeated state byte with raw noise in between
            size_t len = 16 * (1 + rnd() % 700);
            if (o + len > bytes) len = bytes - o;
            if (rnd() % 6 == 0) for (size_t k = 0; k < len; ++k) src[o + k] = (uint8_t)rnd(); else memset(&src[o], pat[rnd() % 4], len);
            o += len;
        }
        const HostCodecLayout L = host_codec_layout(padded);
        const std::vector<uint8_t> stream = encode(src, L);
        const uint32_t* ofs = (const uint32_t*)(stream.data() + L.offOfs);
        const uint64_t streamBytes = L.offRaw + 16ull * ofs[L.blocks];
        std::vector<uint8_t> host((size_t)streamBytes + 4096, 0xEE);   // (the pinned staging block: the stream's size + 4096)
        memcpy(host.data(), stream.data(), (size_t)L.offCodes);        // the head
        const CodecSlicePlan P = plan_codec_slices(L, (const uint32_t*)(host.data() + L.offOfs), streamBytes);
        CHECK(P.ok, "the model's table is accepted");
        std::vector<uint8_t> out(bytes + 16, 0xCD);
        uint32_t arrived = 0;
        for (uint64_t t = 0; t < codec_task_count(L); ++t) {
            uint64_t s0, s1; codec_task_range(L, t, &s0, &s1);
            for (const uint32_t need = last_slice_needed(P, s1); arrived <= need; ++arrived) {
                const CodecSlicePlan::Slice& c = P.slice[arrived];
                memcpy(host.data() + c.c0, stream.data() + c.c0, (size_t)(c.c1 - c.c0)); memcpy(host.data() + c.r0, stream.data() + c.r0, (size_t)(c.r1 - c.r0));
            }
            codec_expand_blocks(out.data(), bytes, host.data(), L, s0, s1);
        }
        bool clean = true; for (int k = 0; k < 16; ++k) clean = clean && out[bytes + k] == 0xCD;
        CHECK(memcmp(out.data(), src.data(), bytes) == 0 && clean, "the expansion in plan order gives the source array (blocks %llu)", (unsigned long long)blocks);
    }
}

int main()
{
    codec_block_carve();
    slice_plans();
    tasks_and_slices();
    round_trip();
    printf("ok %ld\n", g_checks);
    return 0;
}
