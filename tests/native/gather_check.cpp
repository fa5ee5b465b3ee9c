// Host check of the address and shift arithmetic of ommxGatherMicromaps' copy (omm_amd/csrc/gather_copy.h compiled as plain C++) against a byte loop:
//   1. the 128-bit byte shifts gather_down / gather_up for every shift 1..15 on random words;
//   2. gather_vector for every source misalignment 0..15 x every length 1..80 bytes, and for 256, 4096 and 4097 bytes: every output vector equals the
//      block's bytes (zeros behind its end), and NO byte outside the block is read.  Two witnesses of that: the block ends where its heap allocation of
//      exactly misalignment + length bytes ends, so a read behind it is an AddressSanitizer report (a read in front of the allocation too); and every
//      read of the header passes through OMMX_GATHER_READ, which holds it to [block, block + length) -- the bytes in front of a misaligned block share
//      its allocation, where the sanitizer cannot see them;
//   3. gather_small for the block sizes below 16 bytes at every misalignment: the unused bits of a one-byte block are cleared, whatever they held.
// Built and run by tests/test_gather.py:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I omm_amd/csrc tests/native/gather_check.cpp -o gather_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const uint8_t* g_lo = nullptr;
static const uint8_t* g_hi = nullptr;
static unsigned long long g_outside = 0, g_reads = 0;
static void witness(const uint8_t* p, uint32_t n) { g_reads++; if (n && (p < g_lo || p + n > g_hi)) g_outside++; }
#define OMMX_GATHER_READ(p, n) witness((p), (n))
#include "gather_copy.h"

using namespace ommx;

static unsigned long long g_checked = 0, g_bad = 0;
#define EXPECT(cond, ...) do { g_checked++; if (!(cond)) { if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t g_seed = 0x243F6A8885A308D3ull;
static uint64_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

static void check_shifts()
{
    for (int trial = 0; trial < 20000; ++trial) {
        GatherWords x; x.w0 = rnd(); x.w1 = rnd();
        uint8_t b[16];
        memcpy(b, &x.w0, 8); memcpy(b + 8, &x.w1, 8);
        for (uint32_t n = 1; n <= 15; ++n) {
            uint8_t down[16] = { 0 }, up[16] = { 0 };
            for (uint32_t i = 0; i + n < 16; ++i) { down[i] = b[i + n]; up[i + n] = b[i]; }
            const GatherWords d = gather_down(x, n), u = gather_up(x, n);
            EXPECT(memcmp(&d.w0, down, 8) == 0 && memcmp(&d.w1, down + 8, 8) == 0, "gather_down by %u bytes", n);
            EXPECT(memcmp(&u.w0, up, 8) == 0 && memcmp(&u.w1, up + 8, 8) == 0, "gather_up by %u bytes", n);
        }
    }
}

// a block of `len` random bytes at `mis` modulo 16 that ends where its allocation ends
struct Placed {
    uint8_t* base; const uint8_t* block; size_t len;
    Placed(uint32_t mis, size_t n) : len(n)
    {
        base = (uint8_t*)malloc(mis + n);                    // (16-byte aligned: checked below)
        for (size_t i = 0; i < mis + n; ++i) base[i] = (uint8_t)rnd();
        block = base + mis;
        g_lo = block; g_hi = block + n;
    }
    ~Placed() { g_lo = g_hi = nullptr; free(base); }
};

static void check_vectors(uint32_t mis, size_t len)
{
    const Placed p(mis, len);
    EXPECT(((uintptr_t)p.base & 15u) == 0u && gather_shift(p.block) == mis, "the allocator's alignment: %p", (void*)p.base);
    const unsigned long long before = g_outside;
    for (uint64_t j = 0; 16u * j < len; ++j) {
        uint8_t want[16] = { 0 };
        for (uint32_t b = 0; b < 16u && 16u * j + b < len; ++b) want[b] = p.block[16u * j + b];
        const GatherWords got = gather_vector(p.block, len, j);
        EXPECT(memcmp(&got.w0, want, 8) == 0 && memcmp(&got.w1, want + 8, 8) == 0, "misalignment %u, length %zu, vector %llu: %016llx %016llx", mis, len,
               (unsigned long long)j, (unsigned long long)got.w0, (unsigned long long)got.w1);
    }
    EXPECT(g_outside == before, "misalignment %u, length %zu: %llu reads outside the block", mis, len, g_outside - before);
}

static void check_small(uint32_t mis)
{
    for (uint32_t level = 0; level <= 3; ++level)
        for (uint32_t bits = 1; bits <= 2; ++bits) {
            const uint32_t used = bits << (2 * level), bytes = used < 8 ? 1 : used / 8;
            if (bytes >= 16) continue;
            for (int trial = 0; trial < 64; ++trial) {
                const Placed p(mis, bytes);
                uint64_t want = 0;
                for (uint32_t b = 0; b < bytes; ++b) want |= (uint64_t)p.block[b] << (8 * b);
                if (used < 8) want &= (1ull << used) - 1;
                const unsigned long long before = g_outside;
                const uint64_t got = gather_small(p.block, bytes, level, bits);
                EXPECT(got == want && g_outside == before, "small block, misalignment %u, level %u, %u bits: %016llx, want %016llx", mis, level, bits,
                       (unsigned long long)got, (unsigned long long)want);
            }
        }
}

int main()
{
    check_shifts();
    for (uint32_t mis = 0; mis < 16; ++mis) {
        for (size_t len = 1; len <= 80; ++len) check_vectors(mis, len);
        check_vectors(mis, 256); check_vectors(mis, 4096); check_vectors(mis, 4097);
        check_small(mis);
    }
    EXPECT(g_reads > 10000, "the witness saw only %llu reads", g_reads);
    printf("gather_check: %llu checks, %llu reads witnessed, %llu failures\n", g_checked, g_reads, g_bad);
    return g_bad ? 1 : 0;
}
