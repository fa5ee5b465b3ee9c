// Host check of ommxReorientMicromap's map and tile code (omm_amd/csrc/reorient_map.h compiled as plain C++) against the statement of the rule,
// ommx_reorient_index of include/omm_mi355x_lookup.h:
//   1. the walk and the tile tables: the source index that the kernel's path forms for an output index -- reorient_walk over the digits above the
//      tile, then `node` and the emitted digit of the node's state -- equals ommx_reorient_index: every index of levels 0..9 under all six
//      orientations; at levels 10..12 indices at a stride and the first and last field of every tile;
//   2. the tiles on bytes: blocks of levels 3..7 in both formats at every source misalignment 0..15 under every orientation, written tile by tile
//      with reorient_source_tile and reorient_tile2 / reorient_tile4, equal the block permuted field by field; blocks of levels 0..2 through
//      reorient_small.  The block ends where its heap allocation of exactly misalignment + size bytes ends, so a read behind it is an
//      AddressSanitizer report, and every read passes through OMMX_GATHER_READ, which holds it to the block (tests/native/gather_check.cpp).
// Built and run by tests/test_reorient.py:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -I include -I omm_amd/csrc tests/native/reorient_check.cpp -o reorient_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static const uint8_t* g_lo = nullptr;
static const uint8_t* g_hi = nullptr;
static unsigned long long g_outside = 0, g_reads = 0;
static void witness(const uint8_t* p, uint32_t n) { g_reads++; if (n && (p < g_lo || p + n > g_hi)) g_outside++; }
#define OMMX_GATHER_READ(p, n) witness((p), (n))
#include "reorient_map.h"
#include "omm_mi355x_lookup.h"

using namespace ommx;

static unsigned long long g_checked = 0, g_bad = 0;
#define EXPECT(cond, ...) do { g_checked++; if (!(cond)) { if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t g_seed = 0x243F6A8885A308D3ull;
static uint64_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

static ReorientTables g_tables;

// the source index as the kernel's path forms it
static uint32_t path_index(uint32_t index, uint32_t level, uint32_t o)
{
    uint32_t state = o;
    if (level < kReorientTileDepth) return reorient_walk(index, level, &state);
    const uint32_t from = reorient_walk(index >> 6, level - kReorientTileDepth, &state);
    const uint32_t nd = g_tables.node[state][(index >> 2) & 15u];
    return (from << 6) | ((nd & 15u) << 2) | (reorient_code(nd >> 4, index & 3u) & 3u);
}

static void check_map()
{
    for (uint32_t level = 0; level <= 12; ++level)
        for (uint32_t o = 0; o < 6; ++o) {
            const uint32_t n = 1u << (2 * level);
            if (level <= 9) {
                for (uint32_t j = 0; j < n; ++j) EXPECT(path_index(j, level, o) == ommx_reorient_index(j, level, o), "level %u, orientation %u, index %u", level, o, j);
            } else {
                for (uint32_t j = 0; j < n; j += 61) EXPECT(path_index(j, level, o) == ommx_reorient_index(j, level, o), "level %u, orientation %u, index %u", level, o, j);
                for (uint32_t tile = 0; tile < n / 64; ++tile)
                    for (uint32_t j = 64 * tile; j < 64 * tile + 64; j += 63)
                        EXPECT(path_index(j, level, o) == ommx_reorient_index(j, level, o), "level %u, orientation %u, index %u", level, o, j);
            }
        }
}

struct Placed {   // a block of `len` random bytes at `mis` modulo 16 that ends where its allocation ends
    uint8_t* base; const uint8_t* block; size_t len;
    Placed(uint32_t mis, size_t n) : len(n)
    {
        base = (uint8_t*)malloc(mis + n);
        for (size_t i = 0; i < mis + n; ++i) base[i] = (uint8_t)rnd();
        block = base + mis;
        g_lo = block; g_hi = block + n;
    }
    ~Placed() { g_lo = g_hi = nullptr; free(base); }
};

static uint32_t field(const uint8_t* block, uint32_t i, uint32_t bits) { return (block[(i * bits) >> 3] >> ((i * bits) & 7u)) & ((1u << bits) - 1u); }

static void check_tiles(uint32_t mis)
{
    for (uint32_t level = 0; level <= 7; ++level)
        for (uint32_t bits = 1; bits <= 2; ++bits) {
            const uint32_t fields = 1u << (2 * level), used = bits * fields;
            const size_t bytes = used < 8 ? 1 : used / 8;
            const Placed p(mis, bytes);
            EXPECT(((uintptr_t)p.base & 15u) == 0u, "the allocator's alignment: %p", (void*)p.base);
            for (uint32_t o = 1; o < 6; ++o) {
                const unsigned long long before = g_outside;
                std::vector<uint8_t> out(bytes < 16 ? 16 : bytes, 0);
                if (level < kReorientTileDepth) {
                    const uint64_t w = reorient_small(gather_small(p.block, (uint32_t)bytes, level, bits), level, bits, o);
                    memcpy(out.data(), &w, 8);
                    EXPECT(used >= 8 || (w >> used) == 0, "level %u, %u bits: unused bits set", level, bits);
                } else {
                    const uint32_t digits = level - kReorientTileDepth;
                    for (uint32_t tile = 0; tile < (1u << (2 * digits)); ++tile) {
                        uint32_t state = o;
                        const uint32_t from = reorient_walk(tile, digits, &state);
                        const GatherWords x = reorient_source_tile(p.block, bytes, bits, from);
                        if (bits == 2) { const GatherWords y = reorient_tile4(&g_tables, state, x); memcpy(&out[16 * (size_t)tile], &y.w0, 8); memcpy(&out[16 * (size_t)tile + 8], &y.w1, 8); }
                        else { const uint64_t y = reorient_tile2(&g_tables, state, x.w0); memcpy(&out[8 * (size_t)tile], &y, 8); }
                    }
                }
                unsigned long long wrong = 0;
                for (uint32_t j = 0; j < fields; ++j) wrong += field(out.data(), j, bits) != field(p.block, ommx_reorient_index(j, level, o), bits);
                EXPECT(wrong == 0 && g_outside == before, "misalignment %u, level %u, %u bits, orientation %u: %llu fields differ, %llu reads outside the block", mis, level,
                       bits, o, wrong, g_outside - before);
            }
        }
}

int main()
{
    for (uint32_t i = 0; i < kReorientTableEntries; ++i) reorient_tables_fill(&g_tables, i);
    check_map();
    for (uint32_t mis = 0; mis < 16; ++mis) check_tiles(mis);
    EXPECT(g_reads > 10000, "the witness saw only %llu reads", g_reads);
    printf("reorient_check: %llu checks, %llu reads witnessed, %llu failures\n", g_checked, g_reads, g_bad);
    return g_bad ? 1 : 0;
}
