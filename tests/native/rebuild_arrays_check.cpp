// The arrays that ommxCoarsenMicromap, ommxCombineMicromaps and ommxGatherMicromaps hand to the tail (omm_amd/csrc/rebuild_arrays.h), carved between
// an operation's own slots as the three do it; built with AddressSanitizer and UBSan by tests/test_rebuild_arrays.py.  Each shape is carved twice, from a
// null base (the size to reserve) and over an exact-size heap block in which every slot is then written end to end: a slot that is not aligned, overlaps
// its neighbour, holds fewer elements than its users index, or runs over the reservation stops the program.  Prints "ok <number of checks>".
#include "rebuild_arrays.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace ommx;

static long g_checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } ++g_checks; } while (0)

static size_t p256(size_t b) { return (b + 255) / 256 * 256; }   // (written differently from the header's on purpose)

struct Slot { const char* name; uintptr_t at; size_t bytes; };
struct Carved { Slot slot[9]; TailArrays t; size_t bytes; };
// an operation's scratch: a header and its marks in front (as the coarsening and the gather have them), a list behind
static Carved carve(uintptr_t base, size_t n, size_t temp, size_t tail)
{
    Carved c; CarveCursor at{ base };
    uint32_t* header = at.take<uint32_t>(4); uint32_t* marks = at.take<uint32_t>(n);
    c.t = carve_tail_arrays(at, n, temp, tail);
    uint32_t* list = at.take<uint32_t>(n);
    c.bytes = (size_t)(at.at - base);
    const TailArrays& t = c.t;
    const Slot s[9] = { { "header", (uintptr_t)header, 16 }, { "marks", (uintptr_t)marks, 4 * n }, { "item", (uintptr_t)t.item, 4 * n },
                        { "slotStart", (uintptr_t)t.slotStart, 8 * (n + 1) }, { "units", (uintptr_t)t.units, 8 * (n + 1) }, { "digest", (uintptr_t)t.digest, 8 * n },
                        { "umask", (uintptr_t)t.umask, 4 * n }, { "temp", (uintptr_t)t.temp, temp }, { "tailScratch", (uintptr_t)t.tailScratch, tail } };
    memcpy(c.slot, s, sizeof s);
    (void)list;
    return c;
}

int main()
{
    const size_t items[6] = { 0, 1, 255, 256, 257, 65537 }, temps[3] = { 0, 1, 4096 }, tails[2] = { 0, 256 };
    for (size_t n : items) for (size_t temp : temps) for (size_t tail : tails) {
        const Carved sized = carve(0, n, temp, tail);                                  // the sizing pass: offsets from a null base
        uint8_t* block = (uint8_t*)aligned_alloc(256, sized.bytes);                     // (exact size: a slot that runs over is the sanitizer's to report)
        CHECK(block != nullptr, "allocation of %zu bytes", sized.bytes);
        const Carved c = carve((uintptr_t)block, n, temp, tail);
        CHECK(c.bytes == sized.bytes && c.t.bytes == sized.t.bytes && c.t.tempBytes == temp, "both passes agree on the sizes");
        for (int k = 0; k < 9; ++k) {
            const Slot& s = c.slot[k];
            CHECK(s.at % 256 == 0, "%s is 256-aligned", s.name);
            CHECK(s.at - (uintptr_t)block == sized.slot[k].at, "%s: the sizing pass walks the same offsets", s.name);
            if (k < 8) CHECK(s.at + s.bytes <= c.slot[k + 1].at, "%s ends before %s begins", s.name, c.slot[k + 1].name);
            memset((void*)s.at, k + 1, s.bytes);
        }
        // the closing elements that the scans read and write
        c.t.slotStart[n] = 1; c.t.units[n] = 2;
        CHECK(c.t.slotStart[n] == 1 && c.t.units[n] == 2 && (n == 0 || (c.t.item[n - 1] == 0x03030303u && c.t.umask[n - 1] == 0x07070707u)), "slotStart and units hold n + 1 elements");
        // one memset clears an operation's header and the marks behind it
        CHECK(c.slot[1].at == c.slot[0].at + 256, "the marks follow the header");
        // the hand-written sum of coarsen_layout, gather_layout and tuple_layout's common part
        const size_t common = p256(4 * n) + 2 * p256(8 * (n + 1)) + p256(8 * n) + p256(4 * n) + p256(temp) + p256(tail);
        CHECK(c.t.bytes == common, "%zu bytes for the tail's arrays, %zu by hand", c.t.bytes, common);
        CHECK(c.bytes == 256 + p256(4 * n) + common + p256(4 * n), "%zu bytes in all", c.bytes);
        CHECK(c.slot[8].at + p256(tail) + p256(4 * n) == (uintptr_t)block + c.bytes, "the list behind ends with the reservation");
        memset((void*)(c.slot[8].at + p256(tail)), 0x55, 4 * n);
        free(block);
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
