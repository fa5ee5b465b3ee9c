// host_tail_check.cpp -- omm_amd/csrc/host_tail.cpp, compiled unchanged, on work items read from a case file (tests/test_host_tail_reference.py writes
// it from the oracle's decode of a bake and compares what comes back with the oracle's own result, byte for byte).  Built with
// -fsanitize=address,undefined: every case also runs under both sanitizers.
//
//   host_tail_check <cases.bin> <results.bin>
//
// cases.bin, little endian, any number of cases one after the other:
//   u32 magic 0x4c544f48 | i32 format | i32 disableSpecial, disableDedup, nearDup, nearDupBrute | f32 rejectionThreshold, nearDupFactor
//   | u32 maxArrayDataSize, numTris | i32 unresolved | u32 numItems
//   per item: u32 level | i32 format | f32 uv[6] | u32 numPrims | u32 prims[numPrims] | i32 uniform | (uniform < 0) u8 packed[max(1, 4^level / 4)]
// results.bin, per case:
//   i32 returned | u32 arrayDataSize, bytes | u32 numDescs, 8 bytes each | u32 arrayHist entries, 8 bytes each | u32 indexHist entries, 8 bytes each
//   | u32 numIndex, i32 each
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../omm_amd/csrc/host_tail.h"

namespace {
bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T> bool get(FILE* f, T& v) { return rd(f, &v, sizeof v); }
void wr(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { fprintf(stderr, "short write\n"); exit(3); } }
template <class T> void put(FILE* f, const T& v) { wr(f, &v, sizeof v); }
void fail(const char* what) { fprintf(stderr, "host_tail_check: %s\n", what); exit(2); }
}

int main(int argc, char** argv)
{
    static_assert(sizeof(ommCpuOpacityMicromapDesc) == 8 && sizeof(ommCpuOpacityMicromapUsageCount) == 8, "result records are written as they lie in memory");
    if (argc != 3) fail("usage: host_tail_check <cases.bin> <results.bin>");
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) fail("cannot open the files");
    uint32_t cases = 0;
    for (;;) {
        uint32_t magic;
        if (!get(in, magic)) break;
        if (magic != 0x4c544f48u) fail("bad magic");
        ommx::HostTailDesc d; int32_t fmt, fl[4], unresolved; uint32_t numItems;
        if (!get(in, fmt) || !rd(in, fl, sizeof fl) || !get(in, d.rejectionThreshold) || !get(in, d.nearDupFactor) || !get(in, d.maxArrayDataSize)
            || !get(in, d.numTris) || !get(in, unresolved) || !get(in, numItems)) fail("short header");
        d.format = fmt; d.disableSpecial = fl[0] != 0; d.disableDedup = fl[1] != 0; d.nearDup = fl[2] != 0; d.nearDupBrute = fl[3] != 0; d.unresolved = unresolved;
        std::vector<ommx::HostItem> items(numItems);
        for (ommx::HostItem& it : items) {
            int32_t ifmt, uniform; uint32_t np;
            if (!get(in, it.level) || !get(in, ifmt) || !rd(in, it.uv, sizeof it.uv) || !get(in, np)) fail("short item");
            if (it.level > 12 || (ifmt != 1 && ifmt != 2)) fail("item out of range");
            it.format = ifmt; it.prims.resize(np);
            if (!rd(in, it.prims.data(), sizeof(uint32_t) * np) || !get(in, uniform)) fail("short item");
            for (uint32_t p : it.prims) if (p >= d.numTris) fail("triangle out of range");
            it.uniform = uniform;
            if (uniform > 3) fail("uniform state out of range");
            if (uniform < 0) {
                const size_t n = (size_t)1 << (2 * it.level);
                it.packed.resize(n >= 4 ? n / 4 : 1);
                if (!rd(in, it.packed.data(), it.packed.size())) fail("short states");
            }
        }
        ommx::HostTailResult res;
        const int32_t rc = ommx::run_host_tail(d, items, res);
        put(out, rc);
        if (rc != 0) { res = ommx::HostTailResult(); }
        put(out, (uint32_t)res.arrayData.size()); wr(out, res.arrayData.data(), res.arrayData.size());
        put(out, (uint32_t)res.descs.size()); wr(out, res.descs.data(), 8 * res.descs.size());
        put(out, (uint32_t)res.arrayHist.size()); wr(out, res.arrayHist.data(), 8 * res.arrayHist.size());
        put(out, (uint32_t)res.indexHist.size()); wr(out, res.indexHist.data(), 8 * res.indexHist.size());
        put(out, (uint32_t)res.index.size()); wr(out, res.index.data(), 4 * res.index.size());
        ++cases;
    }
    fclose(in);
    if (fclose(out) != 0) fail("close failed");
    printf("ok %u\n", cases);
    return 0;
}
