// Holds the numpy codec encoder of tests/shard_cases.py to code it did not come from: the host expansion of omm_amd/csrc/host_expand.cpp.
// Reads a file of cases written by tests/test_shard_reference.py -- per case: uint64 original bytes (a multiple of 256), uint64 stream bytes, the
// original bytes, the stream -- checks the stream's header and layout against host_codec_layout, expands every stream with codec_expand_blocks (all
// blocks in one call, and block by block into a destination at an odd address: the unaligned store path) and compares with the original bytes.
// Stand-alone, built with -fsanitize=address,undefined: exact-size heap blocks, so a read or write past a stream or a destination is an error.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -Iomm_amd/csrc tests/native/codec_stream_check.cpp omm_amd/csrc/host_expand.cpp -o /tmp/codec_stream_check
//   /tmp/codec_stream_check cases.bin
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "host_expand.h"

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: codec_stream_check cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    unsigned cases = 0; uint64_t bytes = 0;
    for (;;) {
        uint64_t head[2];
        if (fread(head, 1, sizeof head, f) != sizeof head) break;
        const uint64_t n = head[0], sn = head[1];
        // exact-size blocks; the destination gets one more byte in front for the unaligned run
        uint8_t* orig = (uint8_t*)malloc(n ? n : 1); uint8_t* stream = (uint8_t*)malloc(sn ? sn : 1);
        uint8_t* out = (uint8_t*)aligned_alloc(64, n ? (n + 63) / 64 * 64 : 64); uint8_t* odd = (uint8_t*)malloc(n + 1);
        if (!orig || !stream || !out || !odd || !read_exact(f, orig, n) || !read_exact(f, stream, sn)) { fprintf(stderr, "case %u: short file\n", cases); return 2; }
        const ommx::HostCodecLayout L = ommx::host_codec_layout(n);
        uint64_t h[2]; memcpy(h, stream, 16);
        const uint32_t* ofs = (const uint32_t*)(stream + L.offOfs);
        if (n % 256 != 0 || sn < L.offRaw || h[0] != sn || h[1] != L.units || ofs[0] != 0 || L.offRaw + 16ull * ofs[L.blocks] != sn) {
            fprintf(stderr, "case %u: header / layout mismatch: %llu bytes, stream %llu, header %llu / %llu, units %llu, offRaw %llu, raw units %u\n", cases,
                    (unsigned long long)n, (unsigned long long)sn, (unsigned long long)h[0], (unsigned long long)h[1], (unsigned long long)L.units,
                    (unsigned long long)L.offRaw, ofs[L.blocks]);
            return 1;
        }
        memset(out, 0xCD, n ? n : 1); memset(odd, 0xCD, n + 1);
        ommx::codec_expand_blocks(out, n, stream, L, 0, L.blocks);
        for (uint64_t b = 0; b < L.blocks; ++b) ommx::codec_expand_blocks(odd + 1, n, stream, L, b, b + 1);
        if (memcmp(out, orig, n) != 0 || memcmp(odd + 1, orig, n) != 0 || odd[0] != 0xCD) {
            uint64_t k = 0; while (k < n && out[k] == orig[k] && odd[1 + k] == orig[k]) ++k;
            fprintf(stderr, "case %u: expansion differs from the original at byte %llu of %llu\n", cases, (unsigned long long)k, (unsigned long long)n);
            return 1;
        }
        free(orig); free(stream); free(out); free(odd);
        ++cases; bytes += n;
    }
    fclose(f);
    printf("ok %u streams %llu bytes\n", cases, (unsigned long long)bytes);
    return 0;
}
