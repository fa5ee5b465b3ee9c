// Scalar model of the device codec (tail_kernels.hip: codec_code / shard_codec_write), shared by the native host tests.
#pragma once
#include "../../omm_amd/csrc/host_expand.h"
#include <cstring>
#include <vector>

// the codec stream of src[0 .. padded): header 16 B (not filled) | first raw unit per block | one nibble per unit | the raw units; 64 bytes of slack behind
static inline std::vector<uint8_t> encode(const std::vector<uint8_t>& src, const ommx::HostCodecLayout& L)
{
    std::vector<uint8_t> stream(L.offRaw + 16 * L.units + 64, 0xEE);
    uint32_t* ofs = (uint32_t*)(stream.data() + L.offOfs); uint32_t nraw = 0;
    for (uint64_t u = 0; u < L.units; ++u) {
        if (u % 256 == 0) ofs[u / 256] = nraw;
        uint32_t w[4]; memcpy(w, &src[u * 16], 16);
        const bool same = w[0] == w[1] && w[0] == w[2] && w[0] == w[3];
        const uint32_t code = !same ? 4u : (w[0] == 0u ? 0u : (w[0] == 0x55555555u ? 1u : (w[0] == 0xAAAAAAAAu ? 2u : (w[0] == 0xFFFFFFFFu ? 3u : 4u))));
        uint8_t& c = stream[L.offCodes + u / 2];
        c = (uint8_t)((u & 1) ? ((c & 0x0F) | (code << 4)) : code);
        if (code == 4u) { memcpy(&stream[L.offRaw + 16ull * nraw], w, 16); ++nraw; }
    }
    ofs[L.blocks] = nraw;
    return stream;
}
