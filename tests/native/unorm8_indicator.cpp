// The UNORM8 indicator of the summed-area table, compiled by the host compiler: the texel as the texture load returns it,
//     (float)byte * (1.f / 255.f),
// compared with the cut-off by `>`.  tests/test_sat_reference.py holds the numpy expression of tests/sat_util.py to this one for
// all 256 byte values.  Arguments: cut-offs as the hex bit patterns of their float32 values; one line of 256 '0' / '1' per cut-off.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv)
{
    for (int a = 1; a < argc; ++a) {
        const uint32_t bits = (uint32_t)strtoul(argv[a], nullptr, 16);
        float cutoff;
        memcpy(&cutoff, &bits, 4);
        char line[257];
        for (int b = 0; b < 256; ++b) {
            volatile float alpha = (float)(uint8_t)b * (1.f / 255.f);   // volatile: rounded to float32 here, whatever the target keeps in registers
            line[b] = alpha > cutoff ? '1' : '0';
        }
        line[256] = 0;
        puts(line);
    }
    return 0;
}
