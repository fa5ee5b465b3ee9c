// A user of the SDK's own omm.h (C++: that header is not valid C).  tests/test_abi_exports.py links it against libomm-lib.so where
// the SDK headers exist; the omm* symbols it references are recorded in tests/golden/sdk_user_symbols.txt (make_fixtures.py).
#include <omm.h>
int main() {
    ommBakerCreationDesc bd = ommBakerCreationDescDefault(); bd.type = ommBakerType_CPU;
    ommBaker baker = 0; if (ommCreateBaker(&bd, &baker) != ommResult_SUCCESS) return 1;
    ommCpuTextureDesc td = ommCpuTextureDescDefault(); ommCpuTexture tex = 0; (void)ommCpuCreateTexture(baker, &td, &tex);
    ommCpuBakeInputDesc in = ommCpuBakeInputDescDefault(); ommCpuBakeResult res = 0; (void)ommCpuBake(baker, &in, &res);
    const ommCpuBakeResultDesc* out = 0; (void)ommCpuGetBakeResultDesc(res, &out);
    ommDebugStats st = ommDebugStatsDefault(); (void)ommDebugGetStats(baker, out, &st);
    ommCpuDeserializedDesc dd = ommCpuDeserializedDescDefault(); ommCpuSerializedResult sr = 0; (void)ommCpuSerialize(baker, dd, &sr);
    const ommCpuBlobDesc* blob = 0; (void)ommCpuGetSerializedResultDesc(sr, &blob); (void)ommCpuDestroySerializedResult(sr);
    ommCpuBlobDesc bdsc = ommCpuBlobDescDefault(); ommCpuDeserializedResult dr = 0; (void)ommCpuDeserialize(baker, bdsc, &dr);
    const ommCpuDeserializedDesc* ddo = 0; (void)ommCpuGetDeserializedDesc(dr, &ddo); (void)ommCpuDestroyDeserializedResult(dr);
    ommCpuTextureDesc q = ommCpuTextureDescDefault(); (void)ommCpuGetTextureDesc(tex, &q);
    (void)ommCpuDestroyBakeResult(res); (void)ommCpuDestroyTexture(baker, tex); (void)ommGetLibraryDesc();
    return ommDestroyBaker(baker) == ommResult_SUCCESS ? 0 : 2;
}
