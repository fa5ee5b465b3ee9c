// A user of the SDK's own omm.hpp, the header-only C++ wrapper (omm.hpp:1003-1013 forwards to the C symbols).  tests/test_abi_exports.py links it against libomm-lib.so where
// the SDK headers exist; the omm* symbols it references are recorded in tests/golden/sdk_user_symbols.txt (make_fixtures.py).
#include <omm.hpp>
int main() {
    omm::BakerCreationDesc bd; bd.type = omm::BakerType::CPU;
    omm::Baker baker = 0; if (omm::CreateBaker(bd, &baker) != omm::Result::SUCCESS) return 1;
    omm::Cpu::TextureDesc td; omm::Cpu::Texture tex = 0; (void)omm::Cpu::CreateTexture(baker, td, &tex);
    omm::Cpu::BakeInputDesc in; omm::Cpu::BakeResult res = 0; (void)omm::Cpu::Bake(baker, in, &res);
    const omm::Cpu::BakeResultDesc* out = 0; (void)omm::Cpu::GetBakeResultDesc(res, &out);
    (void)omm::Cpu::DestroyBakeResult(res); (void)omm::Cpu::DestroyTexture(baker, tex);
    return omm::DestroyBaker(baker) == omm::Result::SUCCESS ? 0 : 2;
}
