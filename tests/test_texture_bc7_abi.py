"""ommxCreateTextureBC7 / ommxCreateTextureBC7Device without a GPU: the symbols, the layout of the desc against the header, and every argument check of
include/omm_mi355x_ext.h -- all of them are made before the device is touched."""
import ctypes as C
import os
import subprocess
import pytest
import ommtest as ot
import block_texture_util as bu
import bc7_util as b7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3          # ommMessageSeverity_Fatal
SENTINEL = 0x1234  # *outTexture before every refused call


def test_symbols_are_exported():
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    exported = {ln.split()[-1] for ln in dyn.splitlines() if " T " in ln}
    assert "ommxCreateTextureBC7" in exported and "ommxCreateTextureBC7Device" in exported


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    const ommxBC7TextureDesc d = { ommCpuTextureFlags_None, (const ommxBlockTextureMipDesc*)0, 0u, -1.f };
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxBC7TextureDesc), offsetof(ommxBC7TextureDesc, flags), offsetof(ommxBC7TextureDesc, mips),
           offsetof(ommxBC7TextureDesc, mipCount), offsetof(ommxBC7TextureDesc, alphaCutoff));
    printf("%zu %zu %d\n", sizeof(ommxBlockTextureMipDesc), sizeof d.mips[0], (int)ommxBlockFormat_MAX_NUM);
    return 0;
}
"""


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of the header's struct, compiled as C99, against the ctypes mirror of tests/bc7_util.py; the mips are ommxBlockTextureMipDesc and
    the enum of the BC1..BC5 call did not grow"""
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    desc, rest = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    D = b7.BC7TextureDesc
    assert desc == [C.sizeof(D), D.flags.offset, D.mips.offset, D.mipCount.offset, D.alphaCutoff.offset] == [24, 0, 8, 16, 20]
    assert rest == [C.sizeof(bu.BlockTextureMipDesc), 24, 5]


@pytest.fixture()
def session():
    lib = ot.Lib("product")
    b7.bind(lib.dll)
    msgs = []
    baker = lib.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    yield lib, baker, msgs
    assert lib.destroy_baker(baker) == ot.SUCCESS


PTR = 0x10000   # never dereferenced: every case below is refused before the device is touched (16-byte aligned)


def call(lib, device, baker, desc, out):
    if device:
        return lib.dll.ommxCreateTextureBC7Device(baker, desc, None, out)
    return lib.dll.ommxCreateTextureBC7(baker, desc, out)


def good(w=16, h=8, pitch=0, ptr=PTR, mips=None):
    return b7.make_desc(mips if mips is not None else [(w, h, pitch, ptr)], 0.5)


def null_mips():
    d = good()
    d.mips = None       # mipCount stays 1
    return d


# (name, desc, the words its log line must hold): each desc is valid but for the one thing
REFUSED = [
    ("mips null with mipCount 1", null_mips, "mips is not set"),
    ("mipCount 0", lambda: good(mips=[]), "mipCount must be non-zero"),
    ("18 mips", lambda: good(mips=[(4, 4, 0, PTR)] * 18), "more than 17 mips"),
    ("width 0", lambda: good(w=0), "mips.width must be non-zero"),
    ("height 0", lambda: good(h=0), "mips.height must be non-zero"),
    ("width 65537", lambda: good(w=65537), "mips.width must be less than kMaxDim.x (65536)"),
    ("height 65537", lambda: good(h=65537), "mips.height must be less than kMaxDim.y (65536)"),
    ("null data", lambda: good(ptr=None), "mips.textureData is not set"),
    ("null data in mip 1", lambda: good(mips=[(4, 4, 0, PTR), (2, 2, 0, None)]), "mips.textureData is not set"),
    ("pitch below the row (16 wide)", lambda: good(pitch=4 * 16 - 16), "mips.rowPitchInBytes is smaller than ceil(width / 4)"),
    ("pitch below the row (17 wide: 5 blocks)", lambda: good(w=17, pitch=64), "mips.rowPitchInBytes is smaller than ceil(width / 4)"),
    ("pitch below the row in mip 1", lambda: good(mips=[(8, 8, 32, PTR), (4, 4, 8, PTR)]), "mips.rowPitchInBytes is smaller than ceil(width / 4)"),
]
DEVICE_ONLY = [
    ("pointer a multiple of 8 only", lambda: good(ptr=PTR + 8), "mips.rowPitchInBytes and mips.data must be multiples of 16"),
    ("pitch a multiple of 8 only", lambda: good(pitch=4 * 16 + 8), "mips.rowPitchInBytes and mips.data must be multiples of 16"),
    ("pointer not a multiple of 16 in mip 1", lambda: good(mips=[(8, 8, 0, PTR), (4, 4, 0, PTR + 1)]), "mips.rowPitchInBytes and mips.data must be multiples of 16"),
]
CASES = [(dev, c) for dev in (False, True) for c in REFUSED] + [(True, c) for c in DEVICE_ONLY]


@pytest.mark.parametrize("device,case", CASES, ids=[("device: " if dev else "host: ") + c[0] for dev, c in CASES])
def test_refused_before_the_device_is_touched(session, device, case):
    lib, baker, msgs = session
    _, make, words = case
    out = C.c_void_p(SENTINEL)
    r = call(lib, device, baker, C.byref(make()), C.byref(out))
    assert r == ot.INVALID_ARGUMENT and out.value == SENTINEL
    assert len(msgs) == 1 and msgs[0][0] == FATAL and words in msgs[0][1], msgs


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_handles_are_checked_like_ommCpuCreateTexture(session, device):
    lib, baker, msgs = session
    out = C.c_void_p(SENTINEL)
    d = good()
    assert call(lib, device, None, C.byref(d), C.byref(out)) == ot.INVALID_ARGUMENT and not msgs
    assert call(lib, device, baker, None, C.byref(out)) == ot.INVALID_ARGUMENT
    assert msgs[-1] == (FATAL, "texture desc was not set")
    assert call(lib, device, baker, C.byref(d), None) == ot.INVALID_ARGUMENT
    assert msgs[-1][0] == FATAL and "outTexture is not set" in msgs[-1][1]
    gpu_lib = ot.Lib("product")
    gpu = gpu_lib.create_baker(baker_type=0, callback=lambda sev, msg, user: msgs.append((sev, "gpu baker: " + msg.decode())))
    assert call(lib, device, gpu, C.byref(d), C.byref(out)) == ot.INVALID_ARGUMENT
    assert msgs[-1] == (FATAL, "gpu baker: Baker was not created as the right type")
    assert gpu_lib.destroy_baker(gpu) == ot.SUCCESS
    assert out.value == SENTINEL and len(msgs) == 3


def test_no_cpu_fallback_without_a_gpu(session):
    """a desc that passes every check still needs a device: FAILURE and the Fatal line, nothing decoded on the host.  (The unaligned pointer and pitch
    are fine on the host entry only.)"""
    hip = C.CDLL("libamdhip64.so")
    n = C.c_int(0)
    if hip.hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a HIP device is present: the fail-loudly path cannot be exercised here")
    lib, baker, msgs = session
    out = C.c_void_p(SENTINEL)
    for device in (False, True):
        descs = [good(), good(w=13, pitch=4 * 16 + 16), good(mips=[(65536, 65536, 0, PTR)] * 17)] + ([] if device else [good(w=13, pitch=4 * 16 + 3, ptr=PTR + 1)])
        for d in descs:
            del msgs[:]
            assert call(lib, device, baker, C.byref(d), C.byref(out)) == ot.FAILURE and out.value == SENTINEL
            assert len(msgs) == 1 and msgs[0][0] == FATAL and "no usable HIP device" in msgs[0][1] and "no CPU fallback" in msgs[0][1], msgs
