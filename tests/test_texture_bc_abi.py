"""ommxCreateTextureBC / ommxCreateTextureBCDevice without a GPU: the symbols, the layout of the two structs against the header, and every argument
check of include/omm_mi355x_ext.h -- all of them are made before the device is touched."""
import ctypes as C
import os
import subprocess
import pytest
import ommtest as ot
import block_texture_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3          # ommMessageSeverity_Fatal
SENTINEL = 0x1234  # *outTexture before every refused call


def test_symbols_are_exported():
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    exported = {ln.split()[-1] for ln in dyn.splitlines() if " T " in ln}
    assert "ommxCreateTextureBC" in exported and "ommxCreateTextureBCDevice" in exported


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxBlockTextureMipDesc), offsetof(ommxBlockTextureMipDesc, width), offsetof(ommxBlockTextureMipDesc, height),
           offsetof(ommxBlockTextureMipDesc, rowPitchInBytes), offsetof(ommxBlockTextureMipDesc, data));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxBlockTextureDesc), offsetof(ommxBlockTextureDesc, format), offsetof(ommxBlockTextureDesc, channel),
           offsetof(ommxBlockTextureDesc, flags), offsetof(ommxBlockTextureDesc, mips), offsetof(ommxBlockTextureDesc, mipCount), offsetof(ommxBlockTextureDesc, alphaCutoff));
    printf("%d %d %d %d %d %d %zu\n", (int)ommxBlockFormat_BC1, (int)ommxBlockFormat_BC2, (int)ommxBlockFormat_BC3, (int)ommxBlockFormat_BC4, (int)ommxBlockFormat_BC5,
           (int)ommxBlockFormat_MAX_NUM, sizeof(ommxBlockFormat));
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the header's structs, compiled as C99, against the ctypes mirrors of tests/block_texture_util.py"""
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    mip, desc, enum = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    M, D = bu.BlockTextureMipDesc, bu.BlockTextureDesc
    assert mip == [C.sizeof(M), M.width.offset, M.height.offset, M.rowPitchInBytes.offset, M.data.offset] == [24, 0, 4, 8, 16]
    assert desc == [C.sizeof(D), D.format.offset, D.channel.offset, D.flags.offset, D.mips.offset, D.mipCount.offset, D.alphaCutoff.offset] == [32, 0, 4, 8, 16, 24, 28]
    assert enum == [bu.BC1, bu.BC2, bu.BC3, bu.BC4, bu.BC5, 5, 4]


@pytest.fixture()
def session():
    lib = ot.Lib("product")
    bu.bind(lib.dll)
    msgs = []
    baker = lib.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    yield lib, baker, msgs
    assert lib.destroy_baker(baker) == ot.SUCCESS


PTR = 0x10000   # never dereferenced: every case below is refused before the device is touched (16-byte aligned)


def call(lib, device, baker, desc, out):
    if device:
        return lib.dll.ommxCreateTextureBCDevice(baker, desc, None, out)
    return lib.dll.ommxCreateTextureBC(baker, desc, out)


def good(fmt=bu.BC3, channel=0, w=16, h=8, pitch=0, ptr=PTR, mips=None):
    return bu.make_desc(fmt, channel, mips if mips is not None else [(w, h, pitch, ptr)], 0.5)


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
    ("format 5", lambda: good(fmt=5), "format is not set"),
    ("format -1", lambda: good(fmt=-1), "format is not set"),
    ("channel 2 (bc5)", lambda: good(fmt=bu.BC5, channel=2), "channel must be 0 or 1"),
    ("channel 1 (bc1)", lambda: good(fmt=bu.BC1, channel=1), "channel must be 0 for every format but BC5"),
    ("channel 1 (bc2)", lambda: good(fmt=bu.BC2, channel=1), "channel must be 0 for every format but BC5"),
    ("channel 1 (bc3)", lambda: good(fmt=bu.BC3, channel=1), "channel must be 0 for every format but BC5"),
    ("channel 1 (bc4)", lambda: good(fmt=bu.BC4, channel=1), "channel must be 0 for every format but BC5"),
    ("pitch below the row (bc3, 16 wide)", lambda: good(pitch=4 * 16 - 8), "mips.rowPitchInBytes is smaller than ceil(width / 4)"),
    ("pitch below the row (bc1, 17 wide: 5 blocks)", lambda: good(fmt=bu.BC1, w=17, pitch=32), "mips.rowPitchInBytes is smaller than ceil(width / 4)"),
    ("pitch below the row in mip 1", lambda: good(mips=[(8, 8, 32, PTR), (4, 4, 8, PTR)]), "mips.rowPitchInBytes is smaller than ceil(width / 4)"),
]
DEVICE_ONLY = [
    ("pointer not a multiple of 8", lambda: good(ptr=PTR + 4), "mips.rowPitchInBytes and mips.data must be multiples of 8"),
    ("pitch not a multiple of 8", lambda: good(pitch=4 * 16 + 4), "mips.rowPitchInBytes and mips.data must be multiples of 8"),
    ("pointer not a multiple of 8 in mip 1", lambda: good(mips=[(8, 8, 0, PTR), (4, 4, 0, PTR + 1)]), "mips.rowPitchInBytes and mips.data must be multiples of 8"),
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
    """a desc that passes every check still needs a device: FAILURE and the Fatal line, nothing decoded on the host"""
    hip = C.CDLL("libamdhip64.so")
    n = C.c_int(0)
    if hip.hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a HIP device is present: the fail-loudly path cannot be exercised here")
    lib, baker, msgs = session
    out = C.c_void_p(SENTINEL)
    for device in (False, True):
        for d in (good(), good(fmt=bu.BC5, channel=1, w=13, pitch=4 * 16 + 8), good(fmt=bu.BC1, mips=[(65536, 65536, 0, PTR)] * 17)):
            del msgs[:]
            assert call(lib, device, baker, C.byref(d), C.byref(out)) == ot.FAILURE and out.value == SENTINEL
            assert len(msgs) == 1 and msgs[0][0] == FATAL and "no usable HIP device" in msgs[0][1] and "no CPU fallback" in msgs[0][1], msgs
