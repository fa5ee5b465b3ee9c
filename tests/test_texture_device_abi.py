"""ommxCreateTextureDevice without a GPU: the symbol, the layout of its two structs against the header, and every argument check of
include/omm_mi355x_ext.h -- all of them are made before the device is touched."""
import ctypes as C
import os
import subprocess
import pytest
import ommtest as ot
import texture_device_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATAL = 3          # ommMessageSeverity_Fatal
SENTINEL = 0x1234  # *outTexture before every refused call


def test_symbol_is_exported():
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", ot.product_path()], text=True)
    assert "ommxCreateTextureDevice" in {ln.split()[-1] for ln in dyn.splitlines() if " T " in ln}


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "omm_mi355x_ext.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(ommxDeviceTextureMipDesc), offsetof(ommxDeviceTextureMipDesc, width), offsetof(ommxDeviceTextureMipDesc, height),
           offsetof(ommxDeviceTextureMipDesc, rowPitchInBytes), offsetof(ommxDeviceTextureMipDesc, deviceData));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ommxDeviceTextureDesc), offsetof(ommxDeviceTextureDesc, channelFormat), offsetof(ommxDeviceTextureDesc, pixelStrideInBytes),
           offsetof(ommxDeviceTextureDesc, channelOffsetInBytes), offsetof(ommxDeviceTextureDesc, flags), offsetof(ommxDeviceTextureDesc, mips),
           offsetof(ommxDeviceTextureDesc, mipCount), offsetof(ommxDeviceTextureDesc, alphaCutoff));
    printf("%d %d %d %d %zu\n", (int)ommxTexelFormat_UNORM8, (int)ommxTexelFormat_FP32, (int)ommxTexelFormat_FP16, (int)ommxTexelFormat_MAX_NUM, sizeof(ommxTexelFormat));
    return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the header's structs, compiled as C99, against the ctypes mirrors of tests/texture_device_util.py"""
    src, exe = tmp_path / "probe.c", str(tmp_path / "probe")
    src.write_text(PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    mip, desc, enum = ([int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines())
    M, D = tu.DeviceTextureMipDesc, tu.DeviceTextureDesc
    assert mip == [C.sizeof(M), M.width.offset, M.height.offset, M.rowPitchInBytes.offset, M.deviceData.offset] == [24, 0, 4, 8, 16]
    assert desc == [C.sizeof(D), D.channelFormat.offset, D.pixelStrideInBytes.offset, D.channelOffsetInBytes.offset, D.flags.offset, D.mips.offset,
                    D.mipCount.offset, D.alphaCutoff.offset] == [32, 0, 4, 8, 12, 16, 24, 28]
    assert enum == [tu.UNORM8, tu.FP32, tu.FP16, 3, 4]


@pytest.fixture()
def session():
    lib = ot.Lib("product")
    tu.bind(lib.dll)
    msgs = []
    baker = lib.create_baker(callback=lambda sev, msg, user: msgs.append((sev, msg.decode())))
    yield lib, baker, msgs
    assert lib.destroy_baker(baker) == ot.SUCCESS


PTR = 0x10000   # never dereferenced: every case below is refused before the device is touched (16-byte aligned)


def good(fmt=tu.UNORM8, stride=4, offset=3, w=16, h=8, pitch=0, ptr=PTR, mips=None):
    return tu.make_desc(fmt, stride, offset, mips if mips is not None else [(w, h, pitch, ptr)], 0.5)


# (name, desc, the words its log line must hold)
REFUSED = [
    ("mipCount 0", lambda: good(mips=[]), "mipCount must be non-zero"),
    ("18 mips", lambda: good(mips=[(4, 4, 0, PTR)] * 18), "more than 17 mips"),
    ("width 0", lambda: good(w=0), "mips.width must be non-zero"),
    ("height 0", lambda: good(h=0), "mips.height must be non-zero"),
    ("width 65537", lambda: good(w=65537), "mips.width must be less than kMaxDim.x (65536)"),
    ("height 65537", lambda: good(h=65537), "mips.height must be less than kMaxDim.y (65536)"),
    ("null deviceData", lambda: good(ptr=None), "mips.textureData is not set"),
    ("null deviceData in mip 1", lambda: good(mips=[(4, 4, 0, PTR), (2, 2, 0, None)]), "mips.textureData is not set"),
    ("format 3", lambda: good(fmt=3), "format is not set"),
    ("format -1", lambda: good(fmt=-1), "format is not set"),
    ("stride below the channel (fp32, 2)", lambda: good(fmt=tu.FP32, stride=2, offset=0), "pixelStrideInBytes is smaller than one channel"),
    ("stride below the channel (fp16, 1)", lambda: good(fmt=tu.FP16, stride=1, offset=0), "pixelStrideInBytes is smaller than one channel"),
    ("offset + channel above the stride (unorm8)", lambda: good(stride=4, offset=4), "exceeds pixelStrideInBytes"),
    ("offset + channel above the stride (fp16)", lambda: good(fmt=tu.FP16, stride=8, offset=8), "exceeds pixelStrideInBytes"),
    ("offset + channel above the stride (fp32, straddling)", lambda: good(fmt=tu.FP32, stride=16, offset=14), "exceeds pixelStrideInBytes"),
    ("offset with the default stride", lambda: good(stride=0, offset=1), "exceeds pixelStrideInBytes"),
    ("stride not a multiple (fp16, 3)", lambda: good(fmt=tu.FP16, stride=3, offset=0), "must be multiples of the size of the channel"),
    ("stride not a multiple (fp32, 6)", lambda: good(fmt=tu.FP32, stride=6, offset=0), "must be multiples of the size of the channel"),
    ("offset not a multiple (fp32, 2)", lambda: good(fmt=tu.FP32, stride=16, offset=2), "must be multiples of the size of the channel"),
    ("offset not a multiple (fp16, 1)", lambda: good(fmt=tu.FP16, stride=8, offset=1), "must be multiples of the size of the channel"),
    ("pitch not a multiple (fp32)", lambda: good(fmt=tu.FP32, stride=16, offset=0, pitch=16 * 16 + 2), "mips.rowPitchInBytes and mips.deviceData must be multiples"),
    ("pointer not a multiple (fp16)", lambda: good(fmt=tu.FP16, stride=8, offset=0, ptr=PTR + 1), "mips.rowPitchInBytes and mips.deviceData must be multiples"),
    ("pointer not a multiple (fp32)", lambda: good(fmt=tu.FP32, stride=4, offset=0, ptr=PTR + 2), "mips.rowPitchInBytes and mips.deviceData must be multiples"),
    ("pitch below the row", lambda: good(pitch=16 * 4 - 1), "mips.rowPitchInBytes is smaller than width * pixelStrideInBytes"),
    ("pitch below the row in mip 1", lambda: good(mips=[(4, 4, 16, PTR), (2, 2, 4, PTR)]), "mips.rowPitchInBytes is smaller than width * pixelStrideInBytes"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_before_the_device_is_touched(session, case):
    lib, baker, msgs = session
    _, make, words = case
    out = C.c_void_p(SENTINEL)
    r = lib.dll.ommxCreateTextureDevice(baker, C.byref(make()), None, C.byref(out))
    assert r == ot.INVALID_ARGUMENT and out.value == SENTINEL
    assert len(msgs) == 1 and msgs[0][0] == FATAL and words in msgs[0][1], msgs


def test_handles_are_checked_like_ommCpuCreateTexture(session):
    lib, baker, msgs = session
    out = C.c_void_p(SENTINEL)
    d = good()
    assert lib.dll.ommxCreateTextureDevice(None, C.byref(d), None, C.byref(out)) == ot.INVALID_ARGUMENT and not msgs
    assert lib.dll.ommxCreateTextureDevice(baker, None, None, C.byref(out)) == ot.INVALID_ARGUMENT
    assert msgs[-1] == (FATAL, "texture desc was not set")
    assert lib.dll.ommxCreateTextureDevice(baker, C.byref(d), None, None) == ot.INVALID_ARGUMENT
    assert msgs[-1][0] == FATAL and "outTexture is not set" in msgs[-1][1]
    gpu_lib = ot.Lib("product")
    gpu = gpu_lib.create_baker(baker_type=0, callback=lambda sev, msg, user: msgs.append((sev, "gpu baker: " + msg.decode())))
    assert lib.dll.ommxCreateTextureDevice(gpu, C.byref(d), None, C.byref(out)) == ot.INVALID_ARGUMENT
    assert msgs[-1] == (FATAL, "gpu baker: Baker was not created as the right type")
    assert gpu_lib.destroy_baker(gpu) == ot.SUCCESS
    assert out.value == SENTINEL
    # the host-pointer entry answers the same conditions with the same codes and lines
    td = ot.TextureDesc()
    n = len(msgs)
    assert lib.fn("ommCpuCreateTexture")(baker, None, C.byref(out)) == ot.INVALID_ARGUMENT and msgs[n] == (FATAL, "texture desc was not set")
    assert lib.fn("ommCpuCreateTexture")(baker, C.byref(td), C.byref(out)) == ot.INVALID_ARGUMENT and "mipCount must be non-zero" in msgs[n + 1][1]
    assert out.value == SENTINEL


def test_no_cpu_fallback_without_a_gpu(session):
    """a desc that passes every check still needs a device: FAILURE and the Fatal line, nothing computed on the host"""
    hip = C.CDLL("libamdhip64.so")
    n = C.c_int(0)
    if hip.hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a HIP device is present: the fail-loudly path cannot be exercised here")
    lib, baker, msgs = session
    out = C.c_void_p(SENTINEL)
    for d in (good(), good(fmt=tu.FP16, stride=8, offset=6, pitch=16 * 8 + 2), good(fmt=tu.FP32, stride=0, offset=0, mips=[(65536, 65536, 0, PTR)] * 17)):
        del msgs[:]
        assert lib.dll.ommxCreateTextureDevice(baker, C.byref(d), None, C.byref(out)) == ot.FAILURE and out.value == SENTINEL
        assert len(msgs) == 1 and msgs[0][0] == FATAL and "no usable HIP device" in msgs[0][1] and "no CPU fallback" in msgs[0][1], msgs
