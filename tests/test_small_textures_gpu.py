"""HIP library vs oracle, full result arrays (test_gpu_parity.both), on the textures the rest of the suite does not have: smaller than the
32x32 LDS window of classify_tiles, one texel wide or high, around a 64 edge, thin and long, and mip chains down to 1x1.  Triangles lie
over UV [-3.5, 4.5] at three sizes -- about a texel, about the texture, about 3 UV units -- so that texel rectangles wrap the texture
several times and region_rect (classify_device.h) finds a seam at every level of the hierarchy; every address mode, both filters, SAT on
and off, levels 0 .. 7, level 7 in both homes of the generic pass.  The case list is tests/small_texture_cases.py."""
import numpy as np
import pytest
import ommtest as ot
import small_texture_cases as stc
from test_gpu_parity import both

CASES = stc.cases()
CHAIN_CASES = stc.chain_cases()


def test_case_list_coverage():
    """no GPU: what the seeded pick must still cover"""
    assert len(CASES) == len(stc.SHAPES) * 5
    assert {(c[2], c[3]) for c in CASES} == {(s, a) for s in stc.SHAPES for a in stc.ADDRS}       # every shape with every address mode
    for s in stc.SHAPES:
        assert {c[4] for c in CASES if c[2] == s} == {False, True}                                # ... and in both texture formats
    count = {}
    for c in CASES:
        bakes = stc.bakes_of(c[1], *c[2])
        assert len(bakes) == 3 * 3 + 2 * 2 + 2
        assert {(b[0], b[3]) for b in bakes} == {(e, l) for e in ("texel", "texture", "wraps") for l in (0, 2, 5)} | {(e, l) for e in ("texel", "texture") for l in (6, 7)}
        assert sorted(b[6] for b in bakes if b[3] == 7) == sorted(2 * [((ot.KNOB_GENERIC_PASS, 1),), ((ot.KNOB_GENERIC_PASS, 2),)])
        assert all(b[2] == (20 if b[0] == "wraps" else 60) for b in bakes)
        for b in bakes:
            for key in (("shape", c[2], "filter", b[4]), ("shape", c[2], "sat", b[5]), ("level", b[3], "filter", b[4]), ("level", b[3], "sat", b[5]),
                        ("extent", b[0], "filter", b[4]), ("extent", b[0], "sat", b[5]), ("addr", c[3], "filter", b[4]), ("addr", c[3], "sat", b[5])):
                count[key] = count.get(key, 0) + 1
    for kind, values in (("shape", stc.SHAPES), ("level", [0, 2, 5, 6, 7]), ("extent", ["texel", "texture", "wraps"]), ("addr", stc.ADDRS)):
        for v in values:
            for opt, choices in (("filter", [ot.LINEAR, ot.NEAREST]), ("sat", [True, False])):
                for ch in choices:
                    assert count.get((kind, v, opt, ch), 0) >= 2, (kind, v, opt, ch)
    # the textures are mixed: both sides of the cut-off from 4 texels on, neither side above 75 % from 200 texels on
    for c in CASES:
        (w, h) = c[2]
        tex = stc.noise_texture(300 + c[1], w, h, c[4])
        assert tex.shape == (h, w) and tex.dtype == (np.float32 if c[4] else np.uint8)
        above = float(np.mean(tex.astype(np.float32) > (0.5 if c[4] else 127.5)))
        assert w * h < 4 or 0.0 < above < 1.0, (c[0], above)
        assert w * h < 200 or 0.25 < above < 0.75, (c[0], above)
    # UV range and extents
    uv, ix = stc.triangles(3, 2, 20, 3.0)
    assert uv.min() < -3.5 and uv.max() > 4.5 and ix.size == 60
    # mip chains
    assert len(CHAIN_CASES) == 8 and {(c[1], c[4], c[5]) for c in CHAIN_CASES} == {(n, s, a) for n in ("pow2", "odd") for s in (True, False) for a in (ot.WRAP, ot.CLAMP)}
    for name, w, h, sizes in stc.CHAINS:
        for fp32 in (False, True):
            mips = stc.chain(w, h, fp32, 900 + w)
            assert [(m.shape[1], m.shape[0]) for m in mips] == sizes and all(m.dtype == mips[0].dtype and m.flags["C_CONTIGUOUS"] for m in mips)
    assert np.array_equal(stc.halve(np.array([[10, 20, 7], [30, 40, 9], [1, 2, 3]], np.uint8)), np.array([[25]], np.uint8))
    assert np.array_equal(stc.halve(np.array([[1.0, 2.0, 5.0]], np.float32)), np.array([[1.5]], np.float32))
    assert np.array_equal(stc.halve(np.array([[1.0], [2.0]], np.float32)), np.array([[1.5]], np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_small_and_odd_shaped_textures(product, oracle, case):
    stc.run_case(both, product, oracle, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_mip_chains_down_to_one_texel(product, oracle, case):
    """64x64 -> 1x1 and 300x200 -> 150x100 -> 75x50 -> 37x25 -> 18x12 -> 9x6 -> 4x3 -> 2x1 -> 1x1, SAT on / off, Wrap / Clamp; triangles of about a texel of mip 0,
    0.15 and 1 UV unit, and 3 UV units"""
    stc.run_chain_case(both, product, oracle, case)
