"""The reference decoder of tests/bc7_util.py by itself, before anything is compared with it: blocks written out by hand, whose alpha follows from the
definition in include/omm_mi355x_ext.h with a few multiplications; Pillow's BC7 decoder where Pillow is installed; and a committed record of Pillow's
answers (tests/golden/bc7_alpha_blocks.npz, written by tests/golden/make_bc7_fixture.py) everywhere else."""
import io
import os
import numpy as np
import pytest
import bc7_util as b7

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bc7_alpha_blocks.npz")

# ((64 - w) * 0 + w * 255 + 32) >> 6 for the weights of the header
W2 = [0, 84, 171, 255]                         # 0 21 43 64
W3 = [0, 36, 72, 108, 147, 183, 219, 255]      # 0 9 18 27 37 46 55 64
W4 = [0, 16, 36, 52, 68, 84, 104, 120, 135, 151, 171, 187, 203, 219, 239, 255]   # 0 4 9 13 17 21 26 30 34 38 43 47 51 55 60 64


def test_the_weights_are_the_integer_formulas():
    assert b7.WEIGHTS[2] == [(64 * i + 1) // 3 for i in range(4)]
    assert b7.WEIGHTS[3] == [(64 * i + 3) // 7 for i in range(8)]
    assert b7.WEIGHTS[4] == [(64 * i + 7) // 15 for i in range(16)]
    assert len(b7.MASK) == 64 and len(b7.ANCHOR) == 64 and set(b7.ANCHOR) == {2, 6, 8, 15}
    assert all(m & 1 == 0 and (m >> a) & 1 == 1 for m, a in zip(b7.MASK, b7.ANCHOR))   # texel 0 is in subset 0, the anchor in subset 1


def test_blocks_given_byte_by_byte():
    """no builder in between.  Mode 6: bit 6; A0 = 0, P0 = 0; A1 = 127 (bits 56..62), P1 = 1 (bit 64); every index bit set: texel 0 has 3 bits, so index 7
    (weight 30: 120), the others index 15.  Mode 5: bit 5, rot 0; A0 = 0, A1 = 255 (bits 58..65); alpha indices from bit 97, texel 0 one bit: all 1."""
    m6 = bytes.fromhex("40000000" "0000007F" "FFFFFFFF" "FFFFFFFF")
    assert b7.block_alpha(m6) == [120] + [255] * 15
    assert b7.build_mode6((0, 0), (0, 0), (0, 0), (0, 127), (0, 1), [7] + [15] * 15) == m6
    m5 = bytes.fromhex("20000000" "000000FC" "03000000" "56555555")
    assert b7.block_alpha(m5) == [84] * 16
    assert b7.build_mode5(0, (0, 0), (0, 0), (0, 0), (0, 255), [0] * 16, [1] * 16) == m5
    assert b7.block_alpha(bytes(16)) == [0] * 16                                       # reserved: zeros, as D3D defines it
    assert b7.block_alpha(bytes([0]) + bytes([0xFF] * 15)) == [0] * 16
    for m in range(4):                                                                 # no alpha in the block
        assert b7.block_alpha(bytes([1 << m]) + bytes(range(1, 16))) == [255] * 16


IDX3 = [0, 1, 2, 3, 4, 5, 6, 7, 7, 6, 5, 4, 3, 2, 1, 0]
IDX2 = [0, 1, 2, 3] * 4
OTHER2 = [1, 3, 0, 2] * 4
OTHER3 = [3, 6, 1, 0, 7, 2, 5, 4] * 2


def test_mode_4_by_hand():
    """5-bit 0 and 31 widen to 0 and 255, 8 to 66; 6-bit 0 and 63 to 0 and 255"""
    r, g, b = (0, 31), (31, 0), (8, 8)
    # rot 0: A.  idxMode 0: the 3-bit set; idxMode 1: the 2-bit set
    assert b7.block_alpha(b7.build_mode4(0, 0, r, g, b, (0, 63), OTHER2, IDX3)) == [W3[k] for k in IDX3]
    assert b7.block_alpha(b7.build_mode4(0, 1, r, g, b, (0, 63), IDX2, OTHER3)) == [W2[k] for k in IDX2]
    # rot 1, 2, 3: R, G, B with the colour set -- idxMode 0: the 2-bit set; idxMode 1: the 3-bit set.  A (63, 63) would give 255 everywhere.
    assert b7.block_alpha(b7.build_mode4(1, 0, r, g, b, (63, 63), IDX2, OTHER3)) == [W2[k] for k in IDX2]
    assert b7.block_alpha(b7.build_mode4(2, 0, r, g, b, (63, 63), IDX2, OTHER3)) == [W2[3 - k] for k in IDX2]
    assert b7.block_alpha(b7.build_mode4(3, 0, r, g, b, (63, 63), IDX2, OTHER3)) == [66] * 16
    assert b7.block_alpha(b7.build_mode4(1, 1, r, g, b, (63, 63), OTHER2, IDX3)) == [W3[k] for k in IDX3]
    assert b7.block_alpha(b7.build_mode4(2, 1, r, g, b, (63, 63), OTHER2, IDX3)) == [W3[7 - k] for k in IDX3]
    assert b7.block_alpha(b7.build_mode4(3, 1, r, g, b, (63, 63), OTHER2, IDX3)) == [66] * 16


def test_mode_5_by_hand():
    """7-bit 0 and 127 widen to 0 and 255, 64 to 129; A is 8 bits as it stands: 10 .. 250 with the weights 0 21 43 64 is 10, 89, 171, 250"""
    r, g, b = (0, 127), (127, 0), (64, 64)
    assert b7.block_alpha(b7.build_mode5(0, r, g, b, (10, 250), OTHER2, IDX2)) == [[10, 89, 171, 250][k] for k in IDX2]
    assert b7.block_alpha(b7.build_mode5(1, r, g, b, (10, 250), IDX2, OTHER2)) == [W2[k] for k in IDX2]
    assert b7.block_alpha(b7.build_mode5(2, r, g, b, (10, 250), IDX2, OTHER2)) == [W2[3 - k] for k in IDX2]
    assert b7.block_alpha(b7.build_mode5(3, r, g, b, (10, 250), IDX2, OTHER2)) == [129] * 16


def test_mode_6_by_hand():
    c = (5, 99)
    assert b7.block_alpha(b7.build_mode6(c, c, c, (0, 127), (0, 1), list(range(16)))) == W4
    for p0, p1 in ((0, 0), (1, 0), (0, 1), (1, 1)):                                    # the P bit is the endpoint's lowest bit
        assert b7.block_alpha(b7.build_mode6(c, c, c, (0, 127), (p0, p1), [0] * 8 + [15] * 8)) == [p0] * 8 + [254 + p1] * 8


# (partition, its mask and anchor as the header lists them): the four anchors
PARTITIONS = [(0, 0xCCCC, 15), (17, 0x008E, 2), (18, 0x7100, 8), (34, 0x5A5A, 6), (47, 0x0660, 6), (63, 0xEE22, 15)]


@pytest.mark.parametrize("part,mask,anchor", PARTITIONS)
def test_mode_7_by_hand(part, mask, anchor):
    """subset 0 runs 0 -> 255 (A 0, P 0 and A 31, P 1), subset 1 255 -> 0: index 1 everywhere (all an anchor's single bit can hold) is 84 in subset 0 and
    171 in subset 1.  Then the P bits alone: 6-bit 1 widens to 4, 62 to 251."""
    assert (b7.MASK[part], b7.ANCHOR[part]) == (mask, anchor)
    c = (3, 30, 17, 9)
    assert b7.block_alpha(b7.build_mode7(part, c, c, c, (0, 31, 31, 0), (0, 1, 1, 0), [1] * 16)) == [171 if (mask >> i) & 1 else 84 for i in range(16)]
    assert b7.block_alpha(b7.build_mode7(part, c, c, c, (0, 0, 31, 31), (1, 0, 0, 1), [0] * 16)) == [251 if (mask >> i) & 1 else 4 for i in range(16)]
    # every code at the texels that have two bits: index (i % 4) but at the two anchors
    idx = [0 if i in (0, anchor) else i % 4 for i in range(16)]
    want = [(W2[3 - k] if (mask >> i) & 1 else W2[k]) for i, k in enumerate(idx)]
    assert b7.block_alpha(b7.build_mode7(part, c, c, c, (0, 31, 31, 0), (0, 1, 1, 0), idx)) == want


def test_mode_7_partition_0_written_out():
    """mask CCCC: x = 2, 3 of every row are subset 1; anchor 15"""
    c = (0, 0, 0, 0)
    idx = [0, 1, 2, 3] * 3 + [0, 1, 2, 1]
    assert b7.block_alpha(b7.build_mode7(0, c, c, c, (0, 31, 31, 0), (0, 1, 1, 0), idx)) == [0, 84, 84, 0] * 3 + [0, 84, 84, 171]


def test_forced_images_hold_what_they_promise():
    """8 blocks or more: at least half in the modes 4..7, all four present, one reserved block, the rest modes 0..3; fewer: the modes 4..7 by seed"""
    for (w, h, seed) in ((32, 8, 1), (13, 9, 2), (64, 64, 3), (17, 5, 4), (260, 65, 5)):
        blocks = b7.random_blocks(w, h, seed)
        modes = np.array([b7.mode_of(b) for b in blocks.reshape(-1, 16)[:, 0]])
        count = np.bincount(modes, minlength=9)
        assert count[4:8].sum() * 2 >= modes.size and (count[4:8] > 0).all() and count[8] == 1 and count[:4].sum() == modes.size - count[4:8].sum() - 1
        assert (b7.decode(blocks, w, h) != 255).mean() > 0.4
    assert {b7.mode_of(b7.random_blocks(4, 4, seed)[0, 0, 0]) for seed in range(4)} == {4, 5, 6, 7}
    assert [b7.mode_of(b) for b in b7.random_blocks(12, 4, 0)[0, :, 0]] == [4, 5, 6]


def test_against_the_recorded_answers_of_pillow():
    z = np.load(GOLDEN)
    blocks, alpha = z["blocks"], z["alpha"]
    assert blocks.shape == alpha.shape == (8, 256, 16) and blocks.dtype == alpha.dtype == np.uint8
    for m in range(8):
        assert all(b7.mode_of(b) == m for b in blocks[m, :, 0])
        assert np.array_equal(b7.block_texels(blocks[m]), alpha[m]), m
        assert m < 4 or (alpha[m] != 255).mean() > 0.98


def test_against_pillow():
    """1024 forced blocks of each mode 0..7 in a DX10-header DDS (DXGI_FORMAT_BC7_UNORM = 98), byte for byte.  Reserved blocks (byte 0 == 0) are left out:
    Pillow answers 255 for them where D3D defines zeros in every channel -- that case is pinned by hand above."""
    Image = pytest.importorskip("PIL.Image")
    for m in range(8):
        blocks = b7.blocks_of_mode(m, 1024, 100 + m).reshape(32, 32, 16)
        im = Image.open(io.BytesIO(b7.dds_bytes(blocks, 128, 128)))
        got = np.array(im.convert("RGBA"))[..., 3]
        assert np.array_equal(b7.decode(blocks, 128, 128), got), m
