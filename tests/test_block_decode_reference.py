"""The numpy reference decoder of tests/block_texture_util.py, which every GPU test of ommxCreateTextureBC compares against, pinned by itself: blocks
whose bytes and texels are written out by hand below, and -- where Pillow is installed -- 256 random blocks per format, wrapped in an in-memory DDS
file and decoded by Pillow.  Pillow rounds the interpolated formats to a byte by truncation, so there the relation is floor((float)n / (float)D)."""
import io
import numpy as np
import pytest
import block_texture_util as bu

ONE_255TH = np.float32(1.0) / np.float32(255.0)
IDENTITY_CODES = [0x88, 0xC6, 0xFA, 0x88, 0xC6, 0xFA]   # the 3-bit codes 0, 1, ..., 7, 0, 1, ..., 7 as 48 bits, little-endian


def fraction(n, d):
    return (np.array(n, np.float32) / np.float32(d)) * ONE_255TH


def test_bc4_six_step_block():
    """a0 = 200 > a1 = 100: D = 7; n = 7 a0, 7 a1, 6 a0 + a1, 5 a0 + 2 a1, 4 a0 + 3 a1, 3 a0 + 4 a1, 2 a0 + 5 a1, a0 + 6 a1"""
    got = bu.bc4_texels(np.array([200, 100] + IDENTITY_CODES, np.uint8))
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), fraction([1400, 700, 1300, 1200, 1100, 1000, 900, 800] * 2, 7).view(np.uint32))
    n, d = bu.bc4_fraction(np.array([200, 100] + IDENTITY_CODES, np.uint8))
    assert n.tolist() == [1400, 700, 1300, 1200, 1100, 1000, 900, 800] * 2 and d.tolist() == [7]
    assert got[0] == np.float32(200) * ONE_255TH and got[1] == np.float32(100) * ONE_255TH   # the endpoints are the bytes' own values


def test_bc4_four_step_block_with_codes_6_and_7():
    """a0 = 100 < a1 = 200: D = 5; n = 5 a0, 5 a1, 4 a0 + a1, 3 a0 + 2 a1, 2 a0 + 3 a1, a0 + 4 a1, then 0 (code 6) and 5 * 255 (code 7)"""
    got = bu.bc4_texels(np.array([100, 200] + IDENTITY_CODES, np.uint8))
    assert np.array_equal(got.view(np.uint32), fraction([500, 1000, 600, 700, 800, 900, 0, 1275] * 2, 5).view(np.uint32))
    assert got[6] == 0.0 and got[7] == np.float32(255) * ONE_255TH and got[2] == np.float32(120) * ONE_255TH


def test_bc4_equal_endpoints_are_the_four_step_mode():
    got = bu.bc4_texels(np.array([77, 77] + IDENTITY_CODES, np.uint8))
    assert np.array_equal(got.view(np.uint32), fraction([385, 385, 385, 385, 385, 385, 0, 1275] * 2, 5).view(np.uint32))
    assert got[0] == np.float32(77) * ONE_255TH


def test_bc4_texel_order_within_the_block():
    """one code differs: texel 5 (x = 1, y = 1) has code 1, bits 15..17 of the 48"""
    block = np.array([255, 0, 0x00, 0x80, 0x00, 0x00, 0x00, 0x00], np.uint8)
    want = np.full(16, np.float32(255) * ONE_255TH, np.float32)
    want[5] = 0.0
    assert np.array_equal(bu.bc4_texels(block), want)
    blocks = np.zeros((1, 1, 8), np.uint8)
    blocks[0, 0] = block
    assert np.array_equal(np.argwhere(bu.decode(bu.BC4, 0, blocks, 4, 4) == 0.0), [[1, 1]])


def test_bc3_and_bc5_read_their_own_eight_bytes():
    alpha, other = [200, 100] + IDENTITY_CODES, [100, 200] + IDENTITY_CODES
    six, four = fraction([1400, 700, 1300, 1200, 1100, 1000, 900, 800] * 2, 7), fraction([500, 1000, 600, 700, 800, 900, 0, 1275] * 2, 5)
    assert np.array_equal(bu.block_texels(bu.BC3, 0, np.array(alpha + [0xFF] * 8, np.uint8)), six)
    assert np.array_equal(bu.block_texels(bu.BC5, 0, np.array(alpha + other, np.uint8)), six)
    assert np.array_equal(bu.block_texels(bu.BC5, 1, np.array(alpha + other, np.uint8)), four)


BC1_CODES_0123 = [0xE4] * 4   # codes 0, 1, 2, 3 in every row


@pytest.mark.parametrize("endpoints,codes,want", [
    ([0x34, 0x12, 0x78, 0x56], BC1_CODES_0123, [255, 255, 255, 0] * 4),      # c0 = 0x1234 < c1 = 0x5678: code 3 is the hole
    ([0xCD, 0xAB, 0xCD, 0xAB], BC1_CODES_0123, [255, 255, 255, 0] * 4),      # c0 == c1: still the punch-through mode
    ([0x78, 0x56, 0x34, 0x12], BC1_CODES_0123, [255] * 16),                  # c0 > c1: four colours, no hole
    ([0x78, 0x56, 0x34, 0x12], [0xFF] * 4, [255] * 16),                      # ... whatever the codes
    ([0x00, 0x00, 0x01, 0x00], [0xFF, 0x03, 0xC0, 0x00], [0] * 4 + [0, 255, 255, 255] + [255, 255, 255, 0] + [255] * 4),
], ids=["less", "equal", "greater", "greater_all_3", "less_positions"])
def test_bc1_blocks(endpoints, codes, want):
    got = bu.bc1_texels(np.array(endpoints + codes, np.uint8))
    assert got.dtype == np.uint8 and got.tolist() == want


def test_bc2_all_sixteen_nibbles():
    """nibble i = i: the u64 0xFEDCBA9876543210; the colour half is not looked at"""
    block = np.array([0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE] + [0xA5] * 8, np.uint8)
    got = bu.block_texels(bu.BC2, 0, block)
    assert got.dtype == np.uint8 and got.tolist() == [17 * i for i in range(16)] and got[15] == 255


def test_decode_places_blocks_and_crops():
    """a 5 x 6 BC2 image: 2 x 2 blocks; texel (x, y) comes from block (x / 4, y / 4), position 4 * (y % 4) + x % 4"""
    blocks = np.zeros((2, 2, 16), np.uint8)
    for by in range(2):
        for bx in range(2):
            blocks[by, bx, :8] = [(2 * by + bx) * 0x11] * 8       # every nibble of the block = its number
    blocks[1, 0, 2] = 0xF3                                         # texels 4 and 5 of block (0, 1): nibbles 3 and 15
    got = bu.decode(bu.BC2, 0, blocks, 5, 6)
    want = np.zeros((6, 5), np.uint8)
    want[:4, 4:] = 17
    want[4:, :4] = 34
    want[4:, 4:] = 51
    want[5, 0], want[5, 1] = 51, 255
    assert got.shape == (6, 5) and np.array_equal(got, want)


@pytest.mark.parametrize("fc", bu.FORMATS, ids=bu.format_id)
def test_random_blocks_against_pillow(fc):
    Image = pytest.importorskip("PIL.Image")
    fmt, channel = fc
    blocks = np.random.RandomState(100 + fmt).randint(0, 256, size=(16, 16, bu.BLOCK_BYTES[fmt])).astype(np.uint8)   # 256 blocks, 64 x 64 texels
    blocks[0, 0, 8 * channel + 1] = blocks[0, 0, 8 * channel]             # (one block with equal endpoints)
    img = Image.open(io.BytesIO(bu.dds_bytes(fmt, blocks, 64, 64)))
    img.load()
    if fmt in (bu.BC1, bu.BC2, bu.BC3):
        assert img.mode == "RGBA"
        theirs = np.array(img.getchannel("A"))
    elif fmt == bu.BC4:
        assert img.mode == "L"
        theirs = np.array(img)
    else:
        assert img.mode == "RGB"
        theirs = np.array(img)[:, :, channel]
    assert theirs.shape == (64, 64) and theirs.dtype == np.uint8
    if fmt in (bu.BC1, bu.BC2):
        ours = bu.decode(fmt, channel, blocks, 64, 64)
    else:
        n, d = bu.bc4_fraction(bu.relevant_bytes(fmt, channel, blocks))
        floored = np.floor(n.astype(np.float32) / d.astype(np.float32)).astype(np.uint8)
        ours = floored.reshape(16, 16, 4, 4).transpose(0, 2, 1, 3).reshape(64, 64)
    assert np.array_equal(ours, theirs)
