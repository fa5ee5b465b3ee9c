"""Writes tests/golden/bc7_alpha_blocks.npz: 256 forced blocks of each of the modes 0..7 (tests/bc7_util.py) and the alpha Pillow's BC7 decoder gives for them,
so that the reference decoder of tests/bc7_util.py stays pinned on machines without Pillow.  Needs Pillow; run from the repository root:
    python tests/golden/make_bc7_fixture.py"""
import io
import os
import sys
import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bc7_util as b7  # noqa: E402

PER_MODE = 256


def pillow_alpha(blocks):
    """(n, 16) blocks, n a multiple of 16 -> (n, 16) alpha bytes, through a DDS file of 16 blocks a row"""
    n = blocks.shape[0]
    grid = blocks.reshape(n // 16, 16, 16)
    im = Image.open(io.BytesIO(b7.dds_bytes(grid, 64, 4 * (n // 16))))
    a = np.array(im.convert("RGBA"))[..., 3]
    return a.reshape(n // 16, 4, 16, 4).transpose(0, 2, 1, 3).reshape(n, 16)


if __name__ == "__main__":
    blocks = np.stack([b7.blocks_of_mode(m, PER_MODE, 7000 + m) for m in range(8)])
    alpha = np.stack([pillow_alpha(blocks[m]) for m in range(8)])
    np.savez_compressed(os.path.join(HERE, "bc7_alpha_blocks.npz"), blocks=blocks, alpha=alpha.astype(np.uint8))
    print("modes 4..7: texels != 255:", [(alpha[m] != 255).mean() for m in range(4, 8)])
