"""Test images whose structure survives bloom's mip chain.

bloom.frag reads mip levels d1 and d2 = d1 + 1 (oracle.bloom_levels).  Uniform
noise is flat there (each texel the mean of 4^d noise texels), so a tap that
reads the wrong cell moves nothing.  These images are built from blocks of
2^d1 (or 2^d2) texels aligned to index 0: where every level is an exact
halving, texel k of level d is the mean of image texels [k 2^d, (k+1) 2^d),
so one block lands on one texel with its full contrast.

Every generator takes (W, H, rng) and returns an [H, W] uint32 RGBA8 image with
random alpha bytes (bloom ignores alpha and writes 255).  A block is never
smaller than 2 texels, so the images stay structured where d1 = 0 (lod <= 1).
"""
import numpy as np

import oracle

# the sizes of test_bloom_content_gpu.py by the path they take (test_bloom_content.py checks the claims)
PYRAMID = [(64, 448), (128, 896), (256, 1792), (256, 3584), (512, 7168), (1024, 14336)]  # <0>..<3>, s0 = 1, s0 = 2
FR0 = [(64, 640), (256, 2560)]  # lod an integer: level d2 has weight 0
RESAMPLE = [(1025, 333), (333, 1025), (2100, 1300)]  # per-level resample, odd level sizes, chunked scans
LOW_FR = [(1025, 333), (2100, 1300)]  # of RESAMPLE: fr = 0.06 and 0.02, level d2 weighs little
TAILS = [(W, H) for W in (257, 1100) for H in (449, 453, 463)]  # H = 1, 5, 15 (mod 16): strip and batch tails
LOD_BELOW_1 = [(70, 30), (2049, 48), (2049, 30)]  # d1 = 0: the frame itself is a level (2049 x 48: lod 1.26, d1 = 1)
MAGNIFY = [(40, 16), (300, 20), (1, 1), (3, 20)]  # lod <= 0: rm_bloom_kernel
GPU_SIZES = PYRAMID + RESAMPLE + TAILS + LOD_BELOW_1 + MAGNIFY + FR0


def block_sizes(W, H):
    """(2^d1, 2^d2) texels, each at least 2."""
    _, d1, d2 = oracle.bloom_levels(W, H)
    return 1 << max(d1, 1), 1 << max(d2, 1)


def pack(rgb, rng):
    """[H, W, 3] byte values -> [H, W] uint32 RGBA8 with random alpha."""
    out = np.empty(np.shape(rgb)[:2] + (4,), np.uint8)
    out[..., :3] = rgb
    out[..., 3] = rng.integers(0, 256, out.shape[:2], dtype=np.uint8)
    return np.ascontiguousarray(out.view("<u4")[..., 0], np.uint32)


def grid(W, H, B):
    """Blocks along y and x of a W x H image cut into B-texel blocks from index 0."""
    return -(-H // B), -(-W // B)


def spread(colours, W, H, B):
    """One colour per block, [nby, nbx, 3] -> the [H, W, 3] image."""
    return np.repeat(np.repeat(np.asarray(colours, np.uint8), B, 0), B, 1)[:H, :W]


def block(W, H, rng):
    """An independent random colour per 2^d1-texel block."""
    B = block_sizes(W, H)[0]
    return pack(spread(rng.integers(0, 256, grid(W, H, B) + (3,)), W, H, B), rng)


def block2(W, H, rng):
    """An independent random colour per 2^d2-texel block: level d2 has full contrast too."""
    B = block_sizes(W, H)[1]
    return pack(spread(rng.integers(0, 256, grid(W, H, B) + (3,)), W, H, B), rng)


def dark(W, H, rng):
    """Block colours uniform in 0..153 (0.6): the blurred sum straddles bloom.frag's 0.3."""
    B = block_sizes(W, H)[0]
    return pack(spread(rng.integers(0, 154, grid(W, H, B) + (3,)), W, H, B), rng)


def checker(W, H, rng):
    """0/255 checker of 2^d1-texel cells, each channel with its own phase; the
    odd rows of the dark cells carry 1, so that where the levels are exact
    halvings the 4-texel sums of the dark cells at level 1 (0 + 0 + 1 + 1) and
    all those of level d2 (0 + 255 + 255 + 0 of level d1) are exact
    half-to-even ties."""
    B = block_sizes(W, H)[0]
    y, x = np.arange(H), np.arange(W)
    phase = rng.integers(0, 2, (2, 3))
    rgb = np.empty((H, W, 3), np.uint8)
    for c in range(3):
        on = (((x // B + phase[0, c]) & 1)[None, :] ^ ((y // B + phase[1, c]) & 1)[:, None]).astype(np.uint8)
        rgb[..., c] = on * np.uint8(255) + (1 - on) * (y & 1).astype(np.uint8)[:, None]
    return pack(rgb, rng)


def border(W, H, rng):
    """Black inside a bright frame one 2^d1-texel block wide: the taps, which
    reach 0.1 of the image beyond every edge, sum the clamped cells -1 and
    lw - 1 of each level with weight."""
    B = block_sizes(W, H)[0]
    rgb = np.zeros((H, W, 3), np.uint8)
    colour = rng.integers(128, 256, 3, dtype=np.uint8)
    rgb[:B] = rgb[max(H - B, 0):] = rgb[:, :B] = rgb[:, max(W - B, 0):] = colour
    return pack(rgb, rng)


def impulse(W, H, rng):
    """Black with a few single bright 2^d1-texel blocks: one in the corner
    (0, 0), one on the right edge, the others anywhere."""
    B = block_sizes(W, H)[0]
    nby, nbx = grid(W, H, B)
    colours = np.zeros((nby, nbx, 3), np.uint8)
    where = [(0, 0), (nby // 2, nbx - 1)] + [(int(rng.integers(nby)), int(rng.integers(nbx))) for _ in range(4)]
    for by, bx in where:
        colours[by, bx] = rng.integers(128, 256, 3)
    return pack(spread(colours, W, H, B), rng)


def flat0(W, H, rng):
    return pack(np.zeros((H, W, 3), np.uint8), rng)


def flat255(W, H, rng):
    return pack(np.full((H, W, 3), 255, np.uint8), rng)


KINDS = {"block": block, "block2": block2, "dark": dark, "checker": checker, "border": border, "impulse": impulse,
         "flat0": flat0, "flat255": flat255}


def noise(W, H, rng):
    """Uniform random words: the content the older bloom tests use (not in KINDS)."""
    return rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)


def one_block_changed(img, rng):
    """A copy of img with the RGB of one 2^d2-texel block inverted (255 - v
    differs from v in every channel); returns (copy, (y0, y1, x0, x1))."""
    H, W = img.shape
    B = block_sizes(W, H)[1]
    nby, nbx = grid(W, H, B)
    by, bx = int(rng.integers(nby)), int(rng.integers(nbx))
    y0, y1, x0, x1 = by * B, min((by + 1) * B, H), bx * B, min((bx + 1) * B, W)
    out = img.copy()
    out[y0:y1, x0:x1] ^= np.uint32(0x00ffffff)
    return out, (y0, y1, x0, x1)
