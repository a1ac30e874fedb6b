"""float32 numpy restatement of the FXAA pass (post.frag:16-61, main :135-144)
that also returns its intermediates, and the seeded frames the FXAA shape
tests run on (tests/test_fxaa_claims.py, tests/test_fxaa_shapes_gpu.py).

The restatement is independent of oracle/rm_oracle.c (oracle.fxaa) but keeps
its association operation for operation: every intermediate is a float32, no
multiply-add is fused, divisions are correctly rounded, dot(rgb, luma) sums
left to right, dirReduce sums ((NW + NE) + SW) + SE, k1 = 1/3 - 0.5 formed in
float32, and the store is rint(clip(c, 0, 1) * 255).  tests/test_fxaa_claims.py
pins it to oracle.fxaa bit for bit; that licenses reading the intermediates
(the clamped span, the texel every tap addresses) the oracle does not expose.

Coordinates: frames are [H, W] uint32 RGBA8 words, row 0 first.  Output pixel
(x, y) samples around texel (x, H - 1 - y): post.frag flips the frame.
"""
import collections

import numpy as np

f32 = np.float32

K255 = f32(1.0) / f32(255.0)
REDUCE_MIN = f32(1.0) / f32(128.0)
REDUCE_MUL = f32(1.0) / f32(8.0)
SPAN_MAX = f32(8.0)
K1 = f32(1.0) / f32(3.0) - f32(0.5)
K2 = f32(2.0) / f32(3.0) - f32(0.5)
SPAN_K = (K1, K2, f32(-0.5), f32(0.5))  # the four span taps, in post.frag's order
FIXED = ((-1, -1), (1, -1), (-1, 1), (1, 1), (0, 0))  # NW, NE, SW, SE, M as (x, y) steps of inverseVP

Fxaa = collections.namedtuple("Fxaa", "out dxs dys fixed_taps span_taps")


def tex_coord(u, n):
    """The texel texture() addresses on an axis of n texels under GL_NEAREST,
    before CLAMP_TO_EDGE: floor(u * n), float32 product."""
    return np.floor(u * f32(n)).astype(np.int64)


def axis_coords(n, flip):
    """post.frag:138's coordinate of every pixel along an axis of n pixels and
    inverseVP's component: ((c + .5) / n, flipped to 1 - that for rows), 1 / n."""
    t = (np.arange(n, dtype=f32) + f32(0.5)) / f32(n)
    return (f32(1.0) - t if flip else t), f32(1.0) / f32(n)


def fixed_tap_coords(n, flip):
    """The unclamped texel of the taps -1, 0, +1 along an axis: [3, n] int64."""
    c, iv = axis_coords(n, flip)
    return np.stack([tex_coord(c + f32(s) * iv, n) for s in (-1.0, 0.0, 1.0)])


def _chan(t, k):
    return ((t >> np.uint32(8 * k)) & np.uint32(255)).astype(f32) * K255


def _rgb(t):
    return _chan(t, 0), _chan(t, 1), _chan(t, 2)


def _luma(c):
    return (c[0] * f32(0.299) + c[1] * f32(0.587)) + c[2] * f32(0.114)


def _unorm8(c):
    return np.rint(np.minimum(np.maximum(c, f32(0.0)), f32(1.0)) * f32(255.0)).astype(np.uint32)


def fxaa(img_u32, x_range=None):
    """FXAA of an [H, W] RGBA8 frame -> Fxaa(out, dxs, dys, fixed_taps, span_taps).

    out         [H, w] uint32, the stored frame
    dxs, dys    [H, w] float32, the clamped span in texels (before * 1/W, * 1/H)
    fixed_taps  five (tx, ty) of the NW, NE, SW, SE, M taps: unclamped texel
                coordinates, tx [1, w] and ty [H, 1] (they depend on one axis)
    span_taps   four (tx, ty) [H, w] of the span taps, unclamped
    x_range     (x0, x1): only these output columns of the frame (w = x1 - x0),
                addressed as in the whole frame; default every column
    """
    img = np.ascontiguousarray(img_u32, np.uint32)
    H, W = img.shape
    x0, x1 = (0, W) if x_range is None else x_range
    fx, ivx = axis_coords(W, False)
    fy, ivy = axis_coords(H, True)
    fx = fx[None, x0:x1]
    fy = fy[:, None]

    def fetch(tx, ty):
        return img[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]

    fixed_taps, lum = [], []
    for sx, sy in FIXED:
        tx = tex_coord(fx + f32(sx) * ivx, W)
        ty = tex_coord(fy + f32(sy) * ivy, H)
        fixed_taps.append((tx, ty))
        t = fetch(tx, ty)
        lum.append(_luma(_rgb(t)))
    tM = t
    lNW, lNE, lSW, lSE, lM = lum
    lMin = np.minimum(lM, np.minimum(np.minimum(lNW, lNE), np.minimum(lSW, lSE)))
    lMax = np.maximum(lM, np.maximum(np.maximum(lNW, lNE), np.maximum(lSW, lSE)))
    dx = -((lNW + lNE) - (lSW + lSE))
    dy = (lNW + lSW) - (lNE + lSE)
    dir_reduce = np.maximum((((lNW + lNE) + lSW) + lSE) * (f32(0.25) * REDUCE_MUL), REDUCE_MIN)
    rcp = f32(1.0) / (np.minimum(np.abs(dx), np.abs(dy)) + dir_reduce)
    dxs = np.minimum(SPAN_MAX, np.maximum(-SPAN_MAX, dx * rcp))
    dys = np.minimum(SPAN_MAX, np.maximum(-SPAN_MAX, dy * rcp))
    dx = dxs * ivx
    dy = dys * ivy
    span_taps, s = [], []
    for k in SPAN_K:
        tx = tex_coord(fx + dx * k, W)
        ty = tex_coord(fy + dy * k, H)
        span_taps.append((tx, ty))
        s.append(_rgb(fetch(tx, ty)))
    a = [(s[0][c] + s[1][c]) * f32(0.5) for c in range(3)]
    b = [a[c] * f32(0.5) + (s[2][c] + s[3][c]) * f32(0.25) for c in range(3)]
    lB = _luma(b)
    use_a = (lB < lMin) | (lB > lMax)
    c = [np.where(use_a, a[k], b[k]) for k in range(3)]
    out = _unorm8(c[0]) | (_unorm8(c[1]) << 8) | (_unorm8(c[2]) << 16) | (_unorm8(_chan(tM, 3)) << 24)
    return Fxaa(out, dxs, dys, fixed_taps, span_taps)


def short_mask(r):
    """Pixels whose span is short: max(|dxs|, |dys|) <= 0.5 texel."""
    return np.maximum(np.abs(r.dxs), np.abs(r.dys)) <= f32(0.5)


def short_block_share(short):
    """The share of 8 x 8 output blocks (aligned to multiples of 8) that are
    wholly short; cells past the frame count as short."""
    H, W = short.shape
    full = np.ones(((H + 7) // 8 * 8, (W + 7) // 8 * 8), bool)
    full[:H, :W] = short
    blocks = full.reshape(full.shape[0] // 8, 8, full.shape[1] // 8, 8).all(axis=(1, 3))
    return float(blocks.mean())


# ------------------------------------------------------------------ frames


def noise(W, H):
    """Uniform 32-bit words (alpha random too), seeded by the shape."""
    rng = np.random.default_rng(W * 65536 + H)
    return rng.integers(0, 2**32, (H, W), dtype=np.uint64).astype(np.uint32)


def sparks(W, H):
    """Low-contrast ground, (n & 0x03030303) + 0x40506070, with one pixel in a
    hundred replaced by its raw noise word: an isolated pixel makes its
    diagonal neighbours long-span, so a workgroup holds wholly short 8 x 8
    blocks next to blocks with a few long pixels."""
    rng = np.random.default_rng(W * 65536 + H)
    n = rng.integers(0, 2**32, (H, W), dtype=np.uint64).astype(np.uint32)
    base = (n & np.uint32(0x03030303)) + np.uint32(0x40506070)
    return np.where(rng.random((H, W)) < 0.01, n, base)


CONTENTS = {"noise": noise, "sparks": sparks}

# (W, H) by what they exercise (the kernels' tiles are 64 x 32 and 64 x 16, the
# LDS kernel's halo 4, its largest side 2^20)
M = 1 << 20
SMALL = [(1, 1), (2, 1), (1, 2), (3, 3), (7, 5), (1, 300), (300, 1)]
RAGGED = [(63, 31), (64, 32), (65, 33), (130, 70), (257, 3), (8, 200), (191, 97)]
LIMIT = [(M, 3), (M - 1, 2), (3, M), (2, M - 1)]
FALLBACK = [(M + 1, 2), (2, M + 1), (M + 1, 18)]
