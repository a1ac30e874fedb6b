"""bloom.frag for lod > 0 by its definition, in float64, and a float32 numpy
restatement of the run tables (bloom_coord / bloom_cell of oracle/rm_oracle.c
and csrc/rm_post.hip).  CPU only.

per_tap_bloom sums the 25 bilinear taps of each level (CLAMP_TO_EDGE, texel
centres) and blends the two levels by fr.  A bilinear tap over a level L is
Wy L Wx^T with Wy, Wx the tap's row and column interpolation matrices (two
non-zero weights per output row or column); the taps of one tap row j share
Wy, so their weighted sum is Wy L (sum_i g_ij Wx_i)^T: five products per
level instead of 25 gathers per pixel.  `bilinear` is the same filter by
gathers, used for the pixel's own texel (and to check the matrix form).

`rows` / `cols` restrict the evaluation to those pixel rows and columns.
`mutant` names a one-line error of the definition (MUTANTS): what the suite's
content must be able to tell from the real thing.
"""
import numpy as np

import oracle

GAUSS = np.array([[41, 26, 7], [26, 16, 4], [7, 4, 1]]) / 273.0

MUTANTS = {
    "tap_x": "tap (i, j) = (2, 0) reads one cell further in x",
    "tap_y": "tap (i, j) = (0, 2) reads one cell further in y",
    "aspect": "the tap offset's aspect factor is W/H instead of H/W",
    "gauss": "the Gaussian weights 26 and 16 are swapped",
    "threshold": "the threshold is 0.3 + 1/255",
    "d2_as_d1": "level d2 is read as level d1",
    "no_flip": "v is not flipped in the taps",
    "d2_shift": "level d2 is shifted by one texel in x",
}


def channels(a):
    a = np.asarray(a, np.uint32)
    return np.stack([(a >> (8 * c)) & 255 for c in range(4)], -1).astype(np.int64)


def bilinear(L, uu, vv):
    """[len(vv), len(uu), 3]: the level L ([h, w, 3]) at normalized (uu x vv)."""
    h, w = L.shape[:2]
    x = uu * w - 0.5
    y = vv * h - 0.5
    fx, fy = np.floor(x), np.floor(y)
    a, b = (x - fx)[None, :, None], (y - fy)[:, None, None]
    x0, x1 = np.clip(fx, 0, w - 1).astype(int), np.clip(fx + 1, 0, w - 1).astype(int)
    y0, y1 = np.clip(fy, 0, h - 1).astype(int), np.clip(fy + 1, 0, h - 1).astype(int)
    return ((1 - b) * ((1 - a) * L[np.ix_(y0, x0)] + a * L[np.ix_(y0, x1)])
            + b * ((1 - a) * L[np.ix_(y1, x0)] + a * L[np.ix_(y1, x1)]))


def interp_matrix(t, n, shift=0):
    """[len(t), n]: the linear filter over n texels at normalized positions t
    (CLAMP_TO_EDGE), reading `shift` cells further."""
    x = t * n - 0.5
    f = np.floor(x)
    a = x - f
    i0, i1 = np.clip(f + shift, 0, n - 1).astype(int), np.clip(f + shift + 1, 0, n - 1).astype(int)
    M = np.zeros((len(t), n))
    r = np.arange(len(t))
    M[r, i0] += 1 - a
    M[r, i1] += a
    return M


def rgb(a):
    """[h, w] RGBA8 words -> [h, w, 3] uint8 (a view of the words' bytes)."""
    a = np.ascontiguousarray(a, "<u4")
    return a.view(np.uint8).reshape(a.shape + (4,))[..., :3]


def tap_operators(W, H, rows=None, cols=None, mutant=None):
    """The 25 taps of each level as matrices, for the pixels rows x cols of a
    W x H image: [(level, whether it is read as d2, blend weight, Wy, sum_i g_ij
    Wx_i)], one entry per
    tap row j (two for the row that holds the tap_y mutant's tap).  They depend
    on the size alone, so one set serves every image of a size."""
    assert mutant is None or mutant in MUTANTS, mutant
    lod, d1, d2 = oracle.bloom_levels(W, H)
    fr = lod - np.floor(lod)
    sizes = level_sizes(W, H)
    rows = np.arange(H) if rows is None else np.asarray(rows)
    cols = np.arange(W) if cols is None else np.asarray(cols)
    G = GAUSS.copy()
    if mutant == "gauss":
        G[0, 1] = G[1, 0] = 16 / 273.0
        G[1, 1] = 26 / 273.0
    aspect = W / H if mutant == "aspect" else H / W
    u = (cols + 0.5) / W
    v = (rows + 0.5) / H if mutant == "no_flip" else 1.0 - (rows + 0.5) / H
    ops = []
    for second, (lev, wgt) in enumerate(((d1, 1 - fr), (d1 if mutant == "d2_as_d1" else d2, fr))):
        w, h = sizes[lev]
        for j in range(-2, 3):
            for ys in (0, 1):  # the taps of row j by how far off they read in y (1: the tap_y mutant's one tap)
                taps = [i for i in range(-2, 3) if ((mutant == "tap_y" and (i, j) == (0, 2)) == bool(ys))]
                if not taps:
                    continue
                Mx = sum(G[abs(i), abs(j)] * interp_matrix(u + i * aspect * 0.05, w,
                                                           int(mutant == "tap_x" and (i, j) == (2, 0))) for i in taps)
                ops.append((lev, bool(second), wgt, interp_matrix(v + j * 0.05, h, ys), Mx))
    return ops


def blurred(img, levels, rows=None, cols=None, mutant=None, ops=None):
    """bloom.frag's blurred sum `bl` ([rows, cols, 3], before the threshold);
    ops = tap_operators of the same size, rows, cols and mutant, if at hand."""
    H, W = img.shape
    ops = tap_operators(W, H, rows, cols, mutant) if ops is None else ops
    lv = {}
    acc = 0.0
    for lev, second, wgt, My, Mx in ops:
        if (lev, second) not in lv:
            L = rgb(img if lev == 0 else levels[lev - 1]) / 255.0
            if mutant == "d2_shift" and second:
                L = np.concatenate([L[:, 1:], L[:, -1:]], 1)
            lv[lev, second] = L
        L = lv[lev, second]
        h, w = L.shape[:2]
        rowsum = (My @ L.reshape(h, w * 3)).reshape(len(My), w, 3)
        acc = acc + wgt * np.tensordot(rowsum, Mx, axes=([1], [1]))
    return acc.transpose(0, 2, 1)


def per_tap_bloom(img, levels, rows=None, cols=None, mutant=None, ops=None):
    """bloom.frag for lod > 0 by its definition, in float64: 25 bilinear taps
    per level (CLAMP_TO_EDGE, texel centres), the two levels blended by fr.
    [rows, cols, 3] bytes."""
    H, W = img.shape
    rows = np.arange(H) if rows is None else np.asarray(rows)
    cols = np.arange(W) if cols is None else np.asarray(cols)
    acc = blurred(img, levels, rows, cols, mutant, ops)
    base = bilinear(rgb(img), (cols + 0.5) / W, 1.0 - (rows + 0.5) / H) / 255.0
    thr = 0.3 + 1 / 255.0 if mutant == "threshold" else 0.3
    out = np.clip(base + np.maximum(acc - thr, 0.0), 0.0, 1.0)
    return np.rint(out * 255.0).astype(np.int64)


# ------------------------------------------------ run tables, in float32


def level_sizes(W, H):
    """[(w, h)] of levels 0..d2."""
    _, _, d2 = oracle.bloom_levels(W, H)
    out = [(W, H)]
    for _ in range(d2):
        w, h = out[-1]
        out.append((max(1, w >> 1), max(1, h >> 1)))
    return out


def axis_cells(N, lw, is_y, off):
    """bloom_coord and bloom_cell along one axis: (coord float32 [N], cells
    int [N, 5]) for N pixels over a level of lw texels, off = the five tap
    offsets (float32)."""
    f32 = np.float32
    t = (np.arange(N, dtype=f32) + f32(0.5)) / f32(N)
    coord = ((f32(1.0) - t) if is_y else t) * f32(lw) - f32(0.5)
    assert coord.dtype == np.float32
    d = off.astype(np.float64) * float(lw)
    x = np.floor(coord.astype(np.float64)[:, None] + d[None, :])
    return coord, np.clip(x, -1, lw - 1).astype(np.int64)


def axes(W, H):
    """The four axes of launch_bloom / oracle_bloom (level d1 x, y; level d2 x,
    y): dicts of N, lw, is_y, coord, cells."""
    f32 = np.float32
    _, d1, d2 = oracle.bloom_levels(W, H)
    sizes = level_sizes(W, H)
    iaspect, scale = f32(H) / f32(W), f32(0.05)
    taps = np.arange(-2, 3).astype(f32)
    out = []
    for a in range(4):
        is_y = a & 1
        lw = sizes[d1 if a < 2 else d2][is_y]
        off = taps * scale if is_y else (taps * iaspect) * scale
        assert off.dtype == np.float32
        coord, cells = axis_cells(H if is_y else W, lw, is_y, off)
        out.append(dict(N=H if is_y else W, lw=lw, is_y=is_y, coord=coord, cells=cells))
    return out


def run_starts(cells):
    """Indices along the axis where the cell tuple differs from its predecessor's (0 included)."""
    change = np.any(cells[1:] != cells[:-1], axis=1)
    return np.concatenate([[0], 1 + np.flatnonzero(change)])


def base_weights(N, is_y):
    """BloomBase.f along one axis: the float32 bilinear weight of the pixel's own texel."""
    f32 = np.float32
    t = (np.arange(N, dtype=f32) + f32(0.5)) / f32(N)
    x = ((f32(1.0) - t) if is_y else t) * f32(N) - f32(0.5)
    return x - np.floor(x)


def subset(W, H, rng, extra=300, limit=500_000):
    """(rows, cols) to evaluate the definition on: everything up to `limit`
    pixels; above, every row and column where a run of either level starts and
    the one before it, the first and last three, and `extra` random others."""
    if W * H <= limit:
        return np.arange(H), np.arange(W)
    ax = axes(W, H)
    picked = []
    for n, pair in ((W, (ax[0], ax[2])), (H, (ax[1], ax[3]))):
        s = np.concatenate([run_starts(a["cells"]) for a in pair])
        idx = np.concatenate([s, s - 1, np.arange(3), n - 1 - np.arange(3), rng.integers(0, n, extra)])
        picked.append(np.unique(np.clip(idx, 0, n - 1)))
    return picked[1], picked[0]
