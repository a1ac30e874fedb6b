"""Adaptive supersampling (include/rm.h rm_refine_rgba8) restated in numpy: the
edge rule, the sample offsets and the tree mean of a refined pixel.  Written
from the rule's statement, not from the library's code: the tests compare the
two."""
import numpy as np

# sample offsets in pixels from the pixel centre, in lane order
OFFSETS = {
    2: [(0.25, 0.25), (-0.25, -0.25)],
    4: [(-0.125, -0.375), (0.375, -0.125), (-0.375, 0.125), (0.125, 0.375)],
    8: [(v[0] / 16.0, v[1] / 16.0)
        for v in [(1, -3), (-1, 3), (5, 1), (-3, -5), (-5, 5), (-7, -1), (3, 7), (7, -7)]],
}


def offsets(K):
    return np.asarray(OFFSETS[K], np.float32)


def seeds(K):
    """u_seed1 = o + 0.5: the value that makes rm_render_accumulate render sample o."""
    return offsets(K) + np.float32(0.5)


def edge_mask(frame, threshold):
    """uint8 [H, W]: 1 where some channel of R, G, B has max - min >= threshold
    over the pixel's 3x3 neighbourhood (edge-padded: coordinates clamped)."""
    w = np.asarray(frame).view(np.uint32)
    H, W = w.shape
    edge = np.zeros((H, W), bool)
    for shift in (0, 8, 16):
        c = np.pad(((w >> shift) & 255).astype(np.int32), 1, mode="edge")
        win = np.stack([c[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
        edge |= (win.max(0) - win.min(0)) >= int(threshold)
    return edge.astype(np.uint8)


def tree_mean(samples):
    """The mean of K = 2, 4 or 8 float32 arrays as the refine sums them: the
    pairwise tree in order, ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)),
    times 1 / K, each operation rounded to f32."""
    level = [np.asarray(s, np.float32) for s in samples]
    K = len(level)
    assert K in (2, 4, 8)
    while len(level) > 1:
        level = [(level[i] + level[i + 1]).astype(np.float32) for i in range(0, len(level), 2)]
    return (level[0] * np.float32(1.0 / K)).astype(np.float32)
