"""Adjacent-float tools shared by the point generators of the tests
(tests/scene_o_rules.py, tests/lib_edges.py): steps of k ulps, bisection of a
pair of points onto a branch of a boolean function, and the adjacency check.
Test infrastructure only."""
import numpy as np

f32 = np.float32


def ulp_step(v, k):
    """v moved by k float32 ulps (k < 0: down)."""
    v = np.asarray(v, f32).copy()
    to = f32(np.inf) if k > 0 else f32(-np.inf)
    for _ in range(abs(k)):
        v = np.nextafter(v, to)
    return v


def straddle(g, a, b, cross=48):
    """Bisect between points a, b [n, 3] (float32) at which the boolean g
    differs, until neither end moves: each pair ends on floats that are adjacent
    (or equal) in every coordinate, with g still different at its ends.

    Returns (points, a, b): both ends and, per coordinate, their 1..4-ulp
    neighbours: in a coordinate where the ends differ those on the far side of
    the other end (the near side holds the other end's), in a coordinate where
    they are equal those on both sides, for the first `cross` pairs only (the
    point budget)."""
    a = np.ascontiguousarray(a, f32).copy()
    b = np.ascontiguousarray(b, f32).copy()
    ga = g(a)
    assert (ga != g(b)).all(), "straddle: g must differ at the two ends"
    for _ in range(400):  # (a crossing at 0 is bisected down to the denormals: ~180 halvings)
        mid = ((a.astype(np.float64) + b.astype(np.float64)) * 0.5).astype(f32)
        to_a = g(mid) == ga
        na = np.where(to_a[:, None], mid, a)
        nb = np.where(to_a[:, None], b, mid)
        moved = (na != a).any() or (nb != b).any()
        a, b = na, nb
        if not moved:
            break
    else:
        raise AssertionError("straddle: no convergence")
    pts = [a, b]
    first = np.arange(len(a)) < cross
    for end, other in ((a, b), (b, a)):
        for c in range(3):
            # away from the other end (towards it lie the other end's own neighbours)
            side = np.sign(end[:, c].astype(np.float64) - other[:, c])
            for k in (1, 2, 3, 4):
                for s in (1, -1):
                    sel = (side == s) | ((side == 0) & first)
                    if sel.any():
                        n = end[sel].copy()
                        n[:, c] = ulp_step(n[:, c], s * k)
                        pts.append(n)
    return np.concatenate(pts), a, b


def adjacent_pairs(a, b):
    """Pairs that differ in exactly one coordinate, by one ulp."""
    diff = a != b
    one = diff.sum(-1) == 1
    nxt = np.nextafter(a, b)
    return one & ((nxt == b) | ~diff).all(-1)
