"""The adaptive dispatch order's sort (rm_kernels.hip rm_sched_hist and
rm_sched_scatter behind rm::launch_tile_order) restated in
numpy: the log bucket of a tile's duration (rm_device.h sched_bucket), the
dilated sort key (tile_key, tile_key_r), and what an order has to be -- a
permutation whose keys' buckets do not decrease.  Within a bucket any order is
allowed, so nothing here needs a tolerance.

Nothing in this file runs on a GPU; tests/test_tile_order_ref.py checks it
against pure-Python loops, tests/test_tile_order_gpu.py checks the kernels
against it."""
import numpy as np

BUCKETS = 256       # kSchedBuckets
TOP_BUCKET = 47     # bucket(0xffffffff): the costliest bucket a uint32 duration reaches
REACHABLE = BUCKETS - TOP_BUCKET  # 209 buckets, 47..255
U32_MAX = 0xFFFFFFFF


def bucket(cost):
    """sched_bucket: the uint32 duration as float32 (round to nearest even),
    plus float32(64) (rounded again); the exponent and three mantissa bits of
    the sum, counted from 2^6, clamped to 0..255; 255 - that (0 = costliest)."""
    c = np.asarray(cost, dtype=np.uint32)
    f = (c.astype(np.float32) + np.float32(64)).astype(np.float32)
    bits = np.atleast_1d(f).view(np.uint32).reshape(c.shape)
    b = (bits >> np.uint32(20)).astype(np.int64) - ((127 + 6) << 3)
    return (BUCKETS - 1 - np.clip(b, 0, BUCKETS - 1)).astype(np.uint8)


def key(cost, n, gx, r):
    """The sort key of each of the n tiles of a gx-wide grid: the largest
    duration in the (2r + 1)^2 window around it, columns clipped to [0, gx),
    rows to >= 0 and tile indices to < n; r = 0: the duration itself.
    (Shifted maxima, rows then columns: the clipped window is a rectangle, and
    the tiles past n of the last row hold 0, which no maximum notices.)"""
    cost = np.asarray(cost, dtype=np.uint32).reshape(-1)[:n]
    assert cost.size == n and gx >= 1
    if r <= 0:
        return cost.copy()
    gy = -(-n // gx)
    g = np.zeros(gy * gx, np.uint32)
    g[:n] = cost
    g = g.reshape(gy, gx)
    h = g.copy()
    for d in range(1, min(r, gx - 1) + 1):
        np.maximum(h[:, d:], g[:, :-d], out=h[:, d:])
        np.maximum(h[:, :-d], g[:, d:], out=h[:, :-d])
    v = h.copy()
    for d in range(1, min(r, gy - 1) + 1):
        np.maximum(v[d:], h[:-d], out=v[d:])
        np.maximum(v[:-d], h[d:], out=v[:-d])
    return v.reshape(-1)[:n].copy()


def check_order(order, cost, n, gx, r):
    """None if `order` is a dispatch order the sort may give for these
    durations: a permutation of 0..n-1 along which bucket(key) does not
    decrease.  Otherwise a message that names the first offending position."""
    order = np.asarray(order).reshape(-1).astype(np.int64)
    if order.size != n:
        return f"the order has {order.size} entries for {n} tiles"
    bad = np.flatnonzero((order < 0) | (order >= n))
    if bad.size:
        p = int(bad[0])
        return f"position {p}: entry {int(order[p])} is no tile of 0..{n - 1} ({bad.size} such entries)"
    first = np.full(n, -1, np.int64)
    first[order[::-1]] = np.arange(n - 1, -1, -1)  # (the earliest position of each tile wins)
    again = np.flatnonzero(first[order] != np.arange(n))
    if again.size:
        p = int(again[0])
        missing = np.flatnonzero(first < 0)
        return (f"position {p}: tile {int(order[p])} again (first at position {int(first[order[p]])}); "
                f"{missing.size} tiles are never dispatched, the first is tile {int(missing[0])}")
    assert np.array_equal(np.sort(order), np.arange(n))
    b = bucket(key(cost, n, gx, r))[order].astype(np.int64)
    down = np.flatnonzero(b[1:] < b[:-1])
    if down.size:
        p = int(down[0]) + 1
        return (f"position {p}: tile {int(order[p])} of bucket {int(b[p])} after tile {int(order[p - 1])} of bucket "
                f"{int(b[p - 1])}: a costlier tile dispatched later ({down.size} such steps)")
    return None


# ------------------------------------------------------------------ cases

def bucket_floor(b):
    """The smallest duration of bucket b (47..255), by bisection on the
    restated bucket (which does not increase with the duration)."""
    assert TOP_BUCKET <= b < BUCKETS
    lo, hi = 0, U32_MAX  # bucket(lo) may be > b, bucket(hi) <= b
    while lo < hi:
        mid = (lo + hi) // 2
        if int(bucket(mid)) <= b:
            hi = mid
        else:
            lo = mid + 1
    assert int(bucket(lo)) == b, (b, lo)
    return lo


_EDGES = None


def edge_values():
    """Where the bucket can go wrong, in increasing order: every reachable
    bucket's smallest duration and that minus 1, 0 and 0xffffffff, and above
    2^24, where the conversion to float rounds, 2^k (1 + m/8) minus 1, 64, 65,
    127, 128 and 129 for k = 25..31 and m = 0..7."""
    global _EDGES
    if _EDGES is None:
        v = {0, U32_MAX}
        for b in range(TOP_BUCKET, BUCKETS):
            f = bucket_floor(b)
            v.update((f, max(f - 1, 0)))
        for k in range(25, 32):
            for m in range(8):
                v.update((1 << k) + m * (1 << (k - 3)) - d for d in (1, 64, 65, 127, 128, 129))
        _EDGES = np.array(sorted(v), dtype=np.uint32)
    return _EDGES


PATTERNS = ("flat", "log", "edges", "hot")
HOT_COST = 100000


def costs(pattern, n, seed=0, hot=None):
    """n tile durations (uint32) of one pattern:
    flat   every tile 1000: one bucket holds every tile, every scatter block
           reserves from one cursor;
    log    2^U[0, 32);
    edges  edge_values() cycled over the grid, from a start the seed picks;
    hot    zeros and one tile, `hot`, of 100000."""
    rng = np.random.default_rng([seed, n, PATTERNS.index(pattern)])
    if pattern == "flat":
        return np.full(n, 1000, np.uint32)
    if pattern == "log":
        return np.minimum(np.floor(np.exp2(rng.uniform(0.0, 32.0, n))), float(U32_MAX)).astype(np.uint64).astype(np.uint32)
    if pattern == "edges":
        e = edge_values()
        return e[(int(rng.integers(e.size)) + np.arange(n)) % e.size]
    if pattern == "hot":
        c = np.zeros(n, np.uint32)
        c[hot] = HOT_COST
        return c
    raise ValueError(pattern)


def hot_population(n, gx, r, hot):
    """The number of tiles whose key lands in the hot tile's bucket."""
    b = bucket(key(costs("hot", n, hot=hot), n, gx, r))
    return int((b == b[hot]).sum())
