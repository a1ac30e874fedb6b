"""tests/tile_order_ref.py, the numpy restatement the sort kernels are checked
against (tests/test_tile_order_gpu.py), checked itself: bucket and key against
pure-Python loops (integer arithmetic, float32 through struct), the facts
DESIGN.md 2.6 states about the bucket, the hot tile's window counts, and
check_order against hand-made wrong orders -- each of them an order a subtly
wrong sort kernel would give, so a kernel that gave one would fail the GPU
tests."""
import struct

import numpy as np
import pytest

from tests import sentinel
from tests import tile_order_ref as ref

GRIDS = [(1, 1), (35, 7), (10, 2), (80, 2), (33, 7)]  # (n, gx): 1x1, 7x5, 2x5, 2x40, 7 wide with a short last row


def f32(x):
    """x (an int or a float, exact in a double) rounded to float32, to nearest even."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def py_bucket(cost):
    s = f32(f32(cost) + 64.0)  # (the sum of two float32 is exact in a double: one rounding each)
    bits = struct.unpack("<I", struct.pack("<f", s))[0]
    b = (bits >> 20) - ((127 + 6) << 3)
    return 255 - min(max(b, 0), 255)


def py_key(cost, n, gx, r):
    out = []
    for i in range(n):
        x, y = i % gx, i // gx
        m = 0
        for yy in range(y - r, y + r + 1):
            for xx in range(x - r, x + r + 1):
                j = yy * gx + xx
                if yy >= 0 and 0 <= xx < gx and j < n:
                    m = max(m, int(cost[j]))
        out.append(m)
    return out


def wrapped_key(cost, n, gx, r):
    """A wrong key: the window's columns are not clipped, so at column 0 it
    reads the end of the previous row (and at the last column the next row's
    start)."""
    out = []
    for i in range(n):
        m = 0
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                j = i + dy * gx + dx
                if 0 <= j < n:
                    m = max(m, int(cost[j]))
        out.append(m)
    return np.array(out, np.uint32)


def order_by(keys):
    """A right counting sort of these keys: buckets ascending, stable."""
    return np.argsort(ref.bucket(keys).astype(np.int64), kind="stable")


# ------------------------------------------------------------------ bucket

def test_bucket_equals_the_python_loop():
    vals = [int(v) for v in ref.edge_values()] + list(range(0, 600)) + [1000, 100000, (1 << 24) - 1, 1 << 24, (1 << 24) + 1]
    rng = np.random.default_rng(7)
    vals += [int(v) for v in ref.costs("log", 4000, 3)] + [int(v) for v in rng.integers(0, 1 << 32, 4000)]
    got = ref.bucket(np.array(vals, np.uint32))
    assert got.dtype == np.uint8
    assert got.tolist() == [py_bucket(v) for v in vals]
    assert int(ref.bucket(1000)) == py_bucket(1000)  # (a scalar as well)


def test_bucket_reaches_209_buckets_and_never_increases():
    # every duration below 2^20, then each octave strided, with the
    # neighbourhood of every edge value
    parts = [np.arange(1 << 20, dtype=np.uint64)]
    for k in range(20, 32):
        parts.append((1 << k) + np.arange(1 << 14, dtype=np.uint64) * (1 << (k - 14)))
    e = ref.edge_values().astype(np.int64)
    parts.append(np.clip(e[:, None] + np.arange(-130, 131)[None, :], 0, ref.U32_MAX).reshape(-1).astype(np.uint64))
    c = np.unique(np.concatenate(parts)).astype(np.uint32)
    assert c[0] == 0 and c[-1] == ref.U32_MAX
    b = ref.bucket(c).astype(np.int64)
    assert (np.diff(b) <= 0).all()
    assert np.array_equal(np.unique(b), np.arange(ref.TOP_BUCKET, 256)) and ref.REACHABLE == 209
    # the smallest duration of every bucket really is where the bucket changes
    for k in range(ref.TOP_BUCKET, 255):
        f = ref.bucket_floor(k)
        assert py_bucket(f) == k and py_bucket(f - 1) == k + 1, (k, f)
    assert ref.bucket_floor(255) == 0


def test_bucket_ends_and_double_rounding():
    assert ref.bucket(np.arange(8, dtype=np.uint32)).tolist() == [255] * 8
    assert int(ref.bucket(8)) == 254
    assert int(ref.bucket(ref.U32_MAX)) == 47 == ref.TOP_BUCKET
    # above 2^24 the conversion rounds before the sum does: the 128 durations
    # below 2^31 + 2^28 round up to it
    edge = (1 << 31) + (1 << 28)
    assert set(ref.bucket(np.arange(edge - 128, edge, dtype=np.uint64).astype(np.uint32)).tolist()) == {54}
    assert int(ref.bucket(edge - 129)) == 55 and int(ref.bucket(edge)) == 54
    assert [py_bucket(edge - 128), py_bucket(edge - 1), py_bucket(edge - 129)] == [54, 54, 55]


# --------------------------------------------------------------------- key

@pytest.mark.parametrize("n,gx", GRIDS)
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_key_equals_the_python_loop(n, gx, r):
    for pattern in ("log", "edges"):
        cost = ref.costs(pattern, n, seed=r)
        assert ref.key(cost, n, gx, r).tolist() == py_key(cost, n, gx, r), pattern
    for hot in {0, n - 1, n // 2, gx - 1, min(n - 1, gx)}:
        cost = ref.costs("hot", n, hot=hot)
        assert ref.key(cost, n, gx, r).tolist() == py_key(cost, n, gx, r), hot
    assert ref.key(cost, n, gx, 0).tolist() == cost.tolist()


@pytest.mark.parametrize("x,y,want", [(0, 0, 9), (6, 0, 9), (0, 4, 9), (6, 4, 9), (0, 2, 15), (3, 2, 25)])
def test_hot_tile_fills_its_clipped_window(x, y, want):
    n, gx = 35, 7
    assert ref.hot_population(n, gx, 2, y * gx + x) == want
    cost = ref.costs("hot", n, hot=y * gx + x)
    assert sum(py_bucket(k) == py_bucket(ref.HOT_COST) for k in py_key(cost, n, gx, 2)) == want


def test_patterns_are_seeded_and_what_they_say():
    n = 2145
    for p in ("flat", "log", "edges"):
        assert np.array_equal(ref.costs(p, n, 5), ref.costs(p, n, 5)) and ref.costs(p, n, 5).dtype == np.uint32
    assert not np.array_equal(ref.costs("log", n, 5), ref.costs("log", n, 6))
    assert set(ref.costs("flat", n).tolist()) == {1000}
    assert len(np.unique(ref.bucket(ref.costs("flat", n)))) == 1
    e = ref.edge_values()
    assert set(ref.costs("edges", n, 1).tolist()) == set(e.tolist()) and n > e.size
    assert len(np.unique(ref.bucket(e))) == 209
    edge = (1 << 31) + (1 << 28)
    assert {0, ref.U32_MAX, edge - 128, edge - 129, (1 << 25) - 1, (1 << 25) - 65} <= set(e.tolist())
    lg = ref.bucket(ref.costs("log", 1 << 16, 2))
    assert lg.min() <= 50 and lg.max() == 255 and len(np.unique(lg)) > 190


# ------------------------------------------------------------- check_order

@pytest.mark.parametrize("n,gx", GRIDS + [(1025, 25), (2145, 65)])
@pytest.mark.parametrize("r", [0, 2])
def test_check_order_accepts_a_right_sort(n, gx, r):
    for pattern in ("flat", "log", "edges"):
        cost = ref.costs(pattern, n, 11)
        order = order_by(ref.key(cost, n, gx, r))
        assert ref.check_order(order, cost, n, gx, r) is None
        # any order within a bucket: here each bucket reversed
        b = ref.bucket(ref.key(cost, n, gx, r)).astype(np.int64)
        rev = np.lexsort((-np.arange(n), b))
        assert ref.check_order(rev.astype(np.uint32), cost, n, gx, r) is None


def right_order(n=2145, gx=65, r=2, seed=4):
    cost = ref.costs("log", n, seed)
    return cost, order_by(ref.key(cost, n, gx, r)).astype(np.uint32)


def test_check_order_rejects_a_duplicated_entry():
    n, gx = 2145, 65
    cost, order = right_order()
    order[700] = order[699]  # (the same bucket or its neighbour: the buckets still do not decrease)
    msg = ref.check_order(order, cost, n, gx, 2)
    assert msg and "position 700" in msg and "again" in msg and "never dispatched" in msg, msg
    # ... and on one bucket, where nothing but the permutation can tell
    flat = ref.costs("flat", n)
    order = np.arange(n, dtype=np.uint32)
    order[n - 1] = 0
    msg = ref.check_order(order, flat, n, gx, 2)
    assert msg and f"position {n - 1}" in msg and f"tile {n - 1}" in msg, msg


def test_check_order_rejects_an_entry_equal_to_n():
    n, gx = 2145, 65
    cost, order = right_order()
    order[n - 1] = n  # what a histogram that was not cleared gives: offsets past the end
    msg = ref.check_order(order, cost, n, gx, 2)
    assert msg and f"position {n - 1}" in msg and f"entry {n}" in msg, msg
    order[3] = 0xFFFFFFFF  # a word the scatter never wrote
    msg = ref.check_order(order, cost, n, gx, 2)
    assert msg and "position 3:" in msg, msg
    assert ref.check_order(order[:-1], cost, n, gx, 2)  # a short order


def test_check_order_rejects_two_buckets_swapped():
    n, gx = 2145, 65
    cost, order = right_order()
    b = ref.bucket(ref.key(cost, n, gx, 2))[order]
    p = int(np.flatnonzero(b[1:] != b[:-1])[5])  # order[p], order[p + 1]: neighbouring buckets
    order[[p, p + 1]] = order[[p + 1, p]]
    msg = ref.check_order(order, cost, n, gx, 2)
    assert msg and f"position {p + 1}" in msg and "costlier tile dispatched later" in msg, msg


@pytest.mark.parametrize("hot", [0, 17, 34])
def test_check_order_rejects_the_undilated_sort_of_a_hot_tile(hot):
    n, gx = 35, 7
    cost = ref.costs("hot", n, hot=hot)
    order = order_by(cost)  # the hot tile first, then 0..n-1: right for r = 0 ...
    assert ref.check_order(order, cost, n, gx, 0) is None
    msg = ref.check_order(order, cost, n, gx, 2)  # ... but its neighbours belong in front as well
    assert msg and "costlier tile dispatched later" in msg, msg


@pytest.mark.parametrize("n,gx,hot", [(35, 7, 14), (35, 7, 13), (2145, 65, 65 * 16), (2145, 65, 65 * 16 + 64)])
def test_check_order_rejects_a_key_that_wraps_round_the_row_end(n, gx, hot):
    """A hot tile in column 0 (or the last column): a window that wraps marks
    tiles at the other end of the neighbouring row as costly and leaves out
    none, so its order is a permutation with two or more tiles too early."""
    cost = ref.costs("hot", n, hot=hot)
    wrong = wrapped_key(cost, n, gx, 2)
    assert not np.array_equal(wrong, ref.key(cost, n, gx, 2))
    order = order_by(wrong)
    assert np.array_equal(np.sort(order), np.arange(n))
    msg = ref.check_order(order, cost, n, gx, 2)
    assert msg and "costlier tile dispatched later" in msg, msg
    # away from the row ends the two keys agree, and so does the check
    mid = ref.costs("hot", n, hot=hot - hot % gx + gx // 2)
    assert ref.check_order(order_by(wrapped_key(mid, n, gx, 2)), mid, n, gx, 2) is None


# ---------------------------------------------------------------- sentinel

def test_assert_frame_reports_the_tiles_no_launch_wrote():
    """tests/sentinel.py assert_frame on host arrays: a frame with one 8x8 tile
    left at the sentinel word fails and names the tile; the same frame whole
    passes (RGBA8 words and float4)."""
    rng = np.random.default_rng(1)
    ref8 = (rng.integers(0, 1 << 24, (24, 40)).astype(np.uint32) | np.uint32(0xFF000000)).view(np.int32)
    sentinel.assert_frame(ref8.copy(), ref8)
    out8 = ref8.copy()
    out8[8:16, 32:40] = sentinel.RGBA8_WORD
    with pytest.raises(AssertionError, match=r"64 pixels still hold the sentinel.*\[\(4, 1\)\]"):
        sentinel.assert_frame(out8, ref8, "rgba8")
    ref4 = rng.random((24, 40, 4)).astype(np.float32)
    sentinel.assert_frame(ref4.copy(), ref4)
    out4 = ref4.copy()
    out4.view(np.uint32)[16:24, 0:8] = sentinel.FLOAT_WORD
    with pytest.raises(AssertionError, match=r"64 pixels still hold the sentinel.*\[\(0, 2\)\]"):
        sentinel.assert_frame(out4, ref4, "float4")
    out4 = ref4.copy()
    out4[3, 5, 1] += 1.0  # a wrong pixel that is no sentinel
    with pytest.raises(AssertionError, match=r"1 of 960 pixels differ.*x 5, y 3.*; 0 pixels still hold"):
        sentinel.assert_frame(out4, ref4, "float4")
    assert np.isnan(np.array([sentinel.FLOAT_WORD], np.uint32).view(np.float32)[0])
