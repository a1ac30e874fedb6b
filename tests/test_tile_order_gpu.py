"""The adaptive dispatch order (rm_params.schedule = 1) on the GPU.

Part A calls the sort alone -- rm::launch_tile_order of librm.so, the two
kernels rm_sched_hist and rm_sched_scatter -- on buffers laid out as the host
lays them out (rm_ctx_streams.cpp sched_slot), and compares with the numpy
restatement tests/tile_order_ref.py: the order is a permutation whose dilated
keys' buckets do not decrease, the bucket bytes, the histogram and the cursors
are the reference's, and the other parity's words are cleared.  Three sorts in
a row on one buffer set, alternating parities as the host does, reach the
sort that depends on the kernel's own clearing.

Part B renders three sort periods of one geometry through the renderer, every
launch into a target filled with a word no kernel writes (tests/sentinel.py),
so a tile the order never dispatches shows."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import POSES
from tests import sentinel
from tests import tile_order_ref as ref

pytestmark = pytest.mark.gpu

# ================================================================= part A

GRIDS = [(1, 1), (35, 7), (33, 7), (80, 2), (300, 1), (255, 255), (256, 256), (257, 257), (1023, 33), (1024, 32),
         (1025, 25), (2145, 65), (262144, 512), (1048576, 1024)]  # (n, gx); the last two: the 4096^2 and 8192^2 frames
RADIUS = 2  # kSchedDilate (rm_render_host.cpp): the unrolled key, tile_key_r<2>
JUNK = 0x5A5A5A5A  # what the buffers hold where the host does not clear them

# once a parity chain has failed, part B's long sequences are not run: an order
# entry past n makes the render kernel store a duration out of bounds
_CHAIN_FAILED = []


@pytest.fixture(scope="module")
def sort_fn(torch_cuda):
    """rm::launch_tile_order(cost, n, gx, radius, order, hist, next, bucket,
    stream) of librm.so: the one defined dynamic symbol of that name."""
    out = subprocess.run(["nm", "-D", "--defined-only", rm.LIB_PATH], capture_output=True, text=True, check=True)
    names = [ln.split()[-1] for ln in out.stdout.splitlines() if "launch_tile_order" in ln]
    assert len(names) == 1, f"librm.so exports {names or 'no symbol'} for rm::launch_tile_order"
    rm.lib()
    fn = getattr(ctypes.CDLL(rm.LIB_PATH), names[0])
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return fn


class Slot:
    """One geometry's buffers, in words: cost[2][n] | order[2][n] | 2 x
    (hist[256] | cursor[256]) | bucket bytes[n], the 1024 histogram and cursor
    words zeroed once, as the host's one memset does; everything else holds
    JUNK, and so does a guard of 2n + 1024 words behind the bucket bytes."""

    def __init__(self, torch, n):
        self.torch, self.n = torch, n
        self.words = 4 * n + 1024 + (n + 3) // 4
        self.buf = torch.full((self.words + 2 * n + 1024,), JUNK, dtype=torch.int32, device="cuda")
        self.buf[4 * n: 4 * n + 1024] = 0
        self.sorts = 0

    def sort(self, fn, cost, gx, r):
        """The next sort of this geometry (parity = the sort's number & 1) of
        these durations, checked against the reference.  -> the reference's
        bucket bytes."""
        torch, n = self.torch, self.n
        slot = self.sorts & 1
        self.sorts += 1
        cost = np.ascontiguousarray(cost, dtype=np.uint32)
        assert cost.shape == (n,)
        self.buf[slot * n: (slot + 1) * n].copy_(torch.from_numpy(cost.view(np.int32)))
        before = self.buf.cpu().numpy().view(np.uint32).copy()
        base, h = self.buf.data_ptr(), 4 * n
        err = fn(base + 4 * slot * n, n, gx, r, base + 4 * (2 + slot) * n, base + 4 * (h + 512 * slot),
                 base + 4 * (h + 512 * (1 - slot)), base + 4 * (h + 1024), None)
        torch.cuda.synchronize()
        assert err == 0, f"launch_tile_order: hipError_t {err}"
        got = self.buf.cpu().numpy().view(np.uint32)
        what = f"sort {self.sorts - 1} (parity {slot}) of {n} tiles, {gx} wide, radius {r}"

        want_b = ref.bucket(ref.key(cost, n, gx, r))
        counts = np.bincount(want_b, minlength=256).astype(np.uint32)
        hist = got[h + 512 * slot: h + 512 * slot + 256]
        cursor = got[h + 512 * slot + 256: h + 512 * slot + 512]
        nxt = got[h + 512 * (1 - slot): h + 512 * (2 - slot)]
        bucket = got[h + 1024: self.words].view(np.uint8)[:n]
        order = got[(2 + slot) * n: (3 + slot) * n]
        # (the histogram first: too large a count is what sends order entries past n)
        assert np.array_equal(hist, counts), f"{what}: the histogram differs in buckets {np.flatnonzero(hist != counts)[:8]}"
        assert np.array_equal(bucket, want_b), \
            f"{what}: the bucket bytes differ at tiles {np.flatnonzero(bucket != want_b)[:8]}"
        msg = ref.check_order(order, cost, n, gx, r)
        assert msg is None, f"{what}: {msg}"
        assert np.array_equal(cursor, counts), f"{what}: the cursors differ in buckets {np.flatnonzero(cursor != counts)[:8]}"
        assert not nxt.any(), f"{what}: the other parity's words {np.flatnonzero(nxt)[:8]} are not cleared"
        # nothing else is written: the durations, the other parity's order and
        # durations, the bytes behind the last bucket byte, the guard
        keep = np.ones(got.size, bool)
        keep[(2 + slot) * n: (3 + slot) * n] = False
        keep[h: h + 1024] = False
        keep[h + 1024: h + 1024 + (n + 3) // 4] = False
        assert np.array_equal(got[keep], before[keep]), \
            f"{what}: words {np.flatnonzero(keep & (got != before))[:8]} outside the sort's outputs changed"
        tail = got[h + 1024: self.words].view(np.uint8)[n:]
        assert (tail == (JUNK & 0xFF)).all(), f"{what}: bytes behind the last bucket byte changed"
        return want_b


@pytest.mark.parametrize("pattern", ["flat", "log", "edges"])
@pytest.mark.parametrize("n,gx", GRIDS)
def test_sort_equals_the_reference(sort_fn, torch_cuda, n, gx, pattern):
    b = Slot(torch_cuda, n).sort(sort_fn, ref.costs(pattern, n, seed=gx), gx, RADIUS)
    print(f"{pattern} {n}/{gx}: {len(np.unique(b))} buckets reached, {b.min()}..{b.max()}")
    if pattern == "flat":
        assert len(np.unique(b)) == 1


def hot_tiles(n, gx):
    gy = n // gx
    assert gy * gx == n
    return [(0, 0, 9), (gx - 1, 0, 9), (0, gy - 1, 9), (gx - 1, gy - 1, 9), (0, gy // 2, 15), (gx // 2, gy // 2, 25)]


@pytest.mark.parametrize("n,gx,x,y,want", [(n, gx) + t for n, gx in ((35, 7), (2145, 65)) for t in hot_tiles(n, gx)])
def test_hot_tile_is_dilated_into_its_clipped_window(sort_fn, torch_cuda, n, gx, x, y, want):
    """One costly tile among zeros: the tiles within 2 of it, and no tile
    across the row wrap, share its bucket and come first."""
    torch = torch_cuda
    hot = y * gx + x
    slot = Slot(torch, n)
    slot.sort(sort_fn, ref.costs("hot", n, hot=hot), gx, RADIUS)
    got = slot.buf.cpu().numpy().view(np.uint32)
    top = int(ref.bucket(ref.HOT_COST))
    assert int(got[4 * n + top]) == want
    first = got[2 * n: 2 * n + want].astype(np.int64)
    assert (np.abs(first % gx - x) <= 2).all() and (np.abs(first // gx - y) <= 2).all(), first


@pytest.mark.parametrize("pattern", ["log", "edges"])
@pytest.mark.parametrize("r", [0, 1, 3])
@pytest.mark.parametrize("n,gx", [(35, 7), (80, 2), (1025, 25), (2145, 65)])
def test_run_time_radius_equals_the_reference(sort_fn, torch_cuda, n, gx, r, pattern):
    """tile_key, the loop over a run-time radius (production's radius 2 takes
    the unrolled tile_key_r<2>): its own column, row and index guards."""
    b = Slot(torch_cuda, n).sort(sort_fn, ref.costs(pattern, n, seed=r), gx, r)
    if pattern == "edges" and r == 0 and n > ref.edge_values().size:
        # every value of the list undilated: the kernel's bucket on each of the 209 reachable buckets
        assert len(np.unique(b)) == ref.REACHABLE == 209


@pytest.mark.parametrize("n,gx", [(1025, 25), (262144, 512)])
def test_three_sorts_alternate_parities_without_a_host_clear(sort_fn, torch_cuda, n, gx):
    """Sort 0 and sort 1 run on the host's zeros; sort 2 counts into the
    histogram sort 1's scatter cleared (the host clears nothing after its one
    memset).  Counts left standing would make sort 2's histogram too large and
    its order entries run past n."""
    slot = Slot(torch_cuda, n)
    try:
        for s in range(3):
            slot.sort(sort_fn, ref.costs("log", n, seed=100 + s), gx, RADIUS)
    except BaseException:
        _CHAIN_FAILED.append((n, gx))
        raise
    assert slot.sorts == 3


# ================================================================= part B

KNOBS = os.path.join(rm.SCENES_DIR, "output_shader_knobs.hip")  # its kernel states its own order lookup
# 16 = kSchedPeriod (rm_render_host.cpp): launches 0, 16, 32 and 48 measure and
# sort; launch 33 is the first to read sort 2's order, which is the first sort
# that counts into a histogram the scatter kernel cleared
LAUNCHES = 3 * 16 + 4
BAND_LAUNCHES = 2 * 16 + 4
BAND = (8, 3, 1)  # render_band_rgba8(W, H, band, nshards, shard)
STEPS = 128


def load(r, scene, kernel):
    r.load_scene(KNOBS if scene == "knobs" else rm.SCENE_FILES[scene])
    pose = POSES["P3"]
    r.set_pose(pose["pos"], pose["mouse"], pose["time"])
    r.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0, kernel=kernel, schedule=0)


@pytest.fixture
def fresh(torch_cuda):
    """A context of its own for every case: the launch count of a geometry
    starts at 0, so the sorts fall on the launches named above."""
    assert not _CHAIN_FAILED, f"not run: the three-sort chain failed on {_CHAIN_FAILED} (orders may run past n)"
    r = rm.Renderer(0)
    yield r
    r.close()


# 200x120: 25 x 15 = 375 tiles, one scatter block.  520x264: 65 x 33 = 2145
# tiles, 3 scatter and 9 histogram blocks, above scene T's 2048 latency tiles
@pytest.mark.parametrize("W,H", [(200, 120), (520, 264)])
@pytest.mark.parametrize("scene,kernel", [("T", "tile8"), ("T", "persist"), ("O", "tile8"), ("O", "persist"),
                                          ("knobs", "auto")])
def test_three_periods_write_every_tile(fresh, torch_cuda, scene, kernel, W, H):
    torch, R = torch_cuda, fresh
    load(R, scene, kernel)
    ref_f = R.render(W, H)
    ref8 = R.render_rgba8(W, H)
    R.set_params(count_evals=1)
    _, st_rm = R.render(W, H, stats=True)
    assert st_rm["dispatch"] == "row-major" and st_rm["evals"] > 0, st_rm
    R.set_params(count_evals=0, schedule=1)
    for i in range(LAUNCHES):
        what = f"{scene} {kernel} {W}x{H} launch {i}"
        if i % 5 == 4:  # (both forms share the geometry's launch count)
            out, st = R.render(W, H, out=sentinel.target(torch, (H, W, 4), torch.float32), stats=True)
            sentinel.assert_frame(out, ref_f, what + " (float4)")
        else:
            out, st = R.render_rgba8(W, H, out=sentinel.target(torch, (H, W), torch.int32), stats=True)
            sentinel.assert_frame(out, ref8, what + " (RGBA8)")
        assert st["dispatch"] == ("adaptive" if i else "row-major"), (what, st)
        if i == 20:
            # an instrumented launch uses the current order, records no durations
            # and does not advance the launch count: the launches after it are
            # checked like those before it
            R.set_params(count_evals=1)
            out, st = R.render(W, H, out=sentinel.target(torch, (H, W, 4), torch.float32), stats=True)
            R.set_params(count_evals=0)
            assert st["dispatch"] == "adaptive", (what, st)
            assert st["evals"] == st_rm["evals"], (what, st, st_rm)
            sentinel.assert_frame(out, ref_f, what + " + instrumented")


@pytest.mark.parametrize("scene,kernel", [("T", "tile8"), ("T", "persist"), ("O", "tile8"), ("O", "persist"),
                                          ("knobs", "auto")])
def test_two_periods_of_a_row_part_write_every_tile(fresh, torch_cuda, scene, kernel):
    torch, R = torch_cuda, fresh
    W, H = 200, 120
    load(R, scene, kernel)
    rows = rm.shard_rows(H, *BAND)
    ref8 = R.render_band_rgba8(W, H, *BAND)
    assert ref8.shape == (rows, W)
    sentinel.assert_frame(ref8, R.render_rgba8(W, H)[[y for y in range(H) if (y // BAND[0]) % BAND[1] == BAND[2]]],
                          "the row-major part against the frame's rows")
    R.set_params(schedule=1)
    for i in range(BAND_LAUNCHES):
        out, st = R.render_band_rgba8(W, H, *BAND, out=sentinel.target(torch, (rows, W), torch.int32), stats=True)
        sentinel.assert_frame(out, ref8, f"{scene} {kernel} part of {W}x{H} launch {i}")
        assert st["dispatch"] == ("adaptive" if i else "row-major"), (i, st)
