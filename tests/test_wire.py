"""The compressed wire of RGBA8 row parts (raymarching_amd/csrc/rm_wire_tile.h,
rm_wire.hip): the numpy restatement (tests/wire_codec.py)
round-trips on CPU; on the GPU both encoders -- the rows encoder and the
render kernel's epilogue (rm_render_cycle_rows_wire) -- write the
restatement's bytes exactly and the decoder rebuilds every part's frame rows
bit for bit.

Parts of more than 65536 tiles (every multi-GPU headline config) finish
their message with other kernels than small parts, and decode with a
striding grid: the tests from `_LARGE_PARTS` on run both encoders and the
decoder there, against wire_codec.encode_fast and the source image.  Each
asserts the precondition that makes it reach its path, from the constants of
the C++ source, so that a retuned constant fails the test instead of quietly
ending its coverage."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import raymarching_amd as rm
from tests import wire_codec

SENTINEL = 0x5EA1ED00  # a frame word no decode writes (alpha is 255 in every decoded pixel)


def _csrc_constant(name, file="rm_wire.hip"):
    """`constexpr <integer type> name = <product of integers>;` of the C++ source."""
    src = (pathlib.Path(rm.__file__).parent / "csrc" / file).read_text()
    m = re.search(r"constexpr\s+(?:int64_t|long long|int)\s+%s\s*=\s*([0-9][0-9* ]*);" % name, src)
    assert m, f"{file}: no integer constant {name}"
    v = 1
    for f in m.group(1).split("*"):
        v *= int(f)
    return v


def _tile_grid(n, W):
    return (W + 7) // 8, (n + 7) // 8


def _scan_split(T):
    """rm_wire_tile_scan: (64-tile chunks, chunks per thread of its 1024)."""
    C = (T + 63) // 64
    return C, (C + 1023) // 1024


def _decode_grid(W, nrows):
    """launch_wire_decode_parts' grid for parts of `nrows` rows each: (gx, the
    tile rows per part it wants, gridDim.y).  A part of TY > gridDim.y tile
    rows strides (`ty += gridDim.y`); one of TY < gridDim.y leaves grid rows
    without work."""
    per = _csrc_constant("kDecodeTiles") * _csrc_constant("kDecodeWaves")
    gx = (_tile_grid(1, W)[0] + per - 1) // per
    want = -(-_csrc_constant("kDecodeWorkgroups") // (gx * len(nrows)))
    TY = max(_tile_grid(n, W)[1] for n in nrows)
    return gx, want, min(TY, max(want, 1))


def _assert_message(got, ref, T, what):
    diff = wire_codec.first_difference(got, ref, T)
    assert diff is None, f"{what}: {diff}"


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def _smooth(n, W, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:W]
    r = (x * 255 // max(W - 1, 1)).astype(np.uint32)
    g = ((y * 7 + x // 9) % 256).astype(np.uint32)
    b = np.where(rng.random((n, W)) < 0.02, rng.integers(0, 256, (n, W)), 128).astype(np.uint32)
    return r | (g << 8) | (b << 16) | np.uint32(0xFF000000)


def _noise(n, W, seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2**24, (n, W), dtype=np.uint32) | np.uint32(0xFF000000)


@pytest.mark.parametrize("n,W", [(3, 64), (5, 97), (2, 200), (1, 1), (16, 4096), (9, 17)])
@pytest.mark.parametrize("kind", ["smooth", "noise", "flat"])
def test_numpy_codec_round_trip(n, W, kind):
    img = {"smooth": _smooth, "noise": _noise}.get(kind, lambda n, W: np.full((n, W), 0xFF102030, np.uint32))(n, W)
    msg = wire_codec.encode(img)
    assert int(np.frombuffer(msg[:8].tobytes(), np.int64)[0]) == msg.size
    assert msg.size <= rm.wire_capacity(W, n)
    assert np.array_equal(wire_codec.decode(msg, n, W), img)
    T = ((W + 7) // 8) * ((n + 7) // 8)
    if kind == "flat" and W % 8 == 0 and n % 8 == 0:  # one header word per tile plus the offset table
        assert msg.size == wire_codec.header_bytes(T) + 8 * T


def _image(kind, n, W):
    return {"smooth": _smooth, "noise": _noise}.get(kind, lambda n, W: np.full((n, W), 0xFF102030, np.uint32))(n, W)


@pytest.mark.parametrize("n,W,kind",
                         [(n, W, kind) for n, W in [(3, 64), (5, 97), (2, 200), (1, 1), (16, 4096), (9, 17)]
                          for kind in ("smooth", "noise", "flat")] + [(16, 512, "smooth"), (16, 512, "noise")])
def test_fast_restatement_writes_the_loop_codecs_bytes(n, W, kind):
    """wire_codec.encode_fast (whole-array numpy, the reference of the GPU
    tests at production part sizes) against wire_codec.encode (the readable
    specification), byte for byte."""
    img = _image(kind, n, W)
    ref = wire_codec.encode(img)
    fast = wire_codec.encode_fast(img)
    T = ((W + 7) // 8) * ((n + 7) // 8)
    assert fast.dtype == ref.dtype and fast.size == ref.size
    _assert_message(fast, ref, T, "encode_fast against encode")


def test_fast_restatement_of_an_empty_part():
    assert np.array_equal(wire_codec.encode_fast(np.zeros((0, 64), np.uint32)),
                          wire_codec.encode(np.zeros((0, 64), np.uint32)))


def test_first_difference_names_the_tile_and_the_section():
    """The mismatch report of the large-part tests: the first differing tile,
    and whether the table or the payload differs."""
    img = _noise(16, 64)  # 16 tiles of 25 words
    ref = wire_codec.encode_fast(img)
    T, hb = 16, wire_codec.header_bytes(16)
    assert wire_codec.first_difference(ref.copy(), ref, T) is None
    bad = ref.copy()
    bad[8 + 4 * 5] ^= 1  # tile 5's table entry
    assert wire_codec.first_difference(bad, ref, T).startswith("table: tile 5 of 16")
    bad = ref.copy()
    bad[hb + 8 * (25 * 7 + 3)] ^= 1  # word 3 of tile 7
    assert wire_codec.first_difference(bad, ref, T).startswith("payload: word 178 (tile 7 of 16, its word 3)")
    assert wire_codec.first_difference(ref[:-8], ref, T).startswith("sizes")


def test_tile_code_differences_run_along_rows_and_the_first_column():
    """A tile whose rows are ramps and whose first column is another ramp needs
    one bit plane per channel that changes by one: differences are taken to
    the left, and to the pixel above only in the first column."""
    y, x = np.mgrid[0:8, 0:8]
    r = (10 + x + 3 * y).astype(np.uint32)  # +1 along rows, +3 down the first column
    p = (r | (np.uint32(50) << 8) | (np.uint32(7) << 16) | np.uint32(0xFF000000)).ravel()
    w = wire_codec.tile_words(p)
    assert (w[0] >> 24) & 15 == 3 and (w[0] >> 28) & 15 == 0 and (w[0] >> 32) & 15 == 0  # zigzag(3) = 6: 3 bits
    assert w[0] & 0xFFFFFF == 10 | (50 << 8) | (7 << 16)


def test_capacity_and_workspace_sizes():
    T = 512 * 4096 // 64
    assert rm.wire_capacity(4096, 512) == wire_codec.header_bytes(T) + 8 * 25 * T
    # word-major slots, a count byte per tile, a base per 64-tile chunk
    assert rm.wire_workspace_bytes(4096, 512) == ((8 * 25 * T + T + 3) & ~3) + 4 * ((T + 63) // 64)
    with pytest.raises(ValueError):
        rm.wire_capacity(0, 4)


def _reachable(T):
    """(W, n) of a part of exactly T tiles inside W <= 2^18, n <= 65535, or None."""
    for TY in range(1, 8192 + 1):
        if T % TY == 0 and T // TY <= 1 << 15:
            return 8 * (T // TY), 8 * TY - (TY == 8192)
    return None


def test_wire_size_rule_for_capacity_and_workspace():
    """One size rule (include/rm.h): 0 < W <= 2^18, 0 <= nrows <= 65535 and
    25 T < 2^27 (the table entry's 27-bit word offset): the sizing calls
    refuse the smallest part past the bound and size the largest below it."""
    bound = -(-(1 << 27) // 25)  # the least T with 25 T >= 2^27
    over = next(T for T in range(bound, bound + 4096) if _reachable(T))
    under = next(T for T in range(bound - 1, bound - 4096, -1) if _reachable(T))
    assert 25 * under < 1 << 27 <= 25 * over
    for T, ok in ((under, True), (over, False), (32768 * 163, True), (32768 * 164, False)):
        W, n = _reachable(T)
        assert _tile_grid(n, W)[0] * _tile_grid(n, W)[1] == T
        if ok:
            assert rm.wire_capacity(W, n) == wire_codec.header_bytes(T) + 8 * 25 * T
            assert rm.wire_workspace_bytes(W, n) == ((8 * 25 * T + T + 3) & ~3) + 4 * ((T + 63) // 64)
        else:
            with pytest.raises(ValueError):
                rm.wire_capacity(W, n)
            with pytest.raises(ValueError):
                rm.wire_workspace_bytes(W, n)
    # the last row of tile row 163 is in, the first of tile row 164 is out
    assert rm.wire_capacity(1 << 18, 163 * 8) > 0
    for W, n in (((1 << 18), 163 * 8 + 1), (8, 65536), ((1 << 18) + 1, 8), (0, 8), (8, -1)):
        with pytest.raises(ValueError):
            rm.wire_capacity(W, n)
        with pytest.raises(ValueError):
            rm.wire_workspace_bytes(W, n)
    assert rm.wire_capacity(8, 65535) > 0 and rm.wire_workspace_bytes(8, 65535) > 0


def _gpu_encode(R, torch, img):
    n, W = img.shape
    rows = torch.from_numpy(img.view(np.int32)).cuda()
    msg = torch.zeros(rm.wire_capacity(W, n), dtype=torch.uint8, device="cuda")
    ws = torch.empty(rm.wire_workspace_bytes(W, n), dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    R.wire_encode(rows, msg, ws, size)
    torch.cuda.synchronize()
    return msg, int(size.item())


@pytest.mark.gpu
@pytest.mark.parametrize("n,W", [(3, 64), (5, 97), (2, 200), (7, 4096)])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_gpu_encoder_writes_the_restated_bytes(R, torch_cuda, n, W, kind):
    torch = torch_cuda
    img = (_smooth if kind == "smooth" else _noise)(n, W)
    ref = wire_codec.encode(img)
    msg, size = _gpu_encode(R, torch, img)
    assert size == ref.size
    assert np.array_equal(msg[:size].cpu().numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,runs", [(96, 70, (13, 8)), (97, 61, (1, 5, 2)), (4096, 512, (16, 16, 16, 16))])
def test_gpu_wire_rebuilds_rendered_parts(R, torch_cuda, W, H, runs):
    """A rendered frame's parts: rank 0's rows scattered, every other part
    encoded on the GPU and decoded into the frame: equal to rm_render_rgba8."""
    torch = torch_cuda
    from raymarching_amd.frame import ShardPlan
    R.load_scene(rm.SCENE_FILES["T"])
    R.set_uniform("u_resolution", W, H)
    p = rm.POSES["P1"]
    R.set_pose(p["pos"], p["mouse"], p["time"])
    R.set_params(max_steps=128, count_evals=0)
    ref = R.render_rgba8(W, H)
    plan = ShardPlan(W, H, runs[-1], len(runs), runs)
    frame = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    sizes = []
    for s in range(len(runs)):
        n = plan.count(s)
        loc = torch.empty((n, W), dtype=torch.int32, device="cuda")
        R.render_cycle_rows(W, H, plan.cycle, plan.offsets[s], runs[s], 0, n, loc)
        if s == 0:
            R.scatter_part_rgba8(W, H, plan.cycle, plan.offsets[s], runs[s], n, loc, frame)
            continue
        msg = torch.empty(rm.wire_capacity(W, n), dtype=torch.uint8, device="cuda")
        ws = torch.empty(rm.wire_workspace_bytes(W, n), dtype=torch.uint8, device="cuda")
        size = torch.zeros(1, dtype=torch.int64, device="cuda")
        R.wire_encode(loc, msg, ws, size)
        # the message as it would arrive: only its `size` bytes
        got = torch.zeros_like(msg)
        torch.cuda.synchronize()
        k = int(size.item())
        got[:k] = msg[:k]
        R.wire_decode(W, H, plan.cycle, plan.offsets[s], runs[s], n, got, frame)
        sizes.append((k, n * W * 3))
    torch.cuda.synchronize()
    assert torch.equal(frame, ref)
    if W == 4096:  # a rendered frame compresses
        assert all(k * 2 < raw for k, raw in sizes), sizes


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["T", "O"])
@pytest.mark.parametrize("W,H,runs", [(96, 70, (13, 8)), (97, 61, (1, 5, 2)), (4096, 512, (16, 16, 16, 16))])
def test_gpu_render_epilogue_writes_the_encoders_message(R, torch_cuda, scene, W, H, runs):
    """rm_render_cycle_rows_wire: the render kernel encodes its own tiles, and
    the message is byte for byte the rows encoder's (and the numpy
    restatement's) of the rows rm_render_cycle_rows_rgba8 renders; it decodes
    to them (adaptive dispatch order on, so the tiles run out of order)."""
    torch = torch_cuda
    from raymarching_amd.frame import ShardPlan
    R.load_scene(rm.SCENE_FILES[scene])
    R.set_uniform("u_resolution", W, H)
    p = rm.POSES["P1"]
    R.set_pose(p["pos"], p["mouse"], p["time"])
    R.set_params(max_steps=128 if scene == "T" else 256, count_evals=0, schedule=1)
    plan = ShardPlan(W, H, runs[-1], len(runs), runs)
    for s in range(1, len(runs)):
        n = plan.count(s)
        loc = torch.empty((n, W), dtype=torch.int32, device="cuda")
        msg = torch.zeros(rm.wire_capacity(W, n), dtype=torch.uint8, device="cuda")
        ws = torch.empty(rm.wire_workspace_bytes(W, n), dtype=torch.uint8, device="cuda")
        size = torch.zeros(1, dtype=torch.int64, device="cuda")
        for _ in range(3):  # (the second and third launch dispatch costliest tiles first)
            R.render_cycle_rows(W, H, plan.cycle, plan.offsets[s], runs[s], 0, n, loc)
            R.render_cycle_rows_wire(W, H, plan.cycle, plan.offsets[s], runs[s], 0, n, msg, ws, size)
        torch.cuda.synchronize()
        k = int(size.item())
        ref_gpu, k2 = _gpu_encode(R, torch, loc.cpu().numpy().view(np.uint32))
        assert k == k2
        assert torch.equal(msg[:k], ref_gpu[:k])
        if n * W <= 97 * 61:
            assert np.array_equal(msg[:k].cpu().numpy(), wire_codec.encode(loc.cpu().numpy().view(np.uint32)))
        frame = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        R.wire_decode(W, H, plan.cycle, plan.offsets[s], runs[s], n, msg, frame)
        R.scatter_part_rgba8(W, H, plan.cycle, plan.offsets[s], runs[s], n, loc, frame2 := torch.zeros_like(frame))
        torch.cuda.synchronize()
        assert torch.equal(frame, frame2)


@pytest.mark.gpu
def test_gpu_render_wire_empty_part(R, torch_cuda):
    torch = torch_cuda
    R.load_scene(rm.SCENE_FILES["T"])
    msg = torch.full((rm.wire_capacity(64, 0),), 7, dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(1, rm.wire_workspace_bytes(64, 0)), dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    R.render_cycle_rows_wire(64, 8, 16, 8, 8, 0, 0, msg, ws, size)  # H = 8 rows, the part (8, 8) holds none
    torch.cuda.synchronize()
    assert int(size.item()) == 8


@pytest.mark.gpu
def test_gpu_wire_rejects_bad_parts(R, torch_cuda):
    torch = torch_cuda
    frame = torch.zeros((8, 64), dtype=torch.int32, device="cuda")
    msg = torch.zeros(rm.wire_capacity(64, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(rm.RmError):
        R.wire_decode(64, 8, 4, 3, 2, 1, msg, frame)  # offset + run > cycle
    with pytest.raises(rm.RmError):
        R.wire_decode(64, 8, 4, 0, 2, 5, msg, frame)  # more rows than the part has


def test_delta_frame_size_check_on_every_rank():
    """DeltaFrame._check_sizes needs only the plan (no receive buffers), so
    every rank runs it on the gathered sizes before any send or receive: a
    rank reporting more than its part's wire capacity fails them all."""
    from types import SimpleNamespace

    from raymarching_amd.frame import DeltaFrame, ShardPlan
    plan = ShardPlan(4096, 4096, 16, 3)
    stub = SimpleNamespace(world=3, plan=plan)
    caps = [rm.wire_capacity(4096, plan.count(q)) for q in range(3)]
    DeltaFrame._check_sizes(stub, [0, caps[1], 17])
    with pytest.raises(RuntimeError, match="rank 2"):
        DeltaFrame._check_sizes(stub, [0, 5, caps[2] + 1])
    with pytest.raises(RuntimeError, match="rank 1"):
        DeltaFrame._check_sizes(stub, [0, -1, 5])


# ---- parts at and above the finish step's kernel switch (rm_wire.hip launch_wire_finish) ----

# case: rows, width, image kinds (noise: every tile takes all 25 words, the largest offsets)
_LARGE_PARTS = {
    # T = 65536: the last part rm_wire_tile_compact_direct takes, 256 workgroups, its longest prefix loop
    "a_direct_limit": (1024, 4096, ("smooth", "noise")),
    # T = 66048: the first part of rm_wire_tile_scan + rm_wire_tile_compact: two chunks per thread, the
    # 16-byte chunk_sum, threads without a chunk
    "b_scan_aligned": (1032, 4096, ("smooth", "noise")),
    # T = 66199, odd: the counts are not 16-byte aligned, so every chunk takes the byte-wise chunk_sum; the
    # last chunk holds 23 tiles
    "c_scan_odd": (2744, 1544, ("smooth", "noise")),
    # T = 132355, odd: three chunks per thread and 2069 chunks, so the last working thread's range is
    # clipped; a ragged right column and bottom row.  Noise for the largest offsets, smooth for counts
    # that vary from tile to tile (encode_fast takes under a second for either).
    "d_scan_three_clipped": (2052, 4116, ("smooth", "noise")),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", [(c, k) for c, v in _LARGE_PARTS.items() for k in v[2]])
def test_gpu_wire_at_the_finish_kernel_switch(R, torch_cuda, case, kind):
    """The rows encoder writes encode_fast's bytes and the decoder rebuilds
    the image (rows outside the part untouched) at the tile counts where the
    finish step and the decode grid change shape."""
    torch = torch_cuda
    n, W, _ = _LARGE_PARTS[case]
    TX, TY = _tile_grid(n, W)
    T = TX * TY
    direct = _csrc_constant("kDirectTiles")
    C, per = _scan_split(T)
    counts_at = 8 * wire_codec.TILE_WORDS * T  # the counts' byte offset in the (256-byte aligned) workspace
    gx, want, gy = _decode_grid(W, [n])
    if case == "a_direct_limit":
        assert T == direct
    else:
        assert T > direct and per >= 2
        assert TY > want and gy == want  # the decoder's tile rows stride (ty += gridDim.y)
    if case == "b_scan_aligned":
        assert T % 64 == 0 and counts_at % 16 == 0 and per == 2 and 1023 * per >= C
    if case == "c_scan_odd":
        assert T % 2 == 1 and counts_at % 16 == 8 and T % 64 != 0 and W % 8 == 0
    if case == "d_scan_three_clipped":
        assert T % 2 == 1 and per >= 3 and C % per != 0 and W % 8 != 0 and n % 8 != 0
    img = _image(kind, n, W)
    ref = wire_codec.encode_fast(img)
    msg, size = _gpu_encode(R, torch, img)
    assert size == ref.size, f"message size {size}, expected {ref.size} ({T} tiles)"
    _assert_message(msg[:size].cpu().numpy(), ref, T, f"rows encoder, {n} x {W}")
    arrived = msg[:size].clone()  # the message as it would arrive: only its `size` bytes
    del msg
    H = n + 2  # one part of the whole cycle, and two rows of the next cycle that it does not hold
    frame = torch.full((H, W), SENTINEL, dtype=torch.int32, device="cuda")
    R.wire_decode(W, H, n, 0, n, n, arrived, frame)
    torch.cuda.synchronize()
    got = frame.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero((got[:n] != img).any(axis=1))
    assert bad.size == 0, f"{bad.size} decoded rows differ, the first is row {bad[0]} (tile row {bad[0] // 8})"
    assert (got[n:] == SENTINEL).all()


def _part_frame(H, W, cycle, offset, run, rows, frame=None):
    """numpy: a part's packed rows at their frame rows, y = (j // run) cycle + offset + j % run."""
    if frame is None:
        frame = np.full((H, W), SENTINEL, np.uint32)
    j = np.arange(rows.shape[0])
    frame[(j // run) * cycle + offset + j % run] = rows
    return frame


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["T", "O"])
@pytest.mark.parametrize("case,W,H,cycle,offset,run", [
    ("two_kernel_finish_latency_tiles", 4096, 1040, 1040, 0, 1040),  # 66560 tiles
    ("three_chunks_no_latency_tiles", 4096, 2056, 2056, 0, 2056),  # 131584 tiles
    ("band16_part1_of_2", 4096, 2080, 32, 16, 16),  # 1040 rows, 66560 tiles, the cyclic row mapping
])
def test_gpu_render_epilogue_message_above_the_kernel_switch(R, torch_cuda, scene, case, W, H, cycle, offset, run):
    """rm_render_cycle_rows_wire for parts of more than 65536 tiles (the
    two-kernel finish; with and without scene T's latency tiles): the message
    is the rows encoder's and encode_fast's of the rows
    rm_render_cycle_rows_rgba8 renders, and decodes to them."""
    torch = torch_cuda
    n = rm.cycle_rows(H, cycle, offset, run)
    TX, TY = _tile_grid(n, W)
    T = TX * TY
    lat_max = _csrc_constant("kLatMaxTiles", "rm_render_host.cpp")
    assert T > _csrc_constant("kDirectTiles")
    assert TY > _decode_grid(W, [n])[1]
    if case == "three_chunks_no_latency_tiles":
        assert T > lat_max and T > 131072 and _scan_split(T)[1] >= 3
    else:
        assert T <= lat_max and _scan_split(T)[1] == 2
    assert (cycle != run) == (case == "band16_part1_of_2")
    R.load_scene(rm.SCENE_FILES[scene])
    R.set_uniform("u_resolution", W, H)
    p = rm.POSES["P1"]
    R.set_pose(p["pos"], p["mouse"], p["time"])
    R.set_params(max_steps=128 if scene == "T" else 256, count_evals=0, schedule=1)
    loc = torch.empty((n, W), dtype=torch.int32, device="cuda")
    msg = torch.zeros(rm.wire_capacity(W, n), dtype=torch.uint8, device="cuda")
    ws = torch.empty(rm.wire_workspace_bytes(W, n), dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    for _ in range(3):  # (the second and third launch dispatch costliest tiles first)
        R.render_cycle_rows(W, H, cycle, offset, run, 0, n, loc)
        _msg, st = R.render_cycle_rows_wire(W, H, cycle, offset, run, 0, n, msg, ws, size, stats=True)
    torch.cuda.synchronize()
    assert st["dispatch"] == "adaptive", st
    if scene == "T":
        assert st["lat_tiles"] == (2048 if T <= lat_max else 0), st
    k = int(size.item())
    rows = loc.cpu().numpy().view(np.uint32)
    ref = wire_codec.encode_fast(rows)
    assert k == ref.size, f"message size {k}, expected {ref.size} ({T} tiles)"
    got = msg[:k].cpu().numpy()
    _assert_message(got, ref, T, f"render epilogue against encode_fast, scene {scene}")
    del ws
    ref_gpu, k2 = _gpu_encode(R, torch, rows)
    assert k2 == k
    _assert_message(got, ref_gpu[:k2].cpu().numpy(), T, f"render epilogue against the rows encoder, scene {scene}")
    del ref_gpu
    frame = torch.full((H, W), SENTINEL, dtype=torch.int32, device="cuda")
    R.wire_decode(W, H, cycle, offset, run, n, msg[:k].clone(), frame)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), _part_frame(H, W, cycle, offset, run, rows))


@pytest.mark.gpu
def test_gpu_wire_decodes_unequal_parts_in_one_launch(R, torch_cuda):
    """rm_wire_decode_parts as the root of a weighted N = 4 frame calls it:
    three messages of unequal parts in one launch (blockIdx.z; one gridDim.y
    for all), built by encode_fast so that no GPU encoder is involved.  The
    longest part strides over its tile rows, the shortest leaves grid rows
    idle, one has a ragged last tile row, the frame's last cycle is cut, and
    the root's own rows stay untouched.  One rm_wire_decode per message gives
    the same frame."""
    torch = torch_cuda
    from raymarching_amd.frame import ShardPlan
    W, H, runs = 1024, 685, (8, 80, 8, 37)
    plan = ShardPlan(W, H, runs[-1], len(runs), runs)
    parts = (1, 2, 3)
    nrows = [plan.count(s) for s in parts]
    assert nrows == [rm.cycle_rows(H, plan.cycle, plan.offsets[s], runs[s]) for s in parts]
    gx, want, gy = _decode_grid(W, nrows)
    TYs = [_tile_grid(n, W)[1] for n in nrows]
    assert len(parts) >= 2 and max(TYs) > want and gy == want  # the longest part strides
    assert min(TYs) < gy  # grid rows past the shortest part's tile rows
    assert any(n % 8 for n in nrows) and H % plan.cycle != 0
    imgs = [_smooth(nrows[0], W), np.full((nrows[1], W), 0xFF102030, np.uint32), _noise(nrows[2], W)]
    want_frame = np.full((H, W), SENTINEL, np.uint32)
    msgs = []
    for s, img in zip(parts, imgs):
        _part_frame(H, W, plan.cycle, plan.offsets[s], runs[s], img, want_frame)
        msgs.append(torch.from_numpy(wire_codec.encode_fast(img)).cuda())  # exactly its own size
    assert (want_frame[plan.rows(0)] == SENTINEL).all() and (want_frame != SENTINEL).sum() == sum(nrows) * W
    frame = torch.full((H, W), SENTINEL, dtype=torch.int32, device="cuda")
    R.wire_decode_parts(W, H, plan.cycle, [plan.offsets[s] for s in parts], [runs[s] for s in parts], nrows, msgs,
                        frame)
    torch.cuda.synchronize()
    got = frame.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero((got != want_frame).any(axis=1))
    assert bad.size == 0, f"{bad.size} frame rows differ, the first is row {bad[0]} (part {plan.slot_of_row(bad[0])})"
    single = torch.full((H, W), SENTINEL, dtype=torch.int32, device="cuda")
    for s, n, m in zip(parts, nrows, msgs):
        R.wire_decode(W, H, plan.cycle, plan.offsets[s], runs[s], n, m, single)
    torch.cuda.synchronize()
    assert torch.equal(single, frame)


@pytest.mark.gpu
def test_gpu_wire_size_rule_at_every_entry_point(R, torch_cuda):
    """A part past the size rule (include/rm.h) is RM_ERR_INVALID_ARGUMENT at
    rm_wire_encode, rm_wire_decode, rm_wire_decode_parts (for any part) and
    rm_render_cycle_rows_wire, through the C ABI (the Python wrappers would
    stop at wire_capacity): refused before a pointer is used or a kernel
    launched, so tiny buffers stand in, and the context renders on."""
    torch = torch_cuda
    from raymarching_amd._lib import STATUS_CODES, lib
    L, bad_arg = lib(), STATUS_CODES["RM_ERR_INVALID_ARGUMENT"]
    R.load_scene(rm.SCENE_FILES["T"])
    R.set_uniform("u_resolution", 96, 64)
    p = rm.POSES["P1"]
    R.set_pose(p["pos"], p["mouse"], p["time"])
    R.set_params(max_steps=128, count_evals=0, schedule=1)
    before = R.render_rgba8(96, 64).clone()
    buf = [torch.zeros(64, dtype=torch.int64, device="cuda") for _ in range(4)]
    a, b, c, d = (t.data_ptr() for t in buf)
    for W, n in (((1 << 18), 164 * 8), (8, 65536)):  # 25 T >= 2^27; more rows than a launch's grid.y
        with pytest.raises(ValueError):  # (the same rule: nothing below runs unless it holds here)
            rm.wire_capacity(W, n)
        assert L.rm_wire_encode(R._ctx, W, n, a, b, c, d) == bad_arg
        assert L.rm_wire_decode(R._ctx, W, n, n, 0, n, n, a, b) == bad_arg
        assert L.rm_render_cycle_rows_wire(R._ctx, W, n, n, 0, n, 0, n, a, b, c, None) == bad_arg
        # a good first part (8 rows), the second past the rule
        offs, runs, rows = (ctypes.c_int * 2)(0, 8), (ctypes.c_int * 2)(8, n), (ctypes.c_int * 2)(8, n)
        assert rm.wire_capacity(W, 8) > 0
        assert L.rm_wire_decode_parts(R._ctx, W, n + 8, n + 8, 2, offs, runs, rows, (ctypes.c_void_p * 2)(a, b),
                                      c) == bad_arg
    torch.cuda.synchronize()
    assert all(int(t.abs().sum()) == 0 for t in buf)
    assert torch.equal(R.render_rgba8(96, 64), before)
