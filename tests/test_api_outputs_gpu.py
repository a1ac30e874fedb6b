"""The binding's default-output and stats=True paths that no other GPU test
executes (the others are: a census of the suite found render, render_rgba8,
render_band_rgba8, render_step_map, deinterleave in its three dtypes,
deinterleave_cycle_rgb8, pack_rgba8, the single-frame and batched post methods,
the view batches, render_aa*, render_batch_aa and Comm.render covered).  Each
path: the call with the output the method allocates against the same call into
a caller's buffer pre-filled with a sentinel -- the documented shape, dtype and
device, and the same bits -- and with stats=True the stats dict's keys.

Scene S0 at 40 x 24: not a multiple of 16, three rows of 8x8 tiles; bands of
16 rows over 2 shards are uneven (16 and 8 rows)."""
import pytest

import raymarching_amd as rm

pytestmark = pytest.mark.gpu

W, H, BAND, NSHARDS = 40, 24, 16, 2
STATS_KEYS = {"evals", "pixels", "kernel_ms", "scene", "flop", "skipped", "dispatch", "lat_tiles", "gather_ms",
              "deinterleave_ms", "certified", "reflection_cleared", "near_sky"}


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    r.load_scene(rm.SCENE_FILES["S0"])
    r.set_pose(rm.S0_POSE["pos"], rm.S0_POSE["mouse"], rm.S0_POSE["time"])
    yield r
    r.close()


def _is(t, torch, shape, dtype, device):
    return tuple(t.shape) == shape and t.dtype == dtype and t.device == torch.device("cuda", device)


@pytest.mark.parametrize("shard,rows", [(0, 16), (1, 8)])
def test_render_band_with_stats(R, torch_cuda, shard, rows):
    torch = torch_cuda
    assert rm.shard_rows(H, BAND, NSHARDS, shard) == rows
    out, st = R.render_band(W, H, BAND, NSHARDS, shard, stats=True)
    assert _is(out, torch, (rows, W, 4), torch.float32, R.device)
    assert set(st) == STATS_KEYS and st["pixels"] == rows * W
    buf = torch.full((rows, W, 4), -7.0, dtype=torch.float32, device=out.device)
    got, st2 = R.render_band(W, H, BAND, NSHARDS, shard, out=buf, stats=True)
    assert got is buf and set(st2) == STATS_KEYS
    assert torch.equal(out.view(torch.int32), buf.view(torch.int32))
    assert torch.equal(buf, R.render_band(W, H, BAND, NSHARDS, shard))


def test_pack_rgb8_default_output(R, torch_cuda):
    torch = torch_cuda
    frame8 = R.render_rgba8(W, H)
    out = R.pack_rgb8(frame8)
    assert _is(out, torch, (H, 3 * W), torch.uint8, R.device)
    buf = torch.full((H, 3 * W), 0xA5, dtype=torch.uint8, device=frame8.device)
    assert R.pack_rgb8(frame8, out=buf) is buf
    torch.cuda.synchronize()
    assert torch.equal(out, buf)
    assert torch.equal(buf, frame8.view(torch.uint8).reshape(H, W, 4)[..., :3].reshape(H, 3 * W))


def test_comm_render_all_with_stats(R, torch_cuda):
    torch = torch_cuda
    (c,) = rm.Comm.init_all([R])
    try:
        frame, sts = rm.Comm.render_all([c], W, H, BAND, stats=True)
        assert _is(frame, torch, (H, W), torch.int32, R.device)
        assert len(sts) == 1 and set(sts[0]) == STATS_KEYS and sts[0]["pixels"] == W * H
        buf = torch.full((H, W), 0x5A5A5A5A, dtype=torch.int32, device=frame.device)
        got, sts2 = rm.Comm.render_all([c], W, H, BAND, frame=buf, stats=True)
        assert got is buf and len(sts2) == 1 and set(sts2[0]) == STATS_KEYS
        assert torch.equal(frame, buf) and torch.equal(buf, R.render_rgba8(W, H))
    finally:
        c.close()


def test_pack_targets_are_bounded_by_the_pixels_written(R, torch_cuda):
    """pack_rgba8 writes frame.numel() / 4 words and pack_rgb8 3 bytes per word, whatever the frame's shape:
    a caller's buffer with fewer is refused before anything is launched."""
    torch = torch_cuda
    dev = torch.device("cuda", R.device)
    flat = torch.zeros(4 * W * H, dtype=torch.float32, device=dev)
    wide = torch.zeros((H, 4 * W), dtype=torch.float32, device=dev)
    for frame, small in ((flat, 1), (wide, H), (flat, W * H - 1)):
        with pytest.raises(ValueError):
            R.pack_rgba8(frame, out=torch.zeros(small, dtype=torch.int32, device=dev))
    assert R.pack_rgba8(wide, out=torch.zeros(W * H, dtype=torch.int32, device=dev)).numel() == W * H
    frame8 = torch.zeros((H, W), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        R.pack_rgb8(frame8, out=torch.zeros(3 * W * H - 1, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        R.pack_rgb8(frame8, out=torch.zeros(3 * W * H, dtype=torch.int8, device=dev))
