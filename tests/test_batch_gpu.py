"""View batches on the GPU (include/rm.h rm_render_batch, rm_render_batch_rgba8;
DESIGN.md 2.26): every view of a batch against this build's own single-frame
call for the same pose -- every byte, no tolerance; the single-frame kernels are
not touched by the batch.  Ragged tiles, all four scenes, both target formats,
a far-sky view next to a marching one, sub-pixel offsets against
render_accumulate, more views than a byte counts, two batches in flight, a
stream change, the context's state, u_resolution and the reciprocal cache, a
host target, the argument checks and the headless app."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from raymarching_amd import POSES, S0_POSE, _lib
from raymarching_amd.cameras import _rot_rows
from tests import ray_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, SCENE, NO_SCENE = 1, 3, 4
STEPS = 128
SENTINEL8 = 0x5A5A5A5A  # (alpha 0x5A: no pixel the pass writes, whose alpha is 255)
SENTINELF = -7.0        # (the pass writes alpha 1)


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def _setup(r, scene, steps=STEPS):
    r.load_scene(rm.SCENE_FILES[scene])
    r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0)
    r.set_uniform("u_seed1", 0.5, 0.5)
    r.set_uniform("u_sample_part", 1.0)


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _same(a, b):
    """every byte (floats compared as words: a NaN equals itself, -0 differs from +0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _singles(r, W, H, views, rgba8=True):
    """What a caller does today: set_pose + render_rgba8 / render per view -> [n, H, W(, 4)] on the host"""
    frames = []
    for v in views:
        r.set_pose(v["pos"], v["mouse"], v["time"])
        frames.append(_np(r.render_rgba8(W, H) if rgba8 else r.render(W, H)))
    return np.stack(frames)


def _moved(pose, dx):
    return dict(pos=(pose["pos"][0] + dx, pose["pos"][1], pose["pos"][2] + 0.5 * dx), mouse=pose["mouse"],
                time=pose["time"])


# ------------------------------------------------- 1. every scene, ragged tiles, both formats

CASES = [("T", 61, 37, [POSES[k] for k in ("P0", "P1", "P2", "P7")]),
         ("O", 40, 24, [POSES[k] for k in ("P1", "P2")]),
         ("S0", 33, 20, [S0_POSE, _moved(S0_POSE, 0.75), _moved(S0_POSE, -1.5)]),
         ("OG", 48, 32, [POSES[k] for k in ("P3", "P5")])]


@pytest.mark.parametrize("rgba8", [True, False], ids=["rgba8", "float"])
@pytest.mark.parametrize("scene,W,H,views", CASES, ids=[c[0] for c in CASES])
def test_every_view_is_the_single_frame(R, torch_cuda, scene, W, H, views, rgba8):
    torch = torch_cuda
    _setup(R, scene)
    want = _singles(R, W, H, views, rgba8)
    n = len(views)
    # the target is one frame longer than the batch and holds a sentinel
    shape = (n + 1, H, W) if rgba8 else (n + 1, H, W, 4)
    out = torch.full(shape, SENTINEL8 if rgba8 else SENTINELF, dtype=torch.int32 if rgba8 else torch.float32,
                     device="cuda")
    res = R.render_batch(W, H, views, out=out, rgba8=rgba8)
    assert res is out
    got = _np(out)
    ndiff = int((got[:n].view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{scene} {W}x{H} {'rgba8' if rgba8 else 'float'}: {ndiff} of {want.size} words differ over {n} views")
    assert _same(got[:n], want)
    # every pixel before the extra frame was written, the extra frame was not
    if rgba8:
        assert ((got[:n] >> 24) == 255).all() and (got[n] == SENTINEL8).all()
    else:
        assert (got[:n, :, :, 3] == 1.0).all() and (got[n] == np.float32(SENTINELF)).all()
    # the views differ from each other (a batch of one pose repeated would pass otherwise)
    assert all(not _same(want[0], want[k]) for k in range(1, n))
    # n = 1 is the single call, allocated by render_batch in the documented shape
    one = R.render_batch(W, H, views[1:2], rgba8=rgba8)
    assert tuple(one.shape) == ((1, H, W) if rgba8 else (1, H, W, 4))
    assert _same(_np(one), want[1:2])


# ------------------------------------------------- 2. sky next to sponge (scene T)

# A camera at P0's position turned away from the sponge and up: yaw 3.0 puts the sponge behind it, pitch -0.3
# looks above the horizon.  Scene T holds the sponge alone, so nothing lies that way.  That is checked below on
# the CPU, with the reference march (tests/ray_ref.py) over the oracle's sceneSDF along the frame's camera rays.
SKY = dict(pos=POSES["P0"]["pos"], mouse=(3.0, -0.3), time=POSES["P0"]["time"])


def _camera_dirs(W, H, mouse):
    d = ray_ref.camera_dirs_unrotated(W, H)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    y, z = _rot_rows(y, z, np.float32(-mouse[1]))
    x, z = _rot_rows(x, z, np.float32(mouse[0]))
    return np.stack([x, y, z], -1).astype(np.float32).reshape(-1, 3)


def test_sky_view_next_to_sponge_views(R, torch_cuda):
    W, H = 61, 37
    # steps >= 208 (rm_far_sky.h kFarSkyN0), so that the far-sky wave path is taken at all
    steps = 256

    def cast(view):
        return ray_ref.march(lambda p: oracle.scene_dist("T", p, time=view["time"]), np.array(view["pos"], np.float32),
                             _camera_dirs(W, H, view["mouse"]), steps)["status"]
    assert (cast(SKY) == ray_ref.MISS).all(), "the sky view must have no hit"
    hits = int((cast(POSES["P0"]) == ray_ref.HIT).sum())
    assert 0 < hits < W * H, "P0 must show the sponge and some sky"
    _setup(R, "T", steps)
    views = [POSES["P0"], SKY, POSES["P0"], SKY, POSES["P2"]]
    want = _singles(R, W, H, views)
    got = _np(R.render_batch(W, H, views))
    for k in range(len(views)):
        assert _same(got[k], want[k]), f"view {k}"
    assert _same(got[1], got[3]) and not _same(got[0], got[1])


# ------------------------------------------------- 3. offsets

@pytest.mark.parametrize("scene,W,H,rgba8", [("T", 61, 37, True), ("O", 40, 24, False)], ids=["T-rgba8", "O-float"])
def test_offsets_are_render_accumulate_s(R, torch_cuda, scene, W, H, rgba8):
    torch = torch_cuda
    _setup(R, scene)
    pose = POSES["P2"]
    offs = rm.aa_offsets(4)
    R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    want = []
    for o in offs:
        R.set_uniform("u_seed1", float(o[0]) + 0.5, float(o[1]) + 0.5)  # (exact in f32, tests/test_aa_host.py)
        acc = torch.full((H, W) if rgba8 else (H, W, 4), SENTINEL8 if rgba8 else float("nan"),
                         dtype=torch.int32 if rgba8 else torch.float32, device="cuda")
        want.append(_np(R.render_accumulate(W, H, acc)))
    R.set_uniform("u_seed1", 0.5, 0.5)
    centre = _np(R.render_rgba8(W, H) if rgba8 else R.render(W, H))
    views = [dict(pose, offset=(float(o[0]), float(o[1]))) for o in offs] + [pose]
    got = _np(R.render_batch(W, H, views, rgba8=rgba8))
    for k in range(4):
        assert _same(got[k], want[k]), f"offset {offs[k]}"
        assert not _same(got[k], centre), f"offset {offs[k]} gave the centre frame"
    assert _same(got[4], centre)


# ------------------------------------------------- 4. more views than fit casually

def test_300_one_tile_views(R, torch_cuda):
    _setup(R, "S0")
    n, W, H = 300, 8, 8
    views = [dict(pos=(-1.5 + 0.01 * k, 1.0, 0.002 * k), mouse=S0_POSE["mouse"], time=0.0) for k in range(n)]
    want = _singles(R, W, H, views)
    got = _np(R.render_batch(W, H, views))
    bad = [k for k in range(n) if not _same(got[k], want[k])]
    assert not bad, bad[:10]
    # (the line of positions crosses the frame: neighbours differ, so a wrong view index shows)
    assert sum(not _same(want[k], want[k + 1]) for k in range(n - 1)) > n // 2
    assert not _same(want[0], want[256]) and not _same(want[1], want[257])


# ------------------------------------------------- 5. two batches in flight

@pytest.mark.parametrize("scene,W,H", [("T", 61, 37), ("O", 40, 24)])
def test_two_batches_in_flight(R, torch_cuda, scene, W, H):
    torch = torch_cuda
    _setup(R, scene)
    va = [POSES[k] for k in ("P0", "P1", "P2")]
    vb = [POSES[k] for k in ("P3", "P4", "P5", "P6")]
    want_a, want_b = _singles(R, W, H, va), _singles(R, W, H, vb)
    out_a = torch.full((3, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
    out_b = torch.full((4, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
    pa, pb = rm.pack_views(va), rm.pack_views(vb)
    torch.cuda.synchronize()
    R.render_batch(W, H, pa, out=out_a)  # device targets, no stats: both are enqueued and return
    R.render_batch(W, H, pb, out=out_b)
    R.synchronize()
    assert _same(_np(out_a), want_a)
    assert _same(_np(out_b), want_b)
    # ... and more calls in a row than there are upload blocks, each with views of its own
    outs = [torch.full((2, H, W), SENTINEL8, dtype=torch.int32, device="cuda") for _ in range(6)]
    sets = [[vb[k % 4], va[k % 3]] for k in range(6)]
    for o, s in zip(outs, sets):
        R.render_batch(W, H, s, out=o)
    R.synchronize()
    for k, (o, s) in enumerate(zip(outs, sets)):
        assert _same(_np(o), np.stack([want_b[k % 4], want_a[k % 3]])), k


# ------------------------------------------------- 6. stream change

def test_stream_change_between_batches(R, torch_cuda):
    torch = torch_cuda
    W, H = 61, 37
    _setup(R, "T")
    va = [POSES[k] for k in ("P0", "P1", "P2", "P3")]
    vb = [POSES[k] for k in ("P4", "P5")]
    want_a, want_b = _singles(R, W, H, va), _singles(R, W, H, vb)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out_a = torch.full((4, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
    out_b = torch.full((2, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        R.set_stream(s1)
        R.render_batch(W, H, va, out=out_a)
        R.set_stream(s2)
        R.render_batch(W, H, vb, out=out_b)
        R.set_stream(s1)
        out_c = R.render_batch(W, H, va[:2])
        s1.synchronize()
        s2.synchronize()
    finally:
        R.set_stream(None)
    assert _same(_np(out_a), want_a)
    assert _same(_np(out_b), want_b)
    assert _same(_np(out_c), want_a[:2])


# ------------------------------------------------- 7. context state

def test_batch_leaves_the_context_alone(R, torch_cuda):
    W, H = 61, 37
    _setup(R, "T")
    p = POSES["P7"]
    R.set_pose(p["pos"], p["mouse"], p["time"])
    R.set_params(count_evals=1)
    _, st0 = R.render_rgba8(W, H, stats=True)
    assert st0["evals"] > 0
    R.set_params(count_evals=0)
    before = _np(R.render_rgba8(W, H))
    views = [POSES["P0"], POSES["P1"], POSES["P2"]]
    out, st = R.render_batch(W, H, views, stats=True)
    assert R.certified_steps() == 0 and R.reflection_cleared_steps() == 0
    assert st["pixels"] == 3 * W * H and st["kernel_ms"] > 0.0 and st["evals"] == 0
    assert st["dispatch"] == "row-major" and st["scene"] == 1 and st["flop"] == 0 and st["skipped"] == 0
    assert st["lat_tiles"] == 0 and st["certified"] == 0 and st["reflection_cleared"] == 0
    # count_evals does not apply to a batch: the same frames, still nothing counted
    R.set_params(count_evals=1)
    out2, st2 = R.render_batch(W, H, views, stats=True)
    R.set_params(count_evals=0)
    assert st2["evals"] == 0 and _same(_np(out), _np(out2))
    # the context's pose is what it was
    assert _same(_np(R.render_rgba8(W, H)), before)
    assert _same(_np(out), _singles(R, W, H, views))


# ------------------------------------------------- 8. u_resolution and the cache

def test_resolution_uniform_and_cache(torch_cuda):
    W, H = 61, 37
    views = [POSES["P0"], POSES["P1"], POSES["P2"], POSES["P7"]]
    r = rm.Renderer(0)
    try:
        _setup(r, "T")
        assert r.resolution_cache()[0] == 0
        got = _np(r.render_batch(W, H, views))      # a resolution this context has not seen
        assert r.resolution_cache()[0] == 1          # one entry, however many views
        r.render_batch(W, H, views[:2])
        assert r.resolution_cache()[0] == 1
        assert _same(got, _singles(r, W, H, views))
        assert r.resolution_cache()[0] == 1          # (the singles share the entry)
        r.set_uniform("u_resolution", 80.0, 50.0)
        got2 = _np(r.render_batch(W, H, views))
        assert r.resolution_cache()[0] == 2
        assert _same(got2, _singles(r, W, H, views))
        assert not _same(got2, got)
        _setup(r, "O")                               # (scene O divides: no cache entry, same contract)
        assert _same(_np(r.render_batch(40, 24, views[:2], rgba8=False)), _singles(r, 40, 24, views[:2], False))
    finally:
        r.close()


# ------------------------------------------------- 9. host target

@pytest.mark.parametrize("rgba8", [True, False], ids=["rgba8", "float"])
def test_host_target(R, torch_cuda, rgba8):
    W, H = 61, 37
    _setup(R, "T")
    views = [POSES["P0"], POSES["P1"], POSES["P2"]]
    dev = _np(R.render_batch(W, H, views, rgba8=rgba8))
    host = np.full((4, H, W) if rgba8 else (4, H, W, 4), SENTINEL8 if rgba8 else SENTINELF,
                   np.uint32 if rgba8 else np.float32)
    res, st = R.render_batch(W, H, views, out=host, rgba8=rgba8, stats=True)
    assert res is host and st["pixels"] == 3 * W * H
    assert _same(host[:3], dev)
    assert (host[3] == (SENTINEL8 if rgba8 else np.float32(SENTINELF))).all()


# ------------------------------------------------- 10. arguments

def _call(fn, r, W, H, views, n, out):
    vp = ctypes.c_void_p(views.ctypes.data) if views is not None else None
    return fn(r._ctx, W, H, vp, n, ctypes.c_void_p(out) if out else None, None)


@pytest.mark.parametrize("name", ["rm_render_batch", "rm_render_batch_rgba8"])
def test_arguments(R, torch_cuda, name):
    torch = torch_cuda
    fn = getattr(rm.lib(), name)
    _setup(R, "T")
    out = torch.full((2, 8, 8, 4), SENTINELF, dtype=torch.float32, device="cuda")  # (room for either format)
    before = out.clone()
    v = rm.pack_views([POSES["P0"], POSES["P1"]])
    p = out.data_ptr()
    # n = 0: RM_OK, nothing written (views and out may be NULL then)
    assert _call(fn, R, 8, 8, v, 0, p) == 0
    assert _call(fn, R, 8, 8, None, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    # NULL views or out with n > 0
    assert _call(fn, R, 8, 8, None, 2, p) == INVALID
    assert _call(fn, R, 8, 8, v, 2, None) == INVALID
    # the size rule (before any pointer is used: these counts have no such arrays behind them)
    assert _call(fn, R, 8, 8, v, 65536, p) == INVALID
    assert _call(fn, R, 8, 8, v, -1, p) == INVALID
    assert _call(fn, R, 0, 8, v, 2, p) == INVALID
    assert _call(fn, R, 8, 0, v, 2, p) == INVALID
    assert _call(fn, R, 1 << 16, 1 << 15, v, 2, p) == INVALID  # n * W * H = 2^32
    assert _call(fn, R, 8, 65535 * 8 + 1, v, 1, p) == INVALID
    # an offset of 0.5, a NaN offset
    for bad in (0.5, float("nan"), -0.75):
        w = v.copy()
        w[1, 7] = bad
        assert _call(fn, R, 8, 8, w, 2, p) == INVALID, bad
        assert "offset" in rm.lib().rm_last_error(R._ctx).decode()
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    # ... and the same arrays are fine as they were
    assert _call(fn, R, 8, 8, v, 2, p) == 0
    torch.cuda.synchronize()
    assert not torch.equal(out, before)
    # the Python surface refuses a short target and views of another shape
    with pytest.raises(ValueError):
        R.render_batch(8, 8, v, out=torch.empty((1, 8, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        R.render_batch(8, 8, np.zeros((2, 5), np.float32))


def test_scene_plugin_and_no_scene(torch_cuda):
    torch = torch_cuda
    r = rm.Renderer(0)
    try:
        out = torch.full((2, 8, 8, 4), SENTINELF, dtype=torch.float32, device="cuda")
        before = out.clone()
        v = rm.pack_views([POSES["P0"], POSES["P1"]])
        for name in ("rm_render_batch", "rm_render_batch_rgba8"):
            assert _call(getattr(rm.lib(), name), r, 8, 8, v, 2, out.data_ptr()) == NO_SCENE
        r.load_scene(os.path.join(rm.SCENES_DIR, "metaballs.hip"))
        for name in ("rm_render_batch", "rm_render_batch_rgba8"):
            assert _call(getattr(rm.lib(), name), r, 8, 8, v, 2, out.data_ptr()) == SCENE
            assert "view batches: built-in scenes only" in rm.lib().rm_last_error(r._ctx).decode()
        with pytest.raises(rm.RmError):
            r.render_batch(8, 8, v)
        torch.cuda.synchronize()
        assert torch.equal(out, before)
    finally:
        r.close()


# ------------------------------------------------- 11. the app

def test_headless_app_writes_the_views(R, torch_cuda, tmp_path):
    """apps/raymarch_headless --views (rm::Shader::renderBatch): three lines,
    three PPMs, the frames render_batch returns."""
    W, H = 61, 37
    exe = os.path.join(ROOT, "apps", "raymarch_headless")
    views = [POSES["P0"], dict(POSES["P1"], offset=(0.25, -0.375)), POSES["P2"]]
    packed = rm.pack_views(views)
    lines = ["# px py pz mx my t [ox oy]"]
    for k, row in enumerate(packed):
        vals = row if k == 1 else row[:6]  # (with and without the offset columns)
        lines.append(" ".join(repr(float(x)) for x in vals))  # (repr of a float32's double: reads back exactly)
    (tmp_path / "views.txt").write_text("\n".join(lines) + "\n\n")
    run = subprocess.run([exe, "--scene", "template.frag", "--w", str(W), "--h", str(H), "--steps", str(STEPS),
                          "--views", str(tmp_path / "views.txt"), "--ppm", str(tmp_path / "v"), "--stats"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert '"views": 3' in run.stdout and '"kernel_ms"' in run.stdout
    _setup(R, "T")
    want = _np(R.render_batch(W, H, views))
    for k in range(3):
        data = (tmp_path / f"v.{k:04d}.ppm").read_bytes()
        img = np.frombuffer(data[data.index(b"255\n") + 4:], np.uint8).reshape(H, W, 3)
        rgb = np.stack([(want[k] >> s) & 255 for s in (0, 8, 16)], -1).astype(np.uint8)
        assert np.array_equal(img, rgb), k
    assert not (tmp_path / "v.0003.ppm").exists()
    # a malformed line is refused
    (tmp_path / "bad.txt").write_text("1 2 3 4 5\n")
    bad = subprocess.run([exe, "--scene", "template.frag", "--views", str(tmp_path / "bad.txt")], capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 2
