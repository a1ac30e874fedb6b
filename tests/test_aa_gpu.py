"""Adaptive supersampling on the GPU (include/rm.h rm_render_aa_rgba8,
rm_refine_rgba8): the refined pixels against what a caller gets today by
blending rm_render_accumulate's jittered frames on the host (every byte), the
mask against the edge rule's restatement (tests/aa_ref.py) on the GPU's own
frame, crafted frames, a queue longer than one sweep of the grid, the oracle,
the argument checks and the headless app."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from raymarching_amd import POSES, S0_POSE, _lib
from tests import aa_ref
from tests.parity import POLICY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def _setup(r, scene, pose, steps):
    r.load_scene(rm.SCENE_FILES[scene])
    r.set_pose(pose["pos"], pose["mouse"], pose["time"])
    r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0)
    r.set_uniform("u_seed1", 0.5, 0.5)
    r.set_uniform("u_sample_part", 1.0)


_REF = {}  # (scene, W, H, pose, steps, K) -> the every-pixel K-sample frame, computed once and left unchanged


def _supersampled(torch, r, scene, W, H, pose_name, pose, steps, K):
    """Every pixel's K-sample colour as a caller builds it today: the K float
    frames render_accumulate returns with u_sample_part = 1 and u_seed1 =
    o + 0.5, their tree mean, the scene's RGBA8 pack.  Expects _setup's state
    and leaves it."""
    key = (scene, W, H, pose_name, steps, K)
    if key not in _REF:
        frames = []
        for seed in aa_ref.seeds(K):
            r.set_uniform("u_seed1", float(seed[0]), float(seed[1]))
            acc = torch.full((H, W, 4), float("nan"), device="cuda")
            frames.append(r.render_accumulate(W, H, acc).cpu().numpy())
        r.set_uniform("u_seed1", 0.5, 0.5)
        ref = oracle.pack_rgba8(aa_ref.tree_mean(frames))
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _words(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- 1. every pixel

EVERY = [("T", 61, 37, "P2", K) for K in (2, 4, 8)] + [("O", 40, 24, "P1", K) for K in (2, 4, 8)] + \
        [("S0", 33, 20, "S0", 4), ("OG", 48, 32, "P3", 4)]


@pytest.mark.parametrize("scene,W,H,pose_name,K", EVERY)
def test_threshold_zero_supersamples_every_pixel(R, torch_cuda, scene, W, H, pose_name, K):
    pose = S0_POSE if pose_name == "S0" else POSES[pose_name]
    _setup(R, scene, pose, 128)
    want = _supersampled(torch_cuda, R, scene, W, H, pose_name, pose, 128, K)
    out, mask, st = R.render_aa(W, H, samples=K, threshold=0, mask=True, stats=True)
    got = _words(out)
    ndiff = int((got != want).sum())
    print(f"{scene} {W}x{H} K={K}: {ndiff} of {W * H} words differ from the blended accumulate frames")
    assert ndiff == 0
    assert st["refined"] == W * H and bool(mask.all())
    # supersampling did something: the frame differs from the centre samples
    assert not np.array_equal(got, _words(R.render_rgba8(W, H)))


@pytest.mark.parametrize("scene,W,H,pose_name,K", EVERY[:6])
def test_other_lane_layout_gives_the_same_bytes(R, torch_cuda, monkeypatch, scene, W, H, pose_name, K):
    """RM_AA_LAYOUT=pixel (one lane per queue entry, the samples in a loop: the
    layout measured against the default) sums the same tree."""
    pose = POSES[pose_name]
    _setup(R, scene, pose, 128)
    want = _supersampled(torch_cuda, R, scene, W, H, pose_name, pose, 128, K)
    monkeypatch.setenv("RM_AA_LAYOUT", "pixel")
    out, st = R.render_aa(W, H, samples=K, threshold=0, stats=True)
    assert st["refined"] == W * H and int((_words(out) != want).sum()) == 0


# ---------------------------------------------------------------- 2. adaptive

@pytest.mark.parametrize("scene", ["T", "O"])
def test_adaptive_threshold_32(R, torch_cuda, scene):
    torch = torch_cuda
    W, H, K, pose = 61, 37, 4, POSES["P2"]
    _setup(R, scene, pose, 128)
    full = _supersampled(torch, R, scene, W, H, "P2", pose, 128, K)
    base = _words(R.render_rgba8(W, H))
    want_mask = aa_ref.edge_mask(base, 32)
    out, mask, st = R.render_aa(W, H, samples=K, threshold=32, mask=True, stats=True)
    got, m = _words(out), mask.cpu().numpy()
    share = float(want_mask.mean())
    print(f"{scene} {W}x{H}: edge share {share:.3f}, refined {st['refined']}")
    assert 0.03 <= share <= 0.7, share  # both branches
    assert m.dtype == np.uint8 and np.array_equal(m, want_mask)
    assert st["refined"] == int(want_mask.sum())
    assert np.array_equal(got[m == 0], base[m == 0])
    assert np.array_equal(got[m == 1], full[m == 1])
    # render_aa = refine(render_rgba8()), and the mask is optional
    two = R.render_rgba8(W, H)
    assert R.refine(two, samples=K, threshold=32) is two
    assert np.array_equal(_words(two), got)
    # host pointers: staged, the same bytes
    host, host_mask = R.render_aa(W, H, samples=K, threshold=32, out=np.zeros((H, W), np.uint32), mask=True)
    assert np.array_equal(host, got) and np.array_equal(host_mask, m)
    host2 = base.copy()
    R.refine(host2, samples=K, threshold=32)
    assert np.array_equal(host2, got)


def test_queue_follows_the_context_across_streams(R, torch_cuda):
    """One queue per context: a refine on another stream than the last one
    waits for it (the event recorded when the context left that stream)."""
    torch = torch_cuda
    W, H, K, pose = 61, 37, 4, POSES["P2"]
    _setup(R, "T", pose, 128)
    full = _supersampled(torch, R, "T", W, H, "P2", pose, 128, K)
    base = _words(R.render_rgba8(W, H))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        R.set_stream(s1)
        every = R.render_aa(W, H, samples=K, threshold=0)
        R.set_stream(s2)
        some, mask = R.render_aa(W, H, samples=K, threshold=32, mask=True)
        R.set_stream(s1)
        again = R.render_aa(W, H, samples=K, threshold=0)
    finally:
        R.set_stream(None)
    torch.cuda.synchronize()
    assert np.array_equal(_words(every), full) and np.array_equal(_words(again), full)
    assert np.array_equal(_words(some), np.where(mask.cpu().numpy() == 1, full, base))


# ---------------------------------------------------------------- 3. crafted frames

WHITE = 0xFFFFFFFF


def _refine_crafted(torch, R, frame, K, threshold, full):
    """refine() of a crafted frame: the mask is the rule's, refined pixels take
    the supersampled colour, every other word is untouched."""
    H, W = frame.shape
    want_mask = aa_ref.edge_mask(frame, threshold)
    dev = torch.from_numpy(frame.view(np.int32).copy()).cuda()
    _, mask, st = R.refine(dev, samples=K, threshold=threshold, mask=True, stats=True)
    got, m = _words(dev), mask.cpu().numpy()
    assert np.array_equal(m, want_mask)
    assert st["refined"] == int(want_mask.sum())
    assert np.array_equal(got[m == 0], frame[m == 0])
    assert np.array_equal(got[m == 1], full[m == 1])
    return m


@pytest.mark.parametrize("W,H", [(61, 37), (5, 3), (1, 1)])
def test_crafted_frames(R, torch_cuda, W, H):
    torch = torch_cuda
    K = 4
    _setup(R, "S0", S0_POSE, 64)
    full = _supersampled(torch, R, "S0", W, H, "S0", S0_POSE, 64, K)
    for px, py in [(0, 0), (W - 1, H - 1), (8, 8)]:
        if px >= W or py >= H:
            continue
        frame = np.zeros((H, W), np.uint32)
        frame[py, px] = WHITE
        m = _refine_crafted(torch, R, frame, K, 32, full)
        block = np.zeros((H, W), np.uint8)
        if W * H > 1:  # (a 1x1 frame has no edge pixel: its neighbourhood is itself)
            block[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = 1
        assert np.array_equal(m, block), (px, py)
    noise = np.random.default_rng(W * 100 + H).integers(0, 2 ** 32, (H, W), dtype=np.uint32)
    for threshold in (1, 255):
        _refine_crafted(torch, R, noise, K, threshold, full)


# ---------------------------------------------------------------- 4. a long queue

def test_queue_longer_than_one_sweep(R, torch_cuda):
    """512 x 512 at threshold 0: 2^18 queue entries, 2^20 samples, many strides
    of every wave over the queue."""
    W = H = 512
    _setup(R, "S0", S0_POSE, 64)
    want = _supersampled(torch_cuda, R, "S0", W, H, "S0", S0_POSE, 64, 4)
    out, st = R.render_aa(W, H, samples=4, threshold=0, stats=True)
    assert st["refined"] == 1 << 18
    assert int((_words(out) != want).sum()) == 0


# ---------------------------------------------------------------- 5. the oracle

@pytest.mark.parametrize("scene,W,H", [("T", 64, 48), ("O", 48, 32)])
def test_against_the_oracle(R, torch_cuda, scene, W, H):
    """The reference is built on the GPU's mask: the oracle's jittered pixels,
    tree mean, where the mask is set, its centre frame elsewhere, packed.  A
    float within 2e-3 moves a byte by at most one, and a mean of K samples is
    within tolerance when all K are: the share of pixels whose three bytes each
    differ by at most 1 is at least 1 - K (1 - POLICY f2e3)."""
    K, pose = 4, POSES["P3"]
    _setup(R, scene, pose, 128)
    out, mask = R.render_aa(W, H, samples=K, threshold=32, mask=True)
    got, m = _words(out), mask.cpu().numpy().astype(bool)
    kw = dict(pos=pose["pos"], mouse=pose["mouse"], time=pose["time"], max_steps=128)
    ref, _ = oracle.render(scene, W, H, **kw)
    ys, xs = np.nonzero(m)
    assert 0 < len(xs) < W * H
    samples = [oracle.render_pixels(scene, W, H, xs, ys, jitter=(float(o[0]), float(o[1])), **kw)[0]
               for o in aa_ref.offsets(K)]
    ref[ys, xs] = aa_ref.tree_mean(samples)
    want = oracle.pack_rgba8(ref)
    d = np.zeros((H, W), np.int64)
    for shift in (0, 8, 16):
        d = np.maximum(d, np.abs(((got >> shift) & 255).astype(np.int64) - ((want >> shift) & 255).astype(np.int64)))
    share = float(np.mean(d <= 1))
    level = 1.0 - K * (1.0 - POLICY[scene]["f2e3"])
    print(f"{scene} {W}x{H}: {share:.4f} of pixels within one byte of the oracle (level {level:.2f}), "
          f"{int(m.sum())} refined")
    assert share >= level, (share, level)


# ---------------------------------------------------------------- 6. errors

INVALID, SCENE, NO_SCENE = 1, 3, 4


def _call(fn, r, W, H, params, frame, mask=None):
    return fn(r._ctx, W, H, ctypes.byref(params) if params is not None else None,
              ctypes.c_void_p(frame) if frame else None, ctypes.c_void_p(mask) if mask else None, None)


@pytest.mark.parametrize("name", ["rm_refine_rgba8", "rm_render_aa_rgba8"])
def test_argument_checks(R, torch_cuda, name):
    torch = torch_cuda
    fn = getattr(rm.lib(), name)
    _setup(R, "S0", S0_POSE, 64)
    frame = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    good = _lib.RmAaParams(4, 32)
    p = frame.data_ptr()
    assert _call(fn, R, 4, 4, good, p) == 0
    for W, H in [(0, 4), (4, 0), (-1, 4), (4, -1), (1 << 15, 1 << 15), (1 << 30, 1)]:
        assert _call(fn, R, W, H, good, p) == INVALID, (W, H)
    assert _call(fn, R, 4, 4, None, p) == INVALID
    assert _call(fn, R, 4, 4, good, None) == INVALID
    for K in (0, 1, 3, 16, -4):
        assert _call(fn, R, 4, 4, _lib.RmAaParams(K, 32), p) == INVALID, K
    for t in (-1, 256):
        assert _call(fn, R, 4, 4, _lib.RmAaParams(4, t), p) == INVALID, t
    # frame and mask live in the same place
    host_mask = np.zeros((4, 4), np.uint8)
    assert _call(fn, R, 4, 4, good, p, host_mask.ctypes.data) == INVALID
    assert "mixed" in rm.lib().rm_last_error(R._ctx).decode()
    torch.cuda.synchronize()


def test_scene_plugin_and_no_scene(torch_cuda):
    torch = torch_cuda
    r = rm.Renderer(0)
    try:
        frame = torch.full((8, 8), 0x00FFFFFF, dtype=torch.int32, device="cuda")
        frame[0, 0] = 0
        before = frame.clone()
        good = _lib.RmAaParams(4, 32)
        for name in ("rm_refine_rgba8", "rm_render_aa_rgba8"):
            assert _call(getattr(rm.lib(), name), r, 8, 8, good, frame.data_ptr()) == NO_SCENE
        r.load_scene(os.path.join(rm.SCENES_DIR, "metaballs.hip"))
        for name in ("rm_refine_rgba8", "rm_render_aa_rgba8"):
            assert _call(getattr(rm.lib(), name), r, 8, 8, good, frame.data_ptr()) == SCENE
            assert "adaptive supersampling: built-in scenes only" in rm.lib().rm_last_error(r._ctx).decode()
        with pytest.raises(rm.RmError):
            r.render_aa(8, 8)
        torch.cuda.synchronize()
        assert torch.equal(frame, before)
    finally:
        r.close()


# ---------------------------------------------------------------- 7. the headless app

def test_headless_app_writes_render_aa(R, torch_cuda, tmp_path):
    """apps/raymarch_headless --aa 4:32 (rm::RenderTexture::drawAA): the frame
    render_aa returns for the same pose."""
    W, H = 96, 54
    exe = os.path.join(ROOT, "apps", "raymarch_headless")
    ppm = tmp_path / "aa.ppm"
    run = subprocess.run([exe, "--scene", "template.frag", "--w", str(W), "--h", str(H), "--frames", "1",
                          "--time-freeze", "--aa", "4:32", "--ppm", str(ppm)], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stderr
    data = ppm.read_bytes()
    img = np.frombuffer(data[data.index(b"255\n") + 4:], np.uint8).reshape(H, W, 3)
    _setup(R, "T", POSES["P0"], 128)  # the app's start-up pose: main.cpp's
    out, st = R.render_aa(W, H, samples=4, threshold=32, stats=True)
    want = _words(out)
    rgb = np.stack([(want >> s) & 255 for s in (0, 8, 16)], -1).astype(np.uint8)
    assert 0 < st["refined"] < W * H
    assert np.array_equal(img, rgb)
    # a malformed --aa is refused
    bad = subprocess.run([exe, "--aa", "3"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2
