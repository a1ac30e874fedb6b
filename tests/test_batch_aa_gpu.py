"""Adaptive supersampling of a view batch on the GPU (include/rm.h
rm_render_batch_aa_rgba8, rm_refine_batch_rgba8): every view's
frame, mask and count against this build's own single-frame call for the same
pose (set_pose + render_aa) -- every byte, no tolerance; tests/test_aa_gpu.py
ties that call to the oracle.  All four scenes and every sample count, crafted
frames through refine_batch, more groups than the persistent grid holds and more
views than a byte counts, n = 1, host pointers, the context's state, calls in
flight across a stream change, the argument checks and the headless app."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import POSES, S0_POSE, _lib
from tests import aa_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, SCENE, NO_SCENE = 1, 3, 4
STEPS = 128
SENTINEL8 = 0x5A5A5A5A  # (alpha 0x5A: no pixel the pass writes, whose alpha is 255)
SENTINEL_MASK = 0xA5    # (a mask byte is 0 or 1)
WHITE = 0xFFFFFFFF
GREY = 0xFF808080


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
    """every byte"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _moved(pose, dx):
    return dict(pos=(pose["pos"][0] + dx, pose["pos"][1], pose["pos"][2] + 0.5 * dx), mouse=pose["mouse"],
                time=pose["time"])


_LOOP = {}  # (scene, W, H, view names, K, threshold) -> (frames, masks, counts), computed once and left unchanged


def _loop(r, key, W, H, views, K, threshold):
    """What a caller does today: set_pose + render_aa per view -> frames [n, H, W] uint32, masks [n, H, W] uint8,
    counts [n] (each call's rm_aa_stats.refined).  Expects _setup's state for the scene."""
    key = key + (W, H, K, threshold)
    if key not in _LOOP:
        frames, masks, counts = [], [], []
        for v in views:
            r.set_pose(v["pos"], v["mouse"], v["time"])
            out, mask, st = r.render_aa(W, H, samples=K, threshold=threshold, mask=True, stats=True)
            frames.append(_np(out))
            masks.append(mask.cpu().numpy())
            counts.append(st["refined"])
        res = (np.stack(frames), np.stack(masks), np.array(counts, np.int64))
        for a in res:
            a.setflags(write=False)
        _LOOP[key] = res
    return _LOOP[key]


def _raw(fn, r, W, H, packed, n, K, threshold, frames, mask=None, refined=None, stats=None):
    """the C call; frames / mask / refined: addresses or None"""
    p = _lib.RmAaParams(K, threshold)
    vp = ctypes.c_void_p(packed.ctypes.data) if packed is not None else None
    return fn(r._ctx, W, H, vp, n, ctypes.byref(p), ctypes.c_void_p(frames) if frames else None,
              ctypes.c_void_p(mask) if mask else None, ctypes.c_void_p(refined) if refined else None, stats)


# ------------------------------------------------- 1. every view is the single call

SCENES = {"T": (61, 37, ("P0", "P1", "P2", "P7")), "O": (40, 24, ("P1", "P2")), "S0": (33, 20, ("a", "b", "c")),
          "OG": (48, 32, ("P3", "P5"))}
S0_VIEWS = dict(a=S0_POSE, b=_moved(S0_POSE, 0.75), c=_moved(S0_POSE, -1.5))
EVERY = [("T", K) for K in (2, 4, 8)] + [("O", K) for K in (2, 4, 8)] + [("S0", 4), ("OG", 4)]


def _views_of(scene):
    W, H, names = SCENES[scene]
    return W, H, names, [S0_VIEWS[k] if scene == "S0" else POSES[k] for k in names]


@pytest.mark.parametrize("threshold", [0, 32])
@pytest.mark.parametrize("scene,K", EVERY, ids=[f"{s}-K{k}" for s, k in EVERY])
def test_every_view_is_the_single_call(R, torch_cuda, scene, K, threshold):
    torch = torch_cuda
    W, H, names, views = _views_of(scene)
    n = len(views)
    _setup(R, scene)
    want, want_mask, want_n = _loop(R, (scene, names), W, H, views, K, threshold)
    if threshold == 0:
        assert (want_n == W * H).all()
    else:
        # the loop's own numbers: a view with some but not all pixels refined, whose last group is partial
        print(f"{scene} {W}x{H} K={K}: the loop refines {want_n.tolist()} of {W * H}")
        assert any(0 < c < W * H and c % (64 // K) != 0 for c in want_n), want_n
    # the targets are one frame (one word) longer than the batch and hold sentinels
    out = torch.full((n + 1, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
    mask = torch.full((n + 1, H, W), SENTINEL_MASK, dtype=torch.uint8, device="cuda")
    refined = torch.full((n + 1,), SENTINEL8, dtype=torch.int32, device="cuda")
    st = _lib.RmAaStats()
    assert _raw(rm.lib().rm_render_batch_aa_rgba8, R, W, H, rm.pack_views(views), n, K, threshold, out.data_ptr(),
                mask.data_ptr(), refined.data_ptr(), ctypes.byref(st)) == 0
    got, got_mask, got_n = _np(out), mask.cpu().numpy(), _np(refined)
    print(f"{scene} {W}x{H} K={K} threshold {threshold}: {int((got[:n] != want).sum())} words, "
          f"{int((got_mask[:n] != want_mask).sum())} mask bytes differ over {n} views; refined {got_n[:n].tolist()}")
    assert _same(got[:n], want)
    assert _same(got_mask[:n], want_mask)
    assert np.array_equal(got_n[:n].astype(np.int64), want_n)
    assert (got[n] == SENTINEL8).all() and (got_mask[n] == SENTINEL_MASK).all() and got_n[n] == SENTINEL8
    assert st.refined == int(want_n.sum()) and st.base_ms > 0.0 and st.detect_ms > 0.0 and st.refine_ms > 0.0
    # the views differ from each other (a batch of one pose repeated would pass otherwise)
    assert all(not _same(want[0], want[k]) for k in range(1, n))
    # the Python surface, without the optional outputs and with them: the same bytes
    plain = R.render_batch_aa(W, H, views, samples=K, threshold=threshold)
    assert tuple(plain.shape) == (n, H, W) and _same(_np(plain), want)
    o2, m2, r2, s2 = R.render_batch_aa(W, H, views, samples=K, threshold=threshold, mask=True, refined=True, stats=True)
    assert _same(_np(o2), want) and _same(m2.cpu().numpy(), want_mask)
    assert np.array_equal(_np(r2).astype(np.int64), want_n) and s2["refined"] == int(want_n.sum())
    # render_batch_aa = refine_batch(render_batch())
    two = R.render_batch(W, H, views)
    assert R.refine_batch(two, views, samples=K, threshold=threshold) is two
    assert _same(_np(two), want)


@pytest.mark.parametrize("scene,K,threshold", [("T", 4, 32), ("O", 2, 32), ("S0", 4, 0)])
def test_packed_counters_give_the_same_bytes(R, torch_cuda, monkeypatch, scene, K, threshold):
    """RM_BATCH_AA_COUNTERS=packed (the views' counters 4 bytes apart: the layout measured against the default
    line per counter) changes where the counts lie, not what is refined."""
    W, H, names, views = _views_of(scene)
    _setup(R, scene)
    want, want_mask, want_n = _loop(R, (scene, names), W, H, views, K, threshold)
    monkeypatch.setenv("RM_BATCH_AA_COUNTERS", "packed")
    out, mask, refined, st = R.render_batch_aa(W, H, views, samples=K, threshold=threshold, mask=True, refined=True,
                                               stats=True)
    assert _same(_np(out), want) and _same(mask.cpu().numpy(), want_mask)
    assert np.array_equal(_np(refined).astype(np.int64), want_n) and st["refined"] == int(want_n.sum())


# ------------------------------------------------- 2. crafted frames

def _crafted(W, H):
    """all zero | a lone white pixel at (0, 0) | one at an interior tile corner | constant grey | noise | all zero"""
    f = np.zeros((6, H, W), np.uint32)
    f[1, 0, 0] = WHITE
    f[2, min(8, H - 1), min(8, W - 1)] = WHITE
    f[3] = GREY
    f[4] = np.random.default_rng(W * 100 + H).integers(0, 2 ** 32, (H, W), dtype=np.uint32)
    return f


@pytest.mark.parametrize("W,H", [(61, 37), (5, 3), (1, 1)])
def test_crafted_frames_through_refine_batch(R, torch_cuda, W, H):
    torch = torch_cuda
    K = 4
    names = ("P0", "P1", "P2", "P3", "P4", "P5")
    views = [POSES[k] for k in names]
    _setup(R, "T")
    # every pixel of every view supersampled: the batch's threshold-0 frames, which are the single calls'
    full = _np(R.render_batch_aa(W, H, views, samples=K, threshold=0))
    assert _same(full, _loop(R, ("T", names), W, H, views, K, 0)[0])
    frames = _crafted(W, H)
    for threshold in (1, 255):
        want_mask = np.stack([aa_ref.edge_mask(f, threshold) for f in frames])
        dev = torch.from_numpy(frames.view(np.int32).copy()).cuda()
        res, mask, refined, st = R.refine_batch(dev, views, samples=K, threshold=threshold, mask=True, refined=True,
                                                stats=True)
        assert res is dev
        got, m, counts = _np(dev), mask.cpu().numpy(), _np(refined)
        assert m.dtype == np.uint8 and _same(m, want_mask)
        assert np.array_equal(counts.astype(np.int64), want_mask.reshape(6, -1).sum(1))
        assert st["refined"] == int(want_mask.sum()) and st["base_ms"] == 0.0
        # the first, the last and a middle view queue nothing
        assert counts[0] == 0 and counts[5] == 0 and counts[3] == 0
        if (W, H) == (61, 37):
            assert counts[1] == 4 and counts[2] == 9
            if threshold == 1:
                assert counts[4] == W * H
        if (W, H) == (1, 1):
            assert not counts.any()  # (a 1x1 frame has no edge pixel: its neighbourhood is itself)
        assert np.array_equal(got[m == 0], frames[m == 0])  # unmasked words are untouched
        assert np.array_equal(got[m == 1], full[m == 1])    # masked pixels: the views' supersampled colour
        # host pointers: staged, the same bytes
        host = frames.copy()
        _, hm, hr = R.refine_batch(host, views, samples=K, threshold=threshold, mask=True, refined=True)
        assert _same(host, got) and _same(hm, m) and hr.dtype == np.uint32 and _same(hr, counts)


# ------------------------------------------------- 3. more groups than the grid, more views than a byte counts

def test_4096_one_tile_views(R, torch_cuda):
    """S0, 8 x 8, 4096 views cycling four poses, K = 8, threshold 0: 8 groups per view, 32768 groups against
    at most about 8192 resident waves, so every wave strides several times and crosses views."""
    _setup(R, "S0")
    n, W, H, K = 4096, 8, 8, 8
    names = ("a", "b", "c", "d")
    four = [S0_POSE, _moved(S0_POSE, 0.75), _moved(S0_POSE, -1.5), _moved(S0_POSE, 0.3)]
    want4, mask4, n4 = _loop(R, ("S0", names), W, H, four, K, 0)
    assert all(not _same(want4[0], want4[k]) for k in range(1, 4)) and (n4 == 64).all()
    packed = np.tile(rm.pack_views(four), (n // 4, 1))
    out, mask, refined, st = R.render_batch_aa(W, H, packed, samples=K, threshold=0, mask=True, refined=True, stats=True)
    got = _np(out)
    want = np.tile(want4, (n // 4, 1, 1))
    bad = [k for k in range(n) if not _same(got[k], want[k])]
    assert not bad, bad[:10]
    assert bool(mask.all()) and (_np(refined) == 64).all() and st["refined"] == n * 64


# ------------------------------------------------- 4. n = 1, a host target, the context's state, streams

def test_one_view_is_render_aa(R, torch_cuda):
    W, H, K = 96, 54, 4
    _setup(R, "T")
    p = POSES["P0"]
    want, want_mask, want_n = _loop(R, ("T", ("P0",)), W, H, [p], K, 32)
    assert 0 < want_n[0] < W * H
    out, mask, refined = R.render_batch_aa(W, H, [p], samples=K, threshold=32, mask=True, refined=True)
    assert _same(_np(out), want) and _same(mask.cpu().numpy(), want_mask) and int(_np(refined)[0]) == want_n[0]


def test_host_target(R, torch_cuda):
    W, H, K = 61, 37, 4
    _setup(R, "T")
    views = [POSES["P0"], POSES["P1"], POSES["P2"]]
    dev, dev_mask, dev_n = R.render_batch_aa(W, H, views, samples=K, threshold=32, mask=True, refined=True)
    host = np.full((4, H, W), SENTINEL8, np.uint32)
    res, mask, refined, st = R.render_batch_aa(W, H, views, samples=K, threshold=32, out=host, mask=True, refined=True,
                                               stats=True)
    assert res is host and isinstance(mask, np.ndarray) and isinstance(refined, np.ndarray)
    assert _same(host[:3], _np(dev)) and (host[3] == SENTINEL8).all()
    assert _same(mask, dev_mask.cpu().numpy()) and _same(refined, _np(dev_n))
    assert st["refined"] == int(refined.sum()) and 0 < st["refined"] < 3 * W * H
    # a host target without the optional outputs
    host2 = np.zeros((3, H, W), np.uint32)
    assert R.render_batch_aa(W, H, views, samples=K, threshold=32, out=host2) is host2
    assert _same(host2, _np(dev))


def test_batch_aa_leaves_the_context_alone(R, torch_cuda):
    W, H, K = 61, 37, 4
    _setup(R, "T")
    p = POSES["P7"]
    R.set_pose(p["pos"], p["mouse"], p["time"])
    R.set_uniform("u_seed1", 0.25, 0.875)  # (neither read nor changed: render_accumulate below sees it)
    torch = torch_cuda
    acc0 = _np(R.render_accumulate(W, H, torch.full((H, W), SENTINEL8, dtype=torch.int32, device="cuda")))
    before = _np(R.render_rgba8(W, H))
    before_aa = _np(R.render_aa(W, H, samples=K, threshold=32))
    views = [POSES["P0"], POSES["P1"], POSES["P2"]]
    got = _np(R.render_batch_aa(W, H, views, samples=K, threshold=32))
    assert _same(_np(R.render_rgba8(W, H)), before)
    assert _same(_np(R.render_aa(W, H, samples=K, threshold=32)), before_aa)
    assert _same(_np(R.render_accumulate(W, H, torch.full((H, W), SENTINEL8, dtype=torch.int32, device="cuda"))), acc0)
    R.set_uniform("u_seed1", 0.5, 0.5)
    assert _same(got, _loop(R, ("T", ("P0", "P1", "P2")), W, H, views, K, 32)[0])
    # ... and the context's seed did not move the batch's samples
    assert _same(_np(R.render_batch_aa(W, H, views, samples=K, threshold=32)), got)


def test_calls_in_flight_and_a_stream_change(R, torch_cuda):
    """Two calls queued on one stream share the records' and the scratch buffer in stream order; a third on
    another stream waits for them on the device; one synchronisation at the end."""
    torch = torch_cuda
    W, H, K = 61, 37, 4
    _setup(R, "T")
    na, nb = ("P0", "P1", "P2", "P7"), ("P3", "P4")
    va, vb = [POSES[k] for k in na], [POSES[k] for k in nb]
    want_a = _loop(R, ("T", na), W, H, va, K, 32)
    want_b = _loop(R, ("T", nb), W, H, vb, K, 0)
    pa, pb = rm.pack_views(va), rm.pack_views(vb)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        R.set_stream(s1)
        out_a, mask_a, n_a = R.render_batch_aa(W, H, pa, samples=K, threshold=32, mask=True, refined=True)
        out_b, n_b = R.render_batch_aa(W, H, pb, samples=K, threshold=0, refined=True)
        R.set_stream(s2)
        out_c, mask_c = R.render_batch_aa(W, H, pa, samples=K, threshold=32, mask=True)
    finally:
        R.set_stream(None)
    torch.cuda.synchronize()
    assert _same(_np(out_a), want_a[0]) and _same(mask_a.cpu().numpy(), want_a[1])
    assert np.array_equal(_np(n_a).astype(np.int64), want_a[2])
    assert _same(_np(out_b), want_b[0]) and (_np(n_b) == W * H).all()
    assert _same(_np(out_c), want_a[0]) and _same(mask_c.cpu().numpy(), want_a[1])


# ------------------------------------------------- 5. arguments

@pytest.mark.parametrize("name", ["rm_refine_batch_rgba8", "rm_render_batch_aa_rgba8"])
def test_arguments(R, torch_cuda, name):
    torch = torch_cuda
    fn = getattr(rm.lib(), name)
    _setup(R, "T")
    out = torch.full((2, 8, 8), SENTINEL8, dtype=torch.int32, device="cuda")
    out[:, 0, 0] = 0  # (an edge for the refine alone to find)
    mask = torch.full((2, 8, 8), SENTINEL_MASK, dtype=torch.uint8, device="cuda")
    refined = torch.full((2,), SENTINEL8, dtype=torch.int32, device="cuda")
    before = out.clone()
    v = rm.pack_views([POSES["P0"], POSES["P1"]])
    p, m, c = out.data_ptr(), mask.data_ptr(), refined.data_ptr()

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(out, before) and bool((mask == SENTINEL_MASK).all()) and bool((refined == SENTINEL8).all())

    # n = 0: RM_OK, nothing launched, stats zeroed (views and the targets may be NULL then)
    st = _lib.RmAaStats(7, 1.0, 2.0, 3.0)
    assert _raw(fn, R, 8, 8, v, 0, 4, 32, p, m, c, ctypes.byref(st)) == 0
    assert (st.refined, st.base_ms, st.detect_ms, st.refine_ms) == (0, 0.0, 0.0, 0.0)
    assert _raw(fn, R, 8, 8, None, 0, 4, 32, None) == 0
    assert untouched()
    # NULL views, frames or params with n > 0
    assert _raw(fn, R, 8, 8, None, 2, 4, 32, p, m, c) == INVALID
    assert _raw(fn, R, 8, 8, v, 2, 4, 32, None, m, c) == INVALID
    assert fn(R._ctx, 8, 8, ctypes.c_void_p(v.ctypes.data), 2, None, ctypes.c_void_p(p), None, None, None) == INVALID
    # the size rule (before any pointer is used: these counts have no such arrays behind them)
    for W, H, n in [(8, 8, 65536), (8, 8, -1), (0, 8, 2), (8, 0, 2), (1 << 16, 1 << 15, 2), (8, 65535 * 8 + 1, 1),
                    (1 << 15, 1 << 15, 1), (1 << 30, 1, 1), (1 << 16, 1 << 15, 1)]:
        assert _raw(fn, R, W, H, v, n, 4, 32, p, m, c) == INVALID, (W, H, n)
    # samples and threshold
    for K in (0, 1, 3, 16, -4):
        assert _raw(fn, R, 8, 8, v, 2, K, 32, p, m, c) == INVALID, K
    for t in (-1, 256):
        assert _raw(fn, R, 8, 8, v, 2, 4, t, p, m, c) == INVALID, t
    # an offset that is not exactly (0, 0), in either view and component
    for row, col, bad in [(1, 7, 0.25), (0, 6, -0.5), (1, 6, float("nan")), (0, 7, 2.0 ** -30)]:
        w = v.copy()
        w[row, col] = bad
        assert _raw(fn, R, 8, 8, w, 2, 4, 32, p, m, c) == INVALID, bad
        assert "offset" in rm.lib().rm_last_error(R._ctx).decode()
    # frames, mask and refined live in the same place
    host_mask, host_n = np.zeros((2, 8, 8), np.uint8), np.zeros(2, np.uint32)
    assert _raw(fn, R, 8, 8, v, 2, 4, 32, p, host_mask.ctypes.data, c) == INVALID
    assert "mixed" in rm.lib().rm_last_error(R._ctx).decode()
    assert _raw(fn, R, 8, 8, v, 2, 4, 32, p, m, host_n.ctypes.data) == INVALID
    host = np.zeros((2, 8, 8), np.uint32)
    assert _raw(fn, R, 8, 8, v, 2, 4, 32, host.ctypes.data, m, None) == INVALID
    assert untouched()
    # ... and the same arrays are fine as they were (-0 is (0, 0) too)
    w = v.copy()
    w[0, 6] = -0.0
    assert _raw(fn, R, 8, 8, w, 2, 4, 0, p, m, c) == 0
    torch.cuda.synchronize()
    assert not torch.equal(out, before) and bool((mask == 1).all()) and bool((refined == 64).all())
    # the Python surface refuses a short target, a frame count that is not the views', views of another shape
    with pytest.raises(ValueError):
        R.render_batch_aa(8, 8, v, out=torch.empty((1, 8, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        R.refine_batch(torch.zeros((3, 8, 8), dtype=torch.int32, device="cuda"), v)
    with pytest.raises(ValueError):
        R.render_batch_aa(8, 8, np.zeros((2, 5), np.float32))


def test_scene_plugin_and_no_scene(torch_cuda):
    torch = torch_cuda
    r = rm.Renderer(0)
    try:
        out = torch.full((2, 8, 8), 0x00FFFFFF, dtype=torch.int32, device="cuda")
        out[:, 0, 0] = 0
        mask = torch.full((2, 8, 8), SENTINEL_MASK, dtype=torch.uint8, device="cuda")
        before = out.clone()
        v = rm.pack_views([POSES["P0"], POSES["P1"]])
        names = ("rm_refine_batch_rgba8", "rm_render_batch_aa_rgba8")
        for name in names:
            assert _raw(getattr(rm.lib(), name), r, 8, 8, v, 2, 4, 32, out.data_ptr(), mask.data_ptr()) == NO_SCENE
        r.load_scene(os.path.join(rm.SCENES_DIR, "metaballs.hip"))
        for name in names:
            assert _raw(getattr(rm.lib(), name), r, 8, 8, v, 2, 4, 32, out.data_ptr(), mask.data_ptr()) == SCENE
            assert "batch supersampling: built-in scenes only" in rm.lib().rm_last_error(r._ctx).decode()
        with pytest.raises(rm.RmError):
            r.render_batch_aa(8, 8, v)
        torch.cuda.synchronize()
        assert torch.equal(out, before) and bool((mask == SENTINEL_MASK).all())
    finally:
        r.close()


# ------------------------------------------------- 6. the app

def test_headless_app_writes_the_antialiased_views(R, torch_cuda, tmp_path):
    """apps/raymarch_headless --views F --aa 4:32 (rm::Shader::renderBatchAA): three lines, three PPMs, the frames
    render_batch_aa returns, and the JSON line's "aa" and "refined"."""
    W, H = 96, 54
    exe = os.path.join(ROOT, "apps", "raymarch_headless")
    views = [POSES["P0"], POSES["P1"], POSES["P2"]]
    lines = ["# px py pz mx my t"]
    for row in rm.pack_views(views):
        lines.append(" ".join(repr(float(x)) for x in row[:6]))  # (repr of a float32's double: reads back exactly)
    (tmp_path / "views.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, "--scene", "template.frag", "--w", str(W), "--h", str(H), "--steps", str(STEPS),
                          "--views", str(tmp_path / "views.txt"), "--aa", "4:32", "--ppm", str(tmp_path / "v"),
                          "--stats"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    info = json.loads(run.stdout.strip().splitlines()[-1])
    _setup(R, "T")
    out, st = R.render_batch_aa(W, H, views, samples=4, threshold=32, stats=True)
    want = _np(out)
    assert info["views"] == 3 and info["aa"] == 4 and info["kernel_ms"] > 0.0
    assert 0 < info["refined"] < 3 * W * H and info["refined"] == st["refined"]
    for k in range(3):
        data = (tmp_path / f"v.{k:04d}.ppm").read_bytes()
        img = np.frombuffer(data[data.index(b"255\n") + 4:], np.uint8).reshape(H, W, 3)
        rgb = np.stack([(want[k] >> s) & 255 for s in (0, 8, 16)], -1).astype(np.uint8)
        assert np.array_equal(img, rgb), k
    # the antialiased frames are not the plain batch's
    assert not _same(want, _np(R.render_batch(W, H, views)))
    # an offset in the file is refused by the call
    (tmp_path / "off.txt").write_text(lines[1] + " 0.25 0.0\n")
    bad = subprocess.run([exe, "--scene", "template.frag", "--w", str(W), "--h", str(H), "--views",
                          str(tmp_path / "off.txt"), "--aa", "4"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "offset" in bad.stderr
    # --views --aa on more than one GPU stays refused, as --aa refuses it
    multi = subprocess.run([exe, "--views", str(tmp_path / "views.txt"), "--aa", "4", "--gpus", "2"],
                           capture_output=True, text=True, timeout=120)
    assert multi.returncode == 2
