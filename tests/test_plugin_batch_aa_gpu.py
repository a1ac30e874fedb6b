"""Adaptive supersampling of a scene plugin's view batch on the GPU (include/rm.h
rm_render_batch_aa_ex_rgba8, rm_refine_batch_ex_rgba8, rm_batch_aa_prepare;
DESIGN.md 2.32): every word of every view's frame, mask and count against this
build's own loop of set_pose + set_uniform + render_aa_ex of the same plugin --
no tolerance; the single-frame call is held to the accumulate blend by
tests/test_plugin_aa_gpu.py.  Per-view floats, vectors, array elements, ints and
bools, a scene without uniforms, crafted frames with views that queue nothing,
the column rule of the refine's grid, more views than a byte counts, one view,
host pointers, calls in flight, a built-in scene, the argument checks in the
documented order, a reload, the prepare call, and the headless app.  Sentinels
sit after the frames, the mask and the counts."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import POSES, _lib, batch_aa_ex, cameras
from tests import aa_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, SCENE, NO_SCENE = 0, 1, 3, 4
STEPS = 128
SENTINEL8 = 0x5A5A5A5A  # (alpha 0x5A: no pixel the pass writes, whose alpha is 255)
SENTINEL_MASK = 0xA5    # (a mask byte is 0 or 1)
WHITE = 0xFFFFFFFF
GREY = 0xFF808080
KNOBS = os.path.join(rm.SCENES_DIR, "output_shader_knobs.hip")
BALLS = os.path.join(rm.SCENES_DIR, "metaballs.hip")
PLAIN = os.path.join(rm.SCENES_DIR, "output_shader.hip")
EVAL_ONLY = ("#define RM_PLUGIN_EVAL_ONLY 1\nSdResult sceneSDF(vec3 p)\n{\n    return SdResult(sphere(vec4(0.0, 3.0, "
             "0.0, 1.0), p), Material(vec3(0.5), vec3(0.0), 1.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0)));\n}\n")
KNOB_DEFAULTS = dict(u_ball=(3.0, 2.0, 3.0, 1.0), u_box=(-5.0, 4.0, 5.0, 1.0), u_sponge_y=3.0, u_spin=2.0)
COLUMNS = "RM_PLUGIN_BATCH_AA_COLUMNS"


def _load(r, scene):
    r.load_scene(scene)
    r.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0)
    r.set_uniform("u_seed1", 0.5, 0.5)
    r.set_uniform("u_sample_part", 1.0)


def _new(scene):
    r = rm.Renderer(0)
    _load(r, scene)
    return r


# each scene is loaded (and each of its code objects compiled) once per module
@pytest.fixture(scope="module")
def K(torch_cuda):
    r = _new(KNOBS)
    yield r
    r.close()


@pytest.fixture(scope="module")
def M(torch_cuda):
    r = _new(BALLS)
    yield r
    r.close()


@pytest.fixture(scope="module")
def P(torch_cuda):
    r = _new(PLAIN)
    yield r
    r.close()


def _np(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _timed(pose, t):
    return dict(pos=pose["pos"], mouse=pose["mouse"], time=t)


def _knob_defaults(r):
    for name, v in KNOB_DEFAULTS.items():
        r.set_uniform(name, *(v if isinstance(v, tuple) else (v,)))


def _loop(r, W, H, views, samples, threshold, setters=None):
    """What a caller does today: set_pose + set_uniform* + render_aa_ex per view -> frames [n, H, W] uint32, masks
    [n, H, W] uint8, counts [n] (each call's rm_aa_stats.refined).  setters: one callable per view."""
    frames, masks, counts = [], [], []
    for k, v in enumerate(views):
        if setters:
            setters[k](r)
        r.set_pose(v["pos"], v["mouse"], v["time"])
        out, mask, st = r.render_aa_ex(W, H, samples=samples, threshold=threshold, mask=True, stats=True)
        frames.append(_np(out))
        masks.append(mask.cpu().numpy())
        counts.append(st["refined"])
    return np.stack(frames), np.stack(masks), np.array(counts, np.int64)


def _batch(torch, r, W, H, views, uniforms, samples, threshold, fn=None):
    """The batch into targets one frame (one word) longer than it, full of sentinels -> frames, masks, counts of the
    n views, after checking the sentinels; and the call's stats."""
    n = len(views)
    out = torch.full((n + 1, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
    mask = torch.full((n + 1, H, W), SENTINEL_MASK, dtype=torch.uint8, device="cuda")
    refined = torch.full((n + 1,), SENTINEL8, dtype=torch.int32, device="cuda")
    arr, k, _keep = r._view_uniforms("test", uniforms, n)
    st = _lib.RmAaStats()
    p = _lib.RmAaParams(samples, threshold)
    v = rm.pack_views(views)
    fn = fn or rm.lib().rm_render_batch_aa_ex_rgba8
    assert fn(r._ctx, W, H, ctypes.c_void_p(v.ctypes.data), n, arr, k, ctypes.byref(p), ctypes.c_void_p(out.data_ptr()),
              ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(refined.data_ptr()), ctypes.byref(st)) == OK, \
        rm.lib().rm_last_error(r._ctx).decode()
    got, got_mask, got_n = _np(out), mask.cpu().numpy(), _np(refined)
    assert (got[n] == SENTINEL8).all() and (got_mask[n] == SENTINEL_MASK).all() and got_n[n] == SENTINEL8
    return got[:n], got_mask[:n], got_n[:n].astype(np.int64), st


def _report(what, got, want):
    d = [int((np.ascontiguousarray(g) != np.ascontiguousarray(w)).sum()) for g, w in zip(got, want)]
    print(f"{what}: {d[0]} of {want[0].size} frame words, {d[1]} mask bytes, {d[2]} counts differ")


# ------------------------------------------------- 1. u_time, a vec4 and a float per view

_KNOB_LOOP = {}  # (samples, threshold) -> the loop's frames, masks, counts: computed once, left unchanged


def _knob_case():
    views = cameras.turntable(5, 6.0, 4.5)
    for k, v in enumerate(views):
        v["time"] = float(np.float32(1.5 + 2.25 * k))  # u_time advances per view
    # (the ball near the sponge, in sight of every view of the turntable)
    ball = np.array([[0.0, 5.5, 0.0, 0.75], [1.0, 5.0, 1.0, 1.0], [-1.5, 4.5, 0.5, 1.25], [0.5, 6.0, -1.0, 0.5],
                     [2.0, 5.0, 0.0, 1.5]], np.float32)
    spin = np.array([2.0, -9.0, 0.0, 33.5, 7.0], np.float32)
    setters = [lambda r, k=k: (r.set_uniform("u_ball", *map(float, ball[k])), r.set_uniform("u_spin", float(spin[k])))
               for k in range(5)]
    return views, dict(u_ball=ball, u_spin=spin), setters


@pytest.mark.parametrize("threshold", [0, 32])
@pytest.mark.parametrize("samples", [2, 4, 8])
def test_every_view_is_the_single_call(K, torch_cuda, samples, threshold):
    W, H = 41, 27  # (ragged in both directions)
    _knob_defaults(K)
    K.set_uniform("u_sponge_y", 2.5)  # (unlisted, not the default: the batch must read the context's block)
    views, uniforms, setters = _knob_case()
    n = len(views)
    K.set_pose(POSES["P5"]["pos"], POSES["P5"]["mouse"], POSES["P5"]["time"])
    before, own = K.uniforms(), _np(K.render_rgba8(W, H))
    got = _batch(torch_cuda, K, W, H, views, uniforms, samples, threshold)
    # the context's uniform values and pose are what they were: the getters, and a single render's bytes
    assert repr(K.uniforms()) == repr(before)
    assert _same(_np(K.render_rgba8(W, H)), own)
    if (samples, threshold) not in _KNOB_LOOP:
        res = _loop(K, W, H, views, samples, threshold, setters)
        for a in res:
            a.setflags(write=False)
        _KNOB_LOOP[(samples, threshold)] = res
    want = _KNOB_LOOP[(samples, threshold)]
    _report(f"knobs {W}x{H} K={samples} threshold {threshold}", got, want)
    print(f"  the loop refines {want[2].tolist()} of {W * H}")
    for k in range(n):
        assert _same(got[0][k], want[0][k]), f"view {k}"
        assert _same(got[1][k], want[1][k]), f"mask of view {k}"
    assert np.array_equal(got[2], want[2])
    st = got[3]
    assert st.refined == int(want[2].sum()) and st.base_ms > 0.0 and st.detect_ms > 0.0 and st.refine_ms > 0.0
    if threshold == 0:
        assert (want[2] == W * H).all()
    else:  # some but not all pixels, and a last group that is partial
        assert any(0 < c < W * H and c % (64 // samples) != 0 for c in want[2]), want[2]
    # the views differ from each other (a batch of one record repeated would pass otherwise)
    assert len({want[0][k].tobytes() for k in range(n)}) == n
    # the Python surface: without the optional outputs and with them, and refine_batch_ex(render_batch_ex())
    plain = batch_aa_ex.render_batch_aa_ex(K, W, H, views, uniforms, samples=samples, threshold=threshold)
    assert tuple(plain.shape) == (n, H, W) and _same(_np(plain), want[0])
    o2, m2, r2, s2 = batch_aa_ex.render_batch_aa_ex(K, W, H, views, uniforms, samples=samples, threshold=threshold,
                                                    mask=True, refined=True, stats=True)
    assert _same(_np(o2), want[0]) and _same(m2.cpu().numpy(), want[1])
    assert np.array_equal(_np(r2).astype(np.int64), want[2]) and s2["refined"] == int(want[2].sum())
    two = K.render_batch_ex(W, H, views, uniforms=uniforms)
    assert batch_aa_ex.refine_batch_ex(K, two, views, uniforms, samples=samples, threshold=threshold) is two
    assert _same(_np(two), want[0])
    _knob_defaults(K)


# ------------------------------------------------- 2. array elements, an int and a bool per view; no uniforms at all

def test_array_int_and_bool_per_view(M, torch_cuda):
    W, H = 33, 20
    L = rm.lib()
    pose = POSES["P0"]
    views = [_timed(pose, 0.0), _timed(POSES["P1"], 2.0), _timed(POSES["P2"], 5.0)]
    rest = np.array([[k - 3.0, 2.0 + 0.25 * k, 0.5 * k, 0.8] for k in range(8)], np.float32)
    M.set_uniform_array("u_balls", rest)     # all eight from the context ...
    M.set_uniform("u_tint", 0.3, 0.05, 0.2)  # ... and the tint (unlisted)
    balls = np.array([[[0.0, 2.0, 0.0, 1.0], [1.5, 2.5, 0.5, 0.75]], [[-1.0, 3.0, 1.0, 1.25], [2.0, 1.5, -0.5, 1.0]],
                      [[0.5, 2.0, -1.0, 0.5], [0.0, 3.5, 0.0, 1.5]]], np.float32)  # [n, 2, 4]: elements 0 and 1 of 8
    count = np.array([2, 8, 5], np.int32)
    floor = np.array([1, 0, 7], np.int32)  # (non-zero: true)
    uniforms = dict(u_balls=balls, u_count=count, u_floor=floor)
    before = M.uniforms()
    got = _batch(torch_cuda, M, W, H, views, uniforms, 4, 32)
    assert repr(M.uniforms()) == repr(before)

    def setter(k):
        def set_(r):
            flat = np.ascontiguousarray(balls[k])
            assert L.rm_set_uniformfv(r._ctx, b"u_balls", 4, ctypes.c_void_p(flat.ctypes.data), 2) == OK
            assert L.rm_set_uniform1i(r._ctx, b"u_count", int(count[k])) == OK
            assert L.rm_set_uniform1i(r._ctx, b"u_floor", int(floor[k])) == OK
        return set_
    want = _loop(M, W, H, views, 4, 32, [setter(k) for k in range(3)])
    _report(f"metaballs {W}x{H}", got, want)
    print(f"  the loop refines {want[2].tolist()} of {W * H}")
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert want[2].sum() > 0 and len({want[0][k].tobytes() for k in range(3)}) == 3


def test_scene_without_uniforms(P, torch_cuda):
    W, H = 40, 24
    views = [POSES["P1"], POSES["P2"]]
    got = _batch(torch_cuda, P, W, H, views, None, 4, 32)
    want = _loop(P, W, H, views, 4, 32)
    _report(f"output_shader {W}x{H}", got, want)
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert want[2].sum() > 0 and not _same(want[0][0], want[0][1])
    # it declares nothing: any list is refused
    with pytest.raises(rm.RmError) as e:
        batch_aa_ex.render_batch_aa_ex(P, W, H, views, dict(u_ball=np.zeros((2, 4), np.float32)))
    assert e.value.status == INVALID


# ------------------------------------------------- 3. crafted frames

def _crafted(W, H):
    """all zero | a lone white pixel at (0, 0) | one at an interior tile corner | constant grey | noise | all zero"""
    f = np.zeros((6, H, W), np.uint32)
    f[1, 0, 0] = WHITE
    f[2, min(8, H - 1), min(8, W - 1)] = WHITE
    f[3] = GREY
    f[4] = np.random.default_rng(W * 100 + H).integers(0, 2 ** 32, (H, W), dtype=np.uint32)
    return f


@pytest.mark.parametrize("W,H", [(61, 37), (5, 3), (1, 1)])
def test_crafted_frames_through_refine_batch_ex(K, torch_cuda, W, H):
    torch = torch_cuda
    samples = 4
    _knob_defaults(K)
    views = [_timed(POSES[k], 3.0 + i) for i, k in enumerate(("P0", "P1", "P2", "P3", "P4", "P5"))]
    spin = np.array([2.0, -9.0, 0.0, 33.5, 7.0, 1.0], np.float32)
    uniforms = dict(u_spin=spin)
    # every pixel of every view supersampled: the single calls' threshold-0 frames
    full = _loop(K, W, H, views, samples, 0, [lambda r, k=k: r.set_uniform("u_spin", float(spin[k])) for k in range(6)])[0]
    frames = _crafted(W, H)
    for threshold in (1, 255):
        want_mask = np.stack([aa_ref.edge_mask(f, threshold) for f in frames])
        dev = torch.full((7, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
        dev[:6] = torch.from_numpy(frames.view(np.int32).copy()).cuda()
        res, mask, refined, st = batch_aa_ex.refine_batch_ex(K, dev[:6], views, uniforms, samples=samples,
                                                             threshold=threshold, mask=True, refined=True, stats=True)
        got, m, counts = _np(dev), mask.cpu().numpy(), _np(refined)
        assert (got[6] == SENTINEL8).all()
        got = got[:6]
        assert m.dtype == np.uint8 and _same(m, want_mask)
        assert np.array_equal(counts.astype(np.int64), want_mask.reshape(6, -1).sum(1))
        assert st["refined"] == int(want_mask.sum()) and st["base_ms"] == 0.0
        # the first, the last and a middle view queue nothing
        assert counts[0] == 0 and counts[5] == 0 and counts[3] == 0
        if (W, H) == (61, 37):
            assert counts[1] == 4 and counts[2] == 9  # lone edge pixels and their neighbours
            if threshold == 1:
                assert counts[4] == W * H
        if (W, H) == (1, 1):
            assert not counts.any()  # (a 1x1 frame has no edge pixel: its neighbourhood is itself)
        assert np.array_equal(got[m == 0], frames[m == 0])  # every other pixel keeps its bytes
        assert np.array_equal(got[m == 1], full[m == 1])    # masked pixels: the views' supersampled colour
        # host pointers: staged, the same bytes
        host = frames.copy()
        _, hm, hr = batch_aa_ex.refine_batch_ex(K, host, views, uniforms, samples=samples, threshold=threshold,
                                                mask=True, refined=True)
        assert _same(host, got) and _same(hm, m) and hr.dtype == np.uint32 and _same(hr, counts)


# ------------------------------------------------- 4. the column rule

def test_any_number_of_columns_gives_the_same_bytes(K, torch_cuda, monkeypatch):
    W, H, samples = 61, 37, 4
    _knob_defaults(K)
    views, uniforms, _ = _knob_case()
    monkeypatch.delenv(COLUMNS, raising=False)
    want = _batch(torch_cuda, K, W, H, views, uniforms, samples, 0)
    assert (want[2] == W * H).all()
    groups = -(-W * H // (64 // samples))  # 142 groups per view
    # one column: every wave strides over all of its view's groups; more columns than groups: workgroups leave empty
    for columns in ("1", "3", str(groups), str(groups + 59), "100000"):
        monkeypatch.setenv(COLUMNS, columns)
        got = _batch(torch_cuda, K, W, H, views, uniforms, samples, 0)
        assert _same(got[0], want[0]) and _same(got[1], want[1]) and np.array_equal(got[2], want[2]), columns
    # at the usual threshold too, where the views' group counts differ
    monkeypatch.delenv(COLUMNS)
    want32 = _batch(torch_cuda, K, W, H, views, uniforms, samples, 32)
    assert len(set(want32[2].tolist())) > 1
    for columns in ("1", "200"):
        monkeypatch.setenv(COLUMNS, columns)
        got = _batch(torch_cuda, K, W, H, views, uniforms, samples, 32)
        assert _same(got[0], want32[0]) and np.array_equal(got[2], want32[2]), columns


# ------------------------------------------------- 5. more views than a byte counts

def test_300_one_tile_views(K, torch_cuda):
    n, W, H, samples = 300, 8, 8, 8
    _knob_defaults(K)
    # the camera of P0 looks down -z from (2, 3, 3) and walks along x; the ball in front of it pulses with the view
    views = [dict(pos=(2.0 + 0.004 * k, 3.0, 3.0), mouse=(0.0, 0.0), time=0.37 * k) for k in range(n)]
    ball = np.array([[2.0, 3.0, 0.0, 0.75 + 0.75 * (k % 2) + 0.001 * k] for k in range(n)], np.float32)
    got = _batch(torch_cuda, K, W, H, views, dict(u_ball=ball), samples, 0)
    assert (got[2] == 64).all()
    picks = (0, 255, 256, 299)  # (blockIdx.z past 255)
    want = _loop(K, W, H, [views[k] for k in picks], samples, 0,
                 [lambda r, k=k: r.set_uniform("u_ball", *map(float, ball[k])) for k in picks])
    for i, k in enumerate(picks):
        assert _same(got[0][k], want[0][i]), f"view {k}"
    assert len({want[0][i].tobytes() for i in range(4)}) == 4
    _knob_defaults(K)


# ------------------------------------------------- 6. one view, host pointers, no outputs, calls in flight

def test_one_view_host_pointers_and_calls_in_flight(K, torch_cuda):
    torch = torch_cuda
    W, H = 41, 27
    _knob_defaults(K)
    va = [_timed(POSES["P0"], 1.0), _timed(POSES["P1"], 2.0), _timed(POSES["P2"], 3.0)]
    vb = [_timed(POSES["P3"], 4.0), _timed(POSES["P4"], 5.0)]
    sa, sb = np.array([1.0, 20.0, -3.0], np.float32), np.array([8.0, -15.0], np.float32)
    want_a = _loop(K, W, H, va, 4, 32, [lambda r, k=k: r.set_uniform("u_spin", float(sa[k])) for k in range(3)])
    want_b = _loop(K, W, H, vb, 4, 32, [lambda r, k=k: r.set_uniform("u_spin", float(sb[k])) for k in range(2)])
    # n = 1 is render_aa_ex
    one = _batch(torch, K, W, H, va[1:2], dict(u_spin=sa[1:2]), 4, 32)
    assert _same(one[0][0], want_a[0][1]) and _same(one[1][0], want_a[1][1]) and one[2][0] == want_a[2][1]
    # host pointers, with sentinels behind each
    host = np.full((4, H, W), SENTINEL8, np.uint32)
    res, hm, hr, st = batch_aa_ex.render_batch_aa_ex(K, W, H, va, dict(u_spin=sa), out=host[:3], mask=True, refined=True,
                                                     stats=True)
    assert _same(host[:3], want_a[0]) and (host[3] == SENTINEL8).all()
    assert _same(hm, want_a[1]) and np.array_equal(hr.astype(np.int64), want_a[2]) and st["refined"] == want_a[2].sum()
    # no mask and no counts; two calls in flight and one synchronise
    out_a = torch.full((4, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
    out_b = torch.full((3, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    batch_aa_ex.render_batch_aa_ex(K, W, H, va, dict(u_spin=sa), out=out_a[:3])
    batch_aa_ex.render_batch_aa_ex(K, W, H, vb, dict(u_spin=sb), out=out_b[:2])
    K.synchronize()
    assert _same(_np(out_a)[:3], want_a[0]) and _same(_np(out_b)[:2], want_b[0])
    assert (_np(out_a)[3] == SENTINEL8).all() and (_np(out_b)[2] == SENTINEL8).all()
    _knob_defaults(K)


# ------------------------------------------------- 7. a built-in scene

def test_built_in_scene(torch_cuda):
    torch = torch_cuda
    W, H = 61, 37
    r = rm.Renderer(0)
    try:
        _load(r, rm.SCENE_FILES["T"])
        batch_aa_ex.batch_aa_prepare(r)  # (nothing to do)
        views = [POSES["P0"], POSES["P1"], POSES["P2"]]
        want = r.render_batch_aa(W, H, views, samples=4, threshold=32, mask=True, refined=True, stats=True)
        got = batch_aa_ex.render_batch_aa_ex(r, W, H, views, samples=4, threshold=32, mask=True, refined=True,
                                             stats=True)
        assert _same(_np(got[0]), _np(want[0])) and _same(got[1].cpu().numpy(), want[1].cpu().numpy())
        assert _same(_np(got[2]), _np(want[2])) and got[3]["refined"] == want[3]["refined"] > 0
        two = r.render_batch(W, H, views)
        batch_aa_ex.refine_batch_ex(r, two, views, samples=4, threshold=32)
        assert _same(_np(two), _np(want[0]))
        out = torch.full((3, H, W), SENTINEL8, dtype=torch.int32, device="cuda")
        with pytest.raises(rm.RmError) as e:
            batch_aa_ex.render_batch_aa_ex(r, W, H, views, dict(u_ball=np.zeros((3, 4), np.float32)), out=out)
        assert e.value.status == INVALID and "built-in" in str(e.value)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL8).all())
    finally:
        r.close()


# ------------------------------------------------- 8. arguments, in the documented order

def _entry(name, components, count, values):
    return _lib.RmViewUniform(name, components, count, ctypes.c_void_p(values.ctypes.data) if values is not None else None)


def _call(fn, r, W, H, views, n, entries, n_uniforms, params, frames, mask=None, refined=None, stats=None):
    vp = ctypes.c_void_p(views.ctypes.data) if views is not None else None
    arr = (_lib.RmViewUniform * max(1, len(entries)))(*entries) if entries is not None else None
    return fn(r._ctx, W, H, vp, n, ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, n_uniforms,
              ctypes.byref(params) if params is not None else None, ctypes.c_void_p(frames) if frames else None,
              ctypes.c_void_p(mask) if mask else None, ctypes.c_void_p(refined) if refined else None, stats)


@pytest.mark.parametrize("name", ["rm_refine_batch_ex_rgba8", "rm_render_batch_aa_ex_rgba8"])
def test_arguments(K, torch_cuda, name, tmp_path):
    torch = torch_cuda
    fn = getattr(rm.lib(), name)
    err = lambda r: rm.lib().rm_last_error(r._ctx).decode()  # noqa: E731
    _knob_defaults(K)
    out = torch.full((2, 8, 8), SENTINEL8, dtype=torch.int32, device="cuda")
    mask = torch.full((2, 8, 8), SENTINEL_MASK, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), SENTINEL8, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((out == SENTINEL8).all()) and bool((mask == SENTINEL_MASK).all()) and bool((cnt == SENTINEL8).all())
    v = rm.pack_views([POSES["P0"], POSES["P1"]])
    p, m, c = out.data_ptr(), mask.data_ptr(), cnt.data_ptr()
    good_p = _lib.RmAaParams(4, 32)
    f2, f8 = np.array([1.0, 2.0], np.float32), np.zeros((2, 4), np.float32)
    good = [_entry(b"u_spin", 1, 1, f2), _entry(b"u_ball", 4, 1, f8)]
    bad_list = [_entry(b"u_nope", 1, 1, f2)]
    w = v.copy()
    w[1, 7] = 0.25  # a view with an offset
    # each fault is reported although every later one is present too
    # 1. the size rule (before the NULL params, ..., the bad list)
    for W, H, n in ((8, 8, 65536), (8, 8, -1), (0, 8, 2), (1 << 16, 1 << 15, 2), (1 << 15, 1 << 15, 1)):
        assert _call(fn, K, W, H, None, n, bad_list, -1, None, None) == INVALID, (W, H, n)
        assert "W, H > 0" in err(K)
    # 2. NULL params, views or frames
    assert _call(fn, K, 8, 8, w, 2, bad_list, -1, None, p, m, c) == INVALID and "null" in err(K)
    assert _call(fn, K, 8, 8, None, 2, bad_list, -1, _lib.RmAaParams(3, 32), p, m, c) == INVALID and "null" in err(K)
    assert _call(fn, K, 8, 8, w, 2, bad_list, -1, _lib.RmAaParams(3, 32), None, m, c) == INVALID and "null" in err(K)
    # 3. samples and threshold (before the offset)
    for s, t in ((3, 32), (1, 32), (16, 32), (4, -1), (4, 256)):
        assert _call(fn, K, 8, 8, w, 2, bad_list, -1, _lib.RmAaParams(s, t), p, m, c) == INVALID, (s, t)
        assert "samples" in err(K)
    # 4. a view's offset (before the list's length)
    assert _call(fn, K, 8, 8, w, 2, bad_list, -1, good_p, p, m, c) == INVALID and "offset" in err(K)
    # 5. the list's length and pointer (before the scene is looked at: a context without one says the same)
    empty = rm.Renderer(0)
    try:
        for r in (K, empty):
            assert _call(fn, r, 8, 8, v, 2, good, -1, good_p, p, m, c) == INVALID and "n_uniforms" in err(r)
            assert _call(fn, r, 8, 8, v, 2, None, 2, good_p, p, m, c) == INVALID and "n_uniforms" in err(r)
        # 6. no scene (before the list's entries)
        assert _call(fn, empty, 8, 8, v, 2, bad_list, 1, good_p, p, m, c) == NO_SCENE
        assert rm.lib().rm_batch_aa_prepare(empty._ctx) == NO_SCENE
        # 7. an eval-only plugin (before the list's entries, n = 0 and the mixed pointers)
        ball = tmp_path / "ball.hip"
        ball.write_text(EVAL_ONLY)
        empty.load_scene(str(ball))
        host_mask = np.full((2, 8, 8), SENTINEL_MASK, np.uint8)
        assert _call(fn, empty, 8, 8, v, 2, bad_list, 1, good_p, p, host_mask.ctypes.data, c) == SCENE
        assert "RM_PLUGIN_EVAL_ONLY" in err(empty)
        assert _call(fn, empty, 8, 8, v, 0, None, 0, good_p, None) == SCENE
        assert rm.lib().rm_batch_aa_prepare(empty._ctx) == SCENE
        # 8. a built-in scene with a list (before n = 0)
        empty.load_scene(rm.SCENE_FILES["T"])
        assert _call(fn, empty, 8, 8, v, 0, good, 2, good_p, p, m, c) == INVALID and "built-in" in err(empty)
        assert rm.lib().rm_batch_aa_prepare(empty._ctx) == OK
    finally:
        empty.close()
    # 9. the list's faults, rm_render_batch_ex's messages (before n = 0 and the mixed pointers)
    cases = [
        ([_entry(None, 1, 1, f2)], "null name"),
        ([_entry(b"u_spin", 1, 1, None)], "null values"),
        ([_entry(b"u_nope", 1, 1, f2)], "declares no uniform \"u_nope\""),
        ([_entry(b"u_time", 1, 1, f2)], "the pass's own"),
        ([_entry(b"u_spin", 1, 1, f2), _entry(b"u_spin", 1, 1, f2)], "listed twice"),
        ([_entry(b"u_ball", 3, 1, f8)], "is declared vec4, got 3 components"),
        ([_entry(b"u_spin", 1, 0, f2)], "count 0 < 1"),
        ([_entry(b"u_ball", 4, 2, f8)], "not an array"),
    ]
    host_mask = np.full((2, 8, 8), SENTINEL_MASK, np.uint8)
    for entries, msg in cases:
        assert _call(fn, K, 8, 8, v, 2, entries, len(entries), good_p, p, host_mask.ctypes.data, c) == INVALID, msg
        assert msg in err(K), (msg, err(K))
    assert _call(fn, K, 8, 8, v, 0, bad_list, 1, good_p, p, m, c) == INVALID and "u_nope" in err(K)
    # 10. n = 0: RM_OK, stats zeroed, nothing launched (views, frames and values may be NULL then)
    st = _lib.RmAaStats()
    st.refined, st.base_ms = 99, 1.0
    assert _call(fn, K, 8, 8, None, 0, [_entry(b"u_spin", 1, 1, None)], 1, good_p, None, None, None,
                 ctypes.byref(st)) == OK
    assert st.refined == 0 and st.base_ms == 0.0 and st.detect_ms == 0.0 and st.refine_ms == 0.0
    assert _call(fn, K, 8, 8, None, 0, None, 0, good_p, p, host_mask.ctypes.data, c) == OK  # (before the pointers' kinds)
    # 11. frames, mask and refined live in the same place
    host_n, host = np.full(2, SENTINEL8, np.uint32), np.full((2, 8, 8), SENTINEL8, np.uint32)
    st.refined = 77
    assert _call(fn, K, 8, 8, v, 2, good, 2, good_p, p, host_mask.ctypes.data, c, ctypes.byref(st)) == INVALID
    assert "mixed" in err(K) and st.refined == 77
    assert _call(fn, K, 8, 8, v, 2, good, 2, good_p, p, m, host_n.ctypes.data) == INVALID and "mixed" in err(K)
    assert _call(fn, K, 8, 8, v, 2, good, 2, good_p, host.ctypes.data, m, None) == INVALID and "mixed" in err(K)
    assert untouched()
    assert (host_mask == SENTINEL_MASK).all() and (host_n == SENTINEL8).all() and (host == SENTINEL8).all()
    # ... and the same arrays are fine as they were
    assert _call(fn, K, 8, 8, v, 2, good, 2, good_p, p, m, c) == OK
    assert not untouched()
    # the Python surface refuses values for another number of views, and frames for another
    with pytest.raises(ValueError):
        batch_aa_ex.render_batch_aa_ex(K, 8, 8, v, dict(u_spin=np.zeros(3, np.float32)))
    with pytest.raises(ValueError):
        batch_aa_ex.refine_batch_ex(K, out, v[:1])
    # the calls without _ex keep refusing the plugin, with their messages
    for plain, msg in ((lambda: K.render_batch_aa(8, 8, v), "batch supersampling: built-in scenes only"),
                       (lambda: K.refine_batch(out, v), "batch supersampling: built-in scenes only"),
                       (lambda: K.render_batch(8, 8, v), "view batches: built-in scenes only"),
                       (lambda: K.render_aa(8, 8), "adaptive supersampling: built-in scenes only")):
        with pytest.raises(rm.RmError) as e:
            plain()
        assert e.value.status == SCENE and msg in str(e.value)


def test_a_form_that_fails_to_compile_leaves_the_frames(torch_cuda, tmp_path):
    """12. RM_ERR_SCENE with the log: a scene whose frame form compiles and whose batch-AA form does not"""
    torch = torch_cuda
    src = open(PLAIN).read() + "\n#ifdef RM_PLUGIN_BATCH_AA\n#error no batch-AA form of this scene\n#endif\n"
    path = tmp_path / "no_batch_aa.hip"
    path.write_text(src)
    r = rm.Renderer(0)
    try:
        _load(r, str(path))
        views = [POSES["P0"], POSES["P1"]]
        want = _np(r.render_batch_ex(8, 8, views))  # (the batch form is fine)
        out = torch.full((2, 8, 8), SENTINEL8, dtype=torch.int32, device="cuda")
        for call in (lambda: batch_aa_ex.render_batch_aa_ex(r, 8, 8, views, out=out),
                     lambda: batch_aa_ex.refine_batch_ex(r, out, views), lambda: batch_aa_ex.batch_aa_prepare(r)):
            with pytest.raises(rm.RmError) as e:
                call()
            assert e.value.status == SCENE and "no batch-AA form of this scene" in str(e.value)
            assert "batch-AA form failed to compile" in str(e.value)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL8).all())
        assert _same(_np(r.render_batch_ex(8, 8, views)), want)
    finally:
        r.close()


def test_prepare_reload_and_the_other_calls_afterwards(torch_cuda):
    W, H = 33, 20
    views = [_timed(POSES["P0"], 1.0), _timed(POSES["P2"], 6.0)]
    r = rm.Renderer(0)
    try:
        _load(r, KNOBS)
        batch_aa_ex.batch_aa_prepare(r)  # before the first call
        batch_aa_ex.batch_aa_prepare(r)  # (loaded already)
        r.set_uniform("u_spin", 11.0)
        got = _np(batch_aa_ex.render_batch_aa_ex(r, W, H, views))
        want = _loop(r, W, H, views, 4, 32)[0]
        assert _same(got, want)
        # after a batch-AA call, the plain batch and the single AA call of the same scene are what they were
        plain = _np(r.render_batch_ex(W, H, views))
        singles = []
        for v in views:
            r.set_pose(v["pos"], v["mouse"], v["time"])
            singles.append(_np(r.render_rgba8(W, H)))
        assert _same(plain, np.stack(singles)) and not _same(plain, want)
        # another scene after a batch: the call renders the new scene
        _load(r, BALLS)
        r.set_uniform("u_count", 3)
        r.set_uniform_array("u_balls", np.array([[0.0, 2.0, 0.0, 1.0], [1.5, 2.5, 0.5, 0.75], [-1, 3, 1, 1]], np.float32))
        got_m = _np(batch_aa_ex.render_batch_aa_ex(r, W, H, views, dict(u_floor=np.array([1, 0], np.int32))))
        want_m = _loop(r, W, H, views, 4, 32, [lambda q: q.set_uniform("u_floor", 1), lambda q: q.set_uniform("u_floor", 0)])[0]
        assert _same(got_m, want_m) and not _same(got_m, got)
        # and back: a reload of the first file resets the unlisted uniforms to their defaults
        _load(r, KNOBS)
        got_d = _np(batch_aa_ex.render_batch_aa_ex(r, W, H, views))
        assert _same(got_d, _loop(r, W, H, views, 4, 32)[0]) and not _same(got_d, got)
        r.set_uniform("u_spin", 11.0)
        assert _same(_np(batch_aa_ex.render_batch_aa_ex(r, W, H, views)), got)
    finally:
        r.close()


# ------------------------------------------------- 9. the app

def test_headless_app_antialiases_a_plugin_s_views(K, torch_cuda, tmp_path):
    """apps/raymarch_headless --scene <a .hip scene> --views F --aa 4:32 (rm::Shader::renderBatchAAEx)"""
    W, H = 41, 27
    exe = os.path.join(ROOT, "apps", "raymarch_headless")
    views = [_timed(POSES["P0"], 1.5), _timed(POSES["P1"], 9.0), _timed(POSES["P2"], 20.0)]
    packed = rm.pack_views(views)
    lines = ["# px py pz mx my t"]
    for row in packed:
        lines.append(" ".join(repr(float(x)) for x in row[:6]))  # (repr of a float32's double: reads back exactly)
    (tmp_path / "views.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, "--scene", KNOBS, "--w", str(W), "--h", str(H), "--steps", str(STEPS),
                          "--views", str(tmp_path / "views.txt"), "--aa", "4:32", "--ppm", str(tmp_path / "v"),
                          "--stats"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    _knob_defaults(K)
    want, _, counts = _loop(K, W, H, views, 4, 32)
    assert '"views": 3' in run.stdout and '"aa": 4' in run.stdout and f'"refined": {int(counts.sum())}' in run.stdout
    for k in range(3):
        data = (tmp_path / f"v.{k:04d}.ppm").read_bytes()
        img = np.frombuffer(data[data.index(b"255\n") + 4:], np.uint8).reshape(H, W, 3)
        rgb = np.stack([(want[k] >> s) & 255 for s in (0, 8, 16)], -1).astype(np.uint8)
        assert np.array_equal(img, rgb), k
    assert not (tmp_path / "v.0003.ppm").exists()
