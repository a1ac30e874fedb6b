"""View batches of scene plugins on the GPU (include/rm.h rm_render_batch_ex,
rm_render_batch_ex_rgba8, rm_batch_prepare): every view of a
batch against this build's own single-frame render of the same plugin after
set_pose and set_uniform of that view's values -- every byte, no tolerance,
compared as words as tests/test_batch_gpu.py does; the single-frame kernels,
whose parity with the reference tests/test_plugins.py holds, are not touched by
the batch.  Ragged tiles, per-view floats, vectors, array elements, ints and
bools, a scene without uniforms, offsets, more views than a byte counts, a
built-in scene, the argument checks, a host target, batches in flight, the
prepare call, a reload, and the headless app."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import POSES, _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, SCENE, NO_SCENE = 0, 1, 3, 4
STEPS = 128
SENTINEL8 = 0x5A5A5A5A  # (alpha 0x5A: no pixel the pass writes, whose alpha is 255)
SENTINELF = -7.0        # (the pass writes alpha 1)
KNOBS = os.path.join(rm.SCENES_DIR, "output_shader_knobs.hip")
BALLS = os.path.join(rm.SCENES_DIR, "metaballs.hip")
PLAIN = os.path.join(rm.SCENES_DIR, "output_shader.hip")
EVAL_ONLY = ("#define RM_PLUGIN_EVAL_ONLY 1\nSdResult sceneSDF(vec3 p)\n{\n    return SdResult(sphere(vec4(0.0, 3.0, "
             "0.0, 1.0), p), Material(vec3(0.5), vec3(0.0), 1.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0)));\n}\n")


def _new(scene):
    r = rm.Renderer(0)
    _load(r, scene)
    return r


def _load(r, scene):
    r.load_scene(scene)
    r.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0)
    r.set_uniform("u_seed1", 0.5, 0.5)
    r.set_uniform("u_sample_part", 1.0)


# each scene is loaded (and its two code objects compiled) once per module
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
    """every byte (floats compared as words: a NaN equals itself, -0 differs from +0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _single(r, W, H, v, rgba8=True):
    r.set_pose(v["pos"], v["mouse"], v["time"])
    return _np(r.render_rgba8(W, H) if rgba8 else r.render(W, H))


def _singles(r, W, H, views, rgba8=True, setters=None):
    """What a caller does today: set_pose + set_uniform* + render_rgba8 / render per view.  setters: one callable
    per view that sets the view's uniform values on r."""
    frames = []
    for k, v in enumerate(views):
        if setters:
            setters[k](r)
        frames.append(_single(r, W, H, v, rgba8))
    return np.stack(frames)


def _timed(pose, t):
    return dict(pos=pose["pos"], mouse=pose["mouse"], time=t)


def _target(torch, n, H, W, rgba8):
    return torch.full((n, H, W) if rgba8 else (n, H, W, 4), SENTINEL8 if rgba8 else SENTINELF,
                      dtype=torch.int32 if rgba8 else torch.float32, device="cuda")


def _sentinel_kept(frame, rgba8):
    return (frame == SENTINEL8).all() if rgba8 else (frame == np.float32(SENTINELF)).all()


KNOB_DEFAULTS = dict(u_ball=(3.0, 2.0, 3.0, 1.0), u_box=(-5.0, 4.0, 5.0, 1.0), u_sponge_y=3.0, u_spin=2.0)


def _knob_defaults(r):
    for name, v in KNOB_DEFAULTS.items():
        r.set_uniform(name, *(v if isinstance(v, tuple) else (v,)))


# ------------------------------------------------- 1. the pass's uniforms per view, the scene's from the context

@pytest.mark.parametrize("rgba8", [True, False], ids=["rgba8", "float"])
def test_views_with_the_context_s_uniforms(K, torch_cuda, rgba8):
    torch = torch_cuda
    W, H = 41, 27  # (ragged in both directions)
    _knob_defaults(K)
    # (not its default, and in front of P0's camera, which looks down -z: the batch must read the context's block)
    K.set_uniform("u_box", 2.0, 3.0, -1.0, 0.75)
    views = [_timed(POSES["P0"], 0.0), _timed(POSES["P1"], 7.25), _timed(POSES["P2"], 31.5)]
    want = _singles(K, W, H, views, rgba8)
    n = len(views)
    out = _target(torch, n + 1, H, W, rgba8)  # one frame longer than the batch
    res = K.render_batch_ex(W, H, views, out=out, rgba8=rgba8)
    assert res is out
    got = _np(out)
    ndiff = int((got[:n].view(np.uint32) != want.view(np.uint32)).sum())
    print(f"knobs {W}x{H} {'rgba8' if rgba8 else 'float'}: {ndiff} of {want.size} words differ over {n} views")
    assert _same(got[:n], want)
    assert _sentinel_kept(got[n], rgba8)
    if rgba8:
        assert ((got[:n] >> 24) == 255).all()
    else:
        assert (got[:n, :, :, 3] == 1.0).all()
    # the views differ from each other, and u_box did move the cube
    assert not _same(want[0], want[1]) and not _same(want[1], want[2]) and not _same(want[0], want[2])
    K.set_uniform("u_box", *KNOB_DEFAULTS["u_box"])
    assert not _same(_single(K, W, H, views[0], rgba8), want[0])
    # an empty dict is no list; the frames allocated in the documented shape
    one = K.render_batch_ex(W, H, views[1:2], uniforms={}, rgba8=rgba8)
    assert tuple(one.shape) == ((1, H, W) if rgba8 else (1, H, W, 4))
    # render_batch itself still refuses the plugin
    with pytest.raises(rm.RmError):
        K.render_batch(W, H, views)


# ------------------------------------------------- 2. a vec4 and a float per view

def test_vec4_and_float_per_view(K, torch_cuda):
    W, H = 41, 27
    _knob_defaults(K)
    views = [_timed(POSES["P0"], 3.0), _timed(POSES["P0"], 3.0), _timed(POSES["P2"], 12.5), _timed(POSES["P1"], 40.0)]
    # (views 0 and 1: in front of P0's camera, which looks down -z from (2, 3, 3))
    ball = np.array([[2.0, 3.0, 0.0, 0.75], [2.5, 2.5, -0.5, 1.25], [0.5, 3.0, -2.0, 0.5], [3.5, 1.0, 2.0, 2.0]],
                    np.float32)
    spin = np.array([2.0, -9.0, 0.0, 33.5], np.float32)
    K.set_uniform("u_sponge_y", 2.5)  # (unlisted, not the default)
    before = K.uniforms()
    K.set_pose(POSES["P5"]["pos"], POSES["P5"]["mouse"], POSES["P5"]["time"])
    own = _np(K.render_rgba8(W, H))
    got = _np(K.render_batch_ex(W, H, views, uniforms=dict(u_ball=ball, u_spin=spin)))
    # the context's uniform values and pose are what they were: the getters, and a single render's bytes
    assert repr(K.uniforms()) == repr(before)
    assert _same(_np(K.render_rgba8(W, H)), own)
    setters = [lambda r, k=k: (r.set_uniform("u_ball", *map(float, ball[k])), r.set_uniform("u_spin", float(spin[k])))
               for k in range(4)]
    want = _singles(K, W, H, views, setters=setters)
    for k in range(4):
        assert _same(got[k], want[k]), f"view {k}"
    # views 0 and 1 share their pose and differ in the uniforms alone
    assert not _same(want[0], want[1])
    # the float target too
    gotf = _np(K.render_batch_ex(W, H, views, uniforms=dict(u_ball=ball, u_spin=spin), rgba8=False))
    assert _same(gotf, _singles(K, W, H, views, rgba8=False, setters=setters))
    _knob_defaults(K)


# ------------------------------------------------- 3. array elements, an int and a bool per view

def test_array_int_and_bool_per_view(M, torch_cuda):
    W, H = 33, 20
    L = rm.lib()
    pose = POSES["P0"]
    down, up = dict(pose, mouse=(0.0, 0.6)), dict(pose, mouse=(0.0, -0.6))  # (one of them looks at the floor)
    views = [_timed(pose, 0.0), _timed(pose, 5.0), _timed(POSES["P1"], 2.0), _timed(POSES["P2"], 5.0), down, up]
    n = len(views)
    rest = np.array([[k - 3.0, 2.0 + 0.25 * k, 0.5 * k, 0.8] for k in range(8)], np.float32)
    M.set_uniform_array("u_balls", rest)       # all eight from the context ...
    M.set_uniform("u_tint", 0.3, 0.05, 0.2)    # ... and the tint (unlisted)
    balls = np.array([[[0.0, 2.0, 0.0, 1.0], [1.5, 2.5, 0.5, 0.75]], [[-1.0, 3.0, 1.0, 1.25], [2.0, 1.5, -0.5, 1.0]],
                      [[0.5, 2.0, -1.0, 0.5], [0.0, 3.5, 0.0, 1.5]], [[1.0, 1.0, 1.0, 1.0], [-2.0, 2.0, 2.0, 0.9]],
                      [[2.0, 3.0, -1.0, 0.5], [1.0, 3.0, -1.0, 0.5]], [[2.0, 3.0, -1.0, 0.5], [1.0, 3.0, -1.0, 0.5]]],
                     np.float32)  # [n, 2, 4]: elements 0 and 1 of 8
    count = np.array([2, 8, 5, 3, 2, 2], np.int32)
    floor = np.array([1, 0, 7, 0, 0, 0], np.int32)  # (non-zero: true)
    before = M.uniforms()
    got = _np(M.render_batch_ex(W, H, views, uniforms=dict(u_balls=balls, u_count=count, u_floor=floor)))
    assert repr(M.uniforms()) == repr(before)

    def setter(k):
        def set_(r):
            flat = np.ascontiguousarray(balls[k])
            assert L.rm_set_uniformfv(r._ctx, b"u_balls", 4, ctypes.c_void_p(flat.ctypes.data), 2) == OK
            assert L.rm_set_uniform1i(r._ctx, b"u_count", int(count[k])) == OK
            assert L.rm_set_uniform1i(r._ctx, b"u_floor", int(floor[k])) == OK
        return set_
    want = _singles(M, W, H, views, setters=[setter(k) for k in range(n)])
    for k in range(n):
        assert _same(got[k], want[k]), f"view {k}"
    # (the first four; the last two, without a floor and looking past their balls, may both be sky)
    assert len({want[k].tobytes() for k in range(4)}) == 4
    # the tint came from the context (view 0's balls lie in front of its camera) ...
    M.set_uniform("u_tint", 0.02, 0.2, 0.02)
    setter(0)(M)
    assert not _same(_single(M, W, H, views[0]), want[0])
    M.set_uniform("u_tint", 0.3, 0.05, 0.2)
    # ... and the floor from the view: the last two views have none, and one of them would see it
    floored = []
    for k in (4, 5):
        setter(k)(M)
        M.set_uniform("u_floor", 1)
        floored.append(_single(M, W, H, views[k]))
    assert not _same(floored[0], want[4]) or not _same(floored[1], want[5])


# ------------------------------------------------- 4. a scene without uniforms

@pytest.mark.parametrize("rgba8", [True, False], ids=["rgba8", "float"])
def test_scene_without_uniforms(P, torch_cuda, rgba8):
    torch = torch_cuda
    W, H = 40, 24
    views = [POSES["P1"], POSES["P2"]]
    want = _singles(P, W, H, views, rgba8)
    out = _target(torch, 3, H, W, rgba8)
    P.render_batch_ex(W, H, views, out=out, rgba8=rgba8)
    got = _np(out)
    assert _same(got[:2], want) and _sentinel_kept(got[2], rgba8)
    assert not _same(want[0], want[1])
    # it declares nothing: any list is refused, the target untouched
    before = out.clone()
    with pytest.raises(rm.RmError) as e:
        P.render_batch_ex(W, H, views, uniforms=dict(u_ball=np.zeros((2, 4), np.float32)), out=out, rgba8=rgba8)
    assert e.value.status == INVALID
    torch.cuda.synchronize()
    assert torch.equal(out, before)


# ------------------------------------------------- 5. offsets

@pytest.mark.parametrize("rgba8", [True, False], ids=["rgba8", "float"])
def test_offset_is_render_accumulate_s(K, torch_cuda, rgba8):
    torch = torch_cuda
    W, H = 41, 27
    _knob_defaults(K)
    pose = _timed(POSES["P2"], 4.5)
    off = (0.25, -0.5)
    K.set_pose(pose["pos"], pose["mouse"], pose["time"])
    K.set_uniform("u_sample_part", 1.0)
    K.set_uniform("u_seed1", off[0] + 0.5, off[1] + 0.5)
    acc = torch.full((H, W) if rgba8 else (H, W, 4), SENTINEL8 if rgba8 else float("nan"),
                     dtype=torch.int32 if rgba8 else torch.float32, device="cuda")
    want = _np(K.render_accumulate(W, H, acc))
    K.set_uniform("u_seed1", 0.5, 0.5)
    centre = _single(K, W, H, pose, rgba8)
    got = _np(K.render_batch_ex(W, H, [dict(pose, offset=off), pose], uniforms=dict(u_spin=[2.0, 2.0]), rgba8=rgba8))
    assert _same(got[0], want) and _same(got[1], centre)
    assert not _same(want, centre)


# ------------------------------------------------- 6. more views than a byte counts

def test_300_one_tile_views(K, torch_cuda):
    n, W, H = 300, 8, 8
    _knob_defaults(K)
    # the camera of P0 looks down -z from (2, 3, 3) and walks along x; the ball in front of it pulses with the view
    views = [dict(pos=(2.0 + 0.004 * k, 3.0, 3.0), mouse=(0.0, 0.0), time=0.37 * k) for k in range(n)]
    ball = np.array([[2.0, 3.0, 0.0, 0.75 + 0.75 * (k % 2) + 0.001 * k] for k in range(n)], np.float32)
    got = _np(K.render_batch_ex(W, H, views, uniforms=dict(u_ball=ball)))
    picks = (0, 255, 256, 299)
    want = {}
    for k in picks:
        K.set_uniform("u_ball", *map(float, ball[k]))
        want[k] = _single(K, W, H, views[k])
        assert _same(got[k], want[k]), f"view {k}"
    assert len({want[k].tobytes() for k in picks}) == len(picks)
    _knob_defaults(K)


# ------------------------------------------------- 7. a built-in scene

def test_built_in_scene(torch_cuda):
    torch = torch_cuda
    W, H = 61, 37
    r = rm.Renderer(0)
    try:
        _load(r, rm.SCENE_FILES["T"])
        r.batch_prepare()  # (nothing to do)
        views = [POSES["P0"], dict(POSES["P1"], offset=(0.25, -0.375)), POSES["P2"]]
        for rgba8 in (True, False):
            assert _same(_np(r.render_batch_ex(W, H, views, rgba8=rgba8)), _np(r.render_batch(W, H, views, rgba8=rgba8)))
        out = _target(torch, 3, H, W, True)
        before = out.clone()
        with pytest.raises(rm.RmError) as e:
            r.render_batch_ex(W, H, views, uniforms=dict(u_ball=np.zeros((3, 4), np.float32)), out=out)
        assert e.value.status == INVALID and "built-in" in str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(out, before)
    finally:
        r.close()


# ------------------------------------------------- 8. arguments

def _entry(name, components, count, values):
    return _lib.RmViewUniform(name, components, count, ctypes.c_void_p(values.ctypes.data) if values is not None else None)


def _call(fn, r, W, H, views, n, entries, n_uniforms, out):
    vp = ctypes.c_void_p(views.ctypes.data) if views is not None else None
    arr = (_lib.RmViewUniform * max(1, len(entries)))(*entries) if entries is not None else None
    return fn(r._ctx, W, H, vp, n, ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, n_uniforms,
              ctypes.c_void_p(out) if out else None, None)


@pytest.mark.parametrize("name", ["rm_render_batch_ex", "rm_render_batch_ex_rgba8"])
def test_arguments(K, M, torch_cuda, name, tmp_path):
    torch = torch_cuda
    fn = getattr(rm.lib(), name)
    err = lambda r: rm.lib().rm_last_error(r._ctx).decode()  # noqa: E731
    _knob_defaults(K)
    out = torch.full((2, 8, 8, 4), SENTINELF, dtype=torch.float32, device="cuda")  # (room for either format)
    before = out.clone()
    v = rm.pack_views([POSES["P0"], POSES["P1"]])
    p = out.data_ptr()
    f2 = np.array([1.0, 2.0], np.float32)
    f8 = np.zeros((2, 4), np.float32)
    i2 = np.array([1, 0], np.int32)
    good = [_entry(b"u_spin", 1, 1, f2), _entry(b"u_ball", 4, 1, f8)]
    # n = 0: RM_OK, nothing written (views, out and values may be NULL then), stats zeroed
    st = _lib.RmStats()
    st.pixels, st.kernel_ms = 99, 1.0
    vp = ctypes.c_void_p(v.ctypes.data)
    arr = (_lib.RmViewUniform * 1)(_entry(b"u_spin", 1, 1, None))
    assert fn(K._ctx, 8, 8, vp, 0, ctypes.cast(arr, ctypes.c_void_p), 1, ctypes.c_void_p(p), ctypes.byref(st)) == OK
    assert st.pixels == 0 and st.kernel_ms == 0.0 and st.evals == 0
    assert _call(fn, K, 8, 8, None, 0, None, 0, None) == OK
    # rm_render_batch's checks, in its order: the size rule before any pointer, NULL views or out
    assert _call(fn, K, 8, 8, v, 65536, good, 2, p) == INVALID
    assert _call(fn, K, 8, 8, v, -1, good, 2, p) == INVALID
    assert _call(fn, K, 0, 8, v, 2, good, 2, p) == INVALID
    assert _call(fn, K, 1 << 16, 1 << 15, v, 2, good, 2, p) == INVALID
    assert _call(fn, K, 8, 8, None, 2, good, 2, p) == INVALID
    assert _call(fn, K, 8, 8, v, 2, good, 2, None) == INVALID
    # the list itself
    assert _call(fn, K, 8, 8, v, 2, good, -1, p) == INVALID
    assert _call(fn, K, 8, 8, v, 2, None, 2, p) == INVALID
    cases = [
        ([_entry(None, 1, 1, f2)], "null name"),
        ([_entry(b"u_spin", 1, 1, None)], "null values"),
        ([_entry(b"u_nope", 1, 1, f2)], "declares no uniform \"u_nope\""),
        ([_entry(b"u_time", 1, 1, f2)], "the pass's own"),
        ([_entry(b"u_pos", 3, 1, f8)], "the pass's own"),
        ([_entry(b"u_spin", 1, 1, f2), _entry(b"u_spin", 1, 1, f2)], "listed twice"),
        ([_entry(b"u_ball", 3, 1, f8)], "is declared vec4, got 3 components"),
        ([_entry(b"u_spin", 2, 1, f8)], "is declared float, got 2 components"),
        ([_entry(b"u_spin", 1, 0, f2)], "count 0 < 1"),
        ([_entry(b"u_ball", 4, 2, f8)], "not an array"),
    ]
    for entries, msg in cases:
        assert _call(fn, K, 8, 8, v, 2, entries, len(entries), p) == INVALID, msg
        assert msg in err(K), (msg, err(K))
    # the array's length, and the int's and the bool's declared types, on the scene that has them
    a9 = np.zeros((2, 9, 4), np.float32)
    for entries, msg in [([_entry(b"u_balls", 4, 9, a9)], "is declared vec4[8]: count 9"),
                         ([_entry(b"u_balls", 3, 2, a9)], "is declared vec4[8], got 3 components"),
                         ([_entry(b"u_count", 2, 1, i2)], "is declared int, got 2 components"),
                         ([_entry(b"u_floor", 4, 1, f8)], "is declared bool, got 4 components")]:
        assert _call(fn, M, 8, 8, v, 2, entries, 1, p) == INVALID, msg
        assert msg in err(M), (msg, err(M))
    # an offset outside [-0.5, 0.5)
    w = v.copy()
    w[1, 7] = 0.5
    assert _call(fn, K, 8, 8, w, 2, good, 2, p) == INVALID and "offset" in err(K)
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    # an eval-only plugin, and no scene at all
    r = rm.Renderer(0)
    try:
        assert _call(fn, r, 8, 8, v, 2, None, 0, p) == NO_SCENE
        assert rm.lib().rm_batch_prepare(r._ctx) == NO_SCENE
        ball = tmp_path / "ball.hip"
        ball.write_text(EVAL_ONLY)
        r.load_scene(str(ball))
        assert _call(fn, r, 8, 8, v, 2, None, 0, p) == SCENE and "RM_PLUGIN_EVAL_ONLY" in err(r)
        assert rm.lib().rm_batch_prepare(r._ctx) == SCENE
    finally:
        r.close()
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    # ... and the same arrays are fine as they were
    assert _call(fn, K, 8, 8, v, 2, good, 2, p) == OK
    torch.cuda.synchronize()
    assert not torch.equal(out, before)
    # the Python surface refuses values for another number of views
    with pytest.raises(ValueError):
        K.render_batch_ex(8, 8, v, uniforms=dict(u_spin=np.zeros(3, np.float32)))


# ------------------------------------------------- 9. further cases

@pytest.mark.parametrize("rgba8", [True, False], ids=["rgba8", "float"])
def test_host_target(K, torch_cuda, rgba8):
    W, H = 41, 27
    _knob_defaults(K)
    views = [_timed(POSES["P0"], 1.0), _timed(POSES["P1"], 2.0), _timed(POSES["P2"], 3.0)]
    u = dict(u_spin=np.array([1.0, 20.0, -3.0], np.float32))
    dev = _np(K.render_batch_ex(W, H, views, uniforms=u, rgba8=rgba8))
    host = np.full((4, H, W) if rgba8 else (4, H, W, 4), SENTINEL8 if rgba8 else SENTINELF,
                   np.uint32 if rgba8 else np.float32)
    res, st = K.render_batch_ex(W, H, views, uniforms=u, out=host, rgba8=rgba8, stats=True)
    assert res is host and st["pixels"] == 3 * W * H and st["kernel_ms"] > 0.0 and st["dispatch"] == "row-major"
    assert _same(host[:3], dev)
    assert _sentinel_kept(host[3], rgba8)


def test_two_batches_in_flight(K, torch_cuda):
    torch = torch_cuda
    W, H = 41, 27
    _knob_defaults(K)
    va = [_timed(POSES["P0"], 1.0), _timed(POSES["P1"], 2.0), _timed(POSES["P2"], 3.0)]
    vb = [_timed(POSES["P3"], 4.0), _timed(POSES["P4"], 5.0)]
    sa, sb = np.array([1.0, 20.0, -3.0], np.float32), np.array([8.0, -15.0], np.float32)
    want_a = _singles(K, W, H, va, setters=[lambda r, k=k: r.set_uniform("u_spin", float(sa[k])) for k in range(3)])
    want_b = _singles(K, W, H, vb, setters=[lambda r, k=k: r.set_uniform("u_spin", float(sb[k])) for k in range(2)])
    out_a, out_b = _target(torch, 3, H, W, True), _target(torch, 2, H, W, True)
    torch.cuda.synchronize()
    K.render_batch_ex(W, H, va, uniforms=dict(u_spin=sa), out=out_a)  # device targets, no stats: both are enqueued
    K.render_batch_ex(W, H, vb, uniforms=dict(u_spin=sb), out=out_b)
    K.synchronize()
    assert _same(_np(out_a), want_a)
    assert _same(_np(out_b), want_b)
    assert not _same(want_a[0], want_a[1])
    _knob_defaults(K)


def test_prepare_reload_and_another_scene(torch_cuda):
    W, H = 33, 20
    views = [_timed(POSES["P0"], 1.0), _timed(POSES["P2"], 6.0)]
    r = rm.Renderer(0)
    try:
        _load(r, KNOBS)
        r.batch_prepare()  # before the first batch
        r.batch_prepare()  # (loaded already)
        r.set_uniform("u_spin", 11.0)
        got = _np(r.render_batch_ex(W, H, views))
        assert _same(got, _singles(r, W, H, views))
        # another scene after a batch: the batch renders the new scene
        _load(r, BALLS)
        r.set_uniform("u_count", 3)
        r.set_uniform_array("u_balls", np.array([[0.0, 2.0, 0.0, 1.0], [1.5, 2.5, 0.5, 0.75], [-1, 3, 1, 1]], np.float32))
        got_m = _np(r.render_batch_ex(W, H, views, uniforms=dict(u_floor=np.array([1, 0], np.int32))))
        want_m = _singles(r, W, H, views, setters=[lambda q: q.set_uniform("u_floor", 1),
                                                   lambda q: q.set_uniform("u_floor", 0)])
        assert _same(got_m, want_m) and not _same(got_m, got)
        # a reload of the same file resets the unlisted uniforms to their defaults
        _load(r, KNOBS)
        got_d = _np(r.render_batch_ex(W, H, views))
        assert abs(r.uniforms()["u_spin"]["value"] - 2.0) == 0.0
        assert _same(got_d, _singles(r, W, H, views)) and not _same(got_d, got)
        r.set_uniform("u_spin", 11.0)
        assert _same(_np(r.render_batch_ex(W, H, views)), got)
    finally:
        r.close()


# ------------------------------------------------- 10. the app

def test_headless_app_renders_a_plugin_s_views(K, torch_cuda, tmp_path):
    """apps/raymarch_headless --scene <a .hip scene> --views (rm::Shader::renderBatchEx)"""
    W, H = 41, 27
    exe = os.path.join(ROOT, "apps", "raymarch_headless")
    views = [_timed(POSES["P0"], 1.5), dict(_timed(POSES["P1"], 9.0), offset=(0.25, -0.375)), _timed(POSES["P2"], 20.0)]
    packed = rm.pack_views(views)
    lines = ["# px py pz mx my t [ox oy]"]
    for k, row in enumerate(packed):
        vals = row if k == 1 else row[:6]
        lines.append(" ".join(repr(float(x)) for x in vals))  # (repr of a float32's double: reads back exactly)
    (tmp_path / "views.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, "--scene", KNOBS, "--w", str(W), "--h", str(H), "--steps", str(STEPS),
                          "--views", str(tmp_path / "views.txt"), "--ppm", str(tmp_path / "v"), "--stats"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert '"views": 3' in run.stdout and '"kernel_ms"' in run.stdout
    _knob_defaults(K)
    want = _np(K.render_batch_ex(W, H, views))
    for k in range(3):
        data = (tmp_path / f"v.{k:04d}.ppm").read_bytes()
        img = np.frombuffer(data[data.index(b"255\n") + 4:], np.uint8).reshape(H, W, 3)
        rgb = np.stack([(want[k] >> s) & 255 for s in (0, 8, 16)], -1).astype(np.uint8)
        assert np.array_equal(img, rgb), k
    assert not (tmp_path / "v.0003.ppm").exists()
