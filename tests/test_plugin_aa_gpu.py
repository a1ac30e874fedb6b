"""Adaptive supersampling of scene plugins on the GPU (include/rm.h
rm_render_aa_ex_rgba8, rm_refine_ex_rgba8, rm_aa_prepare): the
refined pixels against what a caller gets today by blending this build's own
rm_render_accumulate float frames of the plugin on the host (tests/aa_ref.py's
seeds, its tree mean, the oracle's RGBA8 pack) -- every word, no tolerance --
and the mask against the edge rule's restatement on the GPU's own frame.  The
plugin's frame kernels, whose parity with the reference tests/test_plugins.py
holds, are not touched by the refine.  Ragged sizes, the scene's own uniforms,
an adaptive threshold, device and host pointers, a queue several sweeps long, a
built-in scene, a reload, the prepare call, the argument checks, the oracle and
the headless app."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from raymarching_amd import POSES, _lib
from tests import aa_ref
from tests.parity import POLICY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, SCENE, NO_SCENE = 0, 1, 3, 4
STEPS = 128
SENTINEL8 = 0x5A5A5A5A  # (alpha 0x5A: no pixel the pass writes, whose alpha is 255)
KNOBS = os.path.join(rm.SCENES_DIR, "output_shader_knobs.hip")
BALLS = os.path.join(rm.SCENES_DIR, "metaballs.hip")
PLAIN = os.path.join(rm.SCENES_DIR, "output_shader.hip")
EVAL_ONLY = ("#define RM_PLUGIN_EVAL_ONLY 1\nSdResult sceneSDF(vec3 p)\n{\n    return SdResult(sphere(vec4(0.0, 3.0, "
             "0.0, 1.0), p), Material(vec3(0.5), vec3(0.0), 1.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0)));\n}\n")
# two primitives: a sphere over a plane
SPHERE_OVER_PLANE = (
    "SdResult sceneSDF(vec3 p)\n{\n"
    "    Material red = Material(vec3(0.6, 0.1, 0.1), vec3(0.04), 32.0, 0.1, 0.0, vec3(0.0), 1.0, vec3(0.0));\n"
    "    Material grey = Material(vec3(0.3), vec3(0.03), 64.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0));\n"
    "    SdResult ball = SdResult(sphere(vec4(0.0, 2.0, 0.0, 1.5), p), red);\n"
    "    SdResult ground = SdResult(plane(p), grey);\n"
    "    if (ball.dist < ground.dist) return ball;\n"
    "    return ground;\n}\n")
KNOB_DEFAULTS = dict(u_ball=(3.0, 2.0, 3.0, 1.0), u_box=(-5.0, 4.0, 5.0, 1.0), u_sponge_y=3.0, u_spin=2.0)
THREE_BALLS = np.array([[0.0, 2.0, 0.0, 1.0], [1.5, 2.5, 0.5, 0.75], [-1.0, 3.0, 1.0, 1.25]], np.float32)


def _load(r, scene, steps=STEPS):
    r.load_scene(scene)
    r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0)
    r.set_uniform("u_seed1", 0.5, 0.5)
    r.set_uniform("u_sample_part", 1.0)


def _new(scene, steps=STEPS):
    r = rm.Renderer(0)
    _load(r, scene, steps)
    return r


# each scene is loaded (and its code objects compiled) once per module
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


def _words(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return a.view(np.uint32)


def _pose(r, pose, time=None):
    r.set_pose(pose["pos"], pose["mouse"], pose["time"] if time is None else time)


def _knob_defaults(r):
    for name, v in KNOB_DEFAULTS.items():
        r.set_uniform(name, *(v if isinstance(v, tuple) else (v,)))


def _set_balls(r):
    r.set_uniform_array("u_balls", THREE_BALLS)
    r.set_uniform("u_count", 3)
    r.set_uniform("u_tint", 0.3, 0.05, 0.2)
    r.set_uniform("u_floor", 1)


def _blend(torch, r, W, H, K):
    """Every pixel's K-sample colour as a caller builds it today, under r's
    current uniforms: the K float frames render_accumulate returns with
    u_sample_part = 1 and u_seed1 = o + 0.5, their tree mean, the RGBA8 pack
    (tests/test_aa_gpu.py _supersampled).  Leaves u_seed1 = (0.5, 0.5)."""
    frames = []
    for seed in aa_ref.seeds(K):
        r.set_uniform("u_seed1", float(seed[0]), float(seed[1]))
        acc = torch.full((H, W, 4), float("nan"), device="cuda")
        frames.append(r.render_accumulate(W, H, acc).cpu().numpy())
    r.set_uniform("u_seed1", 0.5, 0.5)
    ref = oracle.pack_rgba8(aa_ref.tree_mean(frames))
    ref.setflags(write=False)
    return ref


_REF = {}  # the knobs scene at its defaults: (W, H, pose, time, K) -> the blend, computed once and left unchanged


def _knobs_ref(torch, r, W, H, pose_name, time, K):
    """Expects the knobs scene at its default uniforms and the pose set."""
    key = (W, H, pose_name, time, K)
    if key not in _REF:
        _REF[key] = _blend(torch, r, W, H, K)
    return _REF[key]


def _ndiff(got, want):
    return int((got != want).sum())


# ---------------------------------------------------------------- 1. every pixel

# (37 x 21: neither a multiple of 8, and 777 pixels fill no wave's last group at any K)
@pytest.mark.parametrize("W,H,samples", [(40, 24, 2), (40, 24, 4), (40, 24, 8), (37, 21, 2), (37, 21, 8)])
def test_threshold_zero_supersamples_every_pixel_knobs(K, torch_cuda, W, H, samples):
    _knob_defaults(K)
    _pose(K, POSES["P1"], 2.75)  # (time != 0: the scene reads u_time from the kernel's first argument)
    want = _knobs_ref(torch_cuda, K, W, H, "P1", 2.75, samples)
    out, mask, st = K.render_aa_ex(W, H, samples=samples, threshold=0, mask=True, stats=True)
    got = _words(out)
    n = _ndiff(got, want)
    print(f"knobs {W}x{H} K={samples}: {n} of {W * H} words differ from the blended accumulate frames")
    assert n == 0
    assert st["refined"] == W * H and bool(mask.all())
    # supersampling did something: the frame differs from the centre samples
    assert not np.array_equal(got, _words(K.render_rgba8(W, H)))


def test_threshold_zero_supersamples_every_pixel_metaballs(M, torch_cuda):
    W, H, samples = 33, 20, 4  # (neither a multiple of 8; 660 pixels, not a multiple of 16)
    _set_balls(M)
    _pose(M, POSES["P0"], 1.5)
    want = _blend(torch_cuda, M, W, H, samples)
    out, mask, st = M.render_aa_ex(W, H, samples=samples, threshold=0, mask=True, stats=True)
    got = _words(out)
    n = _ndiff(got, want)
    print(f"metaballs {W}x{H} K={samples}: {n} of {W * H} words differ from the blended accumulate frames")
    assert n == 0
    assert st["refined"] == W * H and bool(mask.all())
    assert not np.array_equal(got, _words(M.render_rgba8(W, H)))


# ---------------------------------------------------------------- 2. the scene's own uniforms

def test_the_scene_s_own_uniforms_reach_the_refine(K, torch_cuda):
    """Fails if the uniform block is not the refine kernel's second argument or
    is read at another offset: the samples would be the default scene's."""
    torch = torch_cuda
    W, H, samples = 40, 24, 4
    _knob_defaults(K)
    _pose(K, POSES["P1"], 2.75)
    default = _knobs_ref(torch, K, W, H, "P1", 2.75, samples)
    try:
        K.set_uniform("u_ball", 2.0, 2.5, 2.0, 1.5)
        K.set_uniform("u_spin", 0.5)
        K.set_uniform("u_sponge_y", 3.75)
        want = _blend(torch, K, W, H, samples)
        got = _words(K.render_aa_ex(W, H, samples=samples, threshold=0))
        print(f"moved knobs: {_ndiff(got, want)} words differ from the blend, {_ndiff(got, default)} from the defaults'")
        assert _ndiff(got, want) == 0
        assert _ndiff(got, default) > 0 and _ndiff(want, default) > 0
        # one uniform again, with no reload
        K.set_uniform("u_ball", -1.0, 3.0, 2.0, 0.75)
        want2 = _blend(torch, K, W, H, samples)
        got2 = _words(K.render_aa_ex(W, H, samples=samples, threshold=0))
        assert _ndiff(got2, want2) == 0
        assert _ndiff(got2, got) > 0 and _ndiff(want2, want) > 0
    finally:
        _knob_defaults(K)
    # and back at the defaults
    assert _ndiff(_words(K.render_aa_ex(W, H, samples=samples, threshold=0)), default) == 0


# ---------------------------------------------------------------- 3., 4. adaptive, and the equivalent paths

def test_adaptive_threshold_32_and_equivalent_paths(K, torch_cuda):
    torch = torch_cuda
    W, H, samples = 61, 37, 4
    _knob_defaults(K)
    _pose(K, POSES["P2"])
    full = _knobs_ref(torch, K, W, H, "P2", None, samples)
    # (test 1's frame: the call at threshold 0 gives the blend everywhere)
    every = _words(K.render_aa_ex(W, H, samples=samples, threshold=0))
    assert _ndiff(every, full) == 0
    base = _words(K.render_rgba8(W, H))
    want_mask = aa_ref.edge_mask(base, 32)
    out, mask, st = K.render_aa_ex(W, H, samples=samples, threshold=32, mask=True, stats=True)
    got, m = _words(out), mask.cpu().numpy()
    print(f"knobs {W}x{H} P2: edge share {float(want_mask.mean()):.3f}, refined {st['refined']}")
    assert 0 < st["refined"] < W * H  # both branches
    assert m.dtype == np.uint8 and np.array_equal(m, want_mask)
    assert st["refined"] == int(want_mask.sum())
    assert np.array_equal(got[m == 0], base[m == 0])
    assert np.array_equal(got[m == 1], every[m == 1])
    # render_aa_ex = refine_ex(render_rgba8()), and the mask is optional
    two = K.render_rgba8(W, H)
    assert K.refine_ex(two, samples=samples, threshold=32) is two
    assert np.array_equal(_words(two), got)
    # host pointers: staged, the same bytes
    host, host_mask = K.render_aa_ex(W, H, samples=samples, threshold=32, out=np.zeros((H, W), np.uint32), mask=True)
    assert np.array_equal(host, got) and np.array_equal(host_mask, m)
    host2 = base.copy()
    K.refine_ex(host2, samples=samples, threshold=32)
    assert np.array_equal(host2, got)
    host3 = K.render_aa_ex(W, H, samples=samples, threshold=32, out=np.zeros((H, W), np.uint32))
    assert np.array_equal(host3, got)


# ---------------------------------------------------------------- 5. a queue several sweeps long

def test_queue_several_sweeps_long(torch_cuda, tmp_path):
    """512 x 512 at threshold 0 and K = 8: 2^18 queue entries at 8 pixels per
    wave, 2^15 groups -- at 32 resident one-wave workgroups on each of 256
    compute units every wave strides at least four times."""
    W = H = 512
    path = tmp_path / "sphere_over_plane.hip"
    path.write_text(SPHERE_OVER_PLANE)
    r = _new(str(path), steps=32)
    try:
        _pose(r, POSES["P0"])
        want = _blend(torch_cuda, r, W, H, 8)
        out, st = r.render_aa_ex(W, H, samples=8, threshold=0, stats=True)
        assert st["refined"] == 1 << 18
        got = _words(out)
        assert _ndiff(got, want) == 0
        assert len(np.unique(got)) > 16  # (a picture, not one colour)
    finally:
        r.close()


# ---------------------------------------------------------------- 6. a built-in scene through _ex

def test_built_in_scene_through_ex(torch_cuda):
    W, H, samples = 61, 37, 4
    r = _new(rm.SCENE_FILES["T"])
    try:
        _pose(r, POSES["P2"])
        a, am, ast = r.render_aa(W, H, samples=samples, threshold=32, mask=True, stats=True)
        b, bm, bst = r.render_aa_ex(W, H, samples=samples, threshold=32, mask=True, stats=True)
        assert np.array_equal(_words(a), _words(b)) and np.array_equal(am.cpu().numpy(), bm.cpu().numpy())
        assert 0 < ast["refined"] == bst["refined"] < W * H
        two = r.render_rgba8(W, H)
        r.refine_ex(two, samples=samples, threshold=32)
        assert np.array_equal(_words(two), _words(a))
        r.aa_prepare()  # (compiled in: nothing to do)
    finally:
        r.close()


# ---------------------------------------------------------------- 7. reload

def test_reload_drops_the_refine_kernel(K, torch_cuda):
    torch = torch_cuda
    W, H, samples = 40, 24, 4
    _knob_defaults(K)
    _pose(K, POSES["P1"], 2.75)
    want_a = _knobs_ref(torch, K, W, H, "P1", 2.75, samples)
    r = _new(KNOBS)
    try:
        def frame():
            return _words(r.render_aa_ex(W, H, samples=samples, threshold=0))

        _pose(r, POSES["P1"], 2.75)
        assert _ndiff(frame(), want_a) == 0
        _load(r, BALLS)
        _set_balls(r)
        _pose(r, POSES["P1"], 2.75)
        want_b = _blend(torch, r, W, H, samples)
        got_b = frame()
        assert _ndiff(got_b, want_b) == 0  # no stale AA module
        assert _ndiff(got_b, want_a) > 0
        _load(r, KNOBS)  # (from the code cache)
        _pose(r, POSES["P1"], 2.75)
        assert _ndiff(frame(), want_a) == 0
    finally:
        r.close()


# ---------------------------------------------------------------- 8. aa_prepare

def test_aa_prepare(K, torch_cuda, tmp_path):
    W, H, samples = 40, 24, 4
    L = rm.lib()
    _knob_defaults(K)
    _pose(K, POSES["P1"], 2.75)
    lazily = _words(K.render_aa_ex(W, H, samples=samples, threshold=32))
    r = rm.Renderer(0)
    try:
        assert L.rm_aa_prepare(r._ctx) == NO_SCENE
        _load(r, KNOBS)
        assert L.rm_aa_prepare(r._ctx) == OK
        assert L.rm_aa_prepare(r._ctx) == OK  # (loaded already)
        r.aa_prepare()
        _pose(r, POSES["P1"], 2.75)
        assert np.array_equal(_words(r.render_aa_ex(W, H, samples=samples, threshold=32)), lazily)
        path = tmp_path / "ball.hip"
        path.write_text(EVAL_ONLY)
        r.load_scene(str(path))
        assert L.rm_aa_prepare(r._ctx) == SCENE
        assert "RM_PLUGIN_EVAL_ONLY" in L.rm_last_error(r._ctx).decode()
        with pytest.raises(rm.RmError):
            r.aa_prepare()
    finally:
        r.close()


# ---------------------------------------------------------------- 9. errors

def _call(fn, r, W, H, params, frame, mask=None):
    return fn(r._ctx, W, H, ctypes.byref(params) if params is not None else None,
              ctypes.c_void_p(frame) if frame else None, ctypes.c_void_p(mask) if mask else None, None)


@pytest.mark.parametrize("name", ["rm_refine_ex_rgba8", "rm_render_aa_ex_rgba8"])
def test_argument_checks(M, torch_cuda, tmp_path, name):
    torch = torch_cuda
    fn = getattr(rm.lib(), name)
    _set_balls(M)
    _pose(M, POSES["P0"], 1.5)
    good = _lib.RmAaParams(4, 32)
    ok = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    assert _call(fn, M, 4, 4, good, ok.data_ptr()) == OK
    frame = torch.full((4, 4), SENTINEL8, dtype=torch.int32, device="cuda")
    p = frame.data_ptr()
    for W, H in [(0, 4), (4, 0), (-1, 4), (4, -1), (1 << 15, 1 << 15), (1 << 30, 1)]:
        assert _call(fn, M, W, H, good, p) == INVALID, (W, H)
    assert _call(fn, M, 4, 4, None, p) == INVALID
    assert _call(fn, M, 4, 4, good, None) == INVALID
    for samples in (0, 1, 3, 16, -4):
        assert _call(fn, M, 4, 4, _lib.RmAaParams(samples, 32), p) == INVALID, samples
    for t in (-1, 256):
        assert _call(fn, M, 4, 4, _lib.RmAaParams(4, t), p) == INVALID, t
    # frame and mask live in the same place
    host_mask = np.full((4, 4), 0x5A, np.uint8)
    assert _call(fn, M, 4, 4, good, p, host_mask.ctypes.data) == INVALID
    assert "mixed" in rm.lib().rm_last_error(M._ctx).decode()
    host_frame = np.full((4, 4), SENTINEL8, np.uint32)
    dev_mask = torch.full((4, 4), 0x5A, dtype=torch.uint8, device="cuda")
    assert _call(fn, M, 4, 4, good, host_frame.ctypes.data, dev_mask.data_ptr()) == INVALID
    # no scene, and a plugin without render kernels
    r = rm.Renderer(0)
    try:
        assert _call(fn, r, 4, 4, good, p) == NO_SCENE
        # (the order: the arguments are looked at before the scene)
        assert _call(fn, r, 4, 4, _lib.RmAaParams(3, 32), p) == INVALID
        path = tmp_path / "ball.hip"
        path.write_text(EVAL_ONLY)
        r.load_scene(str(path))
        assert _call(fn, r, 4, 4, good, p) == SCENE
        assert "RM_PLUGIN_EVAL_ONLY" in rm.lib().rm_last_error(r._ctx).decode()
        assert _call(fn, r, 4, 4, good, p, host_mask.ctypes.data) == SCENE  # (before the mixed pointers)
    finally:
        r.close()
    torch.cuda.synchronize()
    assert bool((frame == SENTINEL8).all()) and bool((dev_mask == 0x5A).all())
    assert (host_frame == SENTINEL8).all() and (host_mask == 0x5A).all()


# ---------------------------------------------------------------- 10. the oracle

def test_against_the_oracle(P, torch_cuda):
    """scenes/output_shader.hip is the reference's scene O as a plugin, and
    tests/test_plugins.py holds its plain frame to POLICY["O"]; so the bound is
    tests/test_aa_gpu.py's for scene O.  The reference is built on the GPU's
    mask: the oracle's jittered pixels, tree mean, where the mask is set, its
    centre frame elsewhere, packed.  A float within 2e-3 moves a byte by at
    most one, and a mean of K samples is within tolerance when all K are: the
    share of pixels whose three bytes each differ by at most 1 is at least
    1 - K (1 - POLICY f2e3)."""
    W, H, samples, pose = 48, 32, 4, POSES["P3"]
    _pose(P, pose)
    out, mask = P.render_aa_ex(W, H, samples=samples, threshold=32, mask=True)
    got, m = _words(out), mask.cpu().numpy().astype(bool)
    kw = dict(pos=pose["pos"], mouse=pose["mouse"], time=pose["time"], max_steps=STEPS)
    ref, _ = oracle.render("O", W, H, **kw)
    ys, xs = np.nonzero(m)
    assert 0 < len(xs) < W * H
    parts = [oracle.render_pixels("O", W, H, xs, ys, jitter=(float(o[0]), float(o[1])), **kw)[0]
             for o in aa_ref.offsets(samples)]
    ref[ys, xs] = aa_ref.tree_mean(parts)
    want = oracle.pack_rgba8(ref)
    d = np.zeros((H, W), np.int64)
    for shift in (0, 8, 16):
        d = np.maximum(d, np.abs(((got >> shift) & 255).astype(np.int64) - ((want >> shift) & 255).astype(np.int64)))
    share = float(np.mean(d <= 1))
    level = 1.0 - samples * (1.0 - POLICY["O"]["f2e3"])
    print(f"plugin O {W}x{H}: {share:.4f} of pixels within one byte of the oracle (level {level:.2f}), "
          f"{int(m.sum())} refined")
    assert share >= level, (share, level)


# ---------------------------------------------------------------- 11. the headless app

def test_headless_app_writes_render_aa_ex(K, torch_cuda, tmp_path):
    """apps/raymarch_headless --scene x.hip --aa 4:32 (rm::RenderTexture::drawAAEx):
    the frame render_aa_ex returns for the same pose."""
    W, H = 96, 54
    exe = os.path.join(ROOT, "apps", "raymarch_headless")
    ppm = tmp_path / "aa.ppm"
    run = subprocess.run([exe, "--scene", KNOBS, "--w", str(W), "--h", str(H), "--frames", "1", "--time-freeze",
                          "--aa", "4:32", "--ppm", str(ppm)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    data = ppm.read_bytes()
    img = np.frombuffer(data[data.index(b"255\n") + 4:], np.uint8).reshape(H, W, 3)
    _knob_defaults(K)
    _pose(K, POSES["P0"])  # the app's start-up pose: main.cpp's
    out, st = K.render_aa_ex(W, H, samples=4, threshold=32, stats=True)
    want = _words(out)
    rgb = np.stack([(want >> s) & 255 for s in (0, 8, 16)], -1).astype(np.uint8)
    assert 0 < st["refined"] < W * H
    assert np.array_equal(img, rgb)
