"""Uniforms a scene plugin declares itself, on the GPU (include/rm.h,
rm_load_scene and rm_set_uniform*; the CPU side is tests/test_uniforms.py).

The reference for every value is the scene's *baked twin*: the same text with
each `uniform T name [= init];` replaced by `const T name = <value>;` (an
array by `const vec4 name[N] = {vec4(...), ...};`), which needs no uniform
support at all.  Only exact operations separate the two forms (the scenes use
their uniforms in + - *, comparisons, min/max, constructors, loop bounds and
branches, and the moved values avoid 0 and 1), so frames, step maps and
rm_scene_eval results are compared bit for bit.  Frames are 64x64 and 72x40
(partial 8x8 tiles on both edges) at 128 steps."""
import os
import re
import subprocess

import numpy as np
import pytest

import raymarching_amd as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = os.path.join(rm.SCENES_DIR, "output_shader_knobs.hip")
METABALLS = os.path.join(rm.SCENES_DIR, "metaballs.hip")
SIZES = [(64, 64, "P0"), (72, 40, "P3")]
STEPS = 128

KNOB_DEFAULTS = {"u_ball": (3.0, 2.0, 3.0, 1.0), "u_box": (-5.0, 4.0, 5.0, 1.0), "u_sponge_y": 3.0, "u_spin": 2.0}
KNOB_MOVED = {"u_ball": (2.5, 2.25, 3.5, 0.75), "u_box": (-4.5, 3.5, 5.5, 1.25), "u_sponge_y": 2.75, "u_spin": 1.5}
# three balls where scene O has its sponge; every number is a dyadic fraction
BALLS = np.array([[0.0, 2.5, 0.0, 1.25], [1.5, 3.25, -0.5, 0.75], [-1.25, 1.75, 0.5, 0.875]], np.float32)
TINT = (0.25, 0.03125, 0.0625)


def _lit(x):
    return repr(float(x))


def bake(text, values):
    """The baked twin of a scene text: every uniform declaration as a constant
    with the value of `values` (an array: [N, components], all N elements)."""
    def const(m):
        ty, name, n = m.group(1), m.group(2), m.group(3)
        v = values[name]
        if n:
            v = np.asarray(v, np.float32).reshape(int(n), -1)
            elems = ", ".join(f"{ty}({', '.join(_lit(x) for x in e)})" for e in v)
            return f"const {ty} {name}[{n}] = {{{elems}}};"
        if ty == "bool":
            return f"const bool {name} = {'true' if v else 'false'};"
        if ty == "int":
            return f"const int {name} = {int(v)};"
        if ty == "float":
            return f"const float {name} = {_lit(v)};"
        return f"const {ty} {name} = {ty}({', '.join(_lit(x) for x in v)});"
    out, n = re.subn(r"\buniform\s+(\w+)\s+(\w+)\s*(?:\[(\d+)\])?\s*(?:=[^;]*)?;", const, text)
    assert n == len(values), (n, sorted(values))
    return out


def twin_file(tmp_path, scene, values, name):
    p = tmp_path / name
    p.write_text(bake(open(scene).read(), values))
    return str(p)


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def points():
    rng = np.random.default_rng(20261020)
    return rng.uniform([-8, -1, -8], [8, 7, 8], (4096, 3)).astype(np.float32)


def pose(R, name, time=None):
    p = rm.POSES[name]
    R.set_pose(p["pos"], p["mouse"], p["time"] if time is None else time)


def results(R, points, step_map=True):
    """Everything a scene computes at the quoted sizes: per size the float frame
    of the timed kernel, its RGBA8 frame, the instrumented kernel's frame, step
    map and evals total; then rm_scene_eval's distances and materials at u_time = 3.5."""
    out = []
    for W, H, p in SIZES:
        pose(R, p)
        R.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0, kernel="auto", schedule=0)
        out.append(R.render(W, H).cpu().numpy())
        out.append(R.render_rgba8(W, H).cpu().numpy())
        if step_map:
            img, ev, st = R.render_step_map(W, H)
            out += [img.cpu().numpy(), ev.cpu().numpy(), np.int64(st["evals"])]
    pose(R, "P0", time=3.5)
    d, m = R.scene_eval(points, material=True)
    return out + [d, m]


def assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i)
        # bit for bit (floats as their words: a NaN equals itself, -0 differs from 0)
        xb, yb = (x.view(np.uint32), y.view(np.uint32)) if x.dtype == np.float32 else (x, y)
        ndiff = int((xb != yb).sum())
        assert ndiff == 0, f"{what}: result {i} differs in {ndiff} of {x.size} values"


def set_knobs(R, values):
    for k, v in values.items():
        R.set_uniform(k, *(v if isinstance(v, tuple) else (v,)))


# ---- 1

def test_knobs_at_their_defaults_are_scene_o(R, points):
    """output_shader_knobs.hip at its defaults against output_shader.hip, which
    the goldens and the oracle pin (tests/test_plugins.py)."""
    R.load_scene(os.path.join(rm.SCENES_DIR, "output_shader.hip"))
    ref = results(R, points)
    R.load_scene(KNOBS)
    assert_same(results(R, points), ref, "knobs at defaults vs output_shader.hip")


# ---- 2

def test_moved_knobs_match_the_baked_twin(R, points, tmp_path):
    R.load_scene(KNOBS)
    default8 = [r for r in results(R, points, step_map=False) if r.dtype == np.int32]
    set_knobs(R, KNOB_MOVED)
    got = results(R, points)
    R.load_scene(twin_file(tmp_path, KNOBS, KNOB_MOVED, "knobs_moved_twin.hip"))
    assert R.uniforms() == {}
    assert_same(got, results(R, points), "moved knobs vs baked twin")
    for d, g in zip(default8, [r for r in got if r.dtype == np.int32 and r.ndim == 2][::2]):
        assert np.mean(d != g) > 0.01, "the moved knobs move the picture"


# ---- 3

def metaball_values(count, floor, balls=BALLS, tint=TINT):
    b = np.zeros((8, 4), np.float32)
    b[:len(balls)] = balls
    return {"u_balls": b, "u_count": count, "u_tint": tint, "u_floor": floor}


def test_metaballs_set_through_the_array_call(R, points, tmp_path):
    R.load_scene(METABALLS)
    pose(R, SIZES[0][2])
    R.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0, kernel="auto", schedule=0)
    empty = R.render_rgba8(*SIZES[0][:2]).cpu().numpy()
    R.set_uniform("u_count", 3)
    R.set_uniform_array("u_balls", BALLS)
    R.set_uniform("u_tint", *TINT)
    R.set_uniform("u_floor", False)
    u = R.uniforms()
    assert u["u_count"]["value"] == 3 and u["u_floor"]["value"] is False and u["u_tint"]["value"] == TINT
    assert np.array_equal(u["u_balls"]["value"][:3], BALLS) and not u["u_balls"]["value"][3:].any()
    got = results(R, points)
    # elements [0, 2) only: element 2 stays
    R.set_uniform_array("u_balls", BALLS[:2] + np.float32(0.5))
    now = R.uniforms()["u_balls"]["value"]
    assert np.array_equal(now[:2], BALLS[:2] + np.float32(0.5)) and np.array_equal(now[2:3], BALLS[2:3])
    R.load_scene(twin_file(tmp_path, METABALLS, metaball_values(3, False), "metaballs_three_twin.hip"))
    assert_same(got, results(R, points), "three metaballs vs baked twin")
    pose(R, SIZES[0][2])
    assert np.mean(R.render_rgba8(*SIZES[0][:2]).cpu().numpy() != empty) > 0.01, "the balls are in the picture"


def test_metaballs_without_balls_with_the_floor(R, points, tmp_path):
    R.load_scene(METABALLS)
    R.set_uniform_array("u_balls", BALLS)  # placed, but not counted
    R.set_uniform("u_count", 0)
    R.set_uniform("u_floor", True)
    R.set_uniform("u_tint", *TINT)
    got = results(R, points)
    R.load_scene(twin_file(tmp_path, METABALLS, metaball_values(0, True), "metaballs_floor_twin.hip"))
    assert_same(got, results(R, points), "no metaballs, floor, vs baked twin")


# ---- 4

def test_every_launch_path_takes_the_block(R, torch_cuda):
    torch = torch_cuda
    W, H, p = SIZES[1]
    R.load_scene(KNOBS)
    set_knobs(R, KNOB_MOVED)
    pose(R, p)
    R.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0, kernel="auto", schedule=0)
    ref = R.render_rgba8(W, H)
    default = rm.Renderer(0)
    try:  # (the values matter: at the defaults the frame is another)
        default.load_scene(KNOBS)
        pose(default, p)
        default.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0, kernel="auto", schedule=0)
        assert not torch.equal(default.render_rgba8(W, H), ref)
    finally:
        default.close()
    frame = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    for offset, run in ((0, 3), (3, 2)):  # the two parts of cycle = 5
        n = rm.cycle_rows(H, 5, offset, run)
        rows = torch.empty((n, W), dtype=torch.int32, device="cuda")
        R.render_cycle_rows(W, H, 5, offset, run, 0, n, rows)
        R.scatter_part_rgba8(W, H, 5, offset, run, n, rows, frame)
    assert torch.equal(frame, ref), "cycle rows"
    R.set_uniform("u_seed1", 0.5, 0.5)
    R.set_uniform("u_sample_part", 1.0)
    acc = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    R.render_accumulate(W, H, acc)
    assert torch.equal(acc, ref), "accumulate"


# ---- 5

def test_values_are_read_when_the_launch_is_enqueued(R, torch_cuda):
    torch = torch_cuda
    W, H, p = SIZES[0]
    R.load_scene(KNOBS)
    pose(R, p)
    R.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0, kernel="auto", schedule=0)
    ref_a = R.render_rgba8(W, H).clone()
    R.set_uniform("u_ball", *KNOB_MOVED["u_ball"])
    ref_b = R.render_rgba8(W, H).clone()
    torch.cuda.synchronize()
    assert not torch.equal(ref_a, ref_b)
    R.set_uniform("u_ball", *KNOB_DEFAULTS["u_ball"])
    a, b = torch.empty_like(ref_a), torch.empty_like(ref_a)
    s = torch.cuda.Stream()
    R.set_stream(s)
    try:
        R.render_rgba8(W, H, out=a)                       # no synchronisation from here ...
        R.set_uniform("u_ball", *KNOB_MOVED["u_ball"])
        R.render_rgba8(W, H, out=b)
        s.synchronize()                                   # ... to here
    finally:
        R.set_stream(None)
    assert torch.equal(a, ref_a) and torch.equal(b, ref_b)


# ---- 6

def test_state_rules(R, torch_cuda, tmp_path, capfd):
    torch = torch_cuda
    R.load_scene(KNOBS)
    u = R.uniforms()
    assert list(u) == ["u_ball", "u_box", "u_sponge_y", "u_spin"]  # declaration order
    assert {k: v["value"] for k, v in u.items()} == KNOB_DEFAULTS
    assert u["u_ball"] == dict(type="float", components=4, count=0, value=KNOB_DEFAULTS["u_ball"])
    assert u["u_spin"] == dict(type="float", components=1, count=0, value=2.0)
    # set, then the same file again: the defaults are back
    set_knobs(R, KNOB_MOVED)
    assert {k: v["value"] for k, v in R.uniforms().items()} == KNOB_MOVED
    R.load_scene(KNOBS)
    assert {k: v["value"] for k, v in R.uniforms().items()} == KNOB_DEFAULTS
    # a failed reload keeps the values and the frame
    set_knobs(R, KNOB_MOVED)
    pose(R, "P0")
    R.set_params(max_steps=STEPS, shadow_max_steps=0, count_evals=0)
    before = R.render_rgba8(64, 64).clone()
    broken = tmp_path / "broken.hip"
    broken.write_text("uniform float u_other = 4.0;\nuniform float u_bad = 1.0 + 1.0;\n")
    with pytest.raises(rm.RmError) as e:
        R.load_scene(str(broken))
    assert e.value.status == rm._lib.STATUS_CODES["RM_ERR_SCENE"] and "broken.hip:2:" in str(e.value)
    assert {k: v["value"] for k, v in R.uniforms().items()} == KNOB_MOVED
    assert torch.equal(R.render_rgba8(64, 64), before)
    # wrong arity or type
    invalid = rm._lib.STATUS_CODES["RM_ERR_INVALID_ARGUMENT"]
    for bad in (lambda: R.set_uniform("u_ball", 1.0, 2.0, 3.0), lambda: R.set_uniform("u_spin", 1.0, 2.0),
                lambda: R.set_uniform_array("u_ball", np.zeros((2, 4), np.float32)),
                lambda: R.set_uniform("n" * 64, 1.0),
                lambda: rm._lib.check(rm.lib().rm_set_uniform1i(R._ctx, b"u_spin", 2), R._ctx)):
        with pytest.raises(rm.RmError) as e:
            bad()
        assert e.value.status == invalid, str(e.value)
    with pytest.raises(rm.RmError) as e:
        R.set_uniform("u_ball", 1.0, 2.0, 3.0)
    assert "vec4" in str(e.value)  # the declared type
    with pytest.raises(ValueError):
        R.set_uniform("u_ball", 1.0, 2.0, 3.0, 4.0, 5.0)
    assert {k: v["value"] for k, v in R.uniforms().items()} == KNOB_MOVED
    # int and bool: through the int call, refused by the float ones, arrays bounded
    R.load_scene(METABALLS)
    u = R.uniforms()
    assert list(u) == ["u_balls", "u_count", "u_tint", "u_floor"]
    assert (u["u_balls"]["type"], u["u_balls"]["components"], u["u_balls"]["count"]) == ("float", 4, 8)
    assert u["u_balls"]["value"].shape == (8, 4) and not u["u_balls"]["value"].any()
    assert u["u_count"] == dict(type="int", components=1, count=0, value=0)
    assert u["u_floor"] == dict(type="bool", components=1, count=0, value=True)
    assert u["u_tint"]["value"] == tuple(float(np.float32(x)) for x in (0.02, 0.2, 0.02))
    R.set_uniform("u_count", 5)
    R.set_uniform("u_floor", False)
    assert R.uniforms()["u_count"]["value"] == 5 and R.uniforms()["u_floor"]["value"] is False
    for bad in (lambda: rm._lib.check(rm.lib().rm_set_uniform1f(R._ctx, b"u_count", 2.0), R._ctx),
                lambda: R.set_uniform_array("u_balls", np.zeros((9, 4), np.float32)),
                lambda: R.set_uniform_array("u_balls", np.zeros((2, 3), np.float32)),
                lambda: R.set_uniform("u_balls", 1.0, 2.0, 3.0, 4.0)):
        with pytest.raises(rm.RmError) as e:
            bad()
        assert e.value.status == invalid, str(e.value)
    # an undeclared name: one warning, no error
    capfd.readouterr()
    R.set_uniform("u_nobody_declared_this", 1.0)
    R.set_uniform("u_nobody_declared_this", 2.0)
    assert capfd.readouterr().err.count("u_nobody_declared_this") == 1
    # a built-in scene declares none
    R.load_scene(rm.SCENE_FILES["O"])
    assert R.uniforms() == {}
    R.set_uniform("u_ball", 1.0, 2.0, 3.0, 4.0)  # (unknown now: ignored)


# ---- 7

def test_headless_app_sets_uniforms(R, tmp_path):
    """apps/raymarch_headless --uniform: the C++ surface (include/rm_pass.hpp)
    renders the frame the Python one renders with the same values."""
    app = os.path.join(ROOT, "apps", "raymarch_headless")
    ppm = tmp_path / "frame.ppm"
    run = subprocess.run([app, "--scene", METABALLS, "--uniform", "u_count=2", "--uniform", "u_tint=0.2,0.02,0.02",
                          "--w", "64", "--h", "64", "--frames", "1",
                          "--time-freeze", "--ppm", str(ppm)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    data = ppm.read_bytes()
    head = b"P6\n64 64\n255\n"
    assert data.startswith(head)
    rgb = np.frombuffer(data[len(head):], np.uint8).reshape(64, 64, 3)
    R.load_scene(METABALLS)
    R.set_uniform("u_count", 2)
    R.set_uniform("u_tint", 0.2, 0.02, 0.02)
    R.set_uniform("u_resolution", 64.0, 64.0)
    pose(R, "P0")
    R.set_params(max_steps=128, shadow_max_steps=0, count_evals=0)
    px = R.render_rgba8(64, 64).cpu().numpy().view(np.uint8).reshape(64, 64, 4)
    assert np.array_equal(px[..., :3], rgb)
    # a wrong arity is the app's error, with the declared type in the message
    run = subprocess.run([app, "--scene", METABALLS, "--uniform", "u_tint=1,2", "--w", "16", "--h", "16", "--frames",
                          "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 1 and "vec3" in run.stderr, run.stdout + run.stderr
