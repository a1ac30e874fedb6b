"""Ray queries: rm_cast_rays (castRayD / castRayDI, common.frag:879-925, over
caller-supplied rays) and rm_camera_rays (the rays main() builds for a frame),
through the C ABI, the ctypes binding, Renderer and the headless app.

The reference is tests/ray_ref.py's numpy march over the oracle's sceneSDF
(a plugin's: over its own rm_scene_eval).  The first test pins that march
against oracle.render_diag without a GPU; the GPU tests compare the kernels
with it on 4096 rays per scene (ray_ref.ray_set), after asserting that the
reference itself hits and misses at least 15 % of them each."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from raymarching_amd import _lib
from tests import ray_ref
from tests.parity import FULL_SIZE_STEP_MAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TIME = 1.25
EXACT = FULL_SIZE_STEP_MAP["O"]  # 0.9999: scene O's march against the oracle (at 4096 rays: all)
CLOSE = FULL_SIZE_STEP_MAP["T"]  # 0.998


def _within(a, b, rel=1e-5, ab=1e-5):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b) <= ab + rel * np.abs(b)


def _rows(eq):
    return eq if eq.ndim == 1 else eq.all(-1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    """equal bit for bit, per ray (so that NaN equals NaN and -0 differs from 0)"""
    return _rows(_bits(np.asarray(a, np.float32)) == _bits(np.asarray(b, np.float32)))


_REF = {}


def reference(scene, steps=128, inside=False):
    """the numpy march over the oracle's sceneSDF on the scene's ray set, with
    the oracle's normal at its shaded points and material at its last points
    (computed once per case, never modified)"""
    key = (scene, steps, inside)
    if key not in _REF:
        o, d = ray_ref.inside_ray_set() if inside else ray_ref.ray_set(scene)
        r = ray_ref.march(lambda p: oracle.scene_dist(scene, p, time=TIME), o, d, steps, inside=inside)
        shade = r["t"] > 0
        r["normal"] = np.zeros((len(d), 3), np.float32)
        if shade.any():
            r["normal"][shade] = oracle.normal(scene, r["position"][shade], time=TIME)
        r["material"] = oracle.scene_mat(scene, r["last"], time=TIME)
        r["origins"], r["directions"] = o, d
        for v in r.values():
            v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def assert_mixed(ref, what):
    """agreement cannot be trivial: the reference itself hits and misses"""
    hit, miss = np.mean(ref["status"] == ray_ref.HIT), np.mean(ref["status"] == ray_ref.MISS)
    assert hit >= 0.15 and miss >= 0.15, (what, hit, miss)


def exact_share(got, ref, keys=("status", "steps", "t", "position", "normal", "material")):
    ok = np.ones(len(ref["t"]), bool)
    for k in keys:
        a, b = np.asarray(got[k]), ref[k]
        ok &= _same(a, b) if b.dtype == np.float32 else _rows(a == b)
    return float(np.mean(ok)), ok


def per_output(got, ref):
    """the share of rays equal bit for bit, output by output (printed by the tests)"""
    return {k: round(exact_share(got, ref, keys=(k,))[0], 5) for k in ("status", "steps", "t", "position", "normal",
                                                                         "material")}


# ------------------------------------------------------------------ CPU


@pytest.mark.parametrize("W,H,pos", [(64, 64, (2.0, 3.0, 3.0)), (96, 54, (0.5, 2.0, 6.0))])
def test_reference_march_is_the_oracles_primary_march(W, H, pos):
    """The yardstick: ray_ref.march over oracle.scene_dist along the numpy
    camera rays reproduces oracle.render_diag's primary hit depth, and
    oracle.normal at ro + rd * t its primary normal, bit for bit (scene O,
    u_mouse = 0)."""
    diag, _ = oracle.render_diag("O", W, H, pos=pos, mouse=(0.0, 0.0), time=0.0, max_steps=128)
    g = diag[:, :, 0].reshape(-1, 4)
    dirs = ray_ref.camera_dirs_unrotated(W, H).reshape(-1, 3)
    r = ray_ref.march(lambda p: oracle.scene_dist("O", p, time=0.0), np.array(pos, np.float32), dirs, 128)
    shade = r["t"] > 0
    assert 0.15 * W * H < shade.sum() < 0.85 * W * H
    assert np.array_equal(shade, g[:, 3] != -9.0)
    assert np.array_equal(r["t"][shade], g[shade, 3])
    assert np.array_equal(oracle.normal("O", r["position"][shade], time=0.0), g[shade, :3])


def test_reference_outcomes_of_the_ray_sets():
    for scene in ("S0", "T", "O", "OG"):
        assert_mixed(reference(scene), scene)
    assert np.mean(reference("O", steps=8)["status"] == ray_ref.EXHAUSTED) >= 0.10
    assert np.mean(reference("OG", inside=True)["status"] == ray_ref.HIT) >= 0.15


def test_binding_has_the_ray_calls_and_struct(tmp_path):
    assert {"rm_cast_rays", "rm_camera_rays"} <= set(_lib.EXPORTS)
    L = rm.lib()
    assert L.rm_cast_rays.argtypes[6]._type_ is _lib.RmRayHits
    src = tmp_path / "layout.c"
    src.write_text('#include "rm.h"\n#include <stddef.h>\n'
                   f'_Static_assert(sizeof(rm_ray_hits) == {ctypes.sizeof(_lib.RmRayHits)}, "rm_ray_hits");\n'
                   f'_Static_assert(offsetof(rm_ray_hits, material) == {_lib.RmRayHits.material.offset}, "material");\n'
                   '_Static_assert(RM_RAY_MISS == 0 && RM_RAY_HIT == 1 && RM_RAY_EXHAUSTED == 2, "RM_RAY_*");\n')
    subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ------------------------------------------------------------------ GPU


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def load(R, scene, steps=128):
    R.load_scene(rm.SCENE_FILES.get(scene, scene))
    R.set_pose((2.0, 3.0, 3.0), (0.0, 0.0), TIME)
    R.set_params(max_steps=steps, shadow_max_steps=0, count_evals=0, kernel="auto")


def cast_np(R, ref, n=None, **kw):
    o, d = ref["origins"], ref["directions"]
    return R.cast_rays(o[:n], d[:n], material=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["O", "OG"])
def test_scene_o_casts_equal_the_reference_bit_for_bit(R, scene):
    ref = reference(scene)
    assert_mixed(ref, scene)
    load(R, scene)
    got = cast_np(R, ref)
    share, ok = exact_share(got, ref)
    print(f"cast {scene}: {share:.5f} of {len(ok)} rays bit-exact in every output; per output {per_output(got, ref)}")
    assert share >= EXACT, (share, np.flatnonzero(~ok)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("scene,steps", [("O", 128), ("OG", 128), ("O", 8)])
def test_scene_o_materials_equal_the_oracles(R, scene, steps):
    """`material` equals oracle.scene_mat at the reference's last points, bit
    for bit.  The rays that decide it end on the floor inside the blur band of
    its tiles (floorMat, output_shader.frag:16-28; 19 % of the set), where the
    colour depends on the last bit of sin(pi x) and pow(|p|, 1.3): the oracle
    evaluates them with the C library, the cast kernels with its restatement
    (csrc/rm_libm_ref.h, tests/test_libm_ref.py).  With the render kernels'
    floor_mat (GLSL sin, hardware exp2 / log2) the share was 0.814."""
    ref = reference(scene, steps=steps)
    load(R, scene, steps=steps)
    got = cast_np(R, ref)
    share, ok = exact_share(got, ref, keys=("material",))
    print(f"cast {scene}, {steps} steps: material bit-exact on {share:.5f} of {len(ok)} rays, "
          f"max |d| {np.abs(got['material'] - ref['material']).max():.3g}")
    assert share >= EXACT, (share, np.flatnonzero(~ok)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["S0", "T"])
def test_scene_s0_t_casts_match_the_reference(R, scene):
    ref = reference(scene)
    assert_mixed(ref, scene)
    load(R, scene)
    got = cast_np(R, ref)
    same = (got["status"] == ref["status"]) & (got["steps"] == ref["steps"])
    exact, _ = exact_share(got, ref, keys=("status", "steps", "t"))
    print(f"cast {scene}: status+steps equal on {np.mean(same):.5f}, bit-exact (status, steps, t) on {exact:.5f}")
    assert np.mean(same) >= CLOSE
    assert _within(got["t"][same], ref["t"][same]).all()
    # the other outputs on these scenes: zero where nothing is shaded, unit normals where something is,
    # and the scenes' one constant material
    shade = got["t"] > 0
    assert np.array_equal(got["position"][~shade], np.zeros((int((~shade).sum()), 3), np.float32))
    assert np.allclose(np.linalg.norm(got["normal"][shade], axis=1), 1.0, atol=1e-5)
    assert not got["normal"][~shade].any()
    assert (got["material"] == got["material"][0]).all() and got["material"][0, 0] > 0


@pytest.mark.gpu
def test_exhausted_rays_and_small_step_counts(R):
    ref = reference("O", steps=8)
    assert np.mean(ref["status"] == ray_ref.EXHAUSTED) >= 0.10
    load(R, "O", steps=8)
    got = cast_np(R, ref)
    share, ok = exact_share(got, ref)
    print(f"cast O, 8 steps: {share:.5f} bit-exact in every output; exhausted with t > 0: "
          f"{int(((ref['status'] == ray_ref.EXHAUSTED) & (ref['t'] > 0)).sum())}")
    assert share >= EXACT, np.flatnonzero(~ok)[:8]
    for steps in (0, 1, 2):
        r = reference("O", steps=steps)
        R.set_params(max_steps=steps)
        got = cast_np(R, r)
        share, ok = exact_share(got, r)
        assert share >= EXACT, (steps, np.flatnonzero(~ok)[:8])
    R.set_params(max_steps=0)
    r0 = cast_np(R, reference("O", steps=0))
    assert not r0["t"].any() and (r0["status"] == ray_ref.EXHAUSTED).all() and not r0["steps"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65])
def test_partial_waves(R, torch_cuda, n):
    ref = reference("O")
    load(R, "O")
    got = cast_np(R, ref, n=n)
    for k in ("status", "steps", "t", "position", "normal", "material"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k][:n])), k
    # device buffers one ray longer than the launch: the guard leaves the tail alone
    torch = torch_cuda
    o = torch.from_numpy(ref["origins"][:n].copy()).cuda()
    d = torch.from_numpy(ref["directions"][:n].copy()).cuda()
    t = torch.full((n + 64,), -7.0, device="cuda")
    hits = _lib.RmRayHits(t.data_ptr(), None, None, None, None, None)
    _lib.check(rm.lib().rm_cast_rays(R._ctx, o.data_ptr(), 0, d.data_ptr(), n, 0, ctypes.byref(hits), None), R._ctx)
    R.synchronize()
    t = t.cpu().numpy()
    assert np.array_equal(_bits(t[:n]), _bits(ref["t"][:n])) and (t[n:] == -7.0).all()


@pytest.mark.gpu
def test_shared_origin_host_and_device_pointers_and_null_outputs(R, torch_cuda):
    torch = torch_cuda
    ref = reference("O")
    load(R, "O")
    d = ref["directions"]
    o1 = np.array([0.5, 2.0, 6.0], np.float32)
    shared = R.cast_rays(o1, d, material=True)
    repeated = R.cast_rays(np.tile(o1, (len(d), 1)), d, material=True)
    assert np.mean(shared["status"] == ray_ref.HIT) > 0.15
    for k in repeated:
        assert np.array_equal(_bits(shared[k]), _bits(repeated[k])), k
    # device pointers: device results, the same bytes
    dev = R.cast_rays(torch.from_numpy(o1).cuda(), torch.from_numpy(d.copy()).cuda(), material=True)
    R.synchronize()
    for k in repeated:
        assert dev[k].is_cuda
        assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(repeated[k])), k
    # outputs left NULL are not written, and the others do not change by it
    few = R.cast_rays(o1, d, normal=False, material=False)
    assert set(few) == {"t", "status", "steps", "position"}
    for k in few:
        assert np.array_equal(_bits(few[k]), _bits(repeated[k])), k
    n = len(d)
    bufs = {k: torch.full((n * w,), 123.0, device="cuda") for k, w in
            (("t", 1), ("status", 1), ("steps", 1), ("position", 3), ("normal", 3), ("material", 16))}
    hits = _lib.RmRayHits(bufs["t"].data_ptr(), None, None, None, bufs["normal"].data_ptr(), None)
    od, dd = torch.from_numpy(o1).cuda(), torch.from_numpy(d.copy()).cuda()
    _lib.check(rm.lib().rm_cast_rays(R._ctx, od.data_ptr(), 1, dd.data_ptr(), n, 0, ctypes.byref(hits), None), R._ctx)
    R.synchronize()
    for k in ("status", "steps", "position", "material"):
        assert (bufs[k] == 123.0).all(), k
    assert np.array_equal(_bits(bufs["t"].cpu().numpy()), _bits(repeated["t"]))
    assert np.array_equal(_bits(bufs["normal"].cpu().numpy().reshape(-1, 3)), _bits(repeated["normal"]))


@pytest.mark.gpu
def test_inside_marches(R):
    ref = reference("OG", inside=True)
    assert np.mean(ref["status"] == ray_ref.HIT) >= 0.15
    load(R, "OG")
    got = cast_np(R, ref, inside=True)
    share, ok = exact_share(got, ref)
    print(f"cast OG inside: {share:.5f} of {len(ok)} rays bit-exact in every output")
    assert share >= EXACT, np.flatnonzero(~ok)[:8]
    # the outside march of the same rays differs (it starts inside the surface)
    assert np.mean(cast_np(R, ref)["t"] != got["t"]) > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["DIAG_O_96x54_P2", "DIAG_O_64_P6"])
def test_camera_rays_cast_to_the_reference_glsls_primary_hits(R, name):
    """rm_camera_rays + rm_cast_rays against what SwiftShader computed from the
    reference's shader: channel 0 of the diagnostic golden, the primary normal
    and hit depth, set exactly where t > 0."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    m = json.loads(str(z["meta"]))
    W, H = m["W"], m["H"]
    g = z["diag"][:, :, 0].reshape(-1, 4)
    R.load_scene(rm.SCENE_FILES["O"])
    R.set_pose(m["pos"], m["mouse"], m["time"])
    R.set_params(max_steps=m["max_steps"], count_evals=0)
    origin, dirs = R.camera_rays(W, H)
    assert dirs.shape == (H, W, 3)
    assert np.array_equal(origin.cpu().numpy(), np.array(m["pos"], np.float32))
    got = R.cast_rays(origin, dirs.reshape(-1, 3), stats=True)
    t, nrm = got["t"].cpu().numpy(), got["normal"].cpu().numpy()
    shade = g[:, 3] != -9.0
    assert 0.15 < shade.mean() < 0.95
    ok = (shade == (t > 0)) & np.where(shade, _same(t, g[:, 3]) & _same(nrm, g[:, :3]), True)
    print(f"{name}: {np.mean(ok):.5f} of {W * H} pixels equal the golden's primary hit (depth and normal)")
    assert np.mean(ok) >= EXACT
    # rm_stats of the same call: evals is the sum of steps
    assert got["stats"]["evals"] == int(got["steps"].sum().item())
    assert got["stats"]["pixels"] == W * H and got["stats"]["scene"] == 2 and got["stats"]["kernel_ms"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(64, 64), (96, 54), (61, 37)])
def test_camera_rays_unrotated_equal_the_formula(R, W, H):
    R.load_scene(rm.SCENE_FILES["O"])
    R.set_pose(rm.POSES["P0"]["pos"], rm.POSES["P0"]["mouse"], rm.POSES["P0"]["time"])
    origin, dirs = R.camera_rays(W, H)
    assert np.array_equal(_bits(dirs.cpu().numpy()), _bits(ray_ref.camera_dirs_unrotated(W, H)))
    # host buffers: the same bytes
    o = np.zeros(3, np.float32)
    d = np.zeros((H, W, 3), np.float32)
    _lib.check(rm.lib().rm_camera_rays(R._ctx, W, H, ctypes.c_void_p(o.ctypes.data), ctypes.c_void_p(d.ctypes.data)),
               R._ctx)
    assert np.array_equal(o, np.array(rm.POSES["P0"]["pos"], np.float32))
    assert np.array_equal(_bits(d), _bits(dirs.cpu().numpy()))
    # every built-in scene and a plugin answer with unit directions
    for scene in ("S0", "T", os.path.join(rm.SCENES_DIR, "showcase.hip")):
        R.load_scene(rm.SCENE_FILES.get(scene, scene))
        _, dd = R.camera_rays(W, H)
        assert np.allclose(np.linalg.norm(dd.cpu().numpy(), axis=-1), 1.0, atol=1e-6)


def plugin(name):
    return os.path.join(rm.SCENES_DIR, name)


@pytest.mark.gpu
def test_output_shader_plugin_casts_match_builtin_o(R):
    ref = reference("O")
    load(R, "O")
    a = cast_np(R, ref)
    load(R, plugin("output_shader.hip"))
    b = cast_np(R, ref)
    same = a["status"] == b["status"]
    print(f"plugin O vs built-in O: status equal on {np.mean(same):.5f}, all outputs bit-exact on "
          f"{exact_share(b, a)[0]:.5f}")
    assert np.mean(same) >= CLOSE
    assert _within(b["t"][same], a["t"][same]).all()


def host_driven(R, o, d, steps):
    """the reference march with the plugin's own rm_scene_eval as sceneSDF"""
    return ray_ref.march(lambda p: R.scene_eval(p), o, d, steps)


def assert_matches_host_march(R, o, d, steps, what):
    got = R.cast_rays(o, d)
    ref = host_driven(R, o, d, steps)
    same = (got["status"] == ref["status"]) & (got["steps"] == ref["steps"])
    exact = np.mean(same & _same(got["t"], ref["t"]))
    print(f"{what}: status+steps equal on {np.mean(same):.5f}, t bit-exact too on {exact:.5f}; "
          f"hit {np.mean(ref['status'] == 1):.3f}, miss {np.mean(ref['status'] == 0):.3f}")
    assert np.mean(same) >= CLOSE, what
    assert _within(got["t"][same], ref["t"][same]).all(), what
    return got, ref


@pytest.mark.gpu
def test_showcase_plugin_casts_match_its_own_scene_eval(R):
    o, d = ray_ref.ray_set("O")
    load(R, plugin("showcase.hip"), steps=64)
    _, ref = assert_matches_host_march(R, o, d, 64, "showcase.hip")
    assert np.mean(ref["status"] == ray_ref.HIT) >= 0.15 and np.mean(ref["status"] == ray_ref.MISS) >= 0.15


@pytest.mark.gpu
def test_metaballs_uniforms_move_the_hits(R):
    o, d = ray_ref.ray_set("O")  # half of them aimed at (0, 3, 0) +- 1.5
    load(R, plugin("metaballs.hip"), steps=64)
    R.set_uniform_array("u_balls", np.array([[0.0, 3.0, 0.0, 1.0]], np.float32))
    R.set_uniform("u_count", 1)
    a, ref = assert_matches_host_march(R, o, d, 64, "metaballs.hip, ball at (0, 3, 0)")
    assert np.mean(ref["status"] == ray_ref.HIT) >= 0.15 and np.mean(ref["status"] == ray_ref.MISS) >= 0.15
    R.set_uniform_array("u_balls", np.array([[0.5, 3.0, 0.0, 1.0]], np.float32))
    b, _ = assert_matches_host_march(R, o, d, 64, "metaballs.hip, ball moved to (0.5, 3, 0)")
    aimed = slice(0, len(d) // 2)
    assert np.mean(a["t"][aimed] != b["t"][aimed]) > 0.05


@pytest.mark.gpu
def test_eval_only_plugin_casts_and_failed_reload_keeps_casting(R, tmp_path):
    p = tmp_path / "ball.hip"
    p.write_text("#define RM_PLUGIN_EVAL_ONLY 1\nSdResult sceneSDF(vec3 p)\n{\n    return SdResult(sphere(vec4(0.0, 3.0, "
                 "0.0, 1.0), p), Material(vec3(0.5), vec3(0.0), 1.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0)));\n}\n")
    o, d = ray_ref.ray_set("O")
    load(R, str(p), steps=64)
    with pytest.raises(rm.RmError):
        R.render(16, 16)  # (no render kernel in it)
    a, ref = assert_matches_host_march(R, o, d, 64, "RM_PLUGIN_EVAL_ONLY sphere")
    assert 0.02 < np.mean(ref["status"] == ray_ref.HIT) < 0.9
    broken = tmp_path / "broken.hip"
    broken.write_text("SdResult sceneSDF(vec3 p) { return nope; }\n")
    with pytest.raises(rm.RmError):
        R.load_scene(str(broken))
    b = R.cast_rays(o, d)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.gpu
def test_argument_errors(torch_cuda):
    torch = torch_cuda
    L = rm.lib()
    r = rm.Renderer(0)
    try:
        o = np.zeros((4, 3), np.float32)
        d = np.ones((4, 3), np.float32)
        t = np.zeros(4, np.float32)
        hits = _lib.RmRayHits(t.ctypes.data, None, None, None, None, None)
        vp = ctypes.c_void_p

        def cast(origins=o.ctypes.data, directions=d.ctypes.data, n=4, out=hits, ctx=r._ctx):
            return L.rm_cast_rays(ctx, vp(origins), 0, vp(directions), n, 0, ctypes.byref(out) if out else None, None)
        INVALID, NO_SCENE = _lib.STATUS_CODES["RM_ERR_INVALID_ARGUMENT"], _lib.STATUS_CODES["RM_ERR_NO_SCENE"]
        assert cast(ctx=None) == INVALID
        # argument errors come before the scene check
        assert cast(n=-1) == INVALID
        assert cast(n=(1 << 30) + 1) == INVALID
        assert cast(origins=None) == INVALID
        assert cast(directions=None) == INVALID
        assert cast(out=None) == INVALID
        assert cast(out=_lib.RmRayHits(None, t.ctypes.data, None, None, None, None)) == INVALID
        assert cast() == NO_SCENE
        assert cast(n=0) == NO_SCENE
        assert L.rm_camera_rays(r._ctx, 4, 4, vp(o.ctypes.data), vp(d.ctypes.data)) == NO_SCENE
        r.load_scene(rm.SCENE_FILES["O"])
        assert cast(n=0) == 0
        assert cast(n=0, origins=None, directions=None, out=None) == 0
        assert cast() == 0
        # host and device pointers mixed
        td = torch.zeros(4, device="cuda")
        assert cast(out=_lib.RmRayHits(td.data_ptr(), None, None, None, None, None)) == INVALID
        assert "mixed" in L.rm_last_error(r._ctx).decode()
        dd = torch.ones((4, 3), device="cuda")
        assert cast(directions=dd.data_ptr()) == INVALID
        for W, H, po, pd in ((0, 4, o.ctypes.data, d.ctypes.data), (4, -1, o.ctypes.data, d.ctypes.data),
                             (1 << 16, 1 << 15, o.ctypes.data, d.ctypes.data), (2, 2, None, d.ctypes.data),
                             (2, 2, o.ctypes.data, None)):
            assert L.rm_camera_rays(r._ctx, W, H, vp(po), vp(pd)) == INVALID, (W, H)
        assert L.rm_camera_rays(None, 2, 2, vp(o.ctypes.data), vp(d.ctypes.data)) == INVALID
        with pytest.raises(ValueError):
            r.cast_rays(np.zeros((3, 3), np.float32), d)
    finally:
        r.close()


@pytest.mark.gpu
def test_headless_app_pick(R):
    """apps/raymarch_headless --pick X,Y: rm::Shader::cameraRays + castRays
    (include/rm_pass.hpp) print what the Python call returns for that pixel
    (the app's start-up pose is P0; --time-freeze keeps u_time = 0)."""
    exe = os.path.join(ROOT, "apps", "raymarch_headless")
    W, H = 96, 54
    pose = rm.POSES["P0"]
    R.load_scene(rm.SCENE_FILES["O"])
    R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    R.set_params(max_steps=128, count_evals=0)
    origin, dirs = R.camera_rays(W, H)
    got = {k: v.cpu().numpy() for k, v in R.cast_rays(origin, dirs.reshape(-1, 3), material=True).items()}
    hits = np.flatnonzero(got["status"] == ray_ref.HIT)
    assert len(hits) > 0.15 * W * H
    i = int(hits[len(hits) // 2])
    x, y = i % W, i // W
    out = subprocess.run([exe, "--scene", "output_shader.frag", "--w", str(W), "--h", str(H), "--frames", "1",
                          "--time-freeze", "--pick", f"{x},{y}"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{"pick"')]
    assert len(lines) == 1, out.stdout
    p = lines[0]
    assert p["pick"] == [x, y] and p["status"] == "hit" == _lib.RAY_STATUS[int(got["status"][i])]
    assert np.float32(p["t"]) == got["t"][i]
    assert np.array_equal(np.array(p["position"], np.float32), got["position"][i])
    assert np.array_equal(np.array(p["normal"], np.float32), got["normal"][i])
    assert np.array_equal(np.array(p["diffuse"], np.float32), got["material"][i, :3])
