"""HIP path (librm.so on the MI355X) against the oracle and the reference-GLSL
goldens.  Every render goes through the C ABI."""
import glob
import json
import os

import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from raymarching_amd import POSES, S0_POSE
from tests import sentinel
from tests.parity import FULL_SIZE_POLICY, FULL_SIZE_STEP_MAP, assert_parity, diff_stats

pytestmark = pytest.mark.gpu

GOLDEN = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz"))
                if os.path.basename(p).startswith(("S0_", "T_", "O_", "OG_")))

# per-pixel ray-step maps: fraction of pixels whose sceneSDF call count equals
# the reference GLSL's (SURVEY.md 8(c) asks >= 95 %)
STEP_MAP_EXACT = 0.95


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def setup(r, scene, pose, steps=128, kernel="auto", res=None, shadow=0):
    r.load_scene(rm.SCENE_FILES[scene])
    r.set_pose(pose["pos"], pose["mouse"], pose["time"])
    r.set_params(max_steps=steps, shadow_max_steps=shadow, count_evals=1, kernel=kernel)
    if res is not None:
        r.set_uniform("u_resolution", *res)


def hip(r, W, H):
    img, st = r.render(W, H, stats=True)
    return img.cpu().numpy(), st


def ref(scene, W, H, pose, steps=128, **kw):
    return oracle.render(scene, W, H, pos=pose["pos"], mouse=pose["mouse"], time=pose["time"], max_steps=steps,
                         **kw)


def check_evals(st, ev, tol=5e-3):
    tot = int(ev.sum(dtype=np.uint64))
    assert abs(st["evals"] - tot) <= tol * tot + 4, (st["evals"], tot)


# ------------------------------------------------------------ goldens


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_hip_matches_reference_glsl_golden(R, path):
    """Image and per-pixel ray-step map against the reference GLSL's.  Pixels
    whose GLSL result is undefined (pow of a negative base: NaN in the oracle,
    scene OG at P7 only) are not compared (tests/test_oracle_golden.py)."""
    z = np.load(path, allow_pickle=False)
    m = json.loads(str(z["meta"]))
    pose = dict(pos=m["pos"], mouse=m["mouse"], time=m["time"])
    setup(R, m["scene"], pose, m["max_steps"])
    img, evmap, st = R.render_step_map(m["W"], m["H"])
    img, evmap = img.cpu().numpy(), evmap.cpu().numpy()
    o, ev = ref(m["scene"], m["W"], m["H"], pose, m["max_steps"])
    ok = ~np.isnan(o[..., :3]).any(-1)
    # the undefined pixels are undefined on the GPU too: NaN where the oracle's are
    assert np.array_equal(np.isnan(img[..., :3]).any(-1), ~ok)
    sg = assert_parity(m["scene"], img[ok], z["rgba"][ok], label="vs golden")
    so = assert_parity(m["scene"], img[ok], o[ok], label="vs oracle")
    exact = float(np.mean(evmap == z["evals"]))
    print(f"{os.path.basename(path)}: vs golden {sg}, vs oracle {so}, step map exact {exact:.4f}")
    assert exact >= STEP_MAP_EXACT, exact
    assert int(evmap.sum(dtype=np.int64)) == st["evals"]
    check_evals(st, z["evals"])


# per-ray-step FLOP bounds of the instrumented tally (rm_device.h Tally,
# SURVEY.md 8(d)): every term evaluated vs the reference's full tally
FLOP_BOUNDS = {"S0": (9, 9), "T": (6 + 17, 155), "O": (18 + 17 + 16 + 1, 221), "OG": (18 + 17 + 16 + 1, 221)}


@pytest.mark.parametrize("scene,pose", [("S0", None), ("T", "P0"), ("T", "P4"), ("O", "P0"), ("O", "P2"),
                                        ("OG", "P3")])
def test_flop_tally_within_reference_tally(R, scene, pose):
    setup(R, scene, S0_POSE if scene == "S0" else POSES[pose], 128)
    _, st = hip(R, 160, 96)
    lo, hi = FLOP_BOUNDS[scene]
    assert st["evals"] > 0
    per = st["flop"] / st["evals"]
    assert lo <= per <= hi, (scene, per)
    if scene != "S0":
        assert per < hi  # the early exits skip work somewhere in every such frame


# ------------------------------------------------------- configs / poses


def test_c1_sphere_256(R):
    setup(R, "S0", S0_POSE, 64)
    img, st = hip(R, 256, 256)
    o, ev = ref("S0", 256, 256, S0_POSE, 64)
    s = assert_parity("S0", img, o)
    assert s["max"] < 1e-3
    assert st["evals"] == int(ev.sum())


@pytest.mark.parametrize("pose", list(POSES))
def test_scene_T_poses(R, pose):
    setup(R, "T", POSES[pose], 128)
    img, evmap, st = R.render_step_map(192, 108)
    img, evmap = img.cpu().numpy(), evmap.cpu().numpy()
    o, ev = ref("T", 192, 108, POSES[pose], 128)
    s = assert_parity("T", img, o, label=pose)
    exact = float(np.mean(evmap == ev))
    print(f"T {pose} 192x108 vs oracle {s}, step map exact {exact:.4f}")
    assert exact >= STEP_MAP_EXACT
    check_evals(st, ev)


@pytest.mark.parametrize("pose", list(POSES))
def test_scene_O_poses(R, pose):
    setup(R, "O", POSES[pose], 128)
    img, evmap, st = R.render_step_map(128, 96)
    img, evmap = img.cpu().numpy(), evmap.cpu().numpy()
    o, ev = ref("O", 128, 96, POSES[pose], 128)
    s = assert_parity("O", img, o, label=pose)
    exact = float(np.mean(evmap == ev))
    print(f"O {pose} 128x96 vs oracle {s}, step map exact {exact:.4f}")
    assert exact >= STEP_MAP_EXACT
    check_evals(st, ev)


@pytest.mark.parametrize("pose", ["P1", "P3", "P6", "P7", "P8"])
def test_glass_variant_refraction_path(R, pose):
    """Test scene OG: blue objects with transparency 0.9 drive renderRefraction
    (output_shader.frag:298-343) and castRayDI (common.frag:903-925)."""
    setup(R, "OG", POSES[pose], 128)
    img, evmap, st = R.render_step_map(128, 96)
    img, evmap = img.cpu().numpy(), evmap.cpu().numpy()
    o, ev = ref("OG", 128, 96, POSES[pose], 128)
    s = assert_parity("OG", img, o, label=pose)
    exact = float(np.mean(evmap == ev))
    print(f"OG {pose} 128x96 vs oracle {s}, step map exact {exact:.4f}")
    assert exact >= STEP_MAP_EXACT
    check_evals(st, ev)


def test_glass_variant_differs_where_blue_is_visible(R):
    imgs = {}
    for sc in ("O", "OG"):
        o, _ = ref(sc, 96, 64, POSES["P1"], 128)
        imgs[sc] = o
    assert np.abs(imgs["O"] - imgs["OG"]).max() > 0.05  # the pose shows the sphere/cube
    # P7 puts the camera inside the glass cube: every primary ray starts refracting


@pytest.mark.parametrize("steps", [0, 1, 2, 7, 512])
def test_max_steps_edges(R, steps):
    for sc in ("T", "O"):
        setup(R, sc, POSES["P0"], steps)
        img, st = hip(R, 64, 40)
        o, ev = ref(sc, 64, 40, POSES["P0"], steps)
        assert_parity(sc, img, o, label=f"steps={steps}")
        check_evals(st, ev)


def test_shadow_step_cap(R):
    setup(R, "O", POSES["P6"], 128, shadow=16)
    img, st = hip(R, 96, 64)
    o, ev = ref("O", 96, 64, POSES["P6"], 128, shadow_max_steps=16)
    assert_parity("O", img, o)
    check_evals(st, ev)


@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (53, 1), (37, 23), (17, 129), (250, 3)])
def test_ragged_sizes(R, W, H):
    for sc in ("T", "O"):
        setup(R, sc, POSES["P2"], 128)
        img, st = hip(R, W, H)
        o, ev = ref(sc, W, H, POSES["P2"], 128)
        s = diff_stats(img, o)
        assert s["f1e2"] >= 0.99 or W * H < 100 and s["max"] < 5e-2, s
        check_evals(st, ev, tol=2e-2)


def test_u_resolution_independent_of_target(torch_cuda):
    """uv uses u_resolution (output_shader.frag:390); gl_TexCoord uses the target."""
    r = rm.Renderer(0)  # own context: u_resolution stays set on a context
    setup(r, "T", POSES["P0"], 128, res=(1600.0, 900.0))
    img, _ = hip(r, 96, 96)
    o, _ = ref("T", 96, 96, POSES["P0"], 128, res=(1600.0, 900.0))
    assert_parity("T", img, o)
    r.close()


# ------------------------------------------------------ sharding / frames


@pytest.mark.parametrize("W,H,band,n", [(64, 48, 16, 2), (64, 50, 7, 3), (96, 64, 16, 8), (40, 33, 1, 5)])
def test_bands_and_deinterleave_reassemble_the_frame(R, torch_cuda, W, H, band, n):
    torch = torch_cuda
    from raymarching_amd.frame import ShardPlan
    setup(R, "O", POSES["P1"], 128)
    R.set_params(count_evals=0)
    full = R.render(W, H)
    plan = ShardPlan(W, H, band, n)
    rps = plan.rows_per_shard
    g = torch.zeros((n, rps, W, 4), dtype=torch.float32, device="cuda")
    for s in range(n):
        cnt = rm.shard_rows(H, band, n, s)
        assert cnt == plan.count(s) == len(plan.rows(s))
        R.render_band(W, H, band, n, s, out=g[s, :cnt])
        # a band holds exactly the frame rows of that shard, bit for bit
        assert torch.equal(g[s, :cnt], full[plan.rows(s)])
    frame = R.deinterleave(W, H, band, n, rps, g)
    torch.cuda.synchronize()
    assert torch.equal(frame, full)
    # RGBA8 frames de-interleave the same way
    g8 = torch.zeros((n, rps, W), dtype=torch.int32, device="cuda")
    for s in range(n):
        R.pack_rgba8(g[s], out=g8[s])
    f8 = R.deinterleave(W, H, band, n, rps, g8)
    assert torch.equal(f8, R.pack_rgba8(full))


def test_pack_rgba8_rounding(R, torch_cuda):
    torch = torch_cuda
    x = torch.tensor([[0.0, 1.0, 0.5, 1.0], [-1.0, 2.0, 0.25, 0.998], [float("nan"), 0.00196, 0.00197, 1.0]],
                     device="cuda")
    p = R.pack_rgba8(x).cpu().numpy().view(np.uint32)
    b = [[(int(v) >> (8 * c)) & 255 for c in range(4)] for v in p]
    assert b[0] == [0, 255, 128, 255]
    assert b[1] == [0, 255, 64, 254]
    assert b[2] == [0, 0, 1, 255]


def test_render_rgba8_matches_pack(R, torch_cuda):
    setup(R, "T", POSES["P3"], 128)
    full = R.render(80, 60)
    a = R.render_rgba8(80, 60)
    assert torch_cuda.equal(a, R.pack_rgba8(full))
    host = np.zeros((60, 80), np.uint32)
    st = rm.lib().rm_render_rgba8(R._ctx, 80, 60, R._ptr(host), None)
    assert st == 0
    np.testing.assert_array_equal(host.view(np.int32), a.cpu().numpy())


@pytest.mark.parametrize("scene", ["S0", "T", "O", "OG"])
def test_fused_rgba8_epilogue_bit_exact(R, torch_cuda, scene):
    """The RGBA8 kernels (packing in the epilogue) equal rm_render + rm_pack_rgba8
    bit for bit, for whole frames, bands and row sub-ranges, in every tiling,
    and count the same ray-steps and FLOP."""
    torch = torch_cuda
    setup(R, scene, S0_POSE if scene == "S0" else POSES["P3"], 128)
    W, H, band, n = 77, 45, 4, 3
    full, sf = R.render(W, H, stats=True)
    packed = R.pack_rgba8(full)
    for k in ("tile8", "tile16", "tile16x4", "persist"):
        R.set_params(kernel=k)
        a, sa = R.render_rgba8(W, H, stats=True)
        assert torch.equal(a, packed), k
        assert (sa["evals"], sa["flop"]) == (sf["evals"], sf["flop"])
    R.set_params(kernel="auto")
    from raymarching_amd.frame import ShardPlan
    plan = ShardPlan(W, H, band, n)
    for s in range(n):
        b = R.render_band_rgba8(W, H, band, n, s)
        assert torch.equal(b, packed[plan.rows(s)])
        part = torch.zeros_like(b)
        c = b.shape[0]
        R.render_rows(W, H, band, n, s, 0, c // 2, part[: c // 2])
        R.render_rows(W, H, band, n, s, c // 2, c - c // 2, part[c // 2:])
        assert torch.equal(part, b)


def test_host_output_buffer(R, torch_cuda):
    setup(R, "T", POSES["P0"], 128)
    dev = R.render(48, 32).cpu().numpy()
    host = np.zeros((32, 48, 4), np.float32)
    st = rm.lib().rm_render(R._ctx, 48, 32, R._ptr(host), None)
    assert st == 0
    np.testing.assert_array_equal(host, dev)


def test_deterministic(R, torch_cuda):
    setup(R, "O", POSES["P4"], 128)
    a = R.render(128, 72)
    b = R.render(128, 72)
    assert torch_cuda.equal(a, b)


def test_workgroup_tilings_agree(R, torch_cuda):
    """The 16x16-, 8x8- and 16x4-pixel workgroup launches compute the same pixels."""
    for sc in ("S0", "T", "O"):
        setup(R, sc, POSES["P5"] if sc != "S0" else S0_POSE, 128, kernel="tile16")
        a, sa = R.render(99, 83, stats=True)
        for k in ("tile8", "tile16x4"):
            R.set_params(kernel=k)
            b, sb = R.render(99, 83, stats=True)
            assert torch_cuda.equal(a, b), (sc, k)
            assert sa["evals"] == sb["evals"]
        R.set_params(kernel="auto")


# --------------------------------------------------- the reference surface


def test_shader_loader_surface(torch_cuda, tmp_path, capsys):
    sh = rm.Shader(0)
    assert rm.ShaderLoader.loadFromFile("output_shader.frag", rm.Shader.Fragment, sh)
    sh.setUniform("u_resolution", (64.0, 48.0))
    sh.setUniform("u_pos", (2.0, 3.0, 3.0))
    sh.setUniform("u_mouse", (0.0, 0.0))
    sh.setUniform("u_time", 0.0)
    sh.setUniform("u_sample_part", 1.0)     # declared, unused (common.frag:9)
    sh.setUniform("u_seed1", (1.0, 2.0))
    sh.setUniform("u_not_there", 1.0)       # warns once, ignored
    tex = rm.RenderTexture()
    tex.create(64, 48)
    tex.draw(sh)
    o, _ = ref("O", 64, 48, POSES["P0"], 128)
    assert_parity("O", tex.getTexture().cpu().numpy(), o)
    # missing file: false + the reference's message (source/shader_loader.cpp:28)
    assert not rm.ShaderLoader.loadFromFile(str(tmp_path / "nope.frag"), rm.Shader.Fragment, sh)
    err = capsys.readouterr().err
    assert "can't load file" in err
    # an existing file whose #include is missing fails like the reference
    f = tmp_path / "template.frag"
    f.write_text('#include "does_not_exist.frag"\nvoid main() {}\n')
    assert not rm.ShaderLoader.loadFromFile(str(f), rm.Shader.Fragment, sh)
    # an existing file of a registered name whose text is not the reference's
    # is refused (only output_shader.frag's scene part may be redefined), and
    # the previous scene stays loaded
    (tmp_path / "common.frag").write_text("// library\n")
    f.write_text('#include <' + str(tmp_path / "common.frag") + '>\n// scene T\n')
    assert not rm.ShaderLoader.loadFromFile(str(f), rm.Shader.Fragment, sh)
    assert "not the reference's template.frag" in capsys.readouterr().err
    fo = tmp_path / "output_shader.frag"
    fo.write_text('#include "' + str(tmp_path / "common.frag") + '"\nSdResult sceneSDF(vec3 p) { return r; }\nvoid main() {}\n')
    assert not rm.ShaderLoader.loadFromFile(str(fo), rm.Shader.Fragment, sh)
    tex.draw(sh)
    assert_parity("O", tex.getTexture().cpu().numpy(), o)  # scene O still loaded
    # an unknown scene file exists but has no HIP plugin
    u = tmp_path / "other.frag"
    u.write_text("void main() {}\n")
    assert not rm.ShaderLoader.loadFromFile(str(u), rm.Shader.Fragment, sh)
    sh.close()


def test_errors(torch_cuda):
    r = rm.Renderer(0)
    with pytest.raises(rm.RmError) as e:
        r.render(8, 8)
    assert e.value.status == 4  # RM_ERR_NO_SCENE
    r.load_scene("template.frag")
    with pytest.raises(rm.RmError) as e:
        r.set_uniform("u_pos", 1.0, 2.0)
    assert e.value.status == 1
    with pytest.raises(rm.RmError):
        r.set_params(max_steps=-1)
    with pytest.raises(rm.RmError):
        r.render_band(8, 8, 4, 2, 2)
    with pytest.raises(ValueError):
        r.render(8, 8, out=torch_cuda.empty(10, device="cuda"))
    r.close()


# ---------------------------------------------------------- full sizes


def full_size_parity(r, scene, W, H, pose, steps, rows, col_block=None):
    """Image and per-pixel ray-step map of a full-size frame (rm_render_step_map)
    against the oracle on the given rows and, optionally, a column-strided block
    (cols, rows): the image per the full-size policy (tests/parity.py
    FULL_SIZE_POLICY: >= 99.99 % of pixels within 2e-3), step maps exact on
    >= 99.8 % (T) / 99.99 % (O) of pixels (FULL_SIZE_STEP_MAP; SURVEY.md 8(c)
    asks 95 %), the map's sum equal to the launch's count.  Returns (pixels
    checked, [parity stats], step-map exact fraction); with RM_PARITY_LOG set
    the figures are appended to that file as a JSON line."""
    torch = pytest.importorskip("torch")
    setup(r, scene, pose, steps)
    img, evmap, st = r.render_step_map(W, H)
    assert int(evmap.sum(dtype=torch.int64)) == st["evals"]
    kw = dict(pos=pose["pos"], mouse=pose["mouse"], time=pose["time"], max_steps=steps)
    rows = np.asarray(rows, np.int32)
    ri = torch.from_numpy(rows.astype(np.int64)).to(img.device)
    o, ev = oracle.render_rows(scene, W, H, rows, **kw)
    pol = FULL_SIZE_POLICY[scene]
    stats = [assert_parity(scene, img[ri].cpu().numpy(), o, policy=pol, label=f"{W}x{H} {len(rows)} rows")]
    match, n = int(np.sum(evmap[ri].cpu().numpy() == ev)), ev.size
    if col_block is not None:
        cols, brows = (np.asarray(a, np.int32) for a in col_block)
        xs, ys = np.meshgrid(cols, brows)
        o2, ev2 = oracle.render_pixels(scene, W, H, xs, ys, **kw)
        xi = torch.from_numpy(xs.ravel().astype(np.int64)).to(img.device)
        yi = torch.from_numpy(ys.ravel().astype(np.int64)).to(img.device)
        stats.append(assert_parity(scene, img[yi, xi].cpu().numpy(), o2, policy=pol,
                                   label=f"{W}x{H} {len(cols)} cols x {len(brows)} rows"))
        match += int(np.sum(evmap[yi, xi].cpu().numpy() == ev2))
        n += ev2.size
    exact = match / n
    print(f"{scene} {W}x{H} {steps} steps: {n} px, {stats}, step map exact {exact:.5f}")
    if os.environ.get("RM_PARITY_LOG"):
        with open(os.environ["RM_PARITY_LOG"], "a") as fh:
            fh.write(json.dumps(dict(scene=scene, W=W, H=H, steps=steps, pose=pose, pixels=n, stats=stats,
                                     step_map_exact=exact)) + "\n")
    assert exact >= FULL_SIZE_STEP_MAP[scene], (exact, FULL_SIZE_STEP_MAP[scene])
    timed_path_equals_instrumented(r, scene, W, H, img)
    return n, stats, exact


def timed_path_equals_instrumented(r, scene, W, H, img, launches=10):
    """The kernels bench.py times (count_evals=0: the settled-shadow,
    back-face and depth-3 reflection exits) against the
    instrumented frame `img` (every reference ray-step; the frame the oracle
    checks), bit for bit over the whole frame: float4 row-major
    (schedule=0), then RGBA8 as bench renders it -- adaptive order
    after `launches` launches, so a sorted order and, in scene T, the latency
    tiles (2.8) are in effect -- and float4 in that order.  NaN pixels (OG)
    compare by their bits.  References: common.frag:810-831 (soft shadow),
    :931-954 and :991-1002 (castRay in getColorReflect); template.frag:45-76."""
    torch = pytest.importorskip("torch")
    r.set_params(count_evals=0, schedule=0)
    ref_bits = img.view(torch.int32)
    f, st = r.render(W, H, stats=True)
    assert st["dispatch"] == "row-major", st
    assert torch.equal(f.view(torch.int32), ref_bits), f"{scene} {W}x{H}: timed float4 (row-major) != instrumented"
    del f
    r.set_params(schedule=1)
    ref8 = r.pack_rgba8(img)
    out8 = torch.empty((H, W), dtype=torch.int32, device=img.device)
    for _ in range(launches):
        r.render_rgba8(W, H, out=out8)
    _, st8 = r.render_rgba8(W, H, out=out8, stats=True)
    assert st8["dispatch"] == "adaptive", st8
    ntiles = ((W + 7) // 8) * ((H + 7) // 8)
    if scene == "T":  # (latency tiles only in launches of <= 98304 tiles: rm_render_host.cpp lat_tiles_for)
        assert st8["lat_tiles"] == (min(2048, ntiles) if ntiles <= 98304 else 0), st8
    else:
        assert st8["lat_tiles"] == 0, st8
    n8 = int((out8 != ref8).sum())
    assert n8 == 0, f"{scene} {W}x{H}: {n8} RGBA8 pixels of the timed, ordered frame differ from the instrumented frame"
    f, st = r.render(W, H, stats=True)
    assert st["dispatch"] == "adaptive", st
    assert torch.equal(f.view(torch.int32), ref_bits), f"{scene} {W}x{H}: timed float4 (ordered) != instrumented"
    print(f"{scene} {W}x{H}: timed kernel == instrumented frame (float4 row-major and ordered, RGBA8 ordered with "
          f"{st8['lat_tiles']} latency tiles), {st8['kernel_ms']:.3f} ms")
    r.set_params(count_evals=1)


def test_c2_1080p_poses(R, torch_cuda):
    """Config C2 (1920x1080 scene T, 128 steps) at three poses: every pixel's
    colour and ray-step count against the oracle (2.07 M pixels per pose)."""
    for p in ("P0", "P3", "P8"):
        n, _, _ = full_size_parity(R, "T", 1920, 1080, POSES[p], 128, np.arange(1080))
        assert n >= 1_000_000


def test_c3_4096_properties(R, torch_cuda):
    """Config C3 (4096^2 scene T, 256 steps): the whole frame's colours and
    per-pixel ray-step map against the oracle (16.8 M pixels), plus
    determinism and exact reassembly from 8 row-interleaved shards (C4)."""
    torch = torch_cuda
    n, _, _ = full_size_parity(R, "T", 4096, 4096, POSES["P0"], 256, np.arange(4096))
    assert n == 4096 * 4096
    R.set_params(count_evals=0)
    img = R.render(4096, 4096)
    from raymarching_amd.frame import ShardPlan
    plan = ShardPlan(4096, 4096, 16, 8)
    g = torch.empty((8, plan.rows_per_shard, 4096, 4), dtype=torch.float32, device="cuda")
    for sh in range(8):
        R.render_band(4096, 4096, 16, 8, sh, out=g[sh])
    frame = R.deinterleave(4096, 4096, 16, 8, plan.rows_per_shard, g)
    assert torch.equal(frame, img)
    assert torch.isfinite(img).all()
    assert torch.all(img[..., 3] == 1.0)
    assert torch.equal(R.render(4096, 4096), img)
    # the balanced multi-GPU splits bench.py can choose: every
    # part through the timed RGBA8 kernel in adaptive order (after repeated
    # launches), the RGB8 wire back to back, rm_deinterleave_cycle_rgb8
    ref8 = R.pack_rgba8(img)
    R.set_params(schedule=1)
    for runs in ((25, 16), (15,) + (16,) * 7):
        wplan = ShardPlan(4096, 4096, 16, len(runs), runs)
        wire = torch.empty((4096, 3 * 4096), dtype=torch.uint8, device="cuda")
        base = wplan.part_bases()
        for s in range(len(runs)):
            n = wplan.count(s)
            loc = torch.empty((n, 4096), dtype=torch.int32, device="cuda")
            for _ in range(10):
                R.render_cycle_rows(4096, 4096, wplan.cycle, wplan.offsets[s], runs[s], 0, n, loc)
            _, st = R.render_cycle_rows(4096, 4096, wplan.cycle, wplan.offsets[s], runs[s], 0, n, loc, stats=True)
            assert st["dispatch"] == "adaptive", st
            R.pack_rgb8(loc, out=wire[base[s]: base[s] + n])
        frame8 = R.deinterleave_cycle_rgb8(4096, 4096, wplan.cycle, list(wplan.offsets), list(runs),
                                           [b * 3 * 4096 for b in base], wire)
        assert torch.equal(frame8, ref8), runs


def test_c5_8192_scene_O(R, torch_cuda):
    """Config C5's frame (8192^2 scene O, 512 steps): every 8th row (offset 3)
    and every 64th column (offset 5) over the full height, colours and
    per-pixel ray-step counts against the oracle (9.4 M pixels)."""
    n, _, _ = full_size_parity(R, "O", 8192, 8192, POSES["P0"], 512, np.arange(3, 8192, 8),
                               col_block=(np.arange(5, 8192, 64), np.arange(8192)))
    assert n >= 1_000_000


def test_headless_cpp_host_app(tmp_path, torch_cuda):
    """apps/raymarch_headless (main.cpp's frame loop over include/rm_pass.hpp):
    the scripted camera walk ends where main.cpp:153-171 puts it, and the last
    frame matches the oracle at that pose (RGBA8, time frozen at 0)."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(__file__)), "apps", "raymarch_headless")
    ppm = tmp_path / "f.ppm"
    out = subprocess.run([exe, "--scene", "template.frag", "--w", "96", "--h", "54", "--frames", "6", "--script",
                          "WWDDU.", "--time-freeze", "--ppm", str(ppm)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    # W,W,D,D,Up then idle with the mouse centred: x += 0.2, y += 0.1, z -= 0.2
    np.testing.assert_allclose(info["pos"], [2.2, 3.1, 2.8], atol=1e-4)
    data = ppm.read_bytes()
    hdr_end = data.index(b"255\n") + 4
    img = np.frombuffer(data[hdr_end:], np.uint8).reshape(54, 96, 3).astype(np.float32) / 255.0
    pos = [np.float32(v) for v in info["pos"]]
    o, _ = oracle.render("T", 96, 54, pos=pos, mouse=(0.0, 0.0), time=0.0, max_steps=128, res=(96.0, 54.0))
    ref8 = np.clip(np.rint(np.clip(o[..., :3], 0, 1) * 255.0), 0, 255) / 255.0
    d = np.abs(img - ref8).max(-1)
    assert np.mean(d <= 2.0 / 255.0) >= 0.99, float(np.mean(d <= 2.0 / 255.0))


def test_headless_cpp_host_app_sharded_path(tmp_path, torch_cuda):
    """apps/raymarch_headless --sharded: the frame through rm::ShardedRenderTexture
    (rm_comm_init_all + rm_render_sharded_all, RGB8 wire) on one GPU equals the
    plain RenderTexture path's RGBA8 frame byte for byte."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(__file__)), "apps", "raymarch_headless")
    imgs = []
    for extra in ([], ["--sharded", "--band", "8"]):
        ppm = tmp_path / f"f{len(imgs)}.ppm"
        out = subprocess.run([exe, "--scene", "output_shader.frag", "--w", "80", "--h", "45", "--frames", "3",
                              "--script", "WD.", "--time-freeze", "--ppm", str(ppm)] + extra,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        imgs.append(ppm.read_bytes())
    assert imgs[0] == imgs[1]


def test_headless_cpp_host_app_formats_and_stats(tmp_path, torch_cuda):
    """rm::RenderTexture's RGBA8 target (rm_render_rgba8, the default) and its
    RGBA32F target packed on copy give the same bytes; --stats adds the per-frame
    kernel time, without it the frames are queued with no per-frame sync."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(__file__)), "apps", "raymarch_headless")
    imgs, infos = [], []
    for extra in (["--format", "rgba8"], ["--format", "float", "--stats"], ["--warmup", "2"]):
        ppm = tmp_path / f"f{len(imgs)}.ppm"
        out = subprocess.run([exe, "--scene", "output_shader.frag", "--w", "100", "--h", "60", "--frames", "4",
                              "--script", "WD..", "--time-freeze", "--ppm", str(ppm)] + extra,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        infos.append(json.loads(out.stdout.strip().splitlines()[-1]))
        imgs.append(ppm.read_bytes())
    assert imgs[0] == imgs[1]
    assert infos[0]["format"] == "rgba8" and infos[1]["format"] == "float"
    assert "kernel_ms_per_frame" not in infos[0] and infos[1]["kernel_ms_per_frame"] > 0
    assert infos[2]["warmup"] == 2 and infos[2]["frames"] == 4 and infos[2]["fps_wall"] > 0


def test_render_rows_chunks_and_frame_pipeline(R, torch_cuda):
    """rm_render_rows sub-ranges reassemble the band exactly; the chunked
    single-rank DistributedFrame equals rm_render_rgba8."""
    torch = torch_cuda
    from raymarching_amd.frame import DistributedFrame
    setup(R, "T", POSES["P6"], 128)
    R.set_params(count_evals=0)
    W, H, band, n, s = 72, 61, 5, 3, 1
    full = R.render_band(W, H, band, n, s)
    cnt = full.shape[0]
    part = torch.empty_like(full)
    for j0, j1 in ((0, 7), (7, 8), (8, cnt)):
        R.render_rows(W, H, band, n, s, j0, j1 - j0, part[j0:j1])
    assert torch.equal(part, full)
    with pytest.raises(rm.RmError):
        R.render_rows(W, H, band, n, s, cnt - 1, 2, part)
    fr = DistributedFrame(R, 80, 48, 16, 0, 1, fmt="rgba8", chunks=5)
    frame = fr.render()
    assert torch.equal(frame, R.render_rgba8(80, 48))


@pytest.mark.parametrize("W,H,band,n", [(64, 48, 16, 2), (61, 50, 7, 3), (96, 64, 16, 8)])
def test_rgb8_wire_reassembles_the_rgba8_frame(R, torch_cuda, W, H, band, n):
    """rm_pack_rgb8 + rm_deinterleave_rgb8 (the 3 B/px wire) give the frame
    rm_render_rgba8 gives, bit for bit; W % 4 != 0 takes the byte path."""
    torch = torch_cuda
    from raymarching_amd.frame import ShardPlan
    setup(R, "T", POSES["P3"], 128)
    R.set_params(count_evals=0)
    full = R.render_rgba8(W, H)
    plan = ShardPlan(W, H, band, n)
    rps = plan.rows_per_shard
    g = torch.zeros((n, rps, 3 * W), dtype=torch.uint8, device="cuda")
    for s in range(n):
        cnt = plan.count(s)
        b = R.render_band_rgba8(W, H, band, n, s)
        R.pack_rgb8(b, out=g[s, :cnt])
        # the wire holds the RGB bytes of the band in pixel order
        ref = b.cpu().numpy().view(np.uint8).reshape(cnt, W, 4)[..., :3].reshape(cnt, 3 * W)
        assert np.array_equal(g[s, :cnt].cpu().numpy(), ref)
    frame = R.deinterleave(W, H, band, n, rps, g)
    torch.cuda.synchronize()
    assert torch.equal(frame, full)
    assert (frame.cpu().numpy().view(np.uint8).reshape(H, W, 4)[..., 3] == 255).all()


def test_rgb8_pack_misaligned_and_ragged(R, torch_cuda):
    """Unaligned sub-ranges (byte path) pack the same bytes as aligned ones."""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    src = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, 1031, dtype=np.int64).astype(np.int32)).cuda()
    ref = src.cpu().numpy().view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1)
    out = torch.zeros(3 * 1031 + 8, dtype=torch.uint8, device="cuda")
    R.pack_rgb8(src, out=out[:3 * 1031])
    assert np.array_equal(out[:3 * 1031].cpu().numpy(), ref)
    R.pack_rgb8(src[1:], out=out[1:1 + 3 * 1030])
    torch.cuda.synchronize()
    assert np.array_equal(out[1:1 + 3 * 1030].cpu().numpy(), ref[3:])


def _frame_worker(rank, world, port, q):
    import os as _os

    import torch
    import torch.distributed as dist

    from raymarching_amd.frame import DistributedFrame
    _os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    r = rm.Renderer(0)
    setup(r, "T", POSES["P0"], 128)
    r.set_params(count_evals=0)
    fr = DistributedFrame(r, 96, 70, 8, rank, world, fmt="rgba8", chunks=2)
    assert fr.wire == "rgb8"
    for _ in range(2):
        fr.submit()
    frame = fr.flush()
    if rank == 0:
        torch.cuda.synchronize()
        q.put(frame.cpu().numpy())
    dist.barrier()
    r.close()
    dist.destroy_process_group()


def test_distributed_frame_two_ranks_on_one_gpu(R, torch_cuda):
    """Two ranks (gloo, both on cuda:0) through DistributedFrame's RGB8 wire:
    rank 0's frame equals a one-rank rm_render_rgba8 frame."""
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_frame_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    frame = q.get(timeout=100)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    setup(R, "T", POSES["P0"], 128)
    R.set_params(count_evals=0)
    ref = R.render_rgba8(96, 70).cpu().numpy()
    assert np.array_equal(frame, ref)


class _Work:
    """A torch.distributed work of the in-process two-rank tests: wait() makes
    the caller's stream wait for the transfer (`ev`, or the "done" event the
    receiving side leaves in the `entry` both sides share)."""

    def __init__(self, ev=None, entry=None):
        self.ev, self.entry = ev, entry

    def wait(self):
        import torch
        ev = self.ev if self.ev is not None else (self.entry or {}).get("done")
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)


_PAIR_W, _PAIR_H, _PAIR_BAND = 96, 70, 8


def _pair_as_nccl(cls, R, r1, **kw):
    """A frame of class `cls` for each of two ranks living in this process
    (rank 0 on R, rank 1 on r1), made as with the "nccl" backend: the RCCL
    path (pipelined, two frame streams) is taken at construction."""
    frs = []
    for rank, rr in ((0, R), (1, r1)):
        f = cls.__new__(cls)
        f._pipelined = lambda: True  # as with the "nccl" backend
        cls.__init__(f, rr, _PAIR_W, _PAIR_H, _PAIR_BAND, rank, 2, **kw)
        frs.append(f)
    return frs


def _pair_frames_equal_one_rank(torch, frs, R, r1):
    """Four poses submitted through both ranks (rank 1 first), pipelined: every
    frame rank 0 ends up with equals the one-rank rm_render_rgba8 frame."""
    poses = ["P0", "P1", "P2", "P3"]
    refs = []
    for name in poses:
        setup(R, "T", POSES[name], 128)
        R.set_params(count_evals=0)
        refs.append(R.render_rgba8(_PAIR_W, _PAIR_H).cpu().numpy())
    got = []
    for i, name in enumerate(poses):
        for f, rr in ((frs[1], r1), (frs[0], R)):
            setup(rr, "T", POSES[name], 128)
            rr.set_params(count_evals=0)
            f.submit()
        if i > 0:  # frame i-1 is complete on rank 0 once frame i was submitted
            torch.cuda.synchronize()
            got.append(frs[0].frame.cpu().numpy())
    frs[1].flush()
    got.append(frs[0].flush().cpu().numpy())
    torch.cuda.synchronize()
    assert len(got) == len(refs)
    for g, ref in zip(got, refs):
        assert np.array_equal(g, ref)


@pytest.mark.parametrize("runs", [None, (13, 8), (3, 8)])
def test_pipelined_two_stream_frames_in_one_process(R, torch_cuda, runs):
    """DistributedFrame's RCCL path (pipelined gathers, two HIP streams, per-slot
    buffers) for two ranks living in one process, with the gather replaced by
    device copies on a side stream that honour the same stream semantics as
    ProcessGroupNCCL (wait on the caller's stream, work.wait() makes the
    caller's stream wait).  Every frame of a pose sequence must equal the
    one-rank rm_render_rgba8 frame.  runs: round-robin bands (None) or weighted
    cyclic parts (rank 0 renders a longer / shorter run of every cycle; the
    unpadded point-to-point gather and rm_deinterleave_cycle_rgb8)."""
    torch = torch_cuda
    from raymarching_amd.frame import DistributedFrame
    side = torch.cuda.Stream()
    sent = {}

    def fake_gather(fr):
        def gather(slot, c):
            cuts = fr.cuts
            j0, j1 = (0, fr.nmine if fr.plan.weighted else fr.plan.rows_per_shard) if c is None else (cuts[c], cuts[c + 1])
            ev = torch.cuda.Event()
            ev.record()  # the caller's (frame) stream
            if fr.rank == 1:
                sent[(fr.k, c)] = (fr.wires[slot][j0:j1], ev)
                return [_Work()]
            src1, ev1 = sent.pop((fr.k, c))
            side.wait_event(ev)
            side.wait_event(ev1)
            with torch.cuda.stream(side):
                if fr.plan.weighted:  # rank 0's rows are in place; rank 1's chunk c lands after them
                    b = fr.plan.part_bases()[1]
                    k0, k1 = (0, fr.plan.count(1)) if c is None else (fr.all_cuts[1][c], fr.all_cuts[1][c + 1])
                    fr.gathered[slot][b + k0: b + k1].copy_(src1)
                else:
                    fr.gathered[slot][0, j0:j1].copy_(fr.wires[slot][j0:j1])
                    fr.gathered[slot][1, j0:j1].copy_(src1)
            done = torch.cuda.Event()
            done.record(side)
            return [_Work(done)]
        return gather

    r1 = rm.Renderer(0)
    frs = _pair_as_nccl(DistributedFrame, R, r1, fmt="rgba8", chunks=2, runs=runs)
    for f in frs:
        f._gather_async = fake_gather(f)
    assert len(frs[0].streams) == 2 and frs[0].wire == "rgb8"
    _pair_frames_equal_one_rank(torch, frs, R, r1)
    r1.close()


def test_single_rank_two_streams(R, torch_cuda):
    torch = torch_cuda
    from raymarching_amd.frame import DistributedFrame
    setup(R, "T", POSES["P4"], 128)
    R.set_params(count_evals=0)
    ref = R.render_rgba8(80, 48)
    fr = DistributedFrame(R, 80, 48, 16, 0, 1, fmt="rgba8", streams=2)
    for _ in range(3):
        fr.submit()
    frame = fr.flush()
    torch.cuda.synchronize()
    assert torch.equal(frame, ref)


@pytest.mark.parametrize("scene", ["T", "O"])
def test_adaptive_dispatch_order_keeps_pixels(R, torch_cuda, scene):
    """rm_params.schedule = 1: from the second launch of a geometry on, the
    tiles run costliest first (the previous launch's durations); every launch
    writes the frame the row-major order writes, bit for bit, in every output
    form (float4, RGBA8, bands, instrumented)."""
    torch = torch_cuda
    setup(R, scene, POSES["P3"], 128)
    R.set_params(count_evals=0, schedule=0)
    W, H = 200, 120
    ref_f = R.render(W, H)
    ref8 = R.render_rgba8(W, H)
    R.set_params(schedule=1)
    # every ordered launch writes into a target that holds a word no kernel
    # writes (tests/sentinel.py): a fresh torch.empty would be the block the
    # previous iteration freed, with the right frame already in it
    def f4():
        return sentinel.target(torch, (H, W, 4), torch.float32)

    def w8(rows=H):
        return sentinel.target(torch, (rows, W), torch.int32)

    for _ in range(3):
        a = R.render(W, H, out=f4())
        sentinel.assert_frame(a, ref_f)
        assert torch.equal(a, ref_f)
        a = R.render_rgba8(W, H, out=w8())
        sentinel.assert_frame(a, ref8)
        assert torch.equal(a, ref8)
    band = R.render_band_rgba8(W, H, 8, 3, 1, out=w8(rm.shard_rows(H, 8, 3, 1)))
    sentinel.assert_frame(band, ref8[[y for y in range(H) if (y // 8) % 3 == 1]])
    for _ in range(2):
        a = R.render_band_rgba8(W, H, 8, 3, 1, out=w8(band.shape[0]))
        sentinel.assert_frame(a, band)
        assert torch.equal(a, band)
    R.set_params(count_evals=1)
    a, sa = R.render(W, H, out=f4(), stats=True)
    b, sb = R.render(W, H, out=f4(), stats=True)
    sentinel.assert_frame(a, ref_f)
    sentinel.assert_frame(b, ref_f)
    assert torch.equal(a, ref_f) and torch.equal(b, ref_f) and sa["evals"] == sb["evals"]
    # an explicit order takes precedence; a wrong size is ignored
    tx, ty = R.tile_grid(W, H)
    R.set_tile_order(np.arange(tx * ty, dtype=np.uint32)[::-1].copy())
    a = R.render(W, H, out=f4())
    sentinel.assert_frame(a, ref_f)
    assert torch.equal(a, ref_f)
    assert torch.equal(R.render(W + 8, H)[:, :W], R.render(W + 8, H)[:, :W])
    with pytest.raises(rm.RmError):
        R.set_tile_order(np.zeros(tx * ty, np.uint32))  # not a permutation
    R.set_tile_order(None)
    R.set_params(schedule=1)


def test_latency_tiles_keep_pixels(R, torch_cuda):
    """Scene T: the first 2048 workgroups of an ordered launch
    render with one Menger fold exit test instead of three.  A 512x320 frame
    (2560 tiles) mixes both kinds; every ordered launch writes the row-major
    frame bit for bit, and the ray-step count is unchanged."""
    torch = torch_cuda
    setup(R, "T", POSES["P1"], 128)
    W, H = 512, 320
    R.set_params(count_evals=1, schedule=0)
    ref, st = R.render_rgba8(W, H, stats=True)
    R.set_params(count_evals=0, schedule=1)
    for _ in range(4):
        a = R.render_rgba8(W, H, out=sentinel.target(torch, (H, W), torch.int32))
        sentinel.assert_frame(a, ref)
        assert torch.equal(a, ref)
    R.set_params(count_evals=1)
    a, sa = R.render_rgba8(W, H, out=sentinel.target(torch, (H, W), torch.int32), stats=True)
    sentinel.assert_frame(a, ref)
    assert torch.equal(a, ref) and sa["evals"] == st["evals"]
    R.set_params(count_evals=0)


@pytest.mark.parametrize("scene", ["T", "O"])
def test_persistent_waves_equal_hardware_dispatch(R, torch_cuda, scene):
    """KERNEL_PERSIST (persistent waves pulling tiles from an atomic counter):
    the frame of the hardware-dispatched kernel bit for bit, over repeated
    launches (the counters reset themselves), with the adaptive order, on two
    streams, and for shards whose tile count is below the resident-wave count."""
    torch = torch_cuda
    setup(R, scene, POSES["P1"], 128)
    R.set_params(count_evals=0, kernel="tile8")
    W, H = 200, 136
    # (the references too may be ordered launches, the context's schedule being what the tests before left:
    # into sentinel targets, no word of which may remain)
    ref = R.render_rgba8(W, H, out=sentinel.target(torch, (H, W), torch.int32))
    band = R.render_band_rgba8(W, H, 8, 3, 1, out=sentinel.target(torch, (rm.shard_rows(H, 8, 3, 1), W), torch.int32))
    assert int((ref == sentinel.RGBA8_WORD).sum()) == 0
    sentinel.assert_frame(band, ref[[y for y in range(H) if (y // 8) % 3 == 1]], "the reference row part")
    R.set_params(kernel="persist")
    s2 = torch.cuda.Stream()
    for i in range(8):
        # (targets filled on the default stream and complete before the launch
        # on s2: torch.full is ordered there, and synchronize() waits for it)
        ta, tb = sentinel.target(torch, (H, W), torch.int32), sentinel.target(torch, tuple(band.shape), torch.int32)
        torch.cuda.synchronize()
        if i % 2:
            R.set_stream(s2)
        a = R.render_rgba8(W, H, out=ta)
        b = R.render_band_rgba8(W, H, 8, 3, 1, out=tb)
        R.set_stream(None)
        torch.cuda.synchronize()
        sentinel.assert_frame(a, ref, f"launch {i}")
        sentinel.assert_frame(b, band, f"launch {i}, the row part")
        assert torch.equal(a, ref), i
        assert torch.equal(b, band), i
    R.set_params(kernel="auto")


@pytest.mark.parametrize("scene,pose", [("T", p) for p in POSES] + [("O", p) for p in POSES] +
                         [("OG", p) for p in ("P0", "P3", "P7")])
def test_settled_soft_shadows_keep_pixels(R, torch_cuda, scene, pose):
    """The timed kernels of scenes T, O and OG leave out the ray-steps that
    cannot change the frame: a soft-shadow march once settled (DESIGN.md 2.11;
    O/OG test the rule every 8th step), scene T's reflection march past depth 3
    (2.12), and the whole soft shadow of a point facing away from the light
    (2.13).  The instrumented kernel takes every reference step and counts the
    ones left out (rm_stats.skipped).  The timed frame (row-major and ordered,
    float4 and RGBA8) equals the instrumented frame bit for bit, the step map
    stays the reference's, and the share of steps left out is the oracle's
    (shadow_settle: after + refl_after + back_steps), within 2 %."""
    torch = torch_cuda
    steps = 128 if scene == "T" else 512
    setup(R, scene, POSES[pose], steps)
    W, H = 192, 108
    R.set_params(schedule=0)
    ref, st = R.render(W, H, stats=True)
    p = POSES[pose]
    o = oracle.shadow_settle(scene, W, H, every=1 if scene == "T" else 8, pos=p["pos"], mouse=p["mouse"],
                             time=p["time"], max_steps=steps)
    o_skip = o["after"] + o["refl_after"] + o["back_steps"]
    assert (st["skipped"] > 0) == (o_skip > 0), (st, o)  # (O at P4 sees no shadow march, at P7 one step each)
    R.set_params(count_evals=0)
    # bit for bit (OG's camera-inside-glass pixels are NaN)
    assert torch.equal(R.render(W, H).view(torch.int32), ref.view(torch.int32))
    R.set_params(schedule=1)
    ref8 = R.pack_rgba8(ref)
    for _ in range(3):
        assert torch.equal(R.render_rgba8(W, H), ref8)
    # (scene T also leaves the reflection march at depth 3, cast_ray_T RS, and
    # both skip the shadow marches of points facing away from the light)
    frac_hip, frac_ref = st["skipped"] / st["evals"], o_skip / st["evals"]
    assert abs(frac_hip - frac_ref) <= 0.02, (frac_hip, frac_ref, st, o)


@pytest.mark.parametrize("W,H,runs", [(96, 70, (13, 8)), (97, 61, (1, 5, 2)), (128, 300, (40, 16, 16, 16))])
def test_weighted_cycle_parts_rebuild_frame(R, torch_cuda, W, H, runs):
    """Weighted cyclic row parts (bench.py --balance auto): each part rendered
    with rm_render_cycle_rows_rgba8 (and the float4 form), packed to the RGB8
    wire back to back, and rm_deinterleave_cycle_rgb8 gives the one-launch
    rm_render_rgba8 frame bit for bit; parts that do not tile the cycle are
    refused."""
    torch = torch_cuda
    from raymarching_amd.frame import ShardPlan
    setup(R, "T", POSES["P1"], 128)
    R.set_params(count_evals=0)
    ref = R.render_rgba8(W, H)
    ref4 = R.render(W, H)
    plan = ShardPlan(W, H, runs[-1], len(runs), runs)
    gathered = torch.empty((H, 3 * W), dtype=torch.uint8, device="cuda")
    base = plan.part_bases()
    for s in range(len(runs)):
        n = plan.count(s)
        loc = torch.empty((n, W), dtype=torch.int32, device="cuda")
        # two calls over a split of the packed rows, as chunked frames do
        h = n // 2
        R.render_cycle_rows(W, H, plan.cycle, plan.offsets[s], runs[s], 0, h, loc)
        R.render_cycle_rows(W, H, plan.cycle, plan.offsets[s], runs[s], h, n - h, loc[h:])
        R.pack_rgb8(loc, out=gathered[base[s]: base[s] + n])
        f4 = torch.empty((n, W, 4), dtype=torch.float32, device="cuda")
        R.render_cycle_rows(W, H, plan.cycle, plan.offsets[s], runs[s], 0, n, f4)
        assert torch.equal(f4, ref4[plan.rows(s)])
    frame = R.deinterleave_cycle_rgb8(W, H, plan.cycle, list(plan.offsets), list(runs),
                                      [b * 3 * W for b in base], gathered)
    torch.cuda.synchronize()
    assert torch.equal(frame, ref)
    with pytest.raises(rm.RmError):  # a gap in [0, cycle)
        R.deinterleave_cycle_rgb8(W, H, plan.cycle + 1, list(plan.offsets), list(runs), [0] * len(runs), gathered)
    with pytest.raises(rm.RmError):
        R.render_cycle_rows(W, H, 4, 3, 2, 0, 1, frame[:1])


@pytest.mark.parametrize("band,n", [(5, 3), (16, 4)])
def test_band_rows_are_cyclic_part_rows(R, torch_cuda, band, n):
    """Round-robin bands are the cyclic part cycle = band * n, offset =
    band * shard, run = band: rm_render_rows[_rgba8] and
    rm_render_cycle_rows[_rgba8] write the same rows, bit for bit, for every
    shard and for a sub-range of one.  40 x 37 with (5, 3): the last cycle is
    partial and shard 1 ends mid-band; with (16, 4): shard 3 is empty, and
    both forms return no rows without touching the buffer."""
    torch = torch_cuda
    from raymarching_amd.frame import ShardPlan
    W, H = 40, 37
    setup(R, "T", POSES["P1"], 128)
    R.set_params(count_evals=0)
    frame = {torch.float32: R.render(W, H), torch.int32: R.render_rgba8(W, H)}
    plan = ShardPlan(W, H, band, n)
    assert [plan.count(s) for s in range(n)] == {(5, 3): [15, 12, 10], (16, 4): [16, 16, 5, 0]}[band, n]

    def both(s, j0, cnt, dtype):
        """Packed rows [j0, j0 + cnt) of shard s through the band and the
        cyclic form, each into a marked buffer with one row to spare."""
        outs = []
        for cyclic in (False, True):
            out = torch.full((cnt + 1, W) + ((4,) if dtype == torch.float32 else ()), -7, dtype=dtype, device="cuda")
            if cyclic:
                R.render_cycle_rows(W, H, band * n, band * s, band, j0, cnt, out)
            else:
                R.render_rows(W, H, band, n, s, j0, cnt, out)
            outs.append(out.view(torch.int32))
        torch.cuda.synchronize()
        return outs

    for dtype in (torch.float32, torch.int32):
        marked = torch.full((1,), -7, dtype=dtype).view(torch.int32).item()
        for s, j0, cnt in [(s, 0, plan.count(s)) for s in range(n)] + [(0, 3, 4)]:
            a, b = both(s, j0, cnt, dtype)
            assert torch.equal(a, b), (dtype, s, j0, cnt)
            assert torch.equal(a[:cnt], frame[dtype][plan.rows(s)[j0: j0 + cnt]].view(torch.int32)), (dtype, s)
            assert (a[cnt:] == marked).all(), (dtype, s)  # nothing past the rows asked for


def _delta_worker(rank, world, port, runs, q):
    import os as _os

    import torch
    import torch.distributed as dist

    from raymarching_amd.frame import DeltaFrame
    _os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    r = rm.Renderer(0)
    setup(r, "T", POSES["P0"], 128)
    r.set_params(count_evals=0)
    fr = DeltaFrame(r, 96, 70, 8, rank, world, runs=runs)
    for _ in range(3):
        fr.submit()
    frame = fr.flush()
    x = fr.timed_exchange()
    if rank == 0:
        torch.cuda.synchronize()
        q.put((frame.cpu().numpy(), fr.frame.cpu().numpy(), x["wire_bytes"]))
    dist.barrier()
    r.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("runs", [None, (13, 8)])
def test_compressed_wire_frame_two_ranks_on_one_gpu(R, torch_cuda, runs):
    """DeltaFrame over gloo (two ranks on cuda:0): the compressed wire's frame
    equals a one-rank rm_render_rgba8 frame, after pipelined submits and after
    the timed exchange."""
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_delta_worker, args=(r, 2, port, runs, q)) for r in range(2)]
    for p in procs:
        p.start()
    frame, frame2, sizes = q.get(timeout=100)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    setup(R, "T", POSES["P0"], 128)
    R.set_params(count_evals=0)
    ref = R.render_rgba8(96, 70).cpu().numpy()
    assert np.array_equal(frame, ref) and np.array_equal(frame2, ref)
    assert sizes[0] == 0 and sizes[1] > 0


@pytest.mark.parametrize("runs", [None, (13, 8)])
def test_compressed_wire_pipelined_in_one_process(R, torch_cuda, runs):
    """DeltaFrame's RCCL path (size exchange, messages posted on a control
    stream, two frame streams, per-slot buffers) for two ranks in one process,
    with the exchange replaced by device copies on a side stream under the same
    stream semantics: every frame of a pose sequence equals rm_render_rgba8's."""
    torch = torch_cuda
    from raymarching_amd.frame import DeltaFrame
    side = torch.cuda.Stream()
    queue = []

    def fake(fr):
        def exchange(slot):
            if fr.rank == 1:
                fr.size_ev[slot].synchronize()
                mine = int(fr.size_host[slot][0])
                entry = {"msg": fr.msg[slot], "size": mine}
                queue.append(entry)
                return [0, mine], [_Work(entry=entry)]
            entry = queue.pop(0)
            if fr.decoded_recorded[slot]:
                side.wait_event(fr.decoded[slot])
            with torch.cuda.stream(side):
                fr.recv[slot][1][: entry["size"]].copy_(entry["msg"][: entry["size"]])
            done = torch.cuda.Event()
            done.record(side)
            entry["done"] = done
            return [0, entry["size"]], [_Work(ev=done)]
        return exchange

    r1 = rm.Renderer(0)
    frs = _pair_as_nccl(DeltaFrame, R, r1, runs=runs)
    for f in frs:
        f._sizes_and_messages = fake(f)
    assert len(frs[0].streams) == 2
    _pair_frames_equal_one_rank(torch, frs, R, r1)
    r1.close()


@pytest.mark.parametrize("runs", [None, (13, 8)])
def test_compressed_wire_rccl_exchange_code_in_one_process(R, torch_cuda, runs, monkeypatch):
    """DeltaFrame's own RCCL exchange code (_sizes_and_messages with the size
    all-gather on the control stream and the point-to-point messages, as the
    "nccl" backend runs it), two ranks in one process: only the three
    torch.distributed calls it makes are replaced by in-process equivalents
    (all_gather_into_tensor of the device sizes, P2POp, batch_isend_irecv with
    works whose wait() orders the caller's stream).  Every frame equals
    rm_render_rgba8's."""
    torch = torch_cuda
    import torch.distributed as dist
    from raymarching_amd.frame import DeltaFrame
    side = torch.cuda.Stream()
    gathered, sent = {}, {}

    def all_gather_into_tensor(out, inp, group=None):
        # rank 1 (submitted first in each frame) brings its message size, the
        # root 0; both receive [0, size of rank 1]
        v = int(inp.item())
        if v:
            gathered["r1"] = v
        out.copy_(torch.tensor([0, gathered["r1"]], dtype=torch.int64, device=out.device))

    class P2POp:
        def __init__(self, op, tensor, peer, group=None):
            self.op, self.tensor, self.peer = op, tensor, peer

    def batch_isend_irecv(ops):
        works = []
        for o in ops:
            if o.op is dist.isend:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream())
                entry = {"src": o.tensor, "ev": ev}
                sent["msg"] = entry
                works.append(_Work(entry=entry))  # (the sender's buffer is free once the copy is done)
            else:
                entry = sent.pop("msg")
                assert entry["src"].numel() == o.tensor.numel()
                side.wait_stream(torch.cuda.current_stream())
                side.wait_event(entry["ev"])
                with torch.cuda.stream(side):
                    o.tensor.copy_(entry["src"])
                done = torch.cuda.Event()
                done.record(side)
                entry["done"] = done
                works.append(_Work(ev=done))
        return works

    monkeypatch.setattr(dist, "all_gather_into_tensor", all_gather_into_tensor)
    monkeypatch.setattr(dist, "P2POp", P2POp)
    monkeypatch.setattr(dist, "batch_isend_irecv", batch_isend_irecv)
    r1 = rm.Renderer(0)
    frs = _pair_as_nccl(DeltaFrame, R, r1, runs=runs)
    _pair_frames_equal_one_rank(torch, frs, R, r1)
    assert frs[0].last_sizes[0] == 0 and frs[0].last_sizes[1] > 0
    r1.close()


@pytest.mark.parametrize("runs", [None, (13, 8)])
def test_rgb8_rccl_gather_code_in_one_process(R, torch_cuda, runs, monkeypatch):
    """DistributedFrame's own RCCL gather code (_gather_async: the async
    ncclGather of equal bands, or the unpadded point-to-point parts, as the
    "nccl" backend runs them), two ranks in one process with only
    dist.gather / P2POp / batch_isend_irecv replaced by in-process device
    copies whose works order the caller's stream.  Every frame equals
    rm_render_rgba8's."""
    torch = torch_cuda
    import torch.distributed as dist
    from raymarching_amd.frame import DistributedFrame
    side = torch.cuda.Stream()
    pending = {}

    def copy_after(dst, src, ev):
        side.wait_stream(torch.cuda.current_stream())
        side.wait_event(ev)
        with torch.cuda.stream(side):
            dst.copy_(src)

    def gather(tensor, gather_list=None, dst=0, group=None, async_op=False):
        assert async_op and dst == 0
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        if gather_list is None:  # rank 1 (submitted first)
            entry = {"src": tensor, "ev": ev}
            pending["gather"] = entry
            return _Work(entry=entry)
        entry = pending.pop("gather")
        copy_after(gather_list[0], tensor, ev)
        copy_after(gather_list[1], entry["src"], entry["ev"])
        done = torch.cuda.Event()
        done.record(side)
        entry["done"] = done
        return _Work(ev=done)

    class P2POp:
        def __init__(self, op, tensor, peer, group=None):
            self.op, self.tensor, self.peer = op, tensor, peer

    def batch_isend_irecv(ops):
        works = []
        for o in ops:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            if o.op is dist.isend:
                entry = {"src": o.tensor, "ev": ev}
                pending["p2p"] = entry
                works.append(_Work(entry=entry))
            else:
                entry = pending.pop("p2p")
                assert entry["src"].numel() == o.tensor.numel()
                copy_after(o.tensor, entry["src"], entry["ev"])
                done = torch.cuda.Event()
                done.record(side)
                entry["done"] = done
                works.append(_Work(ev=done))
        return works

    monkeypatch.setattr(dist, "gather", gather)
    monkeypatch.setattr(dist, "P2POp", P2POp)
    monkeypatch.setattr(dist, "batch_isend_irecv", batch_isend_irecv)
    r1 = rm.Renderer(0)
    frs = _pair_as_nccl(DistributedFrame, R, r1, fmt="rgba8", runs=runs)
    _pair_frames_equal_one_rank(torch, frs, R, r1)
    r1.close()


def test_context_outlives_a_destroyed_stream(torch_cuda):
    """Completion events are recorded lazily: when the
    context leaves a stream, the event goes on that stream while it still
    exists.  Render on a raw HIP stream, switch away, destroy the stream, keep
    rendering (adaptive order across streams), then destroy the context: no
    wait on a dead stream, and the frames stay right."""
    import ctypes
    torch = torch_cuda
    hip = ctypes.CDLL("libamdhip64.so")
    r = rm.Renderer(0)
    setup(r, "T", POSES["P2"], 64)
    r.set_params(count_evals=0, schedule=1)
    ref = r.render_rgba8(64, 48)
    torch.cuda.synchronize()
    st = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(st), ctypes.c_uint(1)) == 0
    out = torch.empty((48, 64), dtype=torch.int32, device="cuda")
    r.set_stream(st.value)
    for _ in range(10):  # an adaptive order is built on the raw stream
        r.render_rgba8(64, 48, out=out)
    r.set_stream(torch.cuda.current_stream())
    assert hip.hipStreamSynchronize(st) == 0
    assert torch.equal(out, ref)
    assert hip.hipStreamDestroy(st) == 0
    for _ in range(3):
        out2 = r.render_rgba8(64, 48)
    torch.cuda.synchronize()
    assert torch.equal(out2, ref)
    r.close()



@pytest.mark.gpu
def test_schedule_entries_released_after_their_stream_was_left(torch_cuda):
    """Leaving a stream records one marker, `done`, which the adaptive-order
    entries used there borrow.  Ten geometries on two
    alternating streams cycle the eight entries, so entries of a left stream
    are released (least recently used) while their borrowed marker has been
    re-recorded for later leaves; every frame must still be right."""
    torch = torch_cuda
    r = rm.Renderer(0)
    setup(r, "T", POSES["P2"], 64)
    r.set_params(count_evals=0, schedule=1)
    sizes = [(64, 40 + 2 * i) for i in range(10)]
    refs = {s: r.render_rgba8(*s).clone() for s in sizes}
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = []
    for it in range(3):
        for k, s in enumerate(sizes):
            st = streams[(k + it) % 2]
            with torch.cuda.stream(st):
                r.set_stream(st)
                outs.append((it, s, r.render_rgba8(*s)))
    r.set_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for it, s, o in outs:
        assert torch.equal(o, refs[s]), (it, s)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("close_on_kept", [False, True])
def test_kept_streams_frames_and_destroy(torch_cuda, close_on_kept):
    """rm_set_stream_kept (rm.h): leaving a kept stream records nothing.  The
    adaptive-order entries used there are marked on the stream itself when
    they are released (ten geometries over eight entries, on two kept pool
    streams and the caller's), and rm_destroy marks the kept streams still
    owed, also while bound to one (close_on_kept).  Every frame must be right."""
    torch = torch_cuda
    r = rm.Renderer(0)
    setup(r, "T", POSES["P2"], 64)
    r.set_params(count_evals=0, schedule=1)
    sizes = [(64, 40 + 2 * i) for i in range(10)]
    refs = {s: r.render_rgba8(*s).clone() for s in sizes}
    torch.cuda.synchronize()
    caller = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = []
    for it in range(3):
        for k, s in enumerate(sizes):
            st = streams[(k + it) % 2]
            with torch.cuda.stream(st):
                r.set_stream(st, kept=True)
                outs.append((it, s, r.render_rgba8(*s)))
            if k % 3 == 2:  # the caller's (not kept) stream in between
                r.set_stream(caller)
                outs.append((it, s, r.render_rgba8(*s)))
    if not close_on_kept:
        r.set_stream(caller)
    r.close()
    torch.cuda.synchronize()
    for it, s, o in outs:
        assert torch.equal(o, refs[s]), (it, s)
