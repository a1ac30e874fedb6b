"""Scene T's far-sky shortcut on the GPU (csrc/rm_far_sky.h).

With max_steps >= N0 = 208 the timed kernels skip the primary march and the
reflection march of every wave whose rays all provably escape past the sponge
(the march then returns ZFAR and the reflection factor is 1, bit for bit).  The
instrumented kernels (count_evals = 1) take every reference step and count the
ones left out in rm_stats.skipped.  So the timed frame must equal the
instrumented frame in every bit: float4 and RGBA8, for the tile8, tile16 and
persistent kernels, row-major and in adaptive order with scene T's latency
tiles, at sizes with partly filled waves, with max_steps one below N0 (shortcut
off), at N0 and at 256, on poses where no wave, some waves and every wave
qualifies.  rm_shade_rays and rm_render_aa_rgba8 run the same render_T_from;
here they run at 256 steps on the all_sky pose only, and their own tests
(tests/test_shade_rays.py, tests/test_aa_gpu.py) at 128 steps, below N0.  With
the shortcut live they are held to instrumented frames, ray by ray with origins
per ray and in mixed waves, by tests/test_shade_rays_shortcuts.py.
"""
import math

import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from raymarching_amd import POSES
from tests import aa_ref
from tests import sentinel
from tests.parity import FULL_SIZE_STEP_MAP, assert_parity

pytestmark = pytest.mark.gpu

N0 = 208  # rmfs::kFarSkyN0 (csrc/rm_far_sky.h); tests/host/far_sky_test.cpp checks the bound itself
SIZES = [(64, 64), (96, 54), (61, 37)]  # 61x37: ragged tiles, partly filled waves
STEPS = [N0 - 1, N0, 256]

P0 = POSES["P0"]
POSE_SET = {
    # the headline pose: sponge left of centre, most waves all sky
    "P0": P0,
    # P0 turned half round: the sponge is behind the camera, every wave qualifies
    "all_sky": dict(pos=P0["pos"], mouse=(math.pi, 0.0), time=0.0),
    # the sponge rotated by 60 degrees (u_time 30): the inflated cube's silhouette crosses the frame
    "silhouette_t30": dict(pos=(2.0, 3.0, 3.5), mouse=(-0.45, 0.0), time=30.0),
    # inside the inflated cube (max|q| = 1.2 < 1.25), outside the sponge: no ray may qualify
    "inside_inflated": dict(pos=(0.0, 3.0, 1.2), mouse=(0.0, 0.0), time=0.0),
    # 60 away, looking at the sponge: the central rays hit the cube beyond ZFAR, the others qualify
    "from_60": dict(pos=(0.0, 3.0, 60.0), mouse=(0.0, 0.0), time=0.0),
    # 52 away: rays passing beside the sponge end, at depth ZFAR, within 4.1 of it (second condition fails)
    "from_52": dict(pos=(0.0, 3.0, 52.0), mouse=(0.0, 0.0), time=0.0),
}


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def setup(r, pose, steps, count_evals, kernel="auto", schedule=0):
    r.load_scene(rm.SCENE_FILES["T"])
    r.set_pose(pose["pos"], pose["mouse"], pose["time"])
    r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=count_evals, kernel=kernel, schedule=schedule)


@pytest.mark.parametrize("kernel", ["tile8", "tile16", "persist"])
@pytest.mark.parametrize("pose_name", list(POSE_SET))
def test_timed_frame_equals_instrumented_frame(R, torch_cuda, pose_name, kernel):
    torch = torch_cuda
    pose = POSE_SET[pose_name]
    for W, H in SIZES:
        for steps in STEPS:
            setup(R, pose, steps, 1, kernel)
            ref4, st = R.render(W, H, stats=True)
            ref4, ref8 = bits(ref4), bits(R.render_rgba8(W, H))
            assert np.isfinite(ref4.view(np.float32)).all()
            what = f"{pose_name} {kernel} {W}x{H} {steps} steps"
            if pose_name == "all_sky" and steps >= N0:
                assert st["skipped"] >= 2 * W * H, (what, st)
            R.set_params(count_evals=0, schedule=0)
            f, st = R.render(W, H, stats=True)
            assert st["dispatch"] == "row-major", st
            assert np.array_equal(bits(f), ref4), f"{what}: timed float4 (row-major) differs"
            assert np.array_equal(bits(R.render_rgba8(W, H)), ref8), f"{what}: timed RGBA8 (row-major) differs"
            R.set_params(schedule=1)
            # (every launch into a target no launch has written, tests/sentinel.py: a tile the order never
            # dispatched shows instead of keeping the previous launch's pixels)
            for i in range(2):  # (the second launch of a geometry has an order and, in scene T, latency tiles)
                o8, st8 = R.render_rgba8(W, H, out=sentinel.target(torch, (H, W), torch.int32), stats=True)
                sentinel.assert_frame(o8, ref8, f"{what}: timed RGBA8 (schedule 1, launch {i})")
                assert np.array_equal(bits(o8), ref8), f"{what}: timed RGBA8 (schedule 1, launch {i}) differs"
            for i in range(2):
                f, st4 = R.render(W, H, out=sentinel.target(torch, (H, W, 4), torch.float32), stats=True)
                sentinel.assert_frame(f, ref4, f"{what}: timed float4 (schedule 1, launch {i})")
                assert np.array_equal(bits(f), ref4), f"{what}: timed float4 (schedule 1, launch {i}) differs"
            if kernel != "tile16":  # (the four-wave workgroups have no tile order)
                assert st8["dispatch"] == "adaptive" and st8["lat_tiles"] > 0, st8
                assert st4["dispatch"] == "adaptive" and st4["lat_tiles"] > 0, st4
    R.set_params(kernel="auto", schedule=0)


def test_all_sky_steps_are_the_oracles(R):
    """The instrumented kernel still takes and counts every reference step: its
    step map against the oracle's at the tolerance of the full-size frames, the
    image at scene T's parity policy, and at least two steps per pixel (one
    primary step, the reflection's first) reported as left out."""
    pose, (W, H), steps = POSE_SET["all_sky"], (96, 54), 256
    setup(R, pose, steps, 1)
    img, evmap, st = R.render_step_map(W, H)
    ref, ev = oracle.render("T", W, H, pos=pose["pos"], mouse=pose["mouse"], time=pose["time"], max_steps=steps)
    assert_parity("T", img.cpu().numpy(), ref, label="all sky")
    got = evmap.cpu().numpy()
    exact = float(np.mean(got == ev))
    print(f"all sky {W}x{H}: step map exact {exact:.5f}, evals {st['evals']} (oracle {int(ev.sum())}), "
          f"skipped {st['skipped']}")
    assert int(got.sum()) == st["evals"]
    assert exact >= FULL_SIZE_STEP_MAP["T"]
    assert abs(st["evals"] - int(ev.sum())) <= 5e-3 * int(ev.sum())
    assert 2 * W * H <= st["skipped"] <= st["evals"]
    # below N0 the shortcut is off: what is left out is the reflection march past depth 3 alone, less than before
    R.set_params(max_steps=N0 - 1)
    _, st_off = R.render(W, H, stats=True)
    assert st_off["evals"] == st["evals"]  # (every march of this frame escapes within 207 steps)
    assert st_off["skipped"] + 2 * W * H <= st["skipped"]


@pytest.mark.parametrize("W,H", [(61, 37), (64, 64)])
def test_shade_rays_on_the_all_sky_pose(R, W, H):
    """A frame through its own rays (tests/test_shade_rays.py's reference), and
    both against the instrumented frame; origins per ray take render_T_from
    with the lane's own sponge-space origin."""
    torch = pytest.importorskip("torch")
    pose = POSE_SET["all_sky"]
    setup(R, pose, 256, 1)
    ref4, ref8 = bits(R.render(W, H)).reshape(-1, 4), bits(R.render_rgba8(W, H)).reshape(-1)
    R.set_params(count_evals=0)
    frame4, frame8 = bits(R.render(W, H)).reshape(-1, 4), bits(R.render_rgba8(W, H)).reshape(-1)
    assert np.array_equal(frame4, ref4) and np.array_equal(frame8, ref8)
    origin, dirs = R.camera_rays(W, H)
    own = origin.reshape(1, 3).expand(W * H, 3).contiguous()
    assert torch.is_tensor(own) and own.is_cuda
    for width in (W, 0):  # (a list has no pixel positions: no vignette, so no frame to compare with)
        vig = width > 0
        got = R.shade_rays(origin, dirs, width=width, output="display", vignette=vig)
        got8 = R.shade_rays(origin, dirs, width=width, output="display", vignette=vig, rgba8=True)
        if width:
            assert np.array_equal(bits(got), ref4) and np.array_equal(bits(got8), ref8)
        per_ray = R.shade_rays(own, dirs.reshape(-1, 3), width=width, output="display", vignette=vig, rgba8=True)
        assert np.array_equal(bits(per_ray), bits(got8))
    # the list's linear colours are the image's: one layout against the other
    lin_t = R.shade_rays(origin, dirs, width=W, output="linear")
    lin_l = R.shade_rays(origin, dirs, width=0, output="linear")
    assert np.array_equal(bits(lin_t), bits(lin_l))


@pytest.mark.parametrize("K", [2, 4])
def test_render_aa_on_the_all_sky_pose(R, torch_cuda, K):
    """Every pixel supersampled (threshold 0) against the K jittered frames of
    rm_render_accumulate blended on the host (tests/test_aa_gpu.py's reference),
    those frames rendered by the instrumented kernels."""
    torch = torch_cuda
    pose, W, H = POSE_SET["all_sky"], 61, 37
    setup(R, pose, 256, 1)
    R.set_uniform("u_sample_part", 1.0)
    frames = []
    for seed in aa_ref.seeds(K):
        R.set_uniform("u_seed1", float(seed[0]), float(seed[1]))
        acc = torch.full((H, W, 4), float("nan"), device="cuda")
        frames.append(R.render_accumulate(W, H, acc).cpu().numpy())
    R.set_uniform("u_seed1", 0.5, 0.5)
    want = oracle.pack_rgba8(aa_ref.tree_mean(frames))
    R.set_params(count_evals=0)
    out, st = R.render_aa(W, H, samples=K, threshold=0, stats=True)
    assert st["refined"] == W * H
    ndiff = int((bits(out) != want).sum())
    print(f"all sky {W}x{H} K={K}: {ndiff} words differ from the blended instrumented accumulate frames")
    assert ndiff == 0
