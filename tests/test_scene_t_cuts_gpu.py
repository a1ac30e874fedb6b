"""Scene T / S0 per-pixel cuts leave every bit as it was.

tests/golden/scene_t_cuts/T_parent_frames.npz holds frames of the commit
before the cuts (tools/record_scene_t_cuts.py, instrumented kernels): per case
the float4 frame's bits, its RGBA8 words, the per-pixel sceneSDF call counts
and rm_stats' evals / flop / skipped.  tests/test_scene_t_trim.py runs with 128
steps, where the far-sky path is off; these cases run at 256 and 207 steps, on
poses where some, every and no wave is far-sky, on a rotated sponge, on S0 and
with u_resolution different from the frame size.

What each cut could break, and the case that would show it:
  * the per-resolution reciprocals (FrameConst.rcp_*): every frame, and the
    sequence of sizes in one context (a stale entry renders another size's
    camera rays);
  * the one-instruction clamps of sky / ind / fre: every hit pixel;
  * the box-only probes of far-sky waves: the all-sky pose (every wave) and P0
    (the waves next to the sponge must not take it);
  * the per-tile shard_row: the band layouts, aligned (band 16) and
    straddling (band 3), and a part that starts inside a tile row;
  * the shadow loop's reshaped step: every lit pixel's shadow factor.
"""
import math
import os

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import POSES, S0_POSE
from tests import sentinel

pytestmark = pytest.mark.gpu

# (a folder of its own: the golden tests read every golden/T_*.npz as a reference-GLSL fixture)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "scene_t_cuts", "T_parent_frames.npz")

P0 = POSES["P0"]
# P0 turned half round: the sponge is behind the camera, every wave is far-sky
ALL_SKY = dict(pos=P0["pos"], mouse=(math.pi, 0.0), time=0.0)
# inside the inflated cube (max|q| = 1.2 < 1.25), outside the sponge: no ray is far-sky
INSIDE = dict(pos=(0.0, 3.0, 1.2), mouse=(0.0, 0.0), time=0.0)

# name: scene, W, H, pose, max_steps, u_resolution (None: the frame size)
CASES = {
    "T_96x54_P0_256": ("T", 96, 54, P0, 256, None),
    "T_96x54_P0_207": ("T", 96, 54, P0, 207, None),  # one below N0: the far-sky path is off
    "T_61x37_P0_256": ("T", 61, 37, P0, 256, None),  # ragged tiles
    "T_61x37_P0_207": ("T", 61, 37, P0, 207, None),
    "T_64x64_P0_256": ("T", 64, 64, P0, 256, None),
    "T_64x64_P0_207": ("T", 64, 64, P0, 207, None),
    "T_37x23_P0_256": ("T", 37, 23, P0, 256, None),
    "T_96x54_allsky_256": ("T", 96, 54, ALL_SKY, 256, None),
    "T_61x37_inside_256": ("T", 61, 37, INSIDE, 256, None),
    "T_96x54_P7_256": ("T", 96, 54, POSES["P7"], 256, None),
    "T_96x54_P0_res": ("T", 96, 54, P0, 256, (133.0, 71.0)),
    "S0_64x64": ("S0", 64, 64, S0_POSE, 64, None),
}
KERNELS = ["tile8", "tile16", "persist"]
# render_band: (band, nshards).  Band 3: the 8- and 16-row tiles straddle runs; band 16: every tile lies in one run
LAYOUTS = [(3, 2), (16, 2)]
BAND_CASES = ["T_96x54_P0_256", "T_61x37_P0_256", "T_96x54_allsky_256", "S0_64x64"]


def setup_case(r, name, count_evals, kernel="auto", schedule=0):
    scene, W, H, pose, steps, res = CASES[name]
    r.load_scene(rm.SCENE_FILES[scene])
    r.set_pose(pose["pos"], pose["mouse"], pose["time"])
    r.set_uniform("u_resolution", *(res or (float(W), float(H))))
    r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=count_evals, kernel=kernel, schedule=schedule)
    return W, H


def render_instrumented(r, name):
    """The record of one case: what tools/record_scene_t_cuts.py stores."""
    W, H = setup_case(r, name, 1)
    f4, emap, st = r.render_step_map(W, H)
    w8 = r.render_rgba8(W, H)
    return dict(f4=f4.cpu().numpy().view(np.uint32), rgba8=w8.cpu().numpy().view(np.uint32),
                evals_map=emap.cpu().numpy().view(np.uint32),
                stats=np.array([st["evals"], st["flop"], st["skipped"]], np.uint64))


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_instrumented_frames_equal_the_parent(R, golden, name):
    got = render_instrumented(R, name)
    for k, v in got.items():
        assert np.array_equal(v, golden[f"{name}.{k}"]), f"{name}: {k} differs from the parent commit's"
    # the other workgroup shapes' instrumented kernels: the same frame, map and tallies
    W, H = CASES[name][1:3]
    for kernel in ("tile16", "persist"):
        R.set_params(kernel=kernel)
        f4, emap, st = R.render_step_map(W, H)
        assert np.array_equal(bits(f4), golden[f"{name}.f4"]), f"{name} {kernel}: instrumented float4 differs"
        assert np.array_equal(bits(emap), golden[f"{name}.evals_map"]), f"{name} {kernel}: step map differs"
        assert [st["evals"], st["flop"], st["skipped"]] == golden[f"{name}.stats"].tolist(), (name, kernel, st)
        assert np.array_equal(bits(R.render_rgba8(W, H)), golden[f"{name}.rgba8"]), f"{name} {kernel}: RGBA8 differs"
    R.set_params(kernel="auto")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(CASES))
def test_timed_frames_equal_the_parent(R, torch_cuda, golden, name, kernel):
    torch = torch_cuda
    f4, w8 = golden[f"{name}.f4"], golden[f"{name}.rgba8"]
    what = f"{name} {kernel}"
    W, H = setup_case(R, name, 0, kernel, schedule=0)
    f, st = R.render(W, H, stats=True)
    assert st["dispatch"] == "row-major", st
    assert np.array_equal(bits(f), f4), f"{what}: timed float4 (row-major) differs"
    assert np.array_equal(bits(R.render_rgba8(W, H)), w8), f"{what}: timed RGBA8 (row-major) differs"
    R.set_params(schedule=1)
    # (every ordered launch into a target no launch has written, tests/sentinel.py: a tile the order never
    # dispatched shows instead of keeping the previous launch's pixels)
    for _ in range(3):  # (an order exists from the second launch of a geometry on)
        o8, st8 = R.render_rgba8(W, H, out=sentinel.target(torch, (H, W), torch.int32), stats=True)
    sentinel.assert_frame(o8, w8, f"{what}: timed RGBA8 (adaptive)")
    assert np.array_equal(bits(o8), w8), f"{what}: timed RGBA8 (adaptive) differs"
    for _ in range(2):
        f, st4 = R.render(W, H, out=sentinel.target(torch, (H, W, 4), torch.float32), stats=True)
    sentinel.assert_frame(f, f4, f"{what}: timed float4 (adaptive)")
    assert np.array_equal(bits(f), f4), f"{what}: timed float4 (adaptive) differs"
    if kernel != "tile16":  # (the four-wave workgroups have no tile order)
        assert st8["dispatch"] == "adaptive" and st4["dispatch"] == "adaptive", (st8, st4)
    R.set_params(kernel="auto", schedule=0)


def band_rows(H, band, n, s):
    return [y for y in range(H) if (y // band) % n == s]


@pytest.mark.parametrize("band,nshards", LAYOUTS)
@pytest.mark.parametrize("name", BAND_CASES)
def test_bands_equal_the_parents_rows(R, golden, name, band, nshards):
    torch = pytest.importorskip("torch")
    f4, w8 = golden[f"{name}.f4"], golden[f"{name}.rgba8"]
    for kernel in KERNELS:
        for shard in range(nshards):
            W, H = setup_case(R, name, 0, kernel, schedule=0)
            rows = band_rows(H, band, nshards, shard)
            what = f"{name} {kernel} band {band} shard {shard}/{nshards}"
            assert np.array_equal(bits(R.render_band_rgba8(W, H, band, nshards, shard)), w8[rows]), f"{what}: RGBA8"
            assert np.array_equal(bits(R.render_band(W, H, band, nshards, shard)), f4[rows]), f"{what}: float4"
            # a part that starts inside a tile row: packed rows 4.. of the shard
            if len(rows) > 4:
                part = torch.empty((len(rows) - 4, W), dtype=torch.int32, device="cuda")
                R.render_rows(W, H, band, nshards, shard, 4, len(rows) - 4, part)
                assert np.array_equal(bits(part), w8[rows[4:]]), f"{what}: RGBA8 rows from packed row 4"
            R.set_params(schedule=1)
            for _ in range(3):
                b, st = R.render_band_rgba8(W, H, band, nshards, shard, stats=True,
                                            out=sentinel.target(torch, (len(rows), W), torch.int32))
            sentinel.assert_frame(b, w8[rows], f"{what}: RGBA8 (adaptive)")
            assert np.array_equal(bits(b), w8[rows]), f"{what}: RGBA8 (adaptive)"
            assert kernel == "tile16" or st["dispatch"] == "adaptive", st
            # the instrumented kernels take the same rows
            R.set_params(count_evals=1, schedule=0)
            assert np.array_equal(bits(R.render_band_rgba8(W, H, band, nshards, shard)), w8[rows]), \
                f"{what}: instrumented RGBA8"
    R.set_params(kernel="auto", schedule=0, count_evals=0)


def test_resolution_cache_across_sizes(torch_cuda, golden):
    """One context renders 96x54 -> 37x23 -> 96x54 -> 64x64 and a first
    accumulate frame at zero offset: each frame is its record (a stale
    reciprocal would render another size's rays), and the per-resolution cache
    stays within its bound however many sizes pass through it."""
    torch = torch_cuda
    r = rm.Renderer(0)
    try:
        for name in ("T_96x54_P0_256", "T_37x23_P0_256", "T_96x54_P0_256", "T_64x64_P0_256", "T_96x54_P0_res",
                     "T_37x23_P0_256"):
            W, H = setup_case(r, name, 0)
            assert np.array_equal(bits(r.render(W, H)), golden[f"{name}.f4"]), f"{name}: float4 differs"
            assert np.array_equal(bits(r.render_rgba8(W, H)), golden[f"{name}.rgba8"]), f"{name}: RGBA8 differs"
        entries, capacity = r.resolution_cache()
        assert entries == 4 and entries <= capacity, (entries, capacity)  # 96x54, 37x23, 64x64, 96x54 with (133, 71)
        # progressive accumulation's first frame (u_sample_part 1) at zero offset (fract(u_seed1) = 0.5)
        name = "T_61x37_P0_256"
        W, H = setup_case(r, name, 0)
        r.set_uniform("u_sample_part", 1.0)
        r.set_uniform("u_seed1", 0.5, 0.5)
        acc = torch.full((H, W, 4), float("nan"), device="cuda")
        assert np.array_equal(bits(r.render_accumulate(W, H, acc)), golden[f"{name}.f4"]), "accumulate float4 differs"
        acc8 = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        assert np.array_equal(bits(r.render_accumulate(W, H, acc8)), golden[f"{name}.rgba8"]), "accumulate RGBA8 differs"
        # more sizes than the cache holds: it evicts, and a returning size is computed again, the same
        for i in range(capacity + 3):
            r.set_uniform("u_resolution", 8.0 + i, 8.0)
            r.render_rgba8(8 + i, 8)
        entries, capacity = r.resolution_cache()
        assert 1 <= entries <= capacity, (entries, capacity)
        name = "T_96x54_P0_256"
        W, H = setup_case(r, name, 0)
        assert np.array_equal(bits(r.render(W, H)), golden[f"{name}.f4"]), f"{name}: float4 differs after eviction"
    finally:
        r.close()
