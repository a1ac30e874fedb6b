"""Scene T / S0 straight-line trims leave every float as it was.

tests/golden/scene_t_trim/T_parent_frames.npz holds frames of the commit before the trims
(tools/record_scene_t_frames.py, instrumented kernels): per case the float4
frame's bits, its RGBA8 words, the per-pixel sceneSDF call counts and
rm_stats' evals / flop / skipped.  Each case is rendered again through the
instrumented kernels and through the timed ones (row-major and in adaptive
order; rm_render, rm_render_rgba8 and one rm_render_band_rgba8) and must
equal the record bit for bit.  The sizes hold every wave shape: all-sky,
all-hit, mixed, every lane's shadow factor 1, some lane shadowed.

The unguarded square roots and reciprocals (camera normalize, the fog
depth, the reflection length) have no entry point of their own: the frame
cases cover them at every pixel.  The RGBA8 pack has one, rm_pack_rgba8,
and is checked against oracle.pack_rgba8 value by value.
"""
import os

import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from raymarching_amd import POSES, S0_POSE
from tests import sentinel

pytestmark = pytest.mark.gpu

# (a folder of its own: the golden tests read every golden/T_*.npz as a reference-GLSL fixture)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "scene_t_trim", "T_parent_frames.npz")

# name: scene, W, H, pose, max_steps
CASES = {
    "T_96x54_P0": ("T", 96, 54, POSES["P0"], 128),
    "T_96x54_P1": ("T", 96, 54, POSES["P1"], 128),
    "T_96x54_P2": ("T", 96, 54, POSES["P2"], 128),
    "T_96x54_P3": ("T", 96, 54, POSES["P3"], 128),
    "T_37x23_P0": ("T", 37, 23, POSES["P0"], 128),  # ragged tiles
    "S0_64x64": ("S0", 64, 64, S0_POSE, 64),
}
BAND = (8, 3, 1)  # render_band_rgba8: band, nshards, shard


def setup_case(r, name, count_evals, schedule=0):
    scene, W, H, pose, steps = CASES[name]
    r.load_scene(rm.SCENE_FILES[scene])
    r.set_pose(pose["pos"], pose["mouse"], pose["time"])
    r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=count_evals, kernel="auto", schedule=schedule)
    return W, H


def render_instrumented(r, name):
    """The record of one case: what tools/record_scene_t_frames.py stores."""
    W, H = setup_case(r, name, 1)
    f4, emap, st = r.render_step_map(W, H)
    w8 = r.render_rgba8(W, H)
    return dict(f4=f4.cpu().numpy().view(np.uint32), rgba8=w8.cpu().numpy().view(np.uint32),
                evals_map=emap.cpu().numpy().view(np.uint32),
                stats=np.array([st["evals"], st["flop"], st["skipped"]], np.uint64))


def band_rows(H):
    band, n, s = BAND
    return [y for y in range(H) if (y // band) % n == s]


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


@pytest.mark.parametrize("name", list(CASES))
def test_timed_frames_equal_the_parent(R, torch_cuda, golden, name):
    torch = torch_cuda
    f4, w8 = golden[f"{name}.f4"], golden[f"{name}.rgba8"]
    W, H = setup_case(R, name, 0, schedule=0)
    f, st = R.render(W, H, stats=True)
    assert st["dispatch"] == "row-major", st
    assert np.array_equal(bits(f), f4), f"{name}: timed float4 (row-major) differs"
    assert np.array_equal(bits(R.render_rgba8(W, H)), w8), f"{name}: timed RGBA8 (row-major) differs"
    rows = band_rows(H)
    assert np.array_equal(bits(R.render_band_rgba8(W, H, *BAND)), w8[rows]), f"{name}: RGBA8 band (row-major) differs"
    R.set_params(schedule=1)
    # (every ordered launch into a target no launch has written, tests/sentinel.py: a tile the order never
    # dispatched shows instead of keeping the previous launch's pixels)
    for _ in range(3):  # (an order exists from the second launch of a geometry on)
        o8, st = R.render_rgba8(W, H, out=sentinel.target(torch, (H, W), torch.int32), stats=True)
    assert st["dispatch"] == "adaptive", st
    sentinel.assert_frame(o8, w8, f"{name}: timed RGBA8 (adaptive)")
    assert np.array_equal(bits(o8), w8), f"{name}: timed RGBA8 (adaptive) differs"
    for _ in range(2):
        f, st = R.render(W, H, out=sentinel.target(torch, (H, W, 4), torch.float32), stats=True)
    assert st["dispatch"] == "adaptive", st
    sentinel.assert_frame(f, f4, f"{name}: timed float4 (adaptive)")
    assert np.array_equal(bits(f), f4), f"{name}: timed float4 (adaptive) differs"
    for _ in range(2):
        b, st = R.render_band_rgba8(W, H, *BAND, out=sentinel.target(torch, (len(rows), W), torch.int32), stats=True)
    assert st["dispatch"] == "adaptive", st
    sentinel.assert_frame(b, w8[rows], f"{name}: RGBA8 band (adaptive)")
    assert np.array_equal(bits(b), w8[rows]), f"{name}: RGBA8 band (adaptive) differs"
    R.set_params(schedule=0)


def pack_values():
    f32 = np.float32
    ks = (np.arange(256, dtype=np.float64) / 255.0).astype(f32)
    near = [ks]
    lo, hi = ks, ks
    for _ in range(2):  # two float neighbours on each side of every k/255
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        near += [lo, hi]
    # the rounding ties (k + 1/2) / 255 as nearly as float32 holds them, with neighbours
    ties = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(f32)
    near += [ties, np.nextafter(ties, f32(-np.inf)), np.nextafter(ties, f32(np.inf))]
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, -1e-30, -0.25, -1.0,
                        -3.5, -1e30, 1.0000001, 1.5, 2.0, 255.0, 256.0, 1e3, 1e10, 1e30, np.inf, -np.inf, np.nan,
                        -np.nan], f32)
    rnd = np.random.RandomState(7).uniform(-0.5, 1.5, 1 << 16).astype(f32)
    v = np.concatenate(near + [special, rnd])
    return np.concatenate([v, np.zeros((-len(v)) % 4, f32)]).reshape(-1, 4)


def test_pack_rgba8_matches_the_oracle(R, torch_cuda):
    v = pack_values()
    got = bits(R.pack_rgba8(torch_cuda.from_numpy(v).cuda()))
    want = oracle.pack_rgba8(v)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} words differ, first: {v[bad[0]]} -> {got[bad[0]]:#x}, oracle {want[bad[0]]:#x}"
