"""Scene T's reflection certificate on the GPU (csrc/rm_refl_clear.h).

A lane whose reflection ray leaves a face of the sponge's cube outward at a
slope of at least kRatio takes no reflection march in the timed kernels when
max_steps >= kSteps (28): the march provably meets nothing and passes depth 3,
where its factor is 1.0f.  The instrumented kernels (count_evals = 1) still take
every reference step and count those marches' steps below depth 3 apart
(rm_reflection_cleared_steps, `reflection_cleared` in the stats dict).
So nothing may change: every frame here is held, bit for bit, to the frame the
commit before the certificate rendered (tests/golden/refl_clear/
T_parent_frames.npz, tools/record_refl_clear.py: sha256 of the float4 bits, of
the RGBA8 words and of the per-pixel step map, rm_stats' evals / flop / skipped
and the certified count, and the RGBA8 frame itself at 256 steps), and the timed
kernels to the instrumented ones, float4 and RGBA8, tile8, tile16 and
persistent, row-major and in adaptive order with latency tiles, at 27 steps
(kSteps - 1: the certificate is off), 28, 128 and 256.

The poses (tests/refl_clear_ref.py POSE_SET) clear most hit lanes (P0, the top
face from above, the turned sponge, a wall close-up), few (from the central
void: inner walls only), some on either side of kRatio (along the face x = +1)
and have no hit lane at all (P7); the numpy restatement of the predicate says
which, and the new count must agree.
"""
import hashlib
import os

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import POSES, S0_POSE
from tests import refl_clear_ref as ref
from tests import sentinel

pytestmark = pytest.mark.gpu

# (a folder of its own: the golden tests read every golden/T_*.npz as a reference-GLSL fixture)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "refl_clear", "T_parent_frames.npz")

SIZES = ref.SIZES
N = ref.K_STEPS
STEPS = [N - 1, N, 128, 256]  # N - 1: the old path; 128: below the far-sky shortcut's N0; 256: the benchmark's
KERNELS = ["tile8", "tile16", "persist"]


def case_name(pose_name, W, H, steps):
    return f"{pose_name}_{W}x{H}_{steps}"


CASES = {case_name(p, W, H, s): (p, W, H, s) for p in ref.POSE_SET for W, H in SIZES for s in STEPS}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def setup_case(r, name, count_evals, kernel="auto", schedule=0):
    pose_name, W, H, steps = CASES[name]
    pose = ref.POSE_SET[pose_name][0]
    r.load_scene(rm.SCENE_FILES["T"])
    r.set_pose(pose["pos"], pose["mouse"], pose["time"])
    r.set_params(max_steps=steps, shadow_max_steps=0, count_evals=count_evals, kernel=kernel, schedule=schedule)
    return W, H


def render_instrumented(r, name, kernel="auto"):
    """One case through the instrumented kernels -> (float4 bits, RGBA8 words, step map, rm_stats dict)"""
    W, H = setup_case(r, name, 1, kernel)
    f4, emap, st = r.render_step_map(W, H)
    return bits(f4), bits(r.render_rgba8(W, H)), bits(emap), st


def record(r, name):
    """What tools/record_refl_clear.py stores of one case (run on the commit before the certificate)."""
    f4, w8, emap, st = render_instrumented(r, name)
    rec = {f"{name}.sha": np.array([sha(f4), sha(w8), sha(emap)]),
           f"{name}.stats": np.array([st["evals"], st["flop"], st["skipped"], st["certified"]], np.uint64)}
    if CASES[name][3] == 256:
        rec[f"{name}.rgba8"] = w8
    return rec


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def restated():
    """(hit lanes, cleared lanes) of every case by the numpy restatement; computed once"""
    out = {}
    for name, (pose_name, W, H, steps) in CASES.items():
        m = ref.frame_masks(ref.POSE_SET[pose_name][0], W, H, steps)
        out[name] = (int(m["hit"].sum()), int(m["clear"].sum()))
    return out


@pytest.mark.parametrize("pose_name", list(ref.POSE_SET))
def test_instrumented_frames_and_counts(R, golden, restated, pose_name):
    pose, intent = ref.POSE_SET[pose_name]
    for W, H in SIZES:  # the pose's intent, on the CPU, before the GPU is used
        got = ref.cleared_share(pose, W, H, 256)
        assert ref.share_is_as_intended(intent, *got), (pose_name, W, H, intent, got)
    for name in [n for n, c in CASES.items() if c[0] == pose_name]:
        steps = CASES[name][3]
        hit, clear = restated[name]
        for kernel in ["auto", "tile16", "persist"]:
            f4, w8, emap, st = render_instrumented(R, name, kernel)
            what = f"{name} {kernel}"
            print(f"{what}: restated hit {hit} clear {clear}; evals {st['evals']} skipped {st['skipped']} "
                  f"certified {st['certified']} reflection_cleared {st['reflection_cleared']}")
            assert [sha(f4), sha(w8), sha(emap)] == golden[f"{name}.sha"].tolist(), \
                f"{what}: instrumented float4 / RGBA8 / step map differ from the parent commit's"
            if f"{name}.rgba8" in golden:
                assert np.array_equal(w8, golden[f"{name}.rgba8"]), f"{what}: RGBA8 words differ from the parent's"
            # evals, flop, skipped and certified are the parent's: the new count stands beside them, not in them
            assert [st["evals"], st["flop"], st["skipped"], st["certified"]] == golden[f"{name}.stats"].tolist(), \
                (what, st)
            if steps < N:  # the step-cap condition: the certificate is off, the old path
                assert st["reflection_cleared"] == 0, (what, st)
            else:
                assert (st["reflection_cleared"] > 0) == (clear > 0), (what, st, hit, clear)
            assert st["reflection_cleared"] + st["certified"] + st["skipped"] <= st["evals"], (what, st)
            assert st["reflection_cleared"] <= N * W_H(name), (what, st)  # at most kSteps steps of a lane
            assert int(emap.sum()) == st["evals"]
    R.set_params(kernel="auto")


def W_H(name):
    return CASES[name][1] * CASES[name][2]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("pose_name", list(ref.POSE_SET))
def test_timed_frame_equals_instrumented_frame_and_parent(R, torch_cuda, golden, pose_name, kernel):
    torch = torch_cuda
    for name in [n for n, c in CASES.items() if c[0] == pose_name]:
        what = f"{name} {kernel}"
        ref4, ref8, _, _ = render_instrumented(R, name, kernel)
        want4, want8 = golden[f"{name}.sha"][0], golden[f"{name}.sha"][1]
        W, H = setup_case(R, name, 0, kernel, schedule=0)
        f, st = R.render(W, H, stats=True)
        assert st["dispatch"] == "row-major", st
        # (counted by the instrumented kernels only)
        assert st["reflection_cleared"] == 0 and st["certified"] == 0 and st["skipped"] == 0, st
        assert np.array_equal(bits(f), ref4) and sha(bits(f)) == want4, f"{what}: timed float4 (row-major) differs"
        o8 = bits(R.render_rgba8(W, H))
        assert np.array_equal(o8, ref8) and sha(o8) == want8, f"{what}: timed RGBA8 (row-major) differs"
        R.set_params(schedule=1)
        # (every launch into a target no launch has written, tests/sentinel.py: a tile the order never dispatched
        # shows instead of keeping the previous launch's pixels)
        for i in range(2):  # (the second launch of a geometry has an order and latency tiles)
            o8, st8 = R.render_rgba8(W, H, out=sentinel.target(torch, (H, W), torch.int32), stats=True)
            sentinel.assert_frame(o8, ref8, f"{what}: timed RGBA8 (schedule 1, launch {i})")
            assert sha(bits(o8)) == want8, f"{what}: timed RGBA8 (schedule 1, launch {i}) differs"
        for i in range(2):
            f, st4 = R.render(W, H, out=sentinel.target(torch, (H, W, 4), torch.float32), stats=True)
            sentinel.assert_frame(f, ref4, f"{what}: timed float4 (schedule 1, launch {i})")
            assert sha(bits(f)) == want4, f"{what}: timed float4 (schedule 1, launch {i}) differs"
        if kernel != "tile16":  # (the four-wave workgroups have no tile order)
            assert st8["dispatch"] == "adaptive" and st8["lat_tiles"] > 0, st8
            assert st4["dispatch"] == "adaptive" and st4["lat_tiles"] > 0, st4
    R.set_params(kernel="auto", schedule=0)


@pytest.mark.parametrize("scene,pose,steps", [("S0", S0_POSE, 64), ("O", POSES["P0"], 128), ("O", POSES["P2"], 128)])
def test_other_scenes_clear_nothing(R, scene, pose, steps):
    """Scene O's reflection is a full shaded bounce, scene S0 has none: the certificate is scene T's alone."""
    R.load_scene(rm.SCENE_FILES[scene])
    R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    R.set_params(max_steps=steps, shadow_max_steps=0, count_evals=1, kernel="auto", schedule=0)
    for W, H in SIZES:
        _, st = R.render(W, H, stats=True)
        assert st["evals"] > 0 and st["reflection_cleared"] == 0, (scene, W, H, st)


@pytest.mark.parametrize("pose_name", ["P0", "wall", "grazing"])
def test_small_step_caps_march_as_before(R, pose_name):
    """max_steps of 1, 2 and 7, far below kSteps: a reflection march of so few steps ends short of depth 3 and
    its factor is below 1, so the certificate must stay off -- the timed frame is the instrumented one, bit for
    bit, and nothing is counted."""
    pose = ref.POSE_SET[pose_name][0]
    R.load_scene(rm.SCENE_FILES["T"])
    R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    for W, H in SIZES:
        for cap in (1, 2, 7):
            R.set_params(max_steps=cap, shadow_max_steps=0, count_evals=1, kernel="auto", schedule=0)
            want4, st = R.render(W, H, stats=True)
            want8 = bits(R.render_rgba8(W, H))
            assert st["reflection_cleared"] == 0, (pose_name, W, H, cap, st)
            for kernel in KERNELS:
                R.set_params(count_evals=0, kernel=kernel)
                assert np.array_equal(bits(R.render(W, H)), bits(want4)), (pose_name, W, H, cap, kernel)
                assert np.array_equal(bits(R.render_rgba8(W, H)), want8), (pose_name, W, H, cap, kernel)
    R.set_params(kernel="auto")


def test_count_is_the_steps_below_depth_3(R):
    """The instrumented reflection march takes every step to ZFAR and counts those begun at a depth >= 3 in
    `skipped`; `reflection_cleared` holds a cleared lane's steps before that, what the timed
    kernels executed before the certificate.  On the wall pose every lane hits within 12 steps and clears, under
    every cap from kSteps on, and no wave is far-sky: the count is the same at 28, 128 and 256 steps (a cleared
    lane is past depth 3 by step kSteps), it is the CPU restatement's count of those steps within one step per
    lane, and the marches go on past depth 3 (their later steps are in `skipped`: a count of whole marches would
    be that much larger).  At kSteps - 1 the certificate is off and the count is 0."""
    pose = ref.POSE_SET["wall"][0]
    R.load_scene(rm.SCENE_FILES["T"])
    R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    for W, H in SIZES:
        lanes, steps = ref.cleared_steps(pose, W, H, 256)
        assert lanes == W * H and ref.cleared_steps(pose, W, H, N) == (lanes, steps)
        got = {}
        for cap in (N - 1, N, 128, 256):
            R.set_params(max_steps=cap, shadow_max_steps=0, count_evals=1, kernel="auto", schedule=0)
            _, st = R.render(W, H, stats=True)
            got[cap] = (st["reflection_cleared"], st["skipped"], st["evals"])
        print(f"wall {W}x{H}: restated {lanes} lanes, {steps} steps; (reflection_cleared, skipped, evals) by cap {got}")
        assert got[N - 1][0] == 0
        assert got[N][0] == got[128][0] == got[256][0] > 0, got
        assert abs(got[256][0] - steps) <= lanes, (got, steps, lanes)
        assert got[256][0] <= N * lanes
        assert got[256][1] >= lanes, got  # every lane's march takes at least one step from depth >= 3 on
