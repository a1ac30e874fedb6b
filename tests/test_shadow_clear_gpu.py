"""Scene T's soft-shadow certificate on the GPU (csrc/rm_shadow_clear.h).

A lit lane whose shadow ray leaves a face of the sponge's cube outward at a
slope of at least kRatio takes no soft-shadow march in the timed kernels: the
march provably returns 1.0f.  The instrumented kernels (count_evals = 1) still
take every reference step and count those marches' steps apart
(rm_certified_steps, `certified` in the stats dict).
So nothing may change: every frame here is held, bit for bit, to the frame the
commit before the certificate rendered (tests/golden/shadow_clear/
T_parent_frames.npz, tools/record_shadow_clear.py: sha256 of the float4 bits,
of the RGBA8 words and of the per-pixel step map, rm_stats' evals / flop /
skipped, and the RGBA8 frame itself at 256 steps), and the timed kernels to the
instrumented ones, float4 and RGBA8, tile8, tile16 and persistent, row-major
and in adaptive order with latency tiles, at 128, 207 and 256 steps.

The poses (tests/shadow_clear_ref.py POSE_SET) clear most lit lanes (P0, the
top face from above), some (the side face turned until its slopes straddle
kRatio) and none (turned further; inner walls only); the numpy restatement of
the predicate says which, and the certified count must agree.
"""
import hashlib
import os

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import POSES, S0_POSE
from tests import shadow_clear_ref as ref
from tests import sentinel

pytestmark = pytest.mark.gpu

# (a folder of its own: the golden tests read every golden/T_*.npz as a reference-GLSL fixture)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "shadow_clear", "T_parent_frames.npz")

SIZES = ref.SIZES
STEPS = [128, 207, 256]  # 207: one below the far-sky shortcut's N0
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
    """What tools/record_shadow_clear.py stores of one case (run on the commit before the certificate)."""
    f4, w8, emap, st = render_instrumented(r, name)
    rec = {f"{name}.sha": np.array([sha(f4), sha(w8), sha(emap)]),
           f"{name}.stats": np.array([st["evals"], st["flop"], st["skipped"]], np.uint64)}
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
    """(lit lanes, cleared lanes) of every case by the numpy restatement; computed once"""
    out = {}
    for name, (pose_name, W, H, steps) in CASES.items():
        m = ref.frame_masks(ref.POSE_SET[pose_name][0], W, H, steps)
        out[name] = (int(m["lit"].sum()), int(m["clear"].sum()))
    return out


@pytest.mark.parametrize("pose_name", list(ref.POSE_SET))
def test_instrumented_frames_and_counts(R, golden, restated, pose_name):
    intent = ref.POSE_SET[pose_name][1]
    for name in [n for n, c in CASES.items() if c[0] == pose_name]:
        lit, clear = restated[name]
        assert ref.share_is_as_intended(intent, lit, clear / max(lit, 1)), (name, intent, lit, clear)
        for kernel in ["auto", "tile16", "persist"]:
            f4, w8, emap, st = render_instrumented(R, name, kernel)
            what = f"{name} {kernel}"
            print(f"{what}: restated lit {lit} clear {clear}; evals {st['evals']} skipped {st['skipped']} "
                  f"certified {st['certified']}")
            assert [sha(f4), sha(w8), sha(emap)] == golden[f"{name}.sha"].tolist(), \
                f"{what}: instrumented float4 / RGBA8 / step map differ from the parent commit's"
            if f"{name}.rgba8" in golden:
                assert np.array_equal(w8, golden[f"{name}.rgba8"]), f"{what}: RGBA8 words differ from the parent's"
            # evals, flop and skipped are the parent's: certified steps are counted beside them, not in them
            assert [st["evals"], st["flop"], st["skipped"]] == golden[f"{name}.stats"].tolist(), (what, st)
            assert (st["certified"] > 0) == (clear > 0), (what, st, lit, clear)
            assert st["certified"] <= st["evals"] - st["skipped"], (what, st)
            assert int(emap.sum()) == st["evals"]
    R.set_params(kernel="auto")


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
        assert st["certified"] == 0 and st["skipped"] == 0, st  # (counted by the instrumented kernels only)
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
def test_other_scenes_certify_nothing(R, scene, pose, steps):
    """Scene O's distance is a smooth min with its other objects: the sponge's box
    term bounds nothing there, and the certificate is scene T's alone."""
    R.load_scene(rm.SCENE_FILES[scene])
    R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    R.set_params(max_steps=steps, shadow_max_steps=0, count_evals=1, kernel="auto", schedule=0)
    for W, H in SIZES:
        _, st = R.render(W, H, stats=True)
        assert st["evals"] > 0 and st["certified"] == 0, (scene, W, H, st)


@pytest.mark.parametrize("pose_name", ["P0", "above", "side_above"])
def test_certified_steps_are_not_in_skipped(R, pose_name):
    """The instrumented shadow loop takes every step up to maxt and counts those
    after a lane's settle point in `skipped`; `certified` holds
    only the steps before it, what the timed kernels executed before the
    certificate.  Under a shadow step cap k every cleared lane marches exactly k
    steps while k is small (h >= 0.0035 never occludes, t stays far below maxt,
    and no lane settles before its box term reaches 0.1, which from t = 0.01 at
    steps of 0.1 h + 0.001 takes more than 8 steps at any slope <= 1): the count
    is k times the count at k = 1.  A cleared lane has box >= 0.35 t, the settle
    rule's own ratio (2.9 * 0.35 >= 1.01), so it settles soon after box >= 0.1,
    t >= 0.29, which steps growing by >= 3.5 % reach within 100 steps (measured:
    by step 64, profiles/r12/certified_under_step_caps.txt): from a cap of 100
    on, the count no longer grows and equals the uncapped one, while the marches
    themselves go on to about 150 steps, all of them in `skipped`."""
    pose = ref.POSE_SET[pose_name][0]
    R.load_scene(rm.SCENE_FILES["T"])
    R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    for W, H in SIZES:
        got = {}
        for cap in (1, 2, 8, 100, 200, 0):  # 0: uncapped
            R.set_params(max_steps=256, shadow_max_steps=cap, count_evals=1, kernel="auto", schedule=0)
            _, st = R.render(W, H, stats=True)
            assert st["certified"] + st["skipped"] <= st["evals"], (pose_name, W, H, cap, st)
            got[cap] = (st["certified"], st["skipped"])
        print(f"{pose_name} {W}x{H}: (certified, skipped) by shadow step cap {got}")
        lanes = got[1][0]
        assert lanes > 0
        assert got[2][0] == 2 * lanes and got[8][0] == 8 * lanes, (pose_name, W, H, got)
        assert got[100][0] == got[200][0] == got[0][0] < 100 * lanes, (pose_name, W, H, got)
        assert got[100][1] < got[200][1] <= got[0][1], (pose_name, W, H, got)  # the later steps are in skipped
    R.set_params(shadow_max_steps=0)
