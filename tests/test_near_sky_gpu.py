"""Scene T's near-sky ladder on the GPU (csrc/rm_far_sky.h 3.).

The timed kernels take the far-sky vote against the cube of the smallest
half-size their step cap admits (m = 0.25 from 39 steps, 0.1 from 63, 0.05 from
98, 0.02 from 205): a wave whose rays all miss it, and end 3.1 beyond the sponge,
takes neither its primary nor its reflection march.  The instrumented kernels
(count_evals = 1) still take every reference step; `skipped` keeps to the
far-sky vote (m = 0.25, max_steps >= 208) and the steps newly left out are
counted apart (rm_near_sky_steps, `near_sky` in the stats dict).
So nothing may change: every frame here is held, bit for bit, to the frame the
commit before the ladder rendered (tests/golden/near_sky/T_parent_frames.npz,
tools/record_near_sky.py: sha256 of the float4 bits, of the RGBA8 words and of
the per-pixel step map, and rm_stats' evals / flop / skipped with the certified
and reflection-cleared counts), and the timed kernels to the instrumented ones,
float4 and RGBA8, tile8, tile16 and persistent, row-major and in adaptive order
with latency tiles, at N - 1 and N steps of every rung and at 128, 207, 208 and
256.

The poses (tests/near_sky_ref.py POSE_SET): P0; looking along a face from 0.15,
0.07 and 0.03 in front of its plane, where whole waves first qualify at the
second, third and fourth rung; the rotated sponge's silhouette; the camera
inside the cube inflated by 0.1; the sponge behind the camera; origins 60 and
52 away.  The numpy restatement says, on the CPU and before the GPU is used, which
waves qualify under each cap, and the new count must agree.
"""
import hashlib
import os

import numpy as np
import pytest

import raymarching_amd as rm
from raymarching_amd import POSES, S0_POSE
from tests import far_sky_ref as fs
from tests import near_sky_ref as ref
from tests import sentinel

pytestmark = pytest.mark.gpu

# (a folder of its own: the golden tests read every golden/T_*.npz as a reference-GLSL fixture)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "near_sky", "T_parent_frames.npz")

SIZES = ref.SIZES
CAPS = ref.CAPS
KERNELS = ["tile8", "tile16", "persist"]
STATS = ["evals", "flop", "skipped", "certified", "reflection_cleared"]  # the five old counts


def case_name(pose_name, W, H, steps):
    return f"{pose_name}_{W}x{H}_{steps}"


CASES = {case_name(p, W, H, s): (p, W, H, s) for p in ref.POSE_SET for W, H in SIZES for s in CAPS}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


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
    """What tools/record_near_sky.py stores of one case (run on the commit before the ladder)."""
    f4, w8, emap, st = render_instrumented(r, name)
    return {f"{name}.sha": np.array([sha(f4), sha(w8), sha(emap)]),
            f"{name}.stats": np.array([st[k] for k in STATS], np.uint64)}


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def restated(pose_name):
    """case -> (strict, loose) counts of the waves that pass the new vote and not the old one; asserts the pose's
    intent, on the CPU"""
    pose, rung = ref.POSE_SET[pose_name]
    out = {}
    for W, H in SIZES:
        tiles = ((W + 7) // 8) * ((H + 7) // 8)
        for cap in CAPS:
            s, l = ref.near_tiles(pose, W, H, cap)
            assert (s > 0) == (l > 0), (pose_name, W, H, cap, s, l)  # the restatement decides
            out[case_name(pose_name, W, H, cap)] = (s, l)
            n_rung = ref.N_OF[rung]
            if cap < n_rung:
                assert l == 0, (pose_name, W, H, cap, l)  # no wave before the pose's rung
            elif pose_name.startswith(("face", "inside")):
                assert s >= tiles // 4, (pose_name, W, H, cap, s, tiles)  # whole waves from the rung on
            elif cap < fs.K_N0:
                assert s > 0, (pose_name, W, H, cap, s)
        if pose_name == "behind" or pose_name == "from_60":  # with the far-sky vote on, its waves are not new
            assert out[case_name(pose_name, W, H, 256)] == (0, 0) and out[case_name(pose_name, W, H, fs.K_N0)] == (0, 0)
    return out


@pytest.mark.parametrize("pose_name", list(ref.POSE_SET))
def test_instrumented_frames_and_counts(R, golden, pose_name):
    want_near = restated(pose_name)  # (the pose's intent, on the CPU, before the GPU is used)
    near_by = {}
    for name in [n for n, c in CASES.items() if c[0] == pose_name]:
        _, W, H, steps = CASES[name]
        strict, loose = want_near[name]
        for kernel in ["auto", "tile16", "persist"]:
            f4, w8, emap, st = render_instrumented(R, name, kernel)
            what = f"{name} {kernel}"
            print(f"{what}: restated new waves {strict}..{loose}; " + " ".join(f"{k} {st[k]}" for k in STATS + ["near_sky"]))
            assert [sha(f4), sha(w8), sha(emap)] == golden[f"{name}.sha"].tolist(), \
                f"{what}: instrumented float4 / RGBA8 / step map differ from the parent commit's"
            # the five old counts are the parent's: the new count stands beside them, not in them
            assert [st[k] for k in STATS] == golden[f"{name}.stats"].tolist(), (what, st)
            assert (st["near_sky"] > 0) == (strict > 0), (what, st, strict, loose)
            assert st["near_sky"] + st["reflection_cleared"] + st["certified"] + st["skipped"] <= st["evals"], (what, st)
            # a qualifying wave takes at least one primary step per lane, and no march of it more than N(m) steps
            # plus the reflection's steps below depth 3
            assert st["near_sky"] <= (steps + 2) * 64 * loose, (what, st, loose)
            assert int(emap.sum()) == st["evals"]
            near_by.setdefault((W, H, kernel), {})[steps] = st["near_sky"]
    # identical across the caps within one rung (the same waves, the same marches to ZFAR), as long as the
    # far-sky vote does not change under them
    for key, by in near_by.items():
        n = ref.N_OF
        assert by[n[2]] == by[128] == by[n[3] - 1], (pose_name, key, by)
        assert by[n[3]] == by[fs.K_N0 - 1] and by[fs.K_N0] == by[256], (pose_name, key, by)
        assert by[n[0] - 1] == 0, (pose_name, key, by)  # below the smallest N: no rung
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
        # (counted by the instrumented kernels only)
        assert st["near_sky"] == 0 and st["reflection_cleared"] == 0 and st["certified"] == 0 and st["skipped"] == 0, st
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


@pytest.mark.parametrize("scene,pose,steps", [("S0", S0_POSE, 64), ("O", POSES["P0"], 128), ("O", POSES["P2"], 256)])
def test_other_scenes_count_nothing(R, scene, pose, steps):
    """The ladder is scene T's alone: scene O's distance is not bounded below by the sponge's box term."""
    R.load_scene(rm.SCENE_FILES[scene])
    R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    R.set_params(max_steps=steps, shadow_max_steps=0, count_evals=1, kernel="auto", schedule=0)
    for W, H in SIZES:
        _, st = R.render(W, H, stats=True)
        assert st["evals"] > 0 and st["near_sky"] == 0, (scene, W, H, st)


@pytest.mark.parametrize("pose_name", ["face_003", "behind"])
def test_small_step_caps_march_as_before(R, pose_name):
    """max_steps of 1, 7 and 38, below the smallest N: a sky ray's march of so few steps ends short of ZFAR, so no
    rung may be on -- the timed frame is the instrumented one, bit for bit, and nothing is counted."""
    pose = ref.POSE_SET[pose_name][0]
    R.load_scene(rm.SCENE_FILES["T"])
    R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    for W, H in SIZES:
        for cap in (1, 7, ref.N_OF[0] - 1):
            R.set_params(max_steps=cap, shadow_max_steps=0, count_evals=1, kernel="auto", schedule=0)
            want4, st = R.render(W, H, stats=True)
            want8 = bits(R.render_rgba8(W, H))
            assert st["near_sky"] == 0, (pose_name, W, H, cap, st)
            for kernel in KERNELS:
                R.set_params(count_evals=0, kernel=kernel)
                assert np.array_equal(bits(R.render(W, H)), bits(want4)), (pose_name, W, H, cap, kernel)
                assert np.array_equal(bits(R.render_rgba8(W, H)), want8), (pose_name, W, H, cap, kernel)
    R.set_params(kernel="auto")


def test_a_pose_that_does_not_keep_unit_length_falls_back_to_the_far_sky_cube(R):
    """u_time so large that glsl_cos(x) = glsl_sin(x + pi/2) no longer resolves the quarter turn: the sponge's
    rotation is no rotation, the ladder's proof does not hold, and the host offers the far-sky cube alone, from
    N0 steps on (rm_render_host.cpp pose_const).  Whatever the rotation is, timed equals instrumented."""
    pose = ref.POSE_SET["face_003"][0]
    R.load_scene(rm.SCENE_FILES["T"])
    for time in (3.0e7, 1.0e9):
        R.set_pose(pose["pos"], pose["mouse"], time)
        for cap in (ref.N_OF[3], 256):
            R.set_params(max_steps=cap, shadow_max_steps=0, count_evals=1, kernel="auto", schedule=0)
            want4, st = R.render(64, 64, stats=True)
            want8 = bits(R.render_rgba8(64, 64))
            R.set_params(count_evals=0)
            assert np.array_equal(bits(R.render(64, 64)), bits(want4)), (time, cap)
            assert np.array_equal(bits(R.render_rgba8(64, 64)), want8), (time, cap)


# ---- rays of their own (rm_shade_rays): partly filled and mixed waves


def band_rays(time, seed=20261020):
    """sponge-space rays that pass each rung's cube by -0.004 to +0.004, along a face and across an edge, with the
    poses whose 1 x 1 frames look along them -> dict(pos, mouse, o, d)"""
    from tests import shade_t_rays as st
    rng = np.random.RandomState(seed)
    P, D = [], []
    for _, r, _ in ref.LADDER:
        n = 128
        g = float(r) + rng.uniform(-0.004, 0.004, size=n)
        k = rng.randint(0, 3, size=n)
        a, b = (k + 1) % 3, (k + 2) % 3
        sa, sb = rng.choice([-1.0, 1.0], size=n), rng.choice([-1.0, 1.0], size=n)
        i = np.arange(n)
        p, d = np.zeros((n, 3)), np.zeros((n, 3))
        p[i, a], p[i, b], p[i, k] = sa * g, rng.uniform(-1.0, 1.0, size=n) * g, rng.uniform(-1.0, 1.0, size=n) * g
        d[i, a], d[i, b], d[i, k] = 0.0, rng.uniform(-1.0, 1.0, size=n), rng.choice([-1.0, 1.0], size=n)
        edge = i % 3 == 0  # a third across the edge (sa g, sb g) instead
        p[i[edge], b[edge]] = (sb * g)[edge]
        d[i[edge], a[edge]] = (sa * rng.uniform(0.3, 1.0, size=n))[edge]
        d[i[edge], b[edge]] = (-sb * rng.uniform(0.3, 1.0, size=n))[edge]
        d[i[edge], k[edge]] = rng.uniform(-0.6, 0.6, size=n)[edge]
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        P.append(p - d * rng.uniform(2.0, 6.0, size=(n, 1)))
        D.append(d)
    pos, mouse = st.poses_from_sponge(time, np.concatenate(P), np.concatenate(D))
    return dict(pos=np.ascontiguousarray(pos, np.float32), mouse=np.ascontiguousarray(mouse, np.float32))


@pytest.mark.parametrize("cap", [ref.N_OF[0], ref.N_OF[2], ref.N_OF[3], 256])
def test_shade_rays_in_the_new_band_give_their_instrumented_pixels(R, torch_cuda, cap):
    """Rays in each rung's band with tests/shade_t_rays.py's classes (A far-sky, D hits, E inside the far-sky
    cube), as lists and as ray images of width 8: a whole wave that qualifies, the same wave with one lane that does
    not (at lanes 0, 31 and 63), with a hit lane, and a partly filled wave of 37.  Every ray gives its
    instrumented 1 x 1 pixel, float4 and RGBA8, whatever its wave-mates."""
    torch = torch_cuda
    from tests import shade_t_rays as st
    time = 0.0
    s = st.ray_set(time)
    band = band_rays(time)
    A, Dh, E = st.members(s, "A")[:24], st.members(s, "D")[:8], st.members(s, "E")[:4]
    pos = np.concatenate([band["pos"], s["pos"][A], s["pos"][Dh], s["pos"][E]])
    mouse = np.concatenate([band["mouse"], s["mouse"][A], s["mouse"][Dh], s["mouse"][E]])
    nb = len(band["pos"])
    iA, iD, iE = nb + np.arange(24), nb + 24 + np.arange(8), nb + 32 + np.arange(4)

    def one_pixel(count_evals):
        R.load_scene(rm.SCENE_FILES["T"])
        R.set_uniform("u_time", time)
        R.set_params(max_steps=cap, shadow_max_steps=0, count_evals=count_evals, kernel="auto", schedule=0)
        px, w8, dirs = [], [], []
        for p, m in zip(pos, mouse):
            R.set_uniform("u_pos", *map(float, p))
            R.set_uniform("u_mouse", *map(float, m))
            px.append(R.render(1, 1).reshape(4))
            w8.append(R.render_rgba8(1, 1).reshape(1))
            dirs.append(R.camera_rays(1, 1)[1].reshape(3))
        return bits(torch.stack(px)), bits(torch.cat(w8)), torch.stack(dirs).cpu().numpy()

    ref4, ref8, dirs = one_pixel(1)
    # the restatement on the GPU's own directions, with slack both ways: rays that surely pass / surely fail the
    # vote at this cap's radius
    o, d = fs.to_sponge(pos, dirs, time)
    r = ref.radius(cap)
    surely = ref.near_sky_ray(o, d, np.float32(r * (1 + 1e-4)), np.float32(fs.K_FAR * (1 + 1e-4)))
    maybe = ref.near_sky_ray(o, d, np.float32(r * (1 - 1e-4)), np.float32(fs.K_FAR * (1 - 1e-4)))
    old = ref.near_sky_ray(o, d, np.float32(fs.K_R * (1 - 1e-4)), np.float32(fs.K_FAR * (1 - 1e-4)))
    new_only = np.flatnonzero(surely[:nb] & (~old[:nb] if cap >= fs.K_N0 else True))
    fail = np.flatnonzero(~maybe[:nb])
    assert not maybe[iD].any() and surely[iA].all()  # (class E lies inside the far-sky cube, not inside every rung's)
    assert len(fail) >= 8, (cap, len(fail))
    if cap >= ref.N_OF[1]:  # (at the first rung the band rays that pass are the far-sky cube's own)
        assert len(new_only) >= 64, (cap, len(new_only))
    passing = np.concatenate([new_only, iA])[:64] if len(new_only) < 64 else new_only[:64]
    assert len(passing) == 64
    comps = {"whole wave": passing, "partly filled": passing[:37]}
    for lane in (0, 31, 63):
        comps[f"one failing lane at {lane}"] = np.insert(passing[:63], lane, fail[lane % len(fail)])
    comps["a hit lane at 17"] = np.insert(passing[:63], 17, iD[0])
    comps["a class E ray at 40, far-sky rays among them"] = np.insert(np.concatenate([passing[:40], iA[:23]]), 40, iE[0])
    comps["everything"] = np.random.RandomState(3).permutation(len(pos))
    R.set_params(count_evals=0)
    fails, compared = [], 0
    for name, idx in comps.items():
        for width in (0, 8) if len(idx) % 8 == 0 else (0,):
            got4 = bits(R.shade_rays(pos[idx], dirs[idx], width=width, output="display", vignette=False))
            got8 = bits(R.shade_rays(pos[idx], dirs[idx], width=width, output="display", vignette=False, rgba8=True))
            bad = np.flatnonzero((got4.reshape(-1, 4) != ref4[idx]).any(-1) | (got8.reshape(-1) != ref8[idx]))
            compared += len(idx)
            fails += [f"{name}, width {width}, lane {k}: ray {idx[k]}" for k in bad]
    print(f"{cap} steps (r = {r}): {len(new_only)} band rays surely pass, {len(fail)} surely fail; {compared} ray results "
          f"compared with the instrumented 1 x 1 frames, {len(fails)} differ")
    assert not fails, "\n".join(fails[:20])
