"""Scene T's exact shortcuts, ray by ray, through the ray entry points
(rm_shade_rays, rm_render_aa_rgba8, rm_render_accumulate) at step caps where
all four are live: the far-sky wave vote, the box-only probes
of far-sky waves (2.23), the soft-shadow certificate (2.24) and the reflection
certificate (2.25), all in render_T_from.

The yardstick that decides is the instrumented kernel (count_evals = 1), which
takes every reference step: a 1 x 1 frame at pose (pos, mouse) renders exactly
one ray with a vignette factor of 1, so shade_rays(pos, dir, "display") of that
ray, with an origin of its own and whatever rays share its wave, must give that
pixel in every bit, float4 and RGBA8.  tests/shade_t_rays.py draws the rays
(classes A to G) and composes the waves; the numpy restatements there state
what each wave holds and decide no colour.  The oracle's 1 x 1 frames are the
second yardstick, at scene T's parity policy.
"""
import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from tests import aa_ref, far_sky_ref, refl_clear_ref
from tests import shade_t_rays as st
from tests.parity import POLICY, assert_parity, diff_stats
from tests.shade_ref import pose_dirs
from tests.test_far_sky_gpu import POSE_SET as FAR_SKY_POSES

N0 = far_sky_ref.K_N0
CAPS = [N0 - 1, N0, 256]            # far-sky off, on at its bound, the benchmark's cap
K_STEPS = refl_clear_ref.K_STEPS    # 28: the reflection certificate needs max_steps >= kSteps
W, H = 61, 37                       # ragged tiles, partly filled waves
SHARED_POSES = {"P0": FAR_SKY_POSES["P0"], "silhouette_t30": FAR_SKY_POSES["silhouette_t30"],
                "wall": refl_clear_ref.POSE_SET["wall"][0]}
AA_POSES = {k: FAR_SKY_POSES[k] for k in ("P0", "silhouette_t30", "from_52")}


# ------------------------------------------------------------------ CPU


@pytest.mark.parametrize("time", st.TIMES)
def test_ray_sets_meet_their_quotas(time):
    """conditions on the inputs of the GPU tests, by the numpy restatements; no GPU"""
    s = st.ray_set(time)
    q = st.quotas(time)
    print(f"u_time {time}: {q}")
    assert len(s["cls"]) == sum(st.SIZES.values()) == 384 and st.n_poses(s) == 374
    assert np.isfinite(s["pos"][:st.n_poses(s)]).all() and np.isfinite(s["mouse"]).all()
    # A: far-sky with margin, no two origins equal, max-norm 2 to 40, every octant
    assert q["A"] >= 128 and q["A_distinct_origins"] == q["A"]
    assert min(q["A_octants"]) >= 12 and 2.0 <= q["A_shell"][0] and q["A_shell"][1] <= 40.0
    assert min(q["A_shell_thirds"]) >= 16, q["A_shell_thirds"]
    # B: sky rays whose miss test flips within 0.02 of kFarSkyR, 12 on each side (the far point clear: the miss
    # test alone decides far_sky_ray)
    assert q["B_miss"] >= 12 and q["B_graze"] >= 12 and q["B_miss"] + q["B_graze"] >= 32
    assert q["B_far"] == q["B_miss"] and q["B_not_far"] == q["B_graze"]
    # C: far point in [3.9, 4.3], 12 on each side of 4.1, from 46 to 54 away
    assert q["C_above"] >= 12 and q["C_below"] >= 12 and q["C_above"] + q["C_below"] >= 32
    assert 46.0 <= q["C_distance"][0] and q["C_distance"][1] <= 54.0
    # D: hits, in groups
    assert q["D"] >= 128
    for name, least in st.d_quota(time).items():
        assert q["D_" + name] >= least, (name, q["D_" + name], least)
    # E: inside the inflated cube, 0.05 clear of the sponge; none far-sky ("an origin inside the cube fails every test")
    assert q["E"] >= 32 and q["E_inside_unit_cube"] >= 12 and q["E_far"] == 0
    assert q["E_hit"] >= 8 and q["E_sky"] >= 8  # (they look at inner walls and outward)
    # F: the argument edges
    assert q["F"] >= 16 and q["F_below_1024"] >= 2 and q["F_above_1024"] >= 2 and q["F_1e4"] >= 2 and q["F_1e6"] >= 2
    axis = pose_dirs(s["mouse"][s["cls"][:st.n_poses(s)] == "F"][:10])
    assert (np.sort(np.abs(axis), -1)[:, :2] < 1e-7).all()  # (axis-parallel)
    # G: none is a finite unit ray
    g = st.members(s, "G")
    d = st.all_dirs(s)[g].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(s["pos"][g]).all(-1) & (np.abs((d * d).sum(-1) - 1.0) <= 1e-4)
    assert len(g) >= 6 and not ok.any()


def test_shadow_ratio_sides_over_the_three_sets():
    """the soft-shadow slope of an outer face is set by u_time (tests/shade_t_rays.py S_SIDE): each set has one
    side of rmsc::kRatio within 0.05, the three together both"""
    q = {t: st.quotas(t) for t in st.TIMES}
    assert sum(q[t]["D_s_above"] for t in st.TIMES) >= 8 and sum(q[t]["D_s_below"] for t in st.TIMES) >= 8


@pytest.mark.parametrize("time", st.TIMES)
def test_compositions_hold_what_they_say(time):
    s = st.ray_set(time)
    comps = st.compositions(time)
    c = st.classes(time)
    cls = s["cls"]
    assert st.wave_votes(time, comps["A_only"]["idx"]).all()      # both waves vote far
    mixed = comps["mixed"]
    votes = st.wave_votes(time, mixed["idx"])
    assert len(votes) == 20 == len(mixed["waves"])
    for w, lane in enumerate(list(st.MIXED_LANES) * 5):
        wave = mixed["idx"][64 * w:64 * w + 64]
        other = np.flatnonzero(cls[wave] != "A")
        assert other.tolist() == [lane] and cls[wave[lane]] == "BCDEF"[w // 4], mixed["waves"][w]
        assert votes[w] == bool(c["far"][wave[lane]])             # (the one other ray decides the vote)
    assert votes[:8].tolist() == [True, False] * 4                # B and C: the sides of their thresholds in turn
    assert not votes[8:16].any()                                  # no wave with a D or an E ray votes far
    assert c["hit"][mixed["idx"][64 * 8 + 0]] and c["hit"][mixed["idx"][64 * 9 + 31]]
    assert sorted(comps["all_shuffled"]["idx"].tolist()) == list(range(len(cls)))
    assert not st.wave_votes(time, comps["all_shuffled"]["idx"]).all()
    assert len(comps["cut_321"]["idx"]) % 64 == 1 and len(comps["cut_357"]["idx"]) % 64 == 37
    wg = comps["A_with_G"]["idx"]
    assert np.flatnonzero(cls[wg[:64]] == "G").tolist() == [0, 7, 63] and (cls[wg[64:]] == "G").all()


# ------------------------------------------------------------------ GPU


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def load(R, time, steps, count_evals, pose=None):
    R.load_scene(rm.SCENE_FILES["T"])
    if pose is not None:
        R.set_pose(pose["pos"], pose["mouse"], pose["time"])
    else:
        R.set_uniform("u_time", float(time))
    R.set_params(max_steps=steps, shadow_max_steps=0, count_evals=count_evals, kernel="auto", schedule=0)


_DIRS, _REF = {}, {}


def gpu_dirs(R, torch, time):
    """[NP, 3] f32: the direction camera_rays(1, 1) gives at each pose of the set (once per time, read-only)"""
    if time not in _DIRS:
        s = st.ray_set(time)
        load(R, time, 256, 0)
        out = []
        for p, m in zip(s["pos"][:st.n_poses(s)], s["mouse"]):
            R.set_uniform("u_pos", *map(float, p))
            R.set_uniform("u_mouse", *map(float, m))
            o, d = R.camera_rays(1, 1)
            out.append(torch.cat([o.reshape(3), d.reshape(3)]))
        od = torch.stack(out).cpu().numpy()
        assert np.array_equal(od[:, :3], s["pos"][:st.n_poses(s)])
        d = np.ascontiguousarray(od[:, 3:])
        d.setflags(write=False)
        _DIRS[time] = d
    return _DIRS[time]


def one_pixel_frames(R, torch, time, cap, count_evals, which=None):
    """the only pixel of render(1, 1) and the word of render_rgba8(1, 1) at the poses `which` of the set (all of
    them by default) -> (bits [n, 4] u32, words [n] u32)"""
    s = st.ray_set(time)
    which = np.arange(st.n_poses(s)) if which is None else np.asarray(which)
    load(R, time, cap, count_evals)
    px, w8 = [], []
    for i in which:
        R.set_uniform("u_pos", *map(float, s["pos"][i]))
        R.set_uniform("u_mouse", *map(float, s["mouse"][i]))
        px.append(R.render(1, 1).reshape(4))
        w8.append(R.render_rgba8(1, 1).reshape(1))
    return bits(torch.stack(px)), bits(torch.cat(w8))


def instrumented(R, torch, time, cap):
    """the yardstick: one_pixel_frames with count_evals = 1 on the whole set, once per (time, cap), read-only;
    class G's rows are zeros, alpha included"""
    if (time, cap) not in _REF:
        px, w8 = one_pixel_frames(R, torch, time, cap, 1)
        px = np.concatenate([px, np.zeros((st.SIZES["G"], 4), np.uint32)])
        w8 = np.concatenate([w8, np.zeros(st.SIZES["G"], np.uint32)])
        px.setflags(write=False)
        w8.setflags(write=False)
        _REF[(time, cap)] = (px, w8)
    return _REF[(time, cap)]


def shade_compositions(R, time, dirs, comps, ref4, ref8, known=None):
    """every composition in its layouts, float4 and RGBA8, against the rays' reference bits (rows of ref4 / ref8
    by set index; `known`: the rows that have a reference) and against the same ray's bits in the compositions
    before it -> (ray results compared, list of failures, each naming composition, layout and wave)"""
    s = st.ray_set(time)
    first4, first8, first_in = {}, {}, {}
    compared, fails = 0, []
    for name, comp in comps.items():
        idx = comp["idx"]
        for width in comp["layouts"]:
            got4 = bits(R.shade_rays(s["pos"][idx], dirs[idx], width=width, output="display", vignette=False))
            got8 = bits(R.shade_rays(s["pos"][idx], dirs[idx], width=width, output="display", vignette=False, rgba8=True))
            where = f"{name}, {'list' if width == 0 else f'width {width}'}"
            for k, i in enumerate(idx):
                i = int(i)
                wave = comp["waves"][k // 64] if comp["waves"] else f"rays {64 * (k // 64)}-{64 * (k // 64) + 63}"
                tag = f"{where}, {wave}, lane {k % 64}: ray {i} (class {s['cls'][i]})"
                if i in first_in and not (np.array_equal(got4[k], first4[i]) and got8[k] == first8[i]):
                    fails.append(f"{tag} differs from its bits in {first_in[i]}")
                if i not in first_in:
                    first4[i], first8[i], first_in[i] = got4[k].copy(), got8[k], where
                if known is None or known[i]:
                    compared += 1
                    if not (np.array_equal(got4[k], ref4[i]) and got8[k] == ref8[i]):
                        fails.append(f"{tag} differs from its instrumented 1 x 1 frame: {got4[k].view(np.float32)} "
                                     f"/ {got8[k]:08x} against {ref4[i].view(np.float32)} / {ref8[i]:08x}")
    return compared, fails


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("time", st.TIMES)
def test_every_ray_in_every_wave_gives_its_instrumented_pixel(R, torch_cuda, time, cap):
    """Yardstick (a): classes A to F bit for bit against the instrumented 1 x 1 frames, class G zeros, in all five
    compositions and both layouts; a ray's bits do not depend on its wave-mates."""
    s = st.ray_set(time)
    ref4, ref8 = instrumented(R, torch_cuda, time, cap)
    dirs = st.all_dirs(s, gpu_dirs(R, torch_cuda, time))
    assert np.abs(dirs[:st.n_poses(s)] - pose_dirs(s["mouse"])).max() < 1e-6
    assert np.isfinite(ref4[:st.n_poses(s)].view(np.float32)).all() and ((ref8[:st.n_poses(s)] >> 24) == 255).all()
    assert len(np.unique(ref8)) > 32  # (hits and sky, not one colour)
    load(R, time, cap, 0)
    compared, fails = shade_compositions(R, time, dirs, st.compositions(time), ref4, ref8)
    print(f"u_time {time}, {cap} steps: {compared} ray results compared with the instrumented 1 x 1 frames, "
          f"{len(fails)} differ")
    assert not fails, "\n".join(fails[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [K_STEPS - 1, K_STEPS])
@pytest.mark.parametrize("time", st.TIMES)
def test_reflection_certificates_step_bound(R, torch_cuda, time, cap):
    """27 and 28 steps, either side of rmrc::kSteps, on the smallest composition (A_with_G) and on the four waves
    of `mixed` that hold a class D ray (the lanes the certificate can act on)."""
    s = st.ray_set(time)
    all_comps = st.compositions(time)
    mixed = all_comps["mixed"]
    comps = {"A_with_G": all_comps["A_with_G"],
             "mixed (D waves)": dict(idx=mixed["idx"][64 * 8:64 * 12], layouts=mixed["layouts"], waves=mixed["waves"][8:12])}
    used = np.unique(np.concatenate([c["idx"] for c in comps.values()]))
    poses = used[used < st.n_poses(s)]
    px, w8 = one_pixel_frames(R, torch_cuda, time, cap, 1, poses)
    ref4, ref8 = np.zeros((len(s["cls"]), 4), np.uint32), np.zeros(len(s["cls"]), np.uint32)
    ref4[poses], ref8[poses] = px, w8
    known = np.zeros(len(s["cls"]), bool)
    known[used] = True
    dirs = st.all_dirs(s, gpu_dirs(R, torch_cuda, time))
    load(R, time, cap, 0)
    compared, fails = shade_compositions(R, time, dirs, comps, ref4, ref8, known)
    print(f"u_time {time}, {cap} steps: {compared} ray results compared, {len(fails)} differ")
    assert compared == 2 * (128 + 256) and not fails, "\n".join(fails[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("time", st.TIMES)
def test_timed_one_pixel_frames_equal_the_instrumented_ones(R, torch_cuda, time):
    """places a failure of the test above: in the frame kernel (this one fails too) or in the shade path"""
    ref4, ref8 = instrumented(R, torch_cuda, time, 256)
    px, w8 = one_pixel_frames(R, torch_cuda, time, 256, 0)
    n = len(px)
    nd = int(((px != ref4[:n]).any(-1) | (w8 != ref8[:n])).sum())
    print(f"u_time {time}: {nd} of {n} timed 1 x 1 frames differ from the instrumented ones")
    assert nd == 0


@pytest.mark.gpu
@pytest.mark.parametrize("pose_name", list(SHARED_POSES))
def test_a_mixed_frames_own_rays_against_the_instrumented_frame(R, torch_cuda, pose_name):
    """the shared origin and the same origin repeated per ray, at 256 and 208 steps, float4 and RGBA8, as a ray
    image with the vignette: the instrumented frame's bits"""
    pose = SHARED_POSES[pose_name]
    for cap in (256, N0):
        load(R, None, cap, 1, pose)
        ref4, ref8 = bits(R.render(W, H)).reshape(-1, 4), bits(R.render_rgba8(W, H)).reshape(-1)
        assert len(np.unique(ref8)) > 8
        R.set_params(count_evals=0)
        origin, dirs = R.camera_rays(W, H)
        own = origin.reshape(1, 3).repeat(W * H, 1).contiguous()
        for what, o in (("shared origin", origin), ("origins per ray", own)):
            kw = dict(width=W, output="display", vignette=True)
            nd4 = int((bits(R.shade_rays(o, dirs, **kw)) != ref4).any(-1).sum())
            nd8 = int((bits(R.shade_rays(o, dirs, rgba8=True, **kw)) != ref8).sum())
            print(f"{pose_name} {W}x{H}, {cap} steps, {what}: {nd4} float pixels and {nd8} RGBA8 words differ from "
                  f"the instrumented frame")
            assert nd4 == 0 and nd8 == 0, (pose_name, cap, what)


_ORACLE = {}


def oracle_pixels(time, cap):
    if (time, cap) not in _ORACLE:
        s = st.ray_set(time)
        px = np.stack([oracle.render("T", 1, 1, pos=tuple(map(float, p)), mouse=tuple(map(float, m)), time=time,
                                     max_steps=cap)[0][0, 0] for p, m in zip(s["pos"][:st.n_poses(s)], s["mouse"])])
        px.setflags(write=False)
        _ORACLE[(time, cap)] = px
    return _ORACLE[(time, cap)]


@pytest.mark.gpu
@pytest.mark.parametrize("time", st.TIMES)
def test_rays_against_the_oracles_one_pixel_frames(R, torch_cuda, time):
    """Yardstick (b): 256 steps against oracle.render("T", 1, 1) per ray, at scene T's parity policy
    (tests/parity.py), unchanged.

    Classes A to F together miss it on the MI355X while yardstick (a) holds on every ray, because of class F's two
    rays from 1e6 away.  Measured, at u_time 0 / 1.25 / 30: classes A to E, 352 rays, all within 2e-3 (max |d|
    7.5e-5 / 3.6e-5 / 5.1e-5); class F 20 / 19 / 20 of 22 within 2e-3 and 20 of 22 within 1e-2; together f1e2
    0.99465 against the policy's 0.995 and mean 5.35e-3 against 1e-3.  On those two rays the oracle's pixel is
    NaN (where points are 1e6 large its normal's probes, 0.001 apart, cannot differ in float32) and the kernels'
    is finite, instrumented and timed alike: the instrumented march itself differs from the oracle there, and no
    shortcut is involved (the timed and the instrumented pixels are equal in every bit).  So the policy is held on
    the classes with margin, A and the parts of D and E that straddle no certificate's ratio; and, since they
    pass it too, on every ray but those two."""
    s = st.ray_set(time)
    n = st.n_poses(s)
    dirs = gpu_dirs(R, torch_cuda, time)
    load(R, time, 256, 0)
    got = R.shade_rays(s["pos"][:n], dirs, width=0, output="display", vignette=False)
    ref = oracle_pixels(time, 256)
    cls = s["cls"][:n]
    for cl in "ABCDEF":
        m = cls == cl
        print(f"u_time {time} class {cl} ({int(m.sum())} rays): {diff_stats(got[m], ref[m])}")
    print(f"u_time {time} classes A-F ({n} rays): {diff_stats(got, ref)} vs {POLICY['T']}")
    d = np.abs(np.nan_to_num(got[:, :3].astype(np.float64), nan=9.0) - np.nan_to_num(ref[:, :3].astype(np.float64), nan=-9.0)).max(-1)
    for i in np.flatnonzero(d > 2e-3):
        print(f"  ray {i} (class {cls[i]}, pos {s['pos'][i]}): shade_rays {got[i]}, oracle {ref[i]}")
    g = st.d_groups(st.classes(time))
    straddle = g["s_below"] | g["s_above"] | g["r_below"] | g["r_above"]
    margin = (cls == "A") | (((cls == "D") | (cls == "E")) & ~straddle)
    assert margin.sum() >= 128 + 64
    stats = assert_parity("T", got[margin], ref[margin], label=f"oracle 1x1 frames, u_time {time}, A and D, E off the ratios")
    print(f"u_time {time} classes with margin ({int(margin.sum())} rays): {stats}")
    far_off = np.abs(s["pos"][:n]).max(-1) > 5.0e5  # class F's two origins 1e6 away
    assert far_off.sum() == 2 and (cls[far_off] == "F").all()
    assert np.isfinite(got).all() and np.isnan(ref[far_off, :3]).all() and np.isfinite(ref[~far_off]).all()
    stats = assert_parity("T", got[~far_off], ref[~far_off], label=f"oracle 1x1 frames, u_time {time}, all but 1e6 away")
    print(f"u_time {time} every ray but the two from 1e6 away ({int((~far_off).sum())} rays): {stats}")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [N0, 256])
@pytest.mark.parametrize("pose_name", list(AA_POSES))
def test_accumulate_and_render_aa_with_the_shortcuts_on(R, torch_cuda, pose_name, cap):
    """rm_render_accumulate's jittered frames, timed against instrumented, bit for bit; render_aa against those
    instrumented frames blended on the host (tests/test_far_sky_gpu.py's method), every pixel (threshold 0, K = 2
    and 4) and the edge pixels only (threshold 32, K = 4: the others are the plain instrumented frame's)."""
    torch = torch_cuda
    pose = AA_POSES[pose_name]

    def accumulate(K):
        frames = []
        for seed in aa_ref.seeds(K):
            R.set_uniform("u_seed1", float(seed[0]), float(seed[1]))
            acc = torch.full((H, W, 4), float("nan"), device="cuda")
            frames.append(R.render_accumulate(W, H, acc).cpu().numpy())
        R.set_uniform("u_seed1", 0.5, 0.5)
        return frames

    load(R, None, cap, 1, pose)
    R.set_uniform("u_sample_part", 1.0)
    ref = {K: accumulate(K) for K in (2, 4)}
    plain = bits(R.render_rgba8(W, H))
    R.set_params(count_evals=0)
    timed = accumulate(4)
    nd = sum(int((bits(a) != bits(b)).any(-1).sum()) for a, b in zip(timed, ref[4]))
    print(f"{pose_name} {W}x{H}, {cap} steps: {nd} pixels of the 4 timed accumulate frames differ from the instrumented ones")
    assert nd == 0
    for K in (2, 4):
        want = oracle.pack_rgba8(aa_ref.tree_mean(ref[K]))
        out, stt = R.render_aa(W, H, samples=K, threshold=0, stats=True)
        assert stt["refined"] == W * H
        ndiff = int((bits(out) != want).sum())
        print(f"{pose_name} {W}x{H}, {cap} steps, K={K}, threshold 0: {ndiff} words differ from the blend")
        assert ndiff == 0
    want = oracle.pack_rgba8(aa_ref.tree_mean(ref[4]))
    out, mask, stt = R.render_aa(W, H, samples=4, threshold=32, mask=True, stats=True)
    m = mask.cpu().numpy() == 1
    assert np.array_equal(m, aa_ref.edge_mask(plain, 32) == 1) and stt["refined"] == int(m.sum())
    ndiff = int((bits(out) != np.where(m, want, plain)).sum())
    print(f"{pose_name} {W}x{H}, {cap} steps, K=4, threshold 32: {int(m.sum())} refined, {ndiff} words differ")
    assert ndiff == 0
