"""The probe forms of the built-in scene distances, point by point.

Every scene distance exists twice (rm_device.h): the exact form keeps the
GLSL's roundings (tests/test_scene_o_skips.py checks it bit for bit), the
probe form serves the AO / soft-shadow / thickness probes, scene O's
plane_probes and all of scene T's marches, in different arithmetic: fused
rotations and sums of squares, folds as |y - rint(y)| around k + 1/2, sminCubic
as one fma.  rm_scene_eval_form reaches it (RM_FORM_PROBE; RM_FORM_PROBE_NB1:
one fold exit test instead of three, the latency tiles' variant), and with
`aux` the slack of scene_dist_O that plane_probes thresholds.

The reference is the oracle's plain sceneSDF; the bound is test_scene_o_skips'
_close, 1e-5 + 1e-5 |d| with no allowance (3-Lipschitz sponge, <= 1.5 ulp(4)
per fused rotation stage).  Every GPU test prints its measured maxima.
"""
import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from tests import scene_o_rules as rules
from tests.test_scene_o_skips import TIME_IDS, TIMES, _close, _unit

f32 = np.float32
FOLD_SETS = ["fold exit", "fold wall", "fold kink"]
SH = (0.5, 1.5, 4.5)  # sponge_folds' s/2 per fold


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def _err(hip, ref):
    return np.abs(hip.astype(np.float64) - ref.astype(np.float64))


def _report(title, B, time, err, ok):
    """Maximum error per point set and per expected_skip kind (the style of
    test_scene_o_skips._mismatch_report); returns the text."""
    _, kind = rules.expected_skip(B.points, time)
    lines = [f"{title}: max {err.max():.4g}, {int((~ok).sum())} of {len(err)} outside the bound"]
    for what, ids, names in (("kind", kind, rules.KINDS), ("set", B.set_id, B.names)):
        for i, name in enumerate(names):
            sel = ids == i
            if sel.any():
                j = int(np.flatnonzero(sel)[np.argmax(err[sel])])
                lines.append(f"  {what} {name}: max {err[j]:.4g} at p={B.points[j].tolist()}, "
                             f"{int((sel & ~ok).sum())} of {int(sel.sum())} outside")
    return "\n".join(lines)


# --------------------------------------------------- tie points of the folds


def fold_tie_points(time, seed=17, per=48):
    """World points whose sponge-space coordinate times s/2 lies within 4 ulp of
    an integer k (where the exact form's floor steps) or of k + 1/2 (where the
    probe form's rint ties), per fold and axis: the target in sponge space, the
    other two coordinates inside the sponge's box, mapped back by the inverse
    rotation in float64 and rounded; kept where the float32 forward rotation
    (rules.quantities) lands within the 4 ulp.  Returns (points, labels)."""
    rng = np.random.default_rng([seed, int(f32(time).view(np.uint32))])
    ry_c, ry_s, rx_c, rx_s = (float(v) for v in rules.sponge_rotation(time))
    pts, labels = [], []
    for m, sh in enumerate(SH):
        for c in range(3):
            for half in (0.0, 0.5):
                ks = np.arange(np.ceil(-1.4 * sh), np.floor(1.4 * sh) + 1.0) + half
                ks = ks[np.abs(ks / sh) <= 1.45]
                t = np.repeat(ks, per * 24)
                q = rng.uniform(-1.45, 1.45, (len(t), 3))
                ulp = np.spacing(np.maximum(np.abs(t), 0.5).astype(f32)).astype(np.float64)
                q[:, c] = (t + rng.integers(-4, 5, len(t)) * ulp) / sh
                # q = (x1, y2, z2) with x1 = x c + z s, z1 = -x s + z c, y2 = y c' - z1 s', z2 = y s' + z1 c'
                ys = q[:, 1] * rx_c + q[:, 2] * rx_s
                z1 = -q[:, 1] * rx_s + q[:, 2] * rx_c
                x = q[:, 0] * ry_c - z1 * ry_s
                z = q[:, 0] * ry_s + z1 * ry_c
                p = np.stack([x, ys + 3.0, z], -1).astype(f32)
                h = rules.quantities(p, time, d0=False)["q"][:, c] * f32(sh)
                keep = np.abs(h.astype(np.float64) - t) <= 4.0 * ulp
                for k in ks:  # (every k keeps its share)
                    sel = np.flatnonzero(keep & (t == k))[:per]
                    pts.append(p[sel])
                    labels += [(m, c, half, len(sel))]
    return np.concatenate(pts), labels


def test_fold_tie_points_reach_every_fold_axis_and_kind():
    """CPU: the generator lands points on every (fold, axis, k or k + 1/2), and
    at u_time 0 (a rotation by 180 degrees about x alone) some of them exactly
    on a tie."""
    for time in (TIMES[0], TIMES[2], TIMES[4]):
        pts, labels = fold_tie_points(time)
        counts = {}
        for m, c, half, n in labels:
            counts[(m, c, half)] = counts.get((m, c, half), 0) + n
        print(f"u_time {time}: {len(pts)} tie points, fewest per (fold, axis, kind) {min(counts.values())}")
        assert len(counts) == 18 and min(counts.values()) >= 16, counts
        assert np.abs(pts - np.array(rules.SPONGE_C, f32)).max() <= 2.6
    pts, _ = fold_tie_points(TIMES[0])
    q = rules.quantities(pts, TIMES[0], d0=False)["q"]
    on_tie = sum(int((np.mod(q * f32(sh) * f32(2.0), f32(1.0)) == 0).sum()) for sh in SH)
    assert on_tie >= 100, on_tie


# ------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("time", TIMES, ids=TIME_IDS)
@pytest.mark.parametrize("scene", ["O", "OG"])
def test_scene_o_probe_form_and_slack(R, scene, time):
    """scene_dist<SC, kProbeForm> at every branch boundary against the oracle
    under _close, its slack against the float32 rules under the same bound, and
    the skip's claim: wherever the GPU's slack is >= 0 both the GPU's probe
    distance and the oracle's sceneSDF are p.y bit for bit.

    Measured on the MI355X, scenes O and OG alike, maxima over the five TIMES:
    distance 1.9e-6 on the sets near the scene (the sponge-dominance points;
    9.5e-7 on the others) and 9.8e-4 = 2e-7 |d| on "far" (|p| up to 1e4); slack 0
    at u_time 0, 9.5e-7 near the scene, 1.95e-3 = 2e-7 |slack| on "far"."""
    B = rules.boundary_points(time)
    R.load_scene(rm.SCENE_FILES[scene])
    R.set_uniform("u_time", time)
    hip, aux = R.scene_eval(B.points, form="probe", aux=True)
    ref = oracle.scene_dist(scene, B.points, time=time)
    assert np.isfinite(ref).all() and np.isfinite(hip).all() and np.isfinite(aux).all()
    err, ok = _err(hip, ref), _close(hip, ref)
    text = _report(f"scene {scene} u_time {time} probe distance", B, time, err, ok)
    slack = rules.quantities(B.points, time, d0=False)["slack"]
    # The bound on the slack keeps _close's relative term: the reference is the float32 rules with the
    # unfused rotation, the kernel's q is fused, and on "far" both round at |q| ~ 1e4 (ulp 9.8e-4): the
    # measured 1.95e-3 there is two such ulps, 2e-7 |slack|.  Within |p| < 10 the term adds at most 1e-4 to
    # the absolute 1e-5, and the measured maximum there is 9.5e-7, under the absolute part alone.
    serr, sok = _err(aux, slack), _close(aux, slack)
    near = np.abs(B.points).max(-1) < 10.0
    assert (serr[near] <= 1e-5).all(), float(serr[near].max())
    text += "\n" + _report(f"scene {scene} u_time {time} slack", B, time, serr, sok)
    plane = aux >= f32(0.0)
    y = B.points[:, 1]
    text += f"\n  slack >= 0 at {int(plane.sum())} points"
    print(text)
    assert ok.all(), text
    assert sok.all(), text
    assert plane.sum() >= 5000, int(plane.sum())
    assert np.array_equal(hip[plane], y[plane]), B.points[plane][hip[plane] != y[plane]][:4]
    assert np.array_equal(ref[plane], y[plane]), B.points[plane][ref[plane] != y[plane]][:4]


@pytest.mark.gpu
@pytest.mark.parametrize("time", TIMES[:3], ids=TIME_IDS[:3])
def test_scene_o_probe_sets_are_the_plane_on_the_gpu(R, time):
    """plane_probes: where the GPU's slack at a shading point is >= 2.05 the
    GPU's probe form is p'.y at the normal probe points, the AO probe points
    and a sample of the thickness probe points (test_probe_sets_are_plane_only
    states this for the oracle; here for the kernel's own probe form, at shading
    points on both sides of the threshold).

    Measured on the MI355X: no probe off the plane at any of the three times."""
    K = rules.kernel_constants()
    rng = np.random.default_rng(11)
    p = rng.uniform([-30.0, -0.06, -30.0], [30.0, 0.06, 30.0], (40000, 3)).astype(f32)
    s = rules.quantities(p, time, d0=False)["slack"]
    p = p[s >= K["probe_slack"] - f32(1e-4)][:4000]
    # both sides of the threshold: more candidates of the same kind, kept within 0.05 of it
    near = rng.uniform([-30.0, -0.06, -30.0], [30.0, 0.06, 30.0], (400000, 3)).astype(f32)
    near = near[np.abs(rules.quantities(near, time, d0=False)["slack"] - K["probe_slack"]) < f32(0.05)][:2000]
    assert len(near) >= 400, len(near)
    p = np.concatenate([p, near])
    R.load_scene(rm.SCENE_FILES["O"])
    R.set_uniform("u_time", time)
    _, aux = R.scene_eval(p, form="probe", aux=True)
    sel = aux >= K["probe_slack"]
    below = int((~sel).sum())
    p = p[sel]
    n = len(p)
    h = f32(0.001)
    probes = [p + np.array(k, f32) * h for k in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))]
    for _ in range(4):  # ambientOcclusionReal along any unit normal
        nrm = _unit(rng, n).astype(f32)
        probes += [p + nrm * f32(i + 1) * f32(0.2) for i in range(4)]
    for _ in range(8):  # CalculateThickness: sampleDir * sampleLength, length < 1
        probes.append(p + _unit(rng, n).astype(f32) * rng.uniform(0.0, 1.0, (n, 1)).astype(f32))
    probes = np.ascontiguousarray(np.concatenate(probes), f32)
    hip = R.scene_eval(probes, form="probe")
    bad = hip != probes[:, 1]
    print(f"u_time {time}: {n} shading points with GPU slack >= {K['probe_slack']} ({below} candidates below it), "
          f"{len(probes)} probes, {int(bad.sum())} not the plane")
    assert n >= 4000 and below >= 150, (n, below)
    assert not bad.any(), (probes[bad][:4], hip[bad][:4])


@pytest.mark.gpu
@pytest.mark.parametrize("time", (TIMES[0], TIMES[2], TIMES[4]), ids=(TIME_IDS[0], TIME_IDS[2], TIME_IDS[4]))
def test_scene_t_probe_form_at_fold_boundaries_and_ties(R, time):
    """menger<false> (all of scene T's marches: menger_at at t = 0 is this
    distance bit for bit) on the fold exit / wall / kink sets within 2.3 of the
    sponge and on the rint-tie and floor-step points, against the oracle under
    _close; then the one-exit variant (NB = 1) against it bit for bit, the
    points shuffled so that a wave mixes lanes leaving at different folds.

    Measured on the MI355X: 6.0e-8 at u_time 0, 9.5e-7 at 137.59444 and at
    121.64964 (both on the uniform points far from the sponge, |d| ~ 8); NB = 1
    equal to NB = 3 at all 103216 points of each time."""
    B = rules.boundary_points(time)
    pts = B.select(FOLD_SETS)
    pts = pts[(np.abs(pts - np.array(rules.SPONGE_C, f32)).max(-1) <= 2.3)]
    assert len(pts) > 50000, len(pts)
    ties, _ = fold_tie_points(time)
    far = B.sets["uniform"][:4096]  # lanes that leave before the first fold
    pts = np.concatenate([pts, ties, far])
    pts = np.ascontiguousarray(pts[np.random.default_rng(23).permutation(len(pts))], f32)
    R.load_scene(rm.SCENE_FILES["T"])
    R.set_uniform("u_time", time)
    hip = R.scene_eval(pts, form="probe")
    ref = oracle.scene_dist("T", pts, time=time)
    err, ok = _err(hip, ref), _close(hip, ref)
    print(f"scene T u_time {time}: {len(pts)} points ({len(ties)} tie points), probe form max |d| {err.max():.4g} "
          f"at p={pts[np.argmax(err)].tolist()}, {int((hip != ref).sum())} not equal")
    assert ok.all(), (int((~ok).sum()), pts[np.argmax(err)].tolist(), float(err.max()))
    nb1 = R.scene_eval(pts, form="probe_nb1")
    diff = nb1.view(np.uint32) != hip.view(np.uint32)
    print(f"scene T u_time {time}: NB = 1 differs from NB = 3 at {int(diff.sum())} points")
    assert not diff.any(), (pts[diff][:4], nb1[diff][:4], hip[diff][:4])


@pytest.mark.gpu
def test_scene_s0_probe_form_on_the_sphere(R):
    """The probe form of scene S0's sphere at its surface, under _close.
    Measured on the MI355X: 1.2e-7 over 21536 points."""
    pts, _, _ = rules.sphere_surface(rules.S0_SPHERE_C, np.random.default_rng(3), 2000)
    R.load_scene(rm.SCENE_FILES["S0"])
    hip, aux = R.scene_eval(pts, form="probe", aux=True)
    ref = oracle.scene_dist("S0", pts)
    err, ok = _err(hip, ref), _close(hip, ref)
    print(f"scene S0: {len(pts)} points on the sphere, probe form max |d| {err.max():.4g}")
    assert ok.all(), (int((~ok).sum()), pts[np.argmax(err)].tolist(), float(err.max()))
    assert not aux.any()  # aux is scene O's; 0 elsewhere
    assert np.array_equal(R.scene_eval(pts, form="probe_nb1"), hip)  # an alias outside scene T


@pytest.mark.gpu
def test_exact_form_through_the_new_entry_is_rm_scene_eval(R):
    """RM_FORM_EXACT is rm_scene_eval's kernel: the same bits, and aux still
    the probe form's slack."""
    time = TIMES[1]
    B = rules.boundary_points(time)
    pts = B.points[::7]
    for scene in ("O", "T"):
        R.load_scene(rm.SCENE_FILES[scene])
        R.set_uniform("u_time", time)
        d0, m0 = R.scene_eval(pts, material=True)
        d1, m1, a1 = R.scene_eval(pts, material=True, form="exact", aux=True)
        assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(m0, m1)
        _, a2 = R.scene_eval(pts, form="probe", aux=True)
        assert np.array_equal(a1, a2) and (scene == "O") == bool(a1.any())
    with pytest.raises(ValueError):
        R.scene_eval(pts, form="fast")
