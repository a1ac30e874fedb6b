"""Scene O's exact skips, point by point at their branch
boundaries.

scene_dist_O (rm_device.h) returns early in five places and claims the same
float as the full sceneSDF for each.  The CPU tests check the rules themselves,
with the margins parsed from the kernel's source, against the oracle, which
evaluates the plain sceneSDF_O without any skip (tests/scene_o_rules.py).  The
GPU tests compare rm_scene_eval, which runs scene_dist<SC, kExactForm> in scene
O's own translation unit, with the oracle at the same points: by the header's
argument the two are the same float at every finite point, so the expected
result is equality, not a tolerance.
"""
import numpy as np
import pytest

import oracle
import raymarching_amd as rm
from tests import scene_o_rules as rules

f32 = np.float32
TIMES = rules.TIMES
TIME_IDS = [f"t{t:.5f}" for t in TIMES]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------- CPU


def test_header_constants_are_read():
    """All seven statements are found, and the parsed margins keep what the
    comments promise: above the blend widths 0.33 and 0.5 and above k/6."""
    rules._CONSTANTS = None  # (parse now, not a cached copy)
    K = rules.kernel_constants()
    print({k: (tuple(float(x) for x in v) if isinstance(v, tuple) else float(v)) for k, v in K.items()})
    for site in ("slack_box", "box", "dom_box", "dom", "reach"):
        assert K[site] > f32(0.33), (site, K[site])
    for site in ("slack_plane", "plane"):
        assert K[site] > f32(0.5), (site, K[site])
    assert float(K["a_offset"]) >= 0.5 / 6.0, K["a_offset"]
    assert float(K["bound_offset"]) >= 1.0 + 0.5 / 6.0, K["bound_offset"]
    # slack certifies spans by the same two tests the branches take
    assert K["slack_plane"] >= K["plane"] and K["slack_box"] >= K["box"]
    assert K["rate_norm"] >= f32(1.01) and K["probe_slack"] >= f32(2.05)
    assert K["fold_scales"] == (f32(3.0), f32(9.0), f32(27.0)), K["fold_scales"]


@pytest.mark.parametrize("time", TIMES, ids=TIME_IDS)
def test_skip_values_equal_the_oracle(time):
    """Wherever a skip fires, the value it returns is the oracle's sceneSDF as
    floats, on points bisected onto every branch boundary."""
    B = rules.boundary_points(time)
    Q = rules.quantities(B.points, time)
    value, kind = rules.expected_skip(B.points, time, Q)
    ref = oracle.scene_dist("O", B.points, time=time)
    counts = {rules.KINDS[k]: int((kind == k).sum()) for k in range(1, len(rules.KINDS))}
    adjacent = {name: int(rules.adjacent_pairs(*B.pairs[name]).sum()) for name in B.pairs if name.startswith("pred")}
    print(f"u_time {time}: {len(B.points)} points, skip kinds {counts}, adjacent straddling pairs {adjacent}")
    assert min(counts.values()) >= 5000, counts
    assert min(adjacent.values()) >= 2000, adjacent
    fired = kind != rules.KIND_NONE
    bad = fired & ~(value == ref)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"{int(bad.sum())} skip points differ from the oracle, e.g. p={B.points[i]!r} kind "
                    f"{rules.KINDS[kind[i]]} (set {B.names[B.set_id[i]]}): rule {value[i]!r}, oracle {ref[i]!r}")


def test_plane_spans_hold():
    """One evaluation with slack >= 0 certifies the ray span depth < depth0 +
    slack / (1.01 + |rd.y|): there the march takes ro.y + rd.y * depth for
    sceneSDF(ro + rd * depth) (cast_ray_d, rm_render_direct.h)."""
    K = rules.kernel_constants()
    rng = np.random.default_rng(7)
    times = list(np.linspace(0.0, 180.0, 9)) + list(TIMES)
    total = bad = 0
    for t in times:
        n = 100000
        at = rng.uniform([-9.0, -0.5, -9.0], [9.0, 3.5, 9.0], (n, 3)).astype(f32)
        scale = np.where(np.arange(n) % 2 == 0, 1.0, rng.uniform(0.99, 1.01, n))  # unit and 1 +- 0.01
        rd = (_unit(rng, n) * scale[:, None]).astype(f32)
        depth0 = rng.uniform(0.02, 20.0, n).astype(f32)
        ro = at - rd * depth0[:, None]
        p0 = ro + rd * depth0[:, None]  # the point the march evaluates
        slack = rules.quantities(p0, t, d0=False)["slack"]
        keep = slack >= f32(0.0)
        ro, rd, depth0, slack = ro[keep], rd[keep], depth0[keep], slack[keep]
        ia = f32(1.0) / (K["rate_norm"] + np.abs(rd[:, 1]))
        depths = [depth0 + f32(fr) * (slack * ia) for fr in (0.25, 0.7, 0.999, 1.0)]
        # the last depth the kernel's `depth < t_plane` admits, its v_rcp one ulp high
        depths.append(np.maximum(depth0, rules.ulp_step(depth0 + slack * rules.ulp_step(ia, 1), -1)))
        for depth in depths:
            taken = ro[:, 1] + rd[:, 1] * depth
            ref = oracle.scene_dist("O", ro + rd * depth[:, None], time=float(t))
            total += len(ref)
            bad += int((taken != ref).sum())
    print(f"plane spans: {total} span points at {len(times)} times, {bad} exceptions")
    assert total >= 1000000, total
    assert bad == 0, bad


@pytest.mark.parametrize("time", TIMES[:3], ids=TIME_IDS[:3])
def test_probe_sets_are_plane_only(time):
    """At a shading point with slack >= 2.05 (plane_probes) the four normal
    probes, the AO probes and the 32 thickness samples are all the plane's p'.y,
    and the normal is one of the two floor normals `thickness` tests for."""
    K = rules.kernel_constants()
    rng = np.random.default_rng(11)
    p = rng.uniform([-30.0, -0.06, -30.0], [30.0, 0.06, 30.0], (40000, 3)).astype(f32)
    # plane_probes takes the probe form's q, whose fused roundings move mc by a
    # few ulp of |q| < 64 (4e-6 each): the rule has to hold from 1e-4 below
    p = p[rules.quantities(p, time, d0=False)["slack"] >= K["probe_slack"] - f32(1e-4)][:6000]
    n = len(p)
    h = f32(0.001)
    probes = [p + np.array(k, f32) * h for k in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))]
    for _ in range(16):  # ambientOcclusionReal along any unit normal
        nrm = _unit(rng, n).astype(f32)
        probes += [p + nrm * f32(i + 1) * f32(0.2) for i in range(4)]
    for _ in range(32):  # CalculateThickness: sampleDir * sampleLength, length < 1
        probes.append(p + _unit(rng, n).astype(f32) * rng.uniform(0.0, 1.0, (n, 1)).astype(f32))
    probes = np.concatenate(probes)
    ref = oracle.scene_dist("O", probes, time=time)
    bad = int((ref != probes[:, 1]).sum())
    nrm = oracle.normal("O", p, time=time)
    floor = (nrm[:, 0] == 0) & (nrm[:, 2] == 0) & ((nrm[:, 1] == f32(1.0)) | (nrm[:, 1] == f32(1.0 - 2.0 ** -24)))
    print(f"u_time {time}: {n} shading points, {len(probes)} probes, {bad} not the plane, "
          f"{int((~floor).sum())} normals off the floor's")
    assert n >= 4000, n
    assert bad == 0, bad
    assert floor.all(), nrm[~floor][:4]


# ------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def R(torch_cuda):
    r = rm.Renderer(0)
    yield r
    r.close()


def _mismatch_report(B, time, hip, ref):
    """Mismatches per skip kind (the return statement of scene_dist_O a point
    leaves by) and per point set, each with its worst point and both values."""
    _, kind = rules.expected_skip(B.points, time)
    bad = ~(hip == ref)
    err = np.abs(hip.astype(np.float64) - ref.astype(np.float64))
    lines = [f"{int(bad.sum())} of {len(ref)} points differ from the oracle at u_time {time}"]

    def rows(title, ids, names):
        for i, name in enumerate(names):
            sel = bad & (ids == i)
            if sel.any():
                j = int(np.flatnonzero(sel)[np.argmax(err[sel])])
                lines.append(f"  {title} {name}: {int(sel.sum())} of {int((ids == i).sum())}, worst p={B.points[j].tolist()} "
                             f"hip {hip[j]!r} oracle {ref[j]!r}")
    rows("kind", kind, rules.KINDS)
    rows("set", B.set_id, B.names)
    return "\n".join(lines)


@pytest.mark.gpu
@pytest.mark.parametrize("time", TIMES, ids=TIME_IDS)
@pytest.mark.parametrize("scene", ["O", "OG"])
def test_scene_o_distance_is_the_oracle_bit_for_bit(R, scene, time):
    """No tolerance and no allowance; +0 and -0 compare equal (the IEEE-minimum
    form of sminCubic differs from the select only in the sign of a zero)."""
    B = rules.boundary_points(time)
    R.load_scene(rm.SCENE_FILES[scene])
    R.set_uniform("u_time", time)
    hip = R.scene_eval(B.points)
    ref = oracle.scene_dist(scene, B.points, time=time)
    assert np.isfinite(ref).all()
    if not np.array_equal(hip, ref):
        report = _mismatch_report(B, time, hip, ref)
        print(report)
        pytest.fail(report)


def _close(hip, ref):
    return np.abs(hip.astype(np.float64) - ref) <= 1e-5 + 1e-5 * np.abs(ref.astype(np.float64))


@pytest.mark.gpu
def test_scene_t_and_s0_distance_at_fold_boundaries(R):
    """Scenes T and S0 contract and divide through v_rcp, so their distance is
    close to the oracle's, not equal: every point within 1e-5 + 1e-5 |d|
    (test_builtin_scene_eval_matches_oracle's tolerance, here without its 0.1 %
    allowance).  The sponge is 3-Lipschitz and contraction moves q by <= 1.5
    ulp(4) per rotation stage: 7.5e-6 at worst for |q| < 4."""
    for time in (TIMES[2], TIMES[4]):
        B = rules.boundary_points(time)
        pts = B.select(["fold exit", "fold wall", "fold kink"])
        pts = pts[(np.abs(pts - np.array(rules.SPONGE_C, f32)).max(-1) <= 2.3)]
        assert len(pts) > 50000, len(pts)
        R.load_scene(rm.SCENE_FILES["T"])
        R.set_uniform("u_time", time)
        hip = R.scene_eval(pts)
        ref = oracle.scene_dist("T", pts, time=time)
        err = np.abs(hip.astype(np.float64) - ref)
        print(f"scene T u_time {time}: {len(pts)} points, max |d| {err.max():.3g}, {int((hip != ref).sum())} not equal")
        ok = _close(hip, ref)
        assert ok.all(), (int((~ok).sum()), pts[np.argmax(err)].tolist(), float(err.max()))
    pts, _, _ = rules.sphere_surface(rules.S0_SPHERE_C, np.random.default_rng(3), 2000)
    R.load_scene(rm.SCENE_FILES["S0"])
    hip = R.scene_eval(pts)
    ref = oracle.scene_dist("S0", pts)
    err = np.abs(hip.astype(np.float64) - ref)
    print(f"scene S0: {len(pts)} points on the sphere, max |d| {err.max():.3g}")
    ok = _close(hip, ref)
    assert ok.all(), (int((~ok).sum()), pts[np.argmax(err)].tolist(), float(err.max()))


# max |hip - oracle| of Material.diffuse on boundary_points, measured on the
# MI355X (floor_mat's hardware exp2 / log2 / rcp and glsl_sin against the
# oracle's libm pow, sin and division): 5.692e-6 at u_time
# 57.79888 and 5.662e-6 at 121.64964, scenes O and OG alike.  The bound is four
# times the measured maximum, capped at 1e-4.
DIFFUSE_MEASURED = 5.692e-6
DIFFUSE_BOUND = min(4.0 * DIFFUSE_MEASURED, 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("time", (TIMES[1], TIMES[4]), ids=(TIME_IDS[1], TIME_IDS[4]))
@pytest.mark.parametrize("scene", ["O", "OG"])
def test_scene_o_material_is_the_oracle(R, scene, time):
    """scene_mat evaluates every term without skips and picks a blend's side by
    a < b: every Material field but diffuse is the oracle's float; diffuse goes
    through floor_mat's hardware forms and keeps the measured bound."""
    B = rules.boundary_points(time)
    R.load_scene(rm.SCENE_FILES[scene])
    R.set_uniform("u_time", time)
    _, hip = R.scene_eval(B.points, material=True)
    ref = oracle.scene_mat(scene, B.points, time=time)
    d = np.abs(hip[:, :3].astype(np.float64) - ref[:, :3]).max(-1)
    print(f"scene {scene} u_time {time}: max |d diffuse| {d.max():.4g} over {len(d)} points "
          f"(at p={B.points[np.argmax(d)].tolist()}, set {B.names[B.set_id[np.argmax(d)]]})")
    fields = ("specular.x", "specular.y", "specular.z", "shininess", "reflectivity", "transparency", "absorption.x",
              "absorption.y", "absorption.z", "refraction_index", "emission.x", "emission.y", "emission.z")
    bad = ~(hip[:, 3:] == ref[:, 3:])
    if bad.any():
        i, k = (int(v[0]) for v in np.nonzero(bad))
        pytest.fail(f"{int(bad.any(-1).sum())} points differ, by field {dict(zip(fields, bad.sum(0).tolist()))}; e.g. "
                    f"p={B.points[i].tolist()} (set {B.names[B.set_id[i]]}) {fields[k]}: hip {hip[i, 3 + k]!r} "
                    f"oracle {ref[i, 3 + k]!r}")
    assert d.max() <= DIFFUSE_BOUND, (float(d.max()), DIFFUSE_BOUND)
