"""Seeded ray sets for scene T's exact shortcuts through the ray entry points
(tests/test_shade_rays_shortcuts.py), classified on the CPU.

A ray is a pose (pos, mouse): the only ray of a 1 x 1 frame there, whose
direction is what camera_rays(1, 1) gives on the GPU and tests/shade_ref.py's
pose_dirs on the CPU.  One set per u_time (a shade launch has one), drawn by
seeded rejection sampling from pools of fixed size, in these classes:

  A  far-sky with margin: misses the cube of half-size 1.5, far point >= 4.6;
     origins all different, max-norm 2 to 40, all eight octants
  B  grazing the inflated cube: the miss test flips within 0.02 of kFarSkyR
  C  misses with margin, far point fmaf(d, 50, o) within 0.2 of 4.1
  D  hits, in groups on either side of the soft-shadow and the reflection
     certificate
  E  origins inside the inflated cube, outside the sponge
  F  argument edges: axis-parallel directions, |o|_1 on either side of 1024,
     origins 1e4 and 1e6 away
  G  rays the guard rejects (not poses: origin and direction given)

The classes come from the numpy restatements (tests/far_sky_ref.py,
shadow_clear_ref.py, refl_clear_ref.py) and the CPU oracle's distance and
normal.  They state what the inputs are; no expected colour comes from here.
CPU only.
"""
import numpy as np

import oracle
from tests import far_sky_ref as fs
from tests import refl_clear_ref as rc
from tests import shadow_clear_ref as sc
from tests.shade_ref import pose_dirs

F32 = np.float32
SEED = 20261021
TIMES = (0.0, 1.25, 30.0)
CLASSIFY_STEPS = 256
ZNEAR, ZFAR = F32(0.02), F32(50.0)
# class sizes: 374 poses and 10 rejected rays, 384 = 6 waves = 16 rows of 24
SIZES = dict(A=128, B=32, C=32, D=128, E=32, F=22, G=10)
A_MARGIN_R, A_MARGIN_FAR = F32(1.5), F32(4.6)
B_BAND = 0.02
C_LO, C_HI = F32(3.9), F32(4.3)
NEAR = 0.05  # "within 0.05 of the ratio"
MIXED_LANES = (0, 31, 32, 63)


def _rows(time):
    """Q [3, 3] float64: sponge_rot of the unit vectors, so q = v @ Q and v = q @ Q.T"""
    return sc.sponge_rot(sc.sponge_rotation(time), np.eye(3, dtype=F32)).astype(np.float64)


def aim(d):
    """mouse [n, 2] float32 whose 1 x 1 frame looks along the world directions d [n, 3]"""
    d = np.asarray(d, np.float64)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return np.stack([np.arctan2(d[:, 0], -d[:, 2]), -np.arcsin(np.clip(d[:, 1], -1.0, 1.0))], -1).astype(F32)


def poses_from_sponge(time, o, d):
    """sponge-space origins and directions (float64) -> (pos [n, 3] f32, mouse [n, 2] f32) in the world"""
    Q = _rows(time)
    pos = (np.asarray(o, np.float64) @ Q.T + fs.CENTRE.astype(np.float64)).astype(F32)
    return pos, aim(np.asarray(d, np.float64) @ Q.T)


def march(pos, dirs, time, max_steps=CLASSIFY_STEPS):
    """castRay (common.frag:931-954) over scene T's distance, an origin per ray -> (points [n, 3], hit [n])"""
    ro, rd = np.asarray(pos, F32), np.asarray(dirs, F32)
    n = len(rd)
    depth = np.full(n, ZNEAR, F32)
    hit = np.zeros(n, bool)
    live = np.arange(n)
    for _ in range(int(max_steps)):
        if not len(live):
            break
        p = (ro[live] + rd[live] * depth[live, None]).astype(F32)
        d = oracle.scene_dist("T", p, time=time)
        h = d < F32(0.001)
        hit[live[h]] = True
        nd = (depth[live] + d).astype(F32)
        depth[live[~h]] = nd[~h]
        live = live[~h & (nd < ZFAR)]
    return (ro + rd * depth[:, None]).astype(F32), hit


def shadow_slope(o, d, mint=sc.MINT):
    """the slope rmsc::kRatio is held against: max u_i over the axes on which the shadow ray's point at mint lies
    outside the face (-inf if none), as refl_clear_ref.refl_clear's second result"""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    u = np.where(o < 0, -d, d).astype(F32)
    outside = ((np.abs(o) - F32(1.0)).astype(F32) + u * mint).astype(F32) >= F32(0.0)
    return np.where(outside, u, -np.inf).max(-1)


def classify(pos, dirs, time):
    """what the restatements say of world rays (finite, unit) at u_time `time` -> dict of [n] arrays"""
    pos, dirs = np.asarray(pos, F32), np.asarray(dirs, F32)
    o, d = fs.to_sponge(pos, dirs, time)
    n = len(pos)
    out = dict(o=o, d=d, far=fs.far_sky_ray(o, d), miss=fs.ray_misses_cube(o, d), farmax=fs.far_point(o, d),
               miss_lo=fs.ray_misses_cube(o, d, fs.K_R - F32(B_BAND)), miss_hi=fs.ray_misses_cube(o, d, fs.K_R + F32(B_BAND)),
               miss_a=fs.ray_misses_cube(o, d, A_MARGIN_R), omax=np.abs(o).max(-1),
               osum=np.abs(o).sum(-1, dtype=F32), dist0=oracle.scene_dist("T", pos, time=time))
    p, hit = march(pos, dirs, time)
    lit = np.zeros(n, bool)
    sclear = np.zeros(n, bool)
    rclear = np.zeros(n, bool)
    sslope = np.full(n, np.nan)
    rslope = np.full(n, np.nan)
    pmax = np.full(n, np.nan)
    if hit.any():
        ph, rd = p[hit], dirs[hit]
        nrm = oracle.normal("T", ph, time=time).astype(F32)
        L = (sc.LIGHT - ph).astype(F32)
        L = (L / np.sqrt((L * L).sum(-1, dtype=F32))[:, None]).astype(F32)
        l = ~((L * nrm).sum(-1, dtype=F32) < 0)  # shadow_clear_ref.frame_masks' rule
        R = sc.sponge_rotation(time)
        so = sc.sponge_rot(R, (ph - fs.CENTRE).astype(F32))
        sd = sc.sponge_rot(R, L)
        dn = (rd * nrm).sum(-1, dtype=F32)
        rdir = (rd - F32(2.0) * dn[:, None] * nrm).astype(F32)
        ror = (ph + rdir * F32(0.01)).astype(F32)
        c, best = rc.refl_clear(sc.sponge_rot(R, (ror - fs.CENTRE).astype(F32)), sc.sponge_rot(R, rdir))
        lit[hit], sclear[hit], sslope[hit] = l, l & sc.shadow_clear(so, sd), shadow_slope(so, sd)
        rclear[hit], rslope[hit] = c, best
        pmax[hit] = np.abs(so).max(-1)
    out.update(hit=hit, lit=lit, sclear=sclear, rclear=rclear, sslope=sslope, rslope=rslope, pmax=pmax)
    return out


def d_groups(c):
    """class D's groups as masks over classify()'s rows"""
    ks, kr = float(sc.K_RATIO), float(rc.K_RATIO)
    hit, lit = c["hit"], c["lit"]
    with np.errstate(invalid="ignore"):
        return dict(
            clear_lit=hit & lit & c["sclear"], notclear_lit=hit & lit & ~c["sclear"], unlit=hit & ~lit,
            rclear=hit & c["rclear"], rnot=hit & ~c["rclear"],
            inner=hit & (c["pmax"] < 0.99),  # an inner wall: the folds decide the distance there, not the box
            s_below=hit & lit & (c["sslope"] >= ks - NEAR) & (c["sslope"] < ks),
            s_above=hit & lit & (c["sslope"] >= ks) & (c["sslope"] <= ks + NEAR),
            r_below=hit & (c["rslope"] >= kr - NEAR) & (c["rslope"] < kr),
            r_above=hit & (c["rslope"] >= kr) & (c["rslope"] <= kr + NEAR))


# The light stands at (20, 50, 0) and the sponge turns about the vertical by 2 u_time degrees, so the slope of a
# lit outer face's shadow ray is fixed by u_time and the hit point, not by the ray.  Over the faces' points (3072
# draws per time) the lit side face has slopes 0.35-0.40 at u_time 0 and 1.25 and the top face 0.92, the two z
# faces are unlit: no outer-face point lies below rmsc::kRatio = 0.35.  At u_time 30 the sponge has turned by 60
# degrees and its two lit side faces have 0.10-0.20 and 0.30-0.33: none lies above within 0.05.  So each time has
# one side of the soft-shadow ratio within 0.05, and the three sets together have both.
S_SIDE = {0.0: "s_above", 1.25: "s_above", 30.0: "s_below"}
D_QUOTA = dict(clear_lit=12, notclear_lit=12, unlit=12, rclear=12, rnot=12, inner=12, r_below=8, r_above=8)


def d_quota(time):
    return dict(D_QUOTA, **{S_SIDE[float(time)]: 8})


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _first(mask, n, what):
    idx = np.flatnonzero(mask)
    assert len(idx) >= n, f"{what}: {len(idx)} of {len(mask)} draws qualify, {n} needed"
    return idx[:n]


def _draw_A(rng, time):
    n = 4096
    sign = np.array([[1 if (k >> b) & 1 else -1 for b in range(3)] for k in range(8)], np.float64)[np.arange(n) % 8]
    v = rng.uniform(0.0, 1.0, size=(n, 3))
    v[np.arange(n), rng.randint(0, 3, size=n)] = 1.0
    r = np.exp(rng.uniform(np.log(2.0), np.log(40.0), size=n))
    o = sign * v * r[:, None]
    pos, mouse = poses_from_sponge(time, o, _unit(rng, n))
    c = classify(pos, pose_dirs(mouse).astype(F32), time)
    with np.errstate(invalid="ignore"):
        ok = c["far"] & c["miss_a"] & (c["farmax"] >= A_MARGIN_FAR) & (c["omax"] >= 2.0) & (c["omax"] <= 40.0)
    # keep the octants even: the first 16 of each
    so = fs.to_sponge(pos, pose_dirs(mouse).astype(F32), time)[0]
    octant = (so[:, 0] > 0) * 1 + (so[:, 1] > 0) * 2 + (so[:, 2] > 0) * 4
    pick = np.sort(np.concatenate([_first(ok & (octant == k), SIZES["A"] // 8, f"A octant {k}") for k in range(8)]))
    return pos[pick], mouse[pick]


def _draw_B(rng, time):
    n = 4096
    g = float(fs.K_R) + rng.uniform(-0.9 * B_BAND, 0.9 * B_BAND, size=n)
    k = rng.randint(0, 3, size=n)
    a, b = (k + 1) % 3, (k + 2) % 3
    sa, sb = rng.choice([-1.0, 1.0], size=n), rng.choice([-1.0, 1.0], size=n)
    i = np.arange(n)
    P, d = np.zeros((n, 3)), np.zeros((n, 3))
    edge = i % 2 == 0
    # an edge along axis k at (sa g, sb g): the direction crosses it (outward on a, inward on b) and runs along k too
    P[i, a], P[i, b], P[i, k] = sa * g, sb * g, rng.uniform(-1.0, 1.0, size=n) * g
    d[i, a], d[i, b], d[i, k] = sa * rng.uniform(0.3, 1.0, size=n), -sb * rng.uniform(0.3, 1.0, size=n), rng.uniform(-0.6, 0.6, size=n)
    # a face: through a point of the face a = sa g, parallel to it
    P[i[~edge], b[~edge]] = rng.uniform(-1.0, 1.0, size=(~edge).sum()) * g[~edge]
    d[i[~edge], a[~edge]] = 0.0
    d[i[~edge], b[~edge]] = rng.uniform(-1.0, 1.0, size=(~edge).sum())
    d[i[~edge], k[~edge]] = rng.choice([-1.0, 1.0], size=(~edge).sum())
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = P - d * rng.uniform(3.0, 9.0, size=(n, 1))
    pos, mouse = poses_from_sponge(time, o, d)
    c = classify(pos, pose_dirs(mouse).astype(F32), time)
    with np.errstate(invalid="ignore"):
        ok = c["miss_lo"] & ~c["miss_hi"] & (c["farmax"] >= A_MARGIN_FAR) & (c["omax"] > 1.5) & ~c["hit"]
    half = SIZES["B"] // 2
    pick = np.sort(np.concatenate([_first(ok & c["miss"], half, "B missing"), _first(ok & ~c["miss"], half, "B not missing")]))
    return pos[pick], mouse[pick]


def _draw_C(rng, time):
    n = 1 << 16
    o = _unit(rng, n) * rng.uniform(46.0, 54.0, size=(n, 1))
    beside = _unit(rng, n) * rng.uniform(2.2, 4.6, size=(n, 1))
    pos, mouse = poses_from_sponge(time, o, beside - o)
    dirs = pose_dirs(mouse).astype(F32)
    so, sd = fs.to_sponge(pos, dirs, time)
    farmax = fs.far_point(so, sd)
    with np.errstate(invalid="ignore"):
        ok = fs.ray_misses_cube(so, sd, A_MARGIN_R) & (farmax >= C_LO) & (farmax <= C_HI)
    half = SIZES["C"] // 2
    pick = np.sort(np.concatenate([_first(ok & (farmax >= fs.K_FAR), half, "C at or above 4.1"),
                                   _first(ok & (farmax < fs.K_FAR), half, "C below 4.1")]))
    return pos[pick], mouse[pick]


def _draw_D(rng, time):
    n = 3072
    i = np.arange(n)
    k = rng.randint(0, 3, size=n)
    a, b = (k + 1) % 3, (k + 2) % 3
    s = rng.choice([-1.0, 1.0], size=n)
    P = np.zeros((n, 3))
    P[i, k] = s
    P[i, a], P[i, b] = rng.uniform(-1.0, 1.0, size=n), rng.uniform(-1.0, 1.0, size=n)
    cn = rng.uniform(0.08, 1.0, size=n)
    kind = i % 3
    cn[kind == 1] = rng.uniform(0.12, 0.28, size=(kind == 1).sum())  # reflected slopes round rmrc::kRatio
    hole = kind == 2                                                  # into the face's central hole, to an inner wall
    P[i[hole], a[hole]] = rng.uniform(-0.3, 0.3, size=hole.sum())
    P[i[hole], b[hole]] = rng.uniform(-0.3, 0.3, size=hole.sum())
    cn[hole] = rng.uniform(0.35, 0.98, size=hole.sum())
    phi = rng.uniform(0.0, 2.0 * np.pi, size=n)
    d = np.zeros((n, 3))
    d[i, k] = -s * cn
    d[i, a], d[i, b] = np.sqrt(1.0 - cn * cn) * np.cos(phi), np.sqrt(1.0 - cn * cn) * np.sin(phi)
    o = P - d * rng.uniform(1.5, 5.0, size=(n, 1))
    pos, mouse = poses_from_sponge(time, o, d)
    c = classify(pos, pose_dirs(mouse).astype(F32), time)
    g = d_groups(c)
    quota = d_quota(time)
    taken = np.zeros(n, bool)
    for name, q in quota.items():  # the groups first, with a third to spare, then the first hits left
        want = q + (q + 2) // 3
        idx = np.flatnonzero(g[name])
        assert len(idx) >= q, f"D {name} at u_time {time}: {len(idx)} draws, {q} needed"
        have = int((taken & g[name]).sum())
        taken[idx[~taken[idx]][:max(0, want - have)]] = True
    assert taken.sum() <= SIZES["D"]
    rest = np.flatnonzero(c["hit"] & ~taken)
    taken[rest[:SIZES["D"] - int(taken.sum())]] = True
    pick = np.flatnonzero(taken)
    assert len(pick) == SIZES["D"]
    return pos[pick], mouse[pick]


def _draw_E(rng, time):
    n = 4096
    o = rng.uniform(-1.15, 1.15, size=(n, 3))
    pos, mouse = poses_from_sponge(time, o, _unit(rng, n))
    so = fs.to_sponge(pos, pose_dirs(mouse).astype(F32), time)[0]
    omax = np.abs(so).max(-1)
    ok = (oracle.scene_dist("T", pos, time=time) > NEAR) & (omax < 1.2)
    half = SIZES["E"] // 2
    pick = np.sort(np.concatenate([_first(ok & (omax < 0.98), half, "E in the void and the tunnels"),
                                   _first(ok & (omax >= 0.98), half, "E between the sponge and the inflated cube")]))
    return pos[pick], mouse[pick]


AXIS_MOUSE = [(0.0, 0.0), (np.pi / 2, 0.0), (-np.pi / 2, 0.0), (0.0, np.pi / 2), (0.0, -np.pi / 2)]


def _list_F(time):
    pos, mouse = [], []
    for p in ((0.45, 3.55, 4.0), (4.0, 3.1, 0.6)):  # in front of two faces (at u_time 0), beside their central holes
        for m in AXIS_MOUSE:
            pos.append(p)
            mouse.append(m)
    pos, mouse = [np.array(pos, F32)], [np.array(mouse, F32)]
    o, d = [], []
    for shape in ((1.0, 0.0, 0.0), (-0.5, 0.3, -0.2)):  # |o|_1 just below and just above 1024: the `ok` guards flip
        for length in (1024.0 * (1.0 - 2.0 ** -12), 1024.0 * (1.0 + 2.0 ** -12)):
            for towards in (-1.0, 1.0):
                o.append(np.array(shape) * length)
                d.append(towards * np.array(shape))
    far_dir = np.array([0.6, 0.5, 0.62])
    for length in (1.0e4, 1.0e6):
        for towards in (-1.0, 1.0):
            o.append(far_dir / np.linalg.norm(far_dir) * length)
            d.append(towards * far_dir)
    p, m = poses_from_sponge(time, np.array(o), np.array(d))
    pos, mouse = np.concatenate(pos + [p]), np.concatenate(mouse + [m])
    assert len(pos) == SIZES["F"]
    return pos, mouse


def _list_G():
    """(origins, directions) the guard rejects: tests/test_shade_rays.py::test_rejected_rays_are_not_shaded's kinds"""
    p = np.array([2.0, 3.0, 3.0], F32)
    d = pose_dirs(np.array([[-0.45, 0.2]])).astype(F32)[0]
    inf, nan = F32(np.inf), F32(np.nan)
    pos, dirs = np.tile(p, (SIZES["G"], 1)), np.tile(d, (SIZES["G"], 1))
    dirs[0] = d * F32(1.02)
    dirs[1] = 0.0
    dirs[2, 0] = nan
    dirs[3, 1] = inf
    dirs[4, 2] = -inf
    dirs[5] = (nan, inf, 0.0)
    dirs[6] = d * F32(2.0)
    pos[7, 1] = inf
    pos[8, 0] = -inf
    pos[9, 2] = nan
    return pos, dirs


_SETS = {}


def ray_set(time):
    """dict(pos [N, 3] f32, mouse [NP, 2] f32, g_dirs [N - NP, 3] f32, cls [N] of 'A'..'G', time): the poses of
    classes A to F first, then class G's rays.  Seeded per u_time; computed once, read-only."""
    time = float(time)
    if time not in _SETS:
        rng = np.random.RandomState(SEED + int(round(time * 100)))
        parts = [("A", _draw_A(rng, time)), ("B", _draw_B(rng, time)), ("C", _draw_C(rng, time)),
                 ("D", _draw_D(rng, time)), ("E", _draw_E(rng, time)), ("F", _list_F(time))]
        for name, (p, m) in parts:
            assert len(p) == len(m) == SIZES[name], name
        gp, gd = _list_G()
        s = dict(pos=np.ascontiguousarray(np.concatenate([p for _, (p, _) in parts] + [gp]), F32),
                 mouse=np.ascontiguousarray(np.concatenate([m for _, (_, m) in parts]), F32),
                 g_dirs=np.ascontiguousarray(gd, F32),
                 cls=np.array([c for c in "ABCDEFG" for _ in range(SIZES[c])]), time=time)
        for v in s.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SETS[time] = s
    return _SETS[time]


def n_poses(s):
    return len(s["mouse"])


def all_dirs(s, pose_directions=None):
    """[N, 3] f32: the poses' directions (the GPU's, camera_rays(1, 1), when given; else pose_dirs) then class G's"""
    d = pose_dirs(s["mouse"]).astype(F32) if pose_directions is None else np.asarray(pose_directions, F32)
    return np.ascontiguousarray(np.concatenate([d.reshape(-1, 3), s["g_dirs"]]), F32)


_CLASSES = {}


def classes(time):
    """classify() of the set's poses with pose_dirs' directions (computed once)"""
    time = float(time)
    if time not in _CLASSES:
        s = ray_set(time)
        n = n_poses(s)
        _CLASSES[time] = classify(s["pos"][:n], pose_dirs(s["mouse"]).astype(F32), time)
    return _CLASSES[time]


def members(s, c):
    return np.flatnonzero(s["cls"] == c)


def compositions(time):
    """name -> dict(idx: indices into the set, layouts: the `width`s to shade it with (0: a list), waves: a label
    per wave of 64, or None).  In a ray image of width 8, tile `by` is rays 64 by to 64 by + 63, a list's wave."""
    s = ray_set(time)
    c = classes(time)
    A = members(s, "A")
    G = members(s, "G")
    rng = np.random.RandomState(SEED + 7 + int(round(time * 100)))
    comps = {}
    # 1. class A only, every origin different: by the restatement both waves vote far
    comps["A_only"] = dict(idx=A.copy(), layouts=(0, 8), waves=["A 0-63", "A 64-127"])
    # 2. 63 rays of A and one ray of another class, at lane 0, 31, 32 and 63
    g = d_groups(c)
    d_pick = dict(zip(MIXED_LANES, ("clear_lit", "inner", "unlit", "rnot")))
    idx, labels = [], []
    for ci, cl in enumerate("BCDEF"):
        m = members(s, cl)
        for li, lane in enumerate(MIXED_LANES):
            if cl == "D":
                other = np.flatnonzero(g[d_pick[lane]] & (s["cls"][:len(c["hit"])] == "D"))[0]
                label = f"63 A + D ({d_pick[lane]}) at lane {lane}"
            elif cl in "BC":  # the sides of the class's threshold in turn: lanes 0 and 32 pass far_sky_ray, 31 and 63 not
                side = m[c["far"][m] == (li % 2 == 0)]
                other = side[(5 * li + 3) % len(side)]
                label = f"63 A + {cl} ({'far-sky' if li % 2 == 0 else 'not far-sky'}) at lane {lane}"
            else:
                other = m[(5 * li + 3) % len(m)]
                label = f"63 A + {cl} at lane {lane}"
            wave = np.roll(A, -(7 * (4 * ci + li)))[:63]
            idx.append(np.insert(wave, lane, other))
            labels.append(label)
    comps["mixed"] = dict(idx=np.concatenate(idx), layouts=(0, 8), waves=labels)
    # 3. the whole set in seeded random order (at width 24 a tile is 8 x 8 of a 24-wide image: other wave-mates)
    perm = rng.permutation(len(s["cls"]))
    comps["all_shuffled"] = dict(idx=perm, layouts=(0, 8, 24), waves=None)
    # 4. partly filled last waves (lists only)
    comps["cut_321"] = dict(idx=perm[:64 * 5 + 1], layouts=(0,), waves=None)
    comps["cut_357"] = dict(idx=perm[:64 * 5 + 37], layouts=(0,), waves=None)
    # 5. rejected rays among far-sky rays, and a wave of rejected rays only
    wave = A[64:128].copy()
    wave[[0, 7, 63]] = G[[0, 5, 7]]
    comps["A_with_G"] = dict(idx=np.concatenate([wave, G[np.arange(64) % len(G)]]), layouts=(0, 8),
                             waves=["61 A + G at lanes 0, 7, 63", "G only"])
    return comps


def wave_votes(time, idx):
    """per wave of 64 of the composition `idx` (a list, or a ray image of width 8): does the restatement say that
    every shaded lane passes far_sky_ray?  Class G's lanes return before the vote.  -> [waves] bool"""
    far = np.concatenate([classes(time)["far"], np.ones(SIZES["G"], bool)])  # (G: no part in the vote)
    f = far[idx]
    pad = (-len(f)) % 64
    return np.concatenate([f, np.ones(pad, bool)]).reshape(-1, 64).all(-1)


def quotas(time):
    """the counts the CPU test holds to the issue's quotas -> dict"""
    s = ray_set(time)
    c = classes(time)
    cls = s["cls"][:n_poses(s)]
    q = {}
    with np.errstate(invalid="ignore"):
        A = cls == "A"
        q["A"] = int((A & c["far"] & c["miss_a"] & (c["farmax"] >= A_MARGIN_FAR)).sum())
        q["A_distinct_origins"] = len(np.unique(s["pos"][:n_poses(s)][A], axis=0))
        so = c["o"][A]
        q["A_octants"] = np.bincount((so[:, 0] > 0) * 1 + (so[:, 1] > 0) * 2 + (so[:, 2] > 0) * 4, minlength=8).tolist()
        q["A_shell"] = (float(c["omax"][A].min()), float(c["omax"][A].max()))
        q["A_shell_thirds"] = [int(((c["omax"][A] >= lo) & (c["omax"][A] < hi)).sum()) for lo, hi in ((2, 5.5), (5.5, 15), (15, 40.001))]
        B = (cls == "B") & c["miss_lo"] & ~c["miss_hi"] & ~c["hit"] & (c["omax"] > 1.5)
        q["B_miss"], q["B_graze"] = int((B & c["miss"]).sum()), int((B & ~c["miss"]).sum())
        q["B_far"], q["B_not_far"] = int((B & c["far"]).sum()), int((B & ~c["far"]).sum())
        C = (cls == "C") & c["miss_a"] & (c["farmax"] >= C_LO) & (c["farmax"] <= C_HI)
        q["C_above"], q["C_below"] = int((C & (c["farmax"] >= fs.K_FAR)).sum()), int((C & (c["farmax"] < fs.K_FAR)).sum())
        dist = np.linalg.norm(c["o"][cls == "C"].astype(np.float64), axis=-1)
        q["C_distance"] = (float(dist.min()), float(dist.max()))
        D = cls == "D"
        q["D"] = int((D & c["hit"]).sum())
        for name, m in d_groups(c).items():
            q["D_" + name] = int((D & m).sum())
        E = cls == "E"
        q["E"] = int((E & (c["dist0"] > NEAR) & (c["omax"] < fs.K_R)).sum())
        q["E_inside_unit_cube"] = int((E & (c["omax"] < 0.98)).sum())
        q["E_far"] = int((E & c["far"]).sum())
        q["E_hit"], q["E_sky"] = int((E & c["hit"]).sum()), int((E & ~c["hit"]).sum())
        F = np.flatnonzero(cls == "F")
        q["F"] = len(F)
        q["F_below_1024"] = int(((c["osum"][F] > 1023.0) & (c["osum"][F] <= 1024.0)).sum())
        q["F_above_1024"] = int(((c["osum"][F] > 1024.0) & (c["osum"][F] < 1025.0)).sum())
        q["F_1e4"] = int(((c["omax"][F] > 5.0e3) & (c["omax"][F] < 2.0e4)).sum())
        q["F_1e6"] = int((c["omax"][F] > 5.0e5).sum())
    return q
