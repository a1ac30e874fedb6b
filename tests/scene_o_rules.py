"""float32 numpy restatement of scene O's exact skips (scene_dist_O, rm_device.h;
DESIGN.md 2.7) and generators of the points at which they can go wrong.  Test
infrastructure only.

The kernel's margins are read from the source (kernel_constants), so the rules
below judge the constants the kernel uses.  Every operation is rounded to
float32 on its own, in the order rm_device.h writes it (no fused operations,
correctly rounded division and square root): `quantities` returns the
sponge-space point q, the box term mc, the Chebyshev bound lbs, A, slack, t2,
the sponge distance d0 (oracle.scene_dist("T"), which is
mengersponge(transformR(p - (0,3,0)))) and the five comparisons the kernel
branches on; `expected_skip` is the value each early return claims.

`boundary_points` collects, per u_time, adjacent-float pairs straddling each of
those comparisons and each kink of the terms behind them (fold exits, fold cell
walls, fold kinks, blend edges, the cube's faces, the sphere, the plane), a few
ulps around them, plus uniform and far points.
"""
import os
import re
from collections import OrderedDict

import numpy as np

import oracle
from tests.float_edges import adjacent_pairs, straddle, ulp_step  # noqa: F401 (re-exported)

f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raymarching_amd", "csrc")

# the return statement of scene_dist_O a point leaves by: the last one (nothing
# skipped), the three whole skips, and the plane blended with the sponge (skip 1
# alone: sminCubic(d0, p.y, 0.33) without the sphere and the cube)
KINDS = ("none", "plane", "sponge d0", "t2", "plane blend")
KIND_NONE, KIND_PLANE, KIND_D0, KIND_T2, KIND_PLANE_BLEND = range(5)

SPONGE_C = (0.0, 3.0, 0.0)
SPHERE_C = (3.0, 2.0, 3.0)
CUBE_C = (-5.0, 4.0, 5.0)
S0_SPHERE_C = (0.0, 1.0, -3.0)

# ------------------------------------------------- the kernel's constants

_NUM = r"([0-9]+\.[0-9]+)f"
# name -> (file, the statement the constant sits in, matches expected)
_PATTERNS = OrderedDict([
    # lbs = min(...) - 1.0834f
    ("bound_offset", ("rm_device.h", r"fabsf\(p\.z - 5\.0f\)\)\)\) - " + _NUM + r";", 1)),
    # if (lbs >= d3 + 0.51f) and slack's lbs - (d3 + 0.51f)
    ("plane_margin", ("rm_device.h", r"lbs (?:>=|-) \(?d3 \+ " + _NUM + r"\)", 2)),
    # mc >= d3 + 0.34f, slack's mc - (d3 + 0.34f), mc + 0.34f <= A, d0 + 0.34f <= A, mc >= t2 + 0.34f
    ("blend_margin", ("rm_device.h", r"(?:mc (?:>=|-) \(?(?:d3|t2) \+ " + _NUM + r"\)|(?:mc|d0) \+ " + _NUM + r" <= A)", 5)),
    # A = min(lbs, d3) - 0.0834f
    ("a_offset", ("rm_device.h", r"const float A = fminf\(lbs, d3\) - " + _NUM + r";", 1)),
    # plane_rate: rcp(1.01f + |d.y|)
    ("rate_norm", ("rm_render_direct.h", r"__builtin_amdgcn_rcpf\(" + _NUM + r" \+ fabsf\(d\.y\)\)", 1)),
    # plane_probes: slack >= 2.05f
    ("probe_slack", ("rm_render_direct.h", r"return slack >= " + _NUM + r";", 1)),
    # sponge_folds: INV[3] = {1/3, 1/9, 1/27}
    ("fold_exits", ("rm_device.h", r"constexpr float INV\[3\] = \{1\.0f / " + _NUM + r", 1\.0f / " + _NUM + r", 1\.0f / "
                    + _NUM + r"\};", 1)),
])

_CONSTANTS = None


def kernel_constants():
    """The margins scene_dist_O, plane_rate, plane_probes and sponge_folds use,
    parsed from the headers.  The plane margin (0.51) stands at two sites and
    the blend margin (0.34) at five; each site keeps its own entry, so a site
    that is edited alone is judged as edited."""
    global _CONSTANTS
    if _CONSTANTS is not None:
        return _CONSTANTS
    K = {}
    text = {}
    for name, (fname, pat, count) in _PATTERNS.items():
        if fname not in text:
            with open(os.path.join(CSRC, fname)) as f:
                text[fname] = f.read()
        found = re.findall(pat, text[fname])
        if len(found) != count:
            raise AssertionError(f"scene_o_rules: pattern for {name} matched {len(found)} statements of {fname}, "
                                 f"expected {count}: {pat!r} (scene_dist_O changed? restate it here)")
        vals = []
        for m in found:
            vals += [f32(v) for v in (m if isinstance(m, tuple) else (m,)) if v != ""]
        K[name] = vals
    out = dict(bound_offset=K["bound_offset"][0], a_offset=K["a_offset"][0], rate_norm=K["rate_norm"][0],
               probe_slack=K["probe_slack"][0])
    # text order: slack's pair (0.51, 0.34) comes before the branches
    out["slack_plane"], out["plane"] = K["plane_margin"]
    out["slack_box"], out["box"], out["dom_box"], out["dom"], out["reach"] = K["blend_margin"]
    out["fold_exits"] = tuple(f32(1.0) / v for v in K["fold_exits"])  # (RN(1/s), as the constexpr)
    out["fold_scales"] = tuple(K["fold_exits"])
    _CONSTANTS = out
    return out


# ------------------------------------------------------- float32 pieces


def glsl_sin(x):
    """rm_device.h glsl_sin / rm_oracle.c glsl_sin, operation by operation."""
    x = f32(x)
    y = f32(x * f32(1.59154943e-1))
    y = f32(y - np.rint(y))
    y2 = f32(y * y)
    c1 = f32(f32(y2 * f32(f32(y2 * f32(f32(y2 * f32(-0.0204391631)) + f32(0.2536086171))) + f32(-1.2336977925)))
             + f32(1.0))
    s1 = f32(y * f32(f32(y2 * f32(f32(y2 * f32(f32(y2 * f32(-0.0046075748)) + f32(0.0796819754))) + f32(-0.645963615)))
                     + f32(1.5707963235)))
    c2 = f32(f32(c1 * c1) - f32(s1 * s1))
    s2 = f32(f32(f32(2.0) * s1) * c1)
    return f32(f32(f32(f32(2.0) * s2) * c2) * f32(f32(1.0) / f32(f32(s2 * s2) + f32(c2 * c2))))


def glsl_cos(x):
    return glsl_sin(f32(f32(x) + f32(1.57079632)))


def sponge_rotation(time):
    """(ry_c, ry_s, rx_c, rx_s) of transformR(.., vec3(180, 2 u_time, 0)) as
    frame_const (rm_render_host.cpp) and init_ctx (rm_oracle.c) form them."""
    rad = f32(0.017453292519943295)
    rot_y = f32(f32(time) * f32(2.0))
    ay = f32(-rot_y * rad)
    ax = f32(f32(-180.0) * rad)
    return glsl_cos(ay), glsl_sin(ay), glsl_cos(ax), glsl_sin(ax)


def _max3(a, b, c):
    return np.maximum(a, np.maximum(b, c))


def smin_cubic(a, b, k):
    """sminCubic's distance (common.frag:72-80), k = vec2(k)."""
    k = f32(k)
    x = np.maximum(k - np.abs(a - b), f32(0.0))
    h = x / k
    m = h * h * h * f32(0.5)
    s = m * k * f32(f32(1.0) / f32(3.0))
    return np.where(a < b, a, b) - s


def fold_terms(q, m):
    """Fold m of sponge_folds at sponge-space points q: per axis the cell index
    floor(q s / 2) and a = mod(q s, 2) - 1 as the exact form writes it."""
    sh = (f32(0.5), f32(1.5), f32(4.5))[m]
    h = q * sh
    cell = np.floor(h)
    a = f32(2.0) * (h - cell) - f32(1.0)
    return cell, a


def quantities(p, time, d0=True):
    """Everything scene_dist_O forms at world points p [n, 3], in float32."""
    K = kernel_constants()
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    ry_c, ry_s, rx_c, rx_s = sponge_rotation(time)
    # sponge_rot<EXACT>(F, p.x, p.y - 3, p.z)
    ys = y - f32(3.0)
    x1 = x * ry_c + z * ry_s
    z1 = x * -ry_s + z * ry_c
    y2 = ys * rx_c + z1 * -rx_s
    z2 = ys * rx_s + z1 * rx_c
    q = np.stack([x1, y2, z2], -1)
    d3 = y
    lbs = np.minimum(_max3(np.abs(x - f32(3.0)), np.abs(y - f32(2.0)), np.abs(z - f32(3.0))),
                     _max3(np.abs(x + f32(5.0)), np.abs(y - f32(4.0)), np.abs(z - f32(5.0)))) - K["bound_offset"]
    mc = _max3(np.abs(x1), np.abs(y2), np.abs(z2)) - f32(1.0)
    slack = np.minimum(lbs - (d3 + K["slack_plane"]), mc - (d3 + K["slack_box"]))
    A = np.minimum(lbs, d3) - K["a_offset"]
    # the sphere, the cube and their blends (len3<EXACT>, cube<EXACT>)
    sx, sy, sz = x - f32(3.0), y - f32(2.0), z - f32(3.0)
    d1 = np.sqrt(sx * sx + sy * sy + sz * sz) - f32(1.0)
    cx, cy, cz = np.abs(x - f32(-5.0)) - f32(1.0), np.abs(y - f32(4.0)) - f32(1.0), np.abs(z - f32(5.0)) - f32(1.0)
    mx, my, mz = np.maximum(cx, f32(0.0)), np.maximum(cy, f32(0.0)), np.maximum(cz, f32(0.0))
    d2 = np.sqrt(mx * mx + my * my + mz * mz) + np.minimum(_max3(cx, cy, cz), f32(0.0))
    t1 = smin_cubic(d1, d2, 0.5)
    t2 = smin_cubic(t1, d3, 0.5)
    Q = dict(p=p, q=q, d3=d3, lbs=lbs, mc=mc, slack=slack, A=A, d1=d1, d2=d2, t1=t1, t2=t2, cube_q=(cx, cy, cz))
    # the five comparisons, as written
    Q["c_plane"] = lbs >= d3 + K["plane"]
    Q["c_box"] = mc >= d3 + K["box"]
    Q["c_dom_box"] = mc + K["dom_box"] <= A
    Q["c_reach"] = mc >= t2 + K["reach"]
    # the branches they select
    Q["p_plane"] = Q["c_plane"]
    Q["p_span"] = Q["c_plane"] & Q["c_box"]
    Q["p_folded"] = ~Q["c_plane"] & Q["c_dom_box"]
    Q["p_reach"] = ~Q["c_plane"] & ~Q["c_dom_box"] & Q["c_reach"]
    if d0:
        Q["d0"] = oracle.scene_dist("T", p, time=float(time))
        Q["c_dom"] = Q["d0"] + K["dom"] <= A
        Q["p_dom"] = Q["p_folded"] & Q["c_dom"]
    return Q


def expected_skip(p, time, Q=None):
    """(value, kind): what scene_dist_O returns where it returns early (kind
    KIND_PLANE: p.y; KIND_D0: the sponge alone; KIND_T2: t2 without the sponge's
    folds; KIND_PLANE_BLEND: the sponge blended with the plane for t2), NaN with
    KIND_NONE elsewhere; kind indexes KINDS."""
    Q = Q or quantities(p, time)
    n = len(Q["d3"])
    kind = np.zeros(n, np.int8)
    value = np.full(n, np.nan, f32)
    blend = Q["p_plane"] & ~Q["p_span"]
    for k, sel, v in ((KIND_PLANE_BLEND, blend, smin_cubic(Q["d0"], Q["d3"], 0.33)), (KIND_PLANE, Q["p_span"], Q["d3"]),
                      (KIND_D0, Q["p_dom"], Q["d0"]), (KIND_T2, Q["p_reach"], Q["t2"])):
        kind[sel] = k
        value[sel] = v[sel]
    return value, kind


# ------------------------------------------------------------ bisection


# ulp_step, straddle, adjacent_pairs: tests/float_edges.py (shared with tests/lib_edges.py)


def _axis_pairs(rng, lo, hi, n):
    """n pairs of points in the box [lo, hi] that differ in one random coordinate."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    a = rng.uniform(lo, hi, (n, 3)).astype(f32)
    b = a.copy()
    ax = rng.integers(0, 3, n)
    b[np.arange(n), ax] = rng.uniform(lo[ax], hi[ax]).astype(f32)
    return a, b


def _box(c, half):
    c = np.asarray(c, np.float64)
    return c - half, c + half


# ------------------------------------------------------------ the sets

WIDE = ((-9.0, -1.0, -9.0), (9.0, 8.0, 9.0))
N_PRED_PAIRS = 2200    # per scene-level predicate
N_TERM_PAIRS = 600     # box-term levels, blend edges, the sphere
N_FOLD_PAIRS = 200     # per (axis, fold) cell wall and kink
N_FACE_PAIRS = 300


class BoundarySets:
    """sets: name -> points [m, 3]; pairs: name -> (a, b) of the straddling sets;
    points / set_id / names: all of them concatenated."""

    def __init__(self, sets, pairs):
        self.sets, self.pairs = sets, pairs
        self.names = list(sets)
        self.points = np.ascontiguousarray(np.concatenate([sets[k] for k in self.names]), f32)
        self.set_id = np.concatenate([np.full(len(sets[k]), i, np.int16) for i, k in enumerate(self.names)])

    def select(self, prefixes):
        """Points of the sets whose name starts with one of prefixes."""
        return np.concatenate([self.sets[k] for k in self.names if k.startswith(tuple(prefixes))])


def sphere_surface(center, rng, n):
    """Points straddling the surface of the unit sphere at center (radially
    bisected along one coordinate) with their ulp neighbours."""
    c = np.asarray(center, f32)

    def inside(p):
        x, y, z = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        return np.sqrt(x * x + y * y + z * z) - f32(1.0) < f32(0.0)
    a, b = _axis_pairs(rng, *_box(center, 1.5), 12 * n)
    keep = np.flatnonzero(inside(a) != inside(b))[:n]
    return straddle(inside, a[keep], b[keep])


_CACHE = {}


def boundary_points(time, seed=5):
    """The point sets of one u_time (module docstring), cached."""
    key = (float(time), int(seed))
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng([int(seed), int(np.float32(time).view(np.uint32))])
    K = kernel_constants()
    sets, pairs = OrderedDict(), OrderedDict()

    def add(name, g, pools, n):
        """Up to n pairs from the candidate pools at whose ends g differs, bisected."""
        ka, kb = [], []
        for a, b in pools:
            keep = g(a) != g(b)
            ka.append(a[keep])
            kb.append(b[keep])
        a, b = np.concatenate(ka)[:n], np.concatenate(kb)[:n]
        pts, a, b = straddle(g, a, b)
        sets[name], pairs[name] = pts, (a, b)

    def of(key, d0=False):
        return lambda p: quantities(p, time, d0=d0)[key]

    wide = _axis_pairs(rng, *WIDE, 40000)
    near = _axis_pairs(rng, *_box(SPONGE_C, 2.3), 30000)
    core = _axis_pairs(rng, *_box(SPONGE_C, 1.5), 12000)
    cube = _axis_pairs(rng, *_box(CUBE_C, 2.5), 8000)
    # 1-4 (and the `folded` test that precedes 3)
    add("pred1 plane wins", of("p_plane"), [wide], N_PRED_PAIRS)
    # (the plane's margin has the least to spare where the sphere and the cube
    # blend deepest, d1 = d2, nearly face-on to the cube: there t1 comes closest
    # to its bound lbs, within 0.067; short pairs keep both ends near d1 = d2)
    a, _ = _axis_pairs(rng, (-3.5, 1.0, 1.5), (1.5, 4.5, 6.5), 150000)
    Q = quantities(a, time, d0=False)
    a = a[np.abs(Q["d1"] - Q["d2"]) < f32(0.1)]
    b = a.copy()
    ax = rng.integers(0, 3, len(a))
    b[np.arange(len(a)), ax] += rng.uniform(-0.8, 0.8, len(a)).astype(f32)
    add("plane margin where sphere and cube blend", of("p_plane"), [(a, b)], N_TERM_PAIRS)
    add("pred2 box past the blend", of("p_span"), [wide], N_PRED_PAIRS)
    add("pred3 sponge dominance (box)", of("p_folded"), [near, wide], N_PRED_PAIRS)
    add("pred3 sponge dominance", of("p_dom", True), [near, wide], N_PRED_PAIRS)
    add("pred4 sponge out of reach", of("p_reach"), [near, wide], N_PRED_PAIRS)
    # 5: the surface and the three fold exits of the box term
    for name, lvl in (("0", f32(0.0)), ("1/27", K["fold_exits"][2]), ("1/9", K["fold_exits"][1]),
                      ("1/3", K["fold_exits"][0])):
        add(f"fold exit mc {name}", lambda p, lvl=lvl: quantities(p, time, d0=False)["mc"] < lvl, [near], N_TERM_PAIRS)
    for m, s in enumerate(("1", "3", "9")):
        for c, axis in enumerate("xyz"):
            add(f"fold wall {axis} s={s}",
                lambda p, m=m, c=c: np.mod(fold_terms(quantities(p, time, d0=False)["q"][:, c], m)[0], 2) == 0,
                [core], N_FOLD_PAIRS)
            add(f"fold kink {axis} s={s}",
                lambda p, m=m, c=c: np.abs(fold_terms(quantities(p, time, d0=False)["q"][:, c], m)[1])
                < f32(f32(1.0) / f32(3.0)), [core], N_FOLD_PAIRS)

    def edge(ka, kb, w, d0=False):
        def g(p):
            Q = quantities(p, time, d0=d0)
            return np.abs(Q[ka] - Q[kb]) < f32(w)
        return g
    add("blend edge |d1-d2| 0.5", edge("d1", "d2", 0.5), [wide], N_TERM_PAIRS)
    add("blend edge |t1-d3| 0.5", edge("t1", "d3", 0.5), [wide], N_TERM_PAIRS)
    add("blend edge |d0-t2| 0.33", edge("d0", "t2", 0.33, True), [near, wide], N_TERM_PAIRS)
    for c, axis in enumerate("xyz"):
        add(f"cube face {axis}", lambda p, c=c: quantities(p, time, d0=False)["cube_q"][c] < f32(0.0), [cube],
            N_FACE_PAIRS)
    sets["sphere surface"], a, b = sphere_surface(SPHERE_C, rng, N_TERM_PAIRS)
    pairs["sphere surface"] = (a, b)
    # the plane from both sides
    xz = rng.uniform(-9.0, 9.0, (256, 2)).astype(f32)
    tiny = f32(1e-45)  # the smallest denormal
    ys = [f32(0.0), f32(-0.0)]
    for k in (1, 2, 3, 4):
        ys += [ulp_step(f32(0.0), k), ulp_step(f32(-0.0), -k)]
    ys += [f32(s * v) for s in (1, -1) for v in (tiny, 1.1754944e-38, 1e-30, 1e-6, 1e-3, 0.02)]
    sets["plane y=0"] = np.concatenate([np.stack([xz[:, 0], np.full(256, y, f32), xz[:, 1]], -1) for y in ys])
    sets["centres"] = np.array([SPHERE_C, CUBE_C, SPONGE_C], f32)
    sets["uniform"] = rng.uniform(*WIDE, (20000, 3)).astype(f32)
    far = (10.0 ** rng.uniform(1.0, 4.0, (5000, 3))) * rng.choice([-1.0, 1.0], (5000, 3))
    sets["far"] = far.astype(f32)
    B = BoundarySets(sets, pairs)
    assert len(B.points) < 300000, len(B.points)
    _CACHE[key] = B
    return B


# fixed u_times of the tests: the quoted poses' extremes plus one drawn from a fixed seed
TIMES = (0.0, 57.79888, 137.59444, 177.62172, float(f32(np.random.default_rng(2024).uniform(0.0, 180.0))))
