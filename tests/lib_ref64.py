"""float64 numpy restatement of every known-answer case of the scene library
(tests/golden/lib_kat_cases.py CASES, and the angle variants CASES2 below),
written from common.frag's definitions: true sin / cos, true division, no fused
operations, every operation in float64.  Test infrastructure only.

evaluate(name, p) returns a Result:
  out      [n, 17]: dist and the 16 Material floats (rm_scene_eval's order)
  branches list of Branch(value [n], tol_scale [n] or float, decides): the
           signed quantity a comparison of the function branches on (its sign
           is the side taken, |value| the margin).  `decides`: outputs jump
           across it (a smooth minimum's edges and the box terms only kink).
  disc     [17] bool: the outputs that jump across a deciding branch
  period   [17]: > 0 for a folded coordinate of pMod, compared modulo it where
           the point is undecided

A point is undecided for a case when a deciding margin is within the case's
class tolerance (rel, ab) times the branch's scale: tol_scale is the
Lipschitz factor of the branch value in the point, times the magnitude the
relative term applies to.  There only the outputs outside `disc` are compared.
A margin of exactly 0 in float64 is a tie in real arithmetic (mengersponge: a
fold's c equals the d before it on whole regions of the sponge, by its
self-similarity); such points are their own class, `tie`, reported apart from
the near-tie points the 5 % cap is about.
"""
import re
from collections import namedtuple

import numpy as np

from tests.golden import lib_kat_cases as kat

Branch = namedtuple("Branch", "value tol_scale decides")
Result = namedtuple("Result", "out branches disc period")

KA = np.array([0.2, 0.02, 0.02, 0.04, 0.02, 0.02, 32.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
KB = np.array([0.02, 0.3, 0.5, 0.5, 0.25, 0.125, 64.0, 0.25, 0.5, 0.4, 0.4, 0.15, 1.52, 0.0, 0.0, 4.0])
POS = np.array([1.0, -0.5, 2.0])
ROT = (20.0, 35.0, -15.0)
SCL = np.array([1.5, 0.5, 2.0])
DISC_MAT = np.array([False] + [True] * 16)
DISC_NONE = np.zeros(17, bool)


def _len(v):
    return np.sqrt((v * v).sum(-1))


def _out(d, v=None):
    """SdResult(d, kOut(v)): diffuse v, refraction_index 1, the rest 0."""
    o = np.zeros((len(d), 17))
    o[:, 0] = d
    if v is not None:
        o[:, 1:4] = v
    o[:, 13] = 1.0
    return o


def _sd(d, mat):
    o = np.empty((len(d), 17))
    o[:, 0] = d
    o[:, 1:] = mat
    return o


def _res(out, branches=(), disc=DISC_NONE, period=None):
    return Result(out, list(branches), disc, np.zeros(17) if period is None else period)


def _mix(x, y, a):
    return x * (1.0 - a) + y * a


def sphere(s, p):
    return _len(p - np.array(s[:3])) - s[3]


def cube_terms(s, p):
    return np.abs(p - np.array(s[:3])) - s[3]


def cube(s, p):
    q = cube_terms(s, p)
    return _len(np.maximum(q, 0.0)) + np.minimum(q.max(-1), 0.0)


def sd_box(p, b):
    """common.frag:595-600: min(max(di), length(max(di, 0)))."""
    di = np.abs(p) - b
    return np.minimum(di.max(-1), _len(np.maximum(di, 0.0)))


def torus(p, t):
    return np.sqrt((_len(p[:, :2]) - t[0]) ** 2 + p[:, 2] ** 2) - t[1]


def k_sph(p):
    return sphere((0.5, 1.0, 0.0, 1.0), p)


def k_cub(p):
    return cube((-1.0, 0.5, 0.5, 0.8), p)


def k_tor(p):
    return torus(p, (1.0, 0.3))


def _face_branches(q):
    """a box's face and edge terms: kinks only"""
    return [Branch(q[:, c], 1.0, False) for c in range(3)]


def _smooth(fn, sign1=1.0):
    def case(p, k, a=k_sph, b=k_cub):
        d1, d2 = a(p), b(p)
        return _res(_out(fn(d1, d2, k)), [Branch(k - np.abs(d2 - sign1 * d1), 2.0, False),
                                          Branch(d2 - sign1 * d1, 2.0, False)])
    return case


def _op_smooth_union(d1, d2, k):
    h = np.clip(0.5 + 0.5 * (d2 - d1) / k, 0.0, 1.0)
    return _mix(d2, d1, h) - k * h * (1.0 - h)


def _op_smooth_sub(d1, d2, k):
    h = np.clip(0.5 - 0.5 * (d2 + d1) / k, 0.0, 1.0)
    return _mix(d2, -d1, h) + k * h * (1.0 - h)


def _op_smooth_int(d1, d2, k):
    h = np.clip(0.5 - 0.5 * (d2 - d1) / k, 0.0, 1.0)
    return _mix(d2, d1, h) + k * h * (1.0 - h)


def _smin_exp(a, b, k):
    return -np.log(np.maximum(0.0001, np.exp(-k * a) + np.exp(-k * b))) / k


def smin_cubic(a, ma, b, mb, k):
    """sminCubic (common.frag:72-85) with ALLOW_MATERIAL_BLENDING: continuous in
    both parts (at a = b the blend coefficient is 1/2 from either side)."""
    k = np.maximum(np.array(k), 0.0001)
    h = np.maximum(k[None, :] - np.abs(a - b)[:, None], 0.0) / k[None, :]
    m = h * h * h * 0.5
    s = m * k[None, :] / 3.0
    closer = a < b
    coeff = np.where(closer, m[:, 1], 1.0 - m[:, 1])
    out = _sd(np.where(closer, a, b) - s[:, 0], _mix(ma[None, :], mb[None, :], coeff[:, None]))
    return _res(out, [Branch(a - b, 2.0, False), Branch(k[0] - np.abs(a - b), 2.0, False),
                      Branch(k[1] - np.abs(a - b), 2.0, False)])


# ------------------------------------------------------------- rotations


def _cs(deg):
    a = np.radians(deg)
    return np.cos(a), np.sin(a)


def mul_rx(v, deg):  # vec4(v, 1) * rotationX(deg)
    c, s = _cs(deg)
    return np.stack([v[:, 0], c * v[:, 1] - s * v[:, 2], s * v[:, 1] + c * v[:, 2]], -1)


def mul_ry(v, deg):
    c, s = _cs(deg)
    return np.stack([c * v[:, 0] + s * v[:, 2], v[:, 1], -s * v[:, 0] + c * v[:, 2]], -1)


def mul_rz(v, deg):
    c, s = _cs(deg)
    return np.stack([c * v[:, 0] - s * v[:, 1], s * v[:, 0] + c * v[:, 1], v[:, 2]], -1)


def _transform(p, pos=None, rot=None, axis=None, angle=None, scale=None):
    v = p - pos if pos is not None else p
    if rot is not None:
        v = mul_rz(mul_rx(mul_ry(v, -rot[1]), -rot[0]), -rot[2])
    else:
        v = {"X": mul_rx, "Y": mul_ry, "Z": mul_rz}[axis](v, -angle)
    return v / scale if scale is not None else v


def _rotate_point(p, a, i, j):
    """p.ij = cos(a) p.ij + sin(a) vec2(p.j, -p.i)"""
    c, s = np.cos(a), np.sin(a)
    q = p.copy()
    q[:, i] = c * p[:, i] + s * p[:, j]
    q[:, j] = c * p[:, j] - s * p[:, i]
    return q


# ------------------------------------------------------------- fractals


def mengersponge(p):
    """common.frag:654-679.  Returns (res [n, 3], c - d per fold [n, 3], wall
    distances [n, 9]): res = (d, 0.2 da db dc, (1 + m) / 4) of the last fold that
    won `c > d`."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    d = sd_box(p, 1.0)
    res = np.stack([d, np.ones_like(d), np.zeros_like(d)], -1)
    s = 1.0
    diff, walls = [], []
    for m in range(3):
        x = p * s
        a = np.mod(x, 2.0) - 1.0
        walls.append((x * 0.5 - np.round(x * 0.5)) * 2.0 / s)  # distance to the cell wall, in p
        s *= 3.0
        r = np.abs(1.0 - 3.0 * np.abs(a))
        da, db, dc = np.maximum(r[:, 0], r[:, 1]), np.maximum(r[:, 1], r[:, 2]), np.maximum(r[:, 2], r[:, 0])
        c = (np.minimum(da, np.minimum(db, dc)) - 1.0) / s
        diff.append(c - d)
        won = c > d
        d = np.where(won, c, d)
        res = np.where(won[:, None], np.stack([d, 0.2 * da * db * dc, np.full_like(d, (1.0 + m) / 4.0)], -1), res)
    return res, np.stack(diff, -1), np.concatenate(walls, -1)


def mandelbulb(p):
    """common.frag:622-651.  Returns (dist, resColor [n, 4], m - 256 per
    iteration [n, 4] (NaN after the break))."""
    w = p.copy()
    m = (w * w).sum(-1)
    trap = np.concatenate([np.abs(w), m[:, None]], -1)
    dz = np.ones(len(p))
    live = np.ones(len(p), bool)
    marg = np.full((len(p), 4), np.nan)
    with np.errstate(all="ignore"):
        for i in range(4):
            dz_n = 8.0 * np.power(m, 3.5) * dz + 1.0
            r = _len(w)
            b = 8.0 * np.arccos(np.clip(w[:, 1] / r, -1.0, 1.0))
            a = 8.0 * np.arctan2(w[:, 0], w[:, 2])
            w_n = p + np.power(r, 8.0)[:, None] * np.stack([np.sin(b) * np.sin(a), np.cos(b), np.sin(b) * np.cos(a)], -1)
            trap_n = np.minimum(trap, np.concatenate([np.abs(w_n), m[:, None]], -1))
            m_n = (w_n * w_n).sum(-1)
            dz = np.where(live, dz_n, dz)
            w = np.where(live[:, None], w_n, w)
            trap = np.where(live[:, None], trap_n, trap)
            m = np.where(live, m_n, m)
            marg[live, i] = m[live] - 256.0
            live = live & ~(m > 256.0)
        dist = 0.25 * np.log(m) * np.sqrt(m) / dz
    return dist, np.concatenate([m[:, None], trap[:, 1:]], -1), marg


# ------------------------------------------------------------- the cases

_N3 = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
_NR = np.array([1.0, -1.0, 0.5]) / 1.5


def _case_sponge(p):
    res, diff, walls = mengersponge(p * 0.5)
    disc = np.zeros(17, bool)
    disc[2:4] = True  # res.y, res.z: which fold won
    # c - d moves by at most 2 |dp|: c = (med(r) - 1) / (3 s) with |dr| <= 3 s |dp|, the box term 1-Lipschitz
    br = [Branch(diff[:, m], 2.0 * (1.0 + np.abs(res[:, 0])), True) for m in range(3)]
    br += [Branch(walls[:, j], 1.0, False) for j in range(9)]
    return _res(_out(res[:, 0], res), br, disc)


def _case_bulb(p, which):
    d, c, marg = mandelbulb(p * 0.6)
    out = _out(d, c[:, 1:]) if which == 0 else _out(np.log(c[:, 0]) + 0.0 * d)
    # m goes through r^8 per iteration: a relative error e of the float32 m grows to ~8 e each time; the
    # class's relative tolerance on m = 256 is the scale (the margin is in units of m)
    br = [Branch(np.where(np.isnan(marg[:, i]), np.inf, marg[:, i]), 256.0, True) for i in range(4)]
    return _res(out, br, np.ones(17, bool))


def _case_pmod1(p):
    size, h = 1.5, 0.75
    u = (p[:, 0] + h) / size
    q = p.copy()
    q[:, 0] = np.mod(p[:, 0] + h, size) - h
    disc, period = np.zeros(17, bool), np.zeros(17)
    disc[0] = True
    period[1] = size
    return _res(_out(np.floor(u), q), [Branch(u - np.round(u), 1.0 / size, True)], disc, period)


def _case_pmod2(p):
    size = np.array([1.5, 0.8])
    xz = p[:, [0, 2]]
    u = (xz + size * 0.5) / size
    c = np.floor(u)
    q = np.mod(xz + size * 0.5, size) - size * 0.5
    disc, period = np.zeros(17, bool), np.zeros(17)
    disc[[0, 1]] = True
    period[2], period[3] = size
    return _res(_out(c[:, 0], np.stack([c[:, 1], q[:, 0], q[:, 1]], -1)),
                [Branch(u[:, j] - np.round(u[:, j]), 1.0 / size[j], True) for j in range(2)], disc, period)


def _case_pmirror(p):
    q = p.copy()
    q[:, 0] = np.abs(p[:, 0]) - 0.8
    disc = np.zeros(17, bool)
    disc[0] = True
    return _res(_out(np.where(p[:, 0] < 0, -1.0, 1.0), q), [Branch(p[:, 0], 1.0, True)], disc)


def _case_preflect(p):
    t = p @ _NR + 0.3
    q = np.where((t < 0)[:, None], p - (2.0 * t)[:, None] * _NR, p)
    disc = np.zeros(17, bool)
    disc[0] = True
    return _res(_out(np.where(t < 0, -1.0, 1.0), q), [Branch(t, 1.0, True)], disc)


def _case_sdunion(p):
    a, b = k_sph(p), k_tor(p)
    out = np.where((a < b)[:, None], _sd(a, KA[None, :]), _sd(b, KB[None, :]))
    return _res(out, [Branch(a - b, 2.0, True)], DISC_MAT)


def _case_cube(p):
    s = (-0.4, 0.5, 0.2, 0.9)
    return _res(_out(cube(s, p)), _face_branches(cube_terms(s, p)))


def _case_sdbox(p, rounding=0.0):
    b = np.array([1.0, 0.5, 0.7])
    return _res(_out(sd_box(p, b) - rounding), _face_branches(np.abs(p) - b))


def _v(fn):
    return lambda p: _res(_out(fn(p)[:, 0], fn(p)))


def _w1(fn):  # r4(v.w, v.xyz) of vec4(p, 1) * rotation
    return lambda p: _res(_out(np.ones(len(p)), fn(p)))


def _d(fn):
    return lambda p: _res(_out(fn(p)))


def _rot_point2(p, a):
    q = _rotate_point(p, a, 0, 2)
    return _res(_out(q[:, 0], np.stack([q[:, 0], q[:, 2], np.zeros(len(p))], -1)))


def _blend_material(p):
    k = np.clip(p[:, 0] * 0.2 + 0.5, 0.0, 1.0)
    return _res(_sd(np.zeros(len(p)), _mix(KA[None, :], KB[None, :], k[:, None])),
                [Branch(p[:, 0] * 0.2 + 0.5, 0.2, False), Branch(0.5 - p[:, 0] * 0.2, 0.2, False)])


def _axis_cases(axis, angle):
    """The twelve single-axis transform cases of one axis at one angle."""
    kw = dict(axis=axis, angle=angle)
    return {
        f"transformTR{axis}": _v(lambda p: _transform(p, pos=POS, **kw)),
        f"transformTR{axis}S": _v(lambda p: _transform(p, pos=POS, scale=SCL, **kw)),
        f"transformTR{axis}S1": _v(lambda p: _transform(p, pos=POS, scale=1.7, **kw)),
        f"transformR{axis}": _v(lambda p: _transform(p, **kw)),
        f"transformR{axis}S": _v(lambda p: _transform(p, scale=SCL, **kw)),
        f"transformR{axis}S1": _v(lambda p: _transform(p, scale=1.7, **kw)),
    }


REF = {
    "opUnion": _d(lambda p: np.minimum(k_sph(p), k_cub(p))),
    "opSubtraction": _d(lambda p: np.maximum(-k_sph(p), k_cub(p))),
    "opIntersection": _d(lambda p: np.maximum(k_sph(p), k_cub(p))),
    "opSmoothUnion": lambda p: _smooth(_op_smooth_union)(p, 0.7),
    "opSmoothSubtraction": lambda p: _smooth(_op_smooth_sub, -1.0)(p, 0.7),
    "opSmoothIntersection": lambda p: _smooth(_op_smooth_int)(p, 0.7),
    "sdf_blend": _d(lambda p: 0.3 * k_sph(p) + (1.0 - 0.3) * k_tor(p)),
    "smin": lambda p: _smooth(_op_smooth_union)(p, 0.6),
    "smin_exp": _d(lambda p: _smin_exp(k_sph(p), k_cub(p), 4.0)),
    "smin_exp32": _d(lambda p: _smin_exp(k_sph(p) * 0.1, k_cub(p) * 0.1, 32.0)),
    "rounding": lambda p: _case_sdbox(p, 0.1),
    "plane_sdPlane": _d(lambda p: p[:, 1] + 0.5 * (p @ _N3 + 0.5)),
    "sphere": _d(lambda p: sphere((0.3, -0.2, 0.5, 1.2), p)),
    "cube": _case_cube,
    "sdBox": _case_sdbox,
    "cylinder": _d(lambda p: _len(p[:, :2]) - 0.7),
    "cone": _d(lambda p: 0.8 * _len(p[:, :2]) + 0.6 * p[:, 2]),
    "torus": _d(k_tor),
    "mengersponge": _case_sponge,
    "mandelbulb": lambda p: _case_bulb(p, 0),
    "mandelbulb_m": lambda p: _case_bulb(p, 1),
    "rotatePoint": lambda p: _rot_point2(p, 0.7),
    "rotatePointX": _v(lambda p: _rotate_point(p, 0.7, 1, 2)),
    "rotatePointY": _v(lambda p: _rotate_point(p, -1.1, 0, 2)),
    "rotatePointZ": _v(lambda p: _rotate_point(p, 2.3, 0, 1)),
    "translatePoint": _v(lambda p: p - np.array([0.5, -1.0, 2.0])),
    "rotationX": _w1(lambda p: mul_rx(p, 33.0)),
    "rotationY": _w1(lambda p: mul_ry(p, -47.0)),
    "rotationZ": _w1(lambda p: mul_rz(p, 128.0)),
    "transform": _v(lambda p: _transform(p, pos=POS, rot=ROT, scale=SCL)),
    "transformTR": _v(lambda p: _transform(p, pos=POS, rot=ROT)),
    "transformTRS1": _v(lambda p: _transform(p, pos=POS, rot=ROT, scale=1.7)),
    "transformR": _v(lambda p: _transform(p, rot=(180.0, 33.0, 0.0))),
    "transformRS1": _v(lambda p: _transform(p, rot=ROT, scale=1.7)),
    "pMod1": _case_pmod1,
    "pMod2": _case_pmod2,
    "pMirror": _case_pmirror,
    "pReflect": _case_preflect,
    "sdUnion": _case_sdunion,
    "sminCubic": lambda p: smin_cubic(k_sph(p), KA, k_tor(p), KB, (0.8, 0.8)),
    "sminCubic2": lambda p: smin_cubic(k_cub(p), KB, k_tor(p), KA, (0.5, 1.5)),
    "blendMaterial": _blend_material,
    "scaleSDF": _d(lambda p: k_tor(p / 1.7) * 1.7),
    "scaleSDF3": _d(lambda p: k_tor(p / np.array([1.7, 0.8, 1.2])) * 0.8),
}
for _axis, _angle in (("X", 40.0), ("Y", 50.0), ("Z", 60.0)):
    REF.update(_axis_cases(_axis, _angle))
assert sorted(REF) == sorted(c[0] for c in kat.CASES), set(REF) ^ set(c[0] for c in kat.CASES)

# ------------------------------------------- the angle variants (CASES2)

ANGLES = (0.0, 90.0, 180.0, 270.0, 360.0, -90.0, 33.0)
_ANGLE_CASE = re.compile(r"^(rotation[XYZ]|transform(TR|R)[XYZ](S1|S)?)$")


def _with_angle(body, angle_text):
    """The case's body with its rotation angle (the number before `)` or `, vec3`/
    `, 1.7` of a single-axis case; the argument of rotationX/Y/Z) replaced."""
    if body.startswith("vec4 v = vec4(p, 1.0) * rotation"):
        return re.sub(r"(rotation[XYZ]\()[-0-9.]+\)", lambda m: m.group(1) + angle_text + ")", body)
    return re.sub(r"(, )(40\.0|50\.0|60\.0)([,)])", lambda m: m.group(1) + angle_text + m.group(3), body, count=1)


def cases2():
    """(name, body, class, angle): every single-axis rotation case with the angle
    read from u_mouse.x at run time (angle None: set per launch from ANGLES), and
    with the literal 0.0, the one spelling at which the probe instance's
    rot_is_identity drops the rotation."""
    out = []
    for name, body, cls in kat.CASES:
        if _ANGLE_CASE.match(name):
            out.append((name + "@u", _with_angle(body, "u_mouse.x"), cls, None))
            out.append((name + "@0", _with_angle(body, "0.0"), cls, 0.0))
    return out


def ref2(name, angle):
    """The reference of a CASES2 case at an angle in degrees."""
    base = name.split("@")[0]
    if base.startswith("rotation"):
        return _w1(lambda p: {"X": mul_rx, "Y": mul_ry, "Z": mul_rz}[base[-1]](p, angle))
    axis = re.search(r"[XYZ]", base[len("transform"):]).group(0)
    return _axis_cases(axis, angle)[base]


def plugin_source2():
    """CASES followed by CASES2 as one eval-only plugin (lib_kat_cases.plugin_source's form)."""
    allc = [(n, b) for n, b, _ in kat.CASES] + [(n, b) for n, b, _, _ in cases2()]
    body = "\n".join(f"\tif (fn == {i}) {{ {b} }}" for i, (_, b) in enumerate(allc))
    return ("// generated by tests/lib_ref64.py (scene-library edge sets)\n#define RM_PLUGIN_EVAL_ONLY\n"
            "#define RM_PLUGIN_EVAL_PROBE\n" + kat.PRELUDE + "SdResult kat(int fn, vec3 p)\n{\n" + body +
            "\n\treturn r1(0.0);\n}\nSdResult sceneSDF(vec3 p)\n{\n\treturn kat(int(u_time), p);\n}\n")


# ------------------------------------------------------------- judging


def evaluate(name, p, angle=None):
    p = np.ascontiguousarray(p, np.float64).reshape(-1, 3)
    return (ref2(name, angle) if "@" in name else REF[name])(p)


def undecided(res, rel, ab):
    """(undecided [n], tie [n]): a deciding margin within the tolerance; exactly 0."""
    und = np.zeros(len(res.out), bool)
    tie = np.zeros(len(res.out), bool)
    for b in res.branches:
        if b.decides:
            und |= np.abs(b.value) <= (ab + rel) * np.asarray(b.tol_scale, np.float64)
            tie |= b.value == 0.0
    return und, tie


def compare(res, dist, mat, rel, ab):
    """ok [n]: every output within ab + rel |ref| at decided points, the
    continuous ones (folded coordinates modulo their period) at undecided ones;
    also the largest deviation among the compared outputs."""
    got = np.concatenate([np.asarray(dist, np.float64)[:, None], np.asarray(mat, np.float64)], -1)
    und, _ = undecided(res, rel, ab)
    diff = got - res.out
    per = res.period[None, :]
    safe = np.where(per > 0, per, 1.0)
    folded = np.where(per > 0, diff - safe * np.round(diff / safe), diff)
    diff = np.where(und[:, None], folded, diff)
    ok = np.abs(diff) <= ab + rel * np.abs(res.out)
    skip = und[:, None] & res.disc[None, :]
    dev = np.where(skip, 0.0, np.abs(diff))
    return (ok | skip).all(-1), float(np.nanmax(dev)) if dev.size else 0.0
