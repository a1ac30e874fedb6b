"""Edge sets for the scene-library cases (tests/lib_ref64.py): per case a few
hundred float32 points, seeded: a box that reaches past the golden points'
[-2.6, 2.6] into negative and far coordinates, and for every branch of the
case adjacent-float pairs bisected onto the branch (tests/float_edges.py
straddle) with their 1..4-ulp neighbours and the ends moved by +-16 and +-4096
ulps.  Cases with faces get points exactly on them.  Test infrastructure only."""
import zlib

import numpy as np

from tests import lib_ref64 as ref64
from tests.float_edges import straddle, ulp_step

f32 = np.float32
# The box of the random points and of the pairs: past the golden points' 2.6, and no farther.  The class
# tolerances are stated for distances of the golden points' size.  The exact class's 2e-6 (1 + |v|) on a
# blended material needs |a - b| to ~1.5 ulp of the distances (sminCubic: d coeff = 1.5 h^2 / k d|a - b|, times
# the materials' range of 4 in emission.z): that holds to distances of ~5, ulp 4.8e-7, and not at 10 (measured
# at p = (-7.45, 7.45, 3.83), distances 9.8, probe instance: emission.z 8.7e-6 off against 5.4e-6 allowed; at
# |p| ~ 35 pMod2's folded coordinate is ulp(|p|) = 3.1e-6 off in the exact instance too).
BOX = 3.0
FAR = 8.0  # pMod1, pMod2, pMirror: more cells, where only a coordinate's own ulp (<= 9.5e-7) enters
N_BASE = 1024
N_PAIRS = 8  # per deciding branch
N_KINK_PAIRS = 5  # per branch that only kinks
_CACHE = {}


def _branch_side(name, j, angle):
    def g(p):
        v = ref64.evaluate(name, p, angle).branches[j].value
        return np.where(np.isfinite(v), v < 0, False)
    return g


def edge_points(name, angle=33.0):
    key = (name, angle)
    if key in _CACHE:
        return _CACHE[key]
    if name.endswith("@0"):
        angle = 0.0
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pts = [rng.uniform(-BOX, BOX, (N_BASE, 3)).astype(f32),
           np.zeros((1, 3), f32) + f32(1e-3), -np.abs(rng.uniform(0.0, BOX, (32, 3))).astype(f32)]
    base = name.split("@")[0]
    if base in ("cube", "sdBox", "rounding"):  # inside, on and outside the box: faces, edges, corners exactly
        c, r = ((-0.4, 0.5, 0.2), (0.9, 0.9, 0.9)) if base == "cube" else ((0.0, 0.0, 0.0), (1.0, 0.5, 0.7))
        grid = np.array([[f32(c[k]) + f32(s) * f32(r[k]) for k in range(3)] for s in (-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5)])
        pts.append(np.stack(np.meshgrid(grid[:, 0], grid[:, 1], grid[:, 2], indexing="ij"), -1).reshape(-1, 3).astype(f32))
    if base in ("pMod1", "pMod2", "pMirror"):  # farther cells; on the cell walls and the mirror exactly
        pts.append(rng.uniform(-FAR, FAR, (64, 3)).astype(f32))
        t = np.array([-8.25, -2.25, -0.75, 0.0, 0.75, 2.25, 8.25, -0.4, 0.4, 1.2, -2.0], f32)
        pts.append(np.stack([t, rng.uniform(-1, 1, len(t)).astype(f32), t[::-1]], -1))
    branches = ref64.evaluate(name, pts[0], angle).branches
    for j, br in enumerate(branches):
        g = _branch_side(name, j, angle)
        a = rng.uniform(-BOX, BOX, (4000, 3)).astype(f32)
        b = a.copy()
        ax = rng.integers(0, 3, len(a))
        b[np.arange(len(a)), ax] = rng.uniform(-BOX, BOX, len(a)).astype(f32)
        keep = np.flatnonzero(g(a) != g(b))[:N_PAIRS if br.decides else N_KINK_PAIRS]
        if len(keep) == 0:
            continue
        near, ea, eb = straddle(g, a[keep], b[keep], cross=2)
        pts.append(near)
        for end in (ea, eb):
            for k in (16, 4096, -16, -4096):
                moved = end.copy()
                c = ax[keep]
                moved[np.arange(len(end)), c] = ulp_step(end[np.arange(len(end)), c], k)
                pts.append(moved)
    out = np.ascontiguousarray(np.concatenate(pts), f32)
    _CACHE[key] = out
    return out
