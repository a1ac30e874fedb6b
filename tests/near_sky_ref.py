"""Scene T's near-sky ladder (raymarching_amd/csrc/rm_far_sky.h 3., DESIGN.md
2.27) restated in numpy beside tests/far_sky_ref.py: the ladder of (m, r, N)
rungs with N computed from r as the header computes it, the rung a step cap
admits (rmfs::near_sky_radius), the per-ray vote at that radius
(rmfs::near_sky_ray: far_sky_ref's miss test with r as an argument, and its
far-point test) and the per-wave vote of a frame's 8 x 8 tiles.  It states which
waves qualify and decides no colour.  tests/test_near_sky_host.py holds the
ladder, the rung choice and the predicate to the header itself (tests/host/
near_sky_test.cpp --ladder, --radius, --eval) with zero disagreements.

The frame kernels build their rays with the hardware's reciprocal and square
root, whose last bits numpy does not restate, so a wave's vote is stated twice:
`strict`, at a radius and a far-point threshold raised by 1e-4 relative, and
`loose`, lowered by as much.  A test may conclude only where both agree.
CPU only.
"""
import math

import numpy as np

from raymarching_amd.poses import POSES
from tests import far_sky_ref as fs
from tests.shadow_clear_ref import camera_dirs

F32 = np.float32
UNIT_LO, UNIT_HI = 0.999, 1.001  # rmfs::kUnitLo, kUnitHi
UNIT_ROT_TOL = F32(1.0e-4)        # rmfs::kUnitRotTol
RUNG_M = (F32(0.25), F32(0.1), F32(0.05), F32(0.02))


def radius_of(m):
    """1 + m + 2^-10 in float32, the header's order of additions"""
    return F32(F32(F32(1.0) + F32(m)) + F32(2.0 ** -10))


def bound(r):
    """rmfs::near_sky_bound: the same double arithmetic, operation for operation"""
    m = float(F32(r)) - 1.0 - 2.0 ** -10
    e = 2.0 ** -12
    s3lo, s3hi = 1.7320508075, 1.7320508076
    c, vmin = UNIT_LO / s3hi, s3lo * m
    if not m >= 0.015625:
        return 0x7fffffff
    nA, v = 0, 1025.0
    while v > vmin:
        nA += 1
        v *= 1.0 - c
    nB = int(2.0 * s3hi * (1.0 + e + m) / (UNIT_LO * m)) + 1
    nC, g = 0, 1.0
    while (g - 1.0) * vmin < 50.0 * UNIT_HI:
        nC += 1
        g *= 1.0 + c
    return nA + nB + nC


LADDER = tuple((m, radius_of(m), bound(radius_of(m))) for m in RUNG_M)  # widest first
N_OF = tuple(n for _, _, n in LADDER)                                    # 39, 63, 98, 205


def radius(max_steps, unit_dirs=True):
    """rmfs::near_sky_radius -> float32, 0 for none"""
    r = F32(0.0)
    if unit_dirs:
        for _, ri, n in LADDER:
            if max_steps >= n:
                r = ri
    elif max_steps >= fs.K_N0:
        r = fs.K_R
    return r


def unit_rotation(c, s):
    """rmfs::unit_rotation"""
    c, s = F32(c), F32(s)
    with np.errstate(invalid="ignore", over="ignore"):
        n = F32(F32(F32(c * c) + F32(s * s)) - F32(1.0))
        return bool(n <= UNIT_ROT_TOL and n >= -UNIT_ROT_TOL)


def near_sky_ray(o, d, r, far=fs.K_FAR):
    """rmfs::near_sky_ray on rows of sponge-space o, d [n, 3] -> [n] bool.  r: a float32 or one per row."""
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    r = np.asarray(r, F32)
    if r.ndim == 0:
        return fs.ray_misses_cube(o, d, r) & fs.far_point_clear(o, d, far)
    r = np.ascontiguousarray(r)
    out = np.zeros(len(o), bool)
    with np.errstate(invalid="ignore"):
        for v in np.unique(r.view(np.uint32)):  # (by bits: a NaN radius is a radius)
            sel = r.view(np.uint32) == v
            out[sel] = fs.ray_misses_cube(o[sel], d[sel], r[sel][0]) & fs.far_point_clear(o[sel], d[sel], far)
    return out


# ---- the frames of tests/test_near_sky_gpu.py

SIZES = [(64, 64), (96, 54), (61, 37)]  # 61x37: ragged tiles, partly filled waves
# N - 1 and N of every rung, 128 (config C2), either side of the far-sky vote's N0, the benchmark's 256
CAPS = sorted({c for n in N_OF for c in (n - 1, n)} | {128, fs.K_N0 - 1, fs.K_N0, 256})

# pose -> (pose, rung): the widest rung (index into LADDER) at which whole waves of the frame newly qualify
POSE_SET = {
    # the headline pose: sky tiles pass the sponge at every distance
    "P0": (POSES["P0"], 0),
    # looking along the face x = +1 from 0.15, 0.07 and 0.03 in front of its plane, beside the face itself: the
    # origin lies inside the cube of the rung before, where no ray passes, and outside the rung's own, where the
    # half of the frame that looks away from the plane does: whole waves that miss by that much and no more
    "face_015": (dict(pos=(1.15, 3.0, 0.5), mouse=(0.0, 0.0), time=0.0), 1),
    "face_007": (dict(pos=(1.07, 3.0, 0.5), mouse=(0.0, 0.0), time=0.0), 2),
    "face_003": (dict(pos=(1.03, 3.0, 0.5), mouse=(0.0, 0.0), time=0.0), 3),
    # the sponge rotated by 60 degrees (u_time 30): the cube's silhouette crosses the frame
    "silhouette_t30": (dict(pos=(2.0, 3.0, 3.5), mouse=(-0.45, 0.0), time=30.0), 0),
    # inside the cube inflated by 0.1 (max|q| = 1.1), outside those inflated by 0.05 and 0.02, looking along the
    # face: the half of the frame that looks away from it qualifies from the third rung on
    "inside_inflated": (dict(pos=(0.0, 3.0, 1.1), mouse=(math.pi / 2, 0.0), time=0.0), 2),
    # P0 turned half round: the sponge is behind the camera, every wave is the far-sky vote's from N0 steps on
    "behind": (dict(pos=POSES["P0"]["pos"], mouse=(math.pi, 0.0), time=0.0), 0),
    # 60 away, looking at the sponge: the central rays end short of the cube, the others qualify
    "from_60": (dict(pos=(0.0, 3.0, 60.0), mouse=(0.0, 0.0), time=0.0), 0),
    # 52 away: rays passing beside the sponge end, at depth ZFAR, within 4.1 of it: they miss every rung's cube
    # and fail the far-point condition, which alone keeps their reflection march
    "from_52": (dict(pos=(0.0, 3.0, 52.0), mouse=(0.0, 0.0), time=0.0), 0),
}


def frame_rays(pose, W, H):
    """the frame's primary rays in sponge space -> (o [H * W, 3], d [H * W, 3]) float32"""
    rd = camera_dirs(W, H, pose["mouse"])
    ro = np.broadcast_to(np.asarray(pose["pos"], F32), rd.shape)
    return fs.to_sponge(ro, rd, pose["time"])


def tile_all(lanes, W, H):
    """[H * W] bool per pixel -> [tiles] bool: every pixel of the 8 x 8 tile that lies in the frame (a wave's
    active lanes) holds"""
    gy, gx = (H + 7) // 8, (W + 7) // 8
    a = np.ones((gy * 8, gx * 8), bool)
    a[:H, :W] = lanes.reshape(H, W)
    return a.reshape(gy, 8, gx, 8).transpose(0, 2, 1, 3).reshape(gy * gx, 64).all(-1)


def wave_votes(pose, W, H, max_steps, slack=0.0):
    """-> (new [tiles] bool, old [tiles] bool): the timed kernels' vote at the radius max_steps admits, and the
    far-sky vote behind rm_stats.skipped (kFarSkyR, max_steps >= N0).  slack: both thresholds scaled by 1 + slack."""
    o, d = frame_rays(pose, W, H)
    k = F32(1.0 + slack)
    r = radius(max_steps)
    n_tiles = ((H + 7) // 8) * ((W + 7) // 8)
    new = tile_all(near_sky_ray(o, d, F32(r * k), F32(fs.K_FAR * k)), W, H) if r > 0 else np.zeros(n_tiles, bool)
    old = (tile_all(near_sky_ray(o, d, F32(fs.K_R * k), F32(fs.K_FAR * k)), W, H) if max_steps >= fs.K_N0
           else np.zeros(n_tiles, bool))
    return new, old


def near_tiles(pose, W, H, max_steps):
    """the waves whose marches go into the new count: they pass the new vote and not the old one -> (strict,
    loose) counts; the restatement decides only where both are 0 or both are not"""
    s_new, _ = wave_votes(pose, W, H, max_steps, 1.0e-4)
    _, l_old = wave_votes(pose, W, H, max_steps, -1.0e-4)
    l_new, _ = wave_votes(pose, W, H, max_steps, -1.0e-4)
    _, s_old = wave_votes(pose, W, H, max_steps, 1.0e-4)
    return int((s_new & ~l_old).sum()), int((l_new & ~s_old).sum())
