"""Scene T's far-sky predicate (raymarching_amd/csrc/rm_far_sky.h, DESIGN.md
2.22) restated in float32 numpy on rows of sponge-space origins and directions,
for tests/shade_t_rays.py: which rays pass rmfs::far_sky_ray, so that the waves
of tests/test_shade_rays_shortcuts.py can be composed, and asserted, to vote far
or not.  It states a ray's class and decides no expected colour.

fmaf(a, b, c) is formed as float32(float64(a) * float64(b) + float64(c)): the
product of two float32 factors is exact in float64, the sum is rounded to
float64 and then once more to float32, which differs from the fused operation
only where the first rounding lands on a float32 tie.
tests/test_far_sky_host.py holds this file to the header itself (tests/host/
far_sky_test.cpp --eval) on every ray of the sets and on 100 000 random rays,
with zero disagreements.

The world-to-sponge map of an origin (rm_device.h sponge_space<false>,
sponge_rot) is tests/shadow_clear_ref.py's, imported.  CPU only.
"""
import numpy as np

from tests.shadow_clear_ref import sponge_rot, sponge_rotation

F32 = np.float32
F64 = np.float64
K_M = F32(0.25)                                # rmfs::kFarSkyM
K_R = F32(F32(1.0) + K_M + F32(2.0 ** -10))    # rmfs::kFarSkyR, 1.2509765625
K_N0 = 208                                     # rmfs::kFarSkyN0
K_FAR = F32(4.1)                               # rmfs::kFarSkyFar
K_DEPTH = F32(50.0)                            # rmfs::kFarSkyDepth (ZFAR)
TINY = F32(2.0 ** -100)
CENTRE = np.array([0.0, 3.0, 0.0], F32)        # the sponge's centre in the world


def fmaf(a, b, c):
    """a * b + c with the product exact and the sum rounded to float64, then to float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def _mul(a, b):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32)


def ray_misses_cube(o, d, r=K_R):
    """rmfs::ray_misses_cube on rows of o, d [n, 3] -> [n] bool"""
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    r = F32(r)
    ox, oy, oz = o.T
    dx, dy, dz = d.T
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        ax, ay, az = np.abs(ox), np.abs(oy), np.abs(oz)
        bx, by, bz = np.abs(dx), np.abs(dy), np.abs(dz)
        sxy, syz, szx = (bx + by).astype(F32), (by + bz).astype(F32), (bz + bx).astype(F32)
        ok = (((ax + ay).astype(F32) + az).astype(F32) <= F32(1024.0)) & ((sxy + bz).astype(F32) <= F32(4.0))
        cz = np.abs(fmaf(ox, dy, -_mul(oy, dx))) > fmaf(r, sxy, TINY)
        cx = np.abs(fmaf(oy, dz, -_mul(oz, dy))) > fmaf(r, syz, TINY)
        cy = np.abs(fmaf(oz, dx, -_mul(ox, dz))) > fmaf(r, szx, TINY)
        fx = (ax > r) & (_mul(ox, dx) >= F32(0.0))
        fy = (ay > r) & (_mul(oy, dy) >= F32(0.0))
        fz = (az > r) & (_mul(oz, dz) >= F32(0.0))
    return ok & (cx | cy | cz | fx | fy | fz)


def far_point(o, d):
    """max|q| of the primary ray's far point fmaf(d, ZFAR, o) -> [n] float32 (NaN where a coordinate is)"""
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    q = np.abs(fmaf(d, K_DEPTH, o))
    # __builtin_fmaxf returns the other argument for a NaN; the comparison with kFarSkyFar decides the same
    # way for np.fmax, which has that rule
    return np.fmax(q[:, 0], np.fmax(q[:, 1], q[:, 2]))


def far_point_clear(o, d, far=K_FAR):
    """rmfs::far_point_clear -> [n] bool"""
    with np.errstate(invalid="ignore"):
        return far_point(o, d) >= F32(far)


def far_sky_ray(o, d):
    """rmfs::far_sky_ray -> [n] bool"""
    return ray_misses_cube(o, d, K_R) & far_point_clear(o, d)


def to_sponge(pos, dirs, time):
    """world origins and directions [n, 3] -> (o, d) in sponge space at u_time `time`: sponge_space<false> of the
    origin, sponge_rot of the direction, in tests/shadow_clear_ref.py's float32 form"""
    R = sponge_rotation(time)
    pos, dirs = np.asarray(pos, F32).reshape(-1, 3), np.asarray(dirs, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return sponge_rot(R, (pos - CENTRE).astype(F32)), sponge_rot(R, dirs)
