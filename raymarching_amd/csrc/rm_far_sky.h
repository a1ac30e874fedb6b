// rm_far_sky.h -- scene T's far-sky shortcut: the two per-ray
// conditions under which render_T_from (rm_render_direct.h) knows the result of
// the primary march and of the reflection march without taking a step.  Shared
// by the device and by the host (rm_render_host.cpp sets FrameConst.far_sky from
// kFarSkyN0).  Plain C++ on the host, no HIP and no library call:
// tests/host/far_sky_test.cpp includes this file alone.
//
// 1. The primary march.  Scene T's distance is max(box, folds) with box =
//    max|q| - 1 (sponge_box) and the folds only raising it (sponge_folds: "the
//    result is >= d"), in the exact and in the fast form alike: dist >= box at
//    every point.  Let the sponge-space ray o + d t miss the cube max|q| <=
//    1 + m for every t in [0, 2^20].  A marched point is fmaf(d, t, o) per axis,
//    one rounding each, so on the axis where the exact point leaves the cube the
//    rounded one is >= RN(1 + m) in magnitude (rounding is monotonic; the slack
//    below pays for it): every step has dist >= box >= m = 0.25 > 0.001.  No step
//    hits, and depth, which starts at ZNEAR and stays below ZFAR = 50 while the
//    march runs (half an ulp there is 2^-19), grows by >= m - 2^-19 per step:
//    after N0 = 208 steps it is >= 0.02 + 208 (0.25 - 2^-19) > 51.9 >= ZFAR.
//    With max_steps >= N0 the march leaves through depth >= ZFAR and cast_ray_T
//    returns ZFAR itself (`depth >= ZFAR ? ZFAR : depth`), whatever the steps
//    were.  (The bound uses no property of |d|.)
// 2. The reflection march.  Its colour term is c = clamp01(|pr - p| / 3) with
//    pr = ror + rdir depth, ror = p + rdir 0.01, and its first point lies at
//    depth ZNEAR: 0.03 |rdir| from p, |rdir| = |rd| within 1e-4 (shade_ray_ok,
//    camera_ray; the normal is v_rsq-normalized).  If max|at(prim, ZFAR)| >=
//    4.1 then at that first point max|q| >= 4.1 - 0.031 - roundings (a few
//    2^-24 |q|, |q| <= 1100) > 4.06, so the first distance is >= box > 3.06:
//    no hit, depth >= 3.08 >= 3, the timed march (RS = 1) leaves there and the
//    reference's depth never decreases, |pr - p| >= 0.9999 * 3.09 > 3 and the
//    clamp gives exactly 1 (max_steps >= N0 >= 1: the step is taken).
//
// The miss test is the separating-axis test of a half-line against a cube, in
// cross-multiplied form (no division, no transcendental): the ray misses iff
//    on some axis i: |o_i| > r and o_i d_i >= 0 (outside a face, not approaching), or
//    on some axis k = i x j: |o_i d_j - o_j d_i| > r (|d_i| + |d_j|)
//                                   (its projection along k misses the square).
// These are the face normals of the Minkowski sum of the cube and the ray, so
// the test is exact in real arithmetic; in floats it is conservative for
// r = 1 + m + 2^-10: with |o_i| <= 2^10 the cross term A - B is computed as
// fmaf(o_i, d_j, -RN(o_j d_i)) within 2^-24 (|B| + |A - B|) + 2^-115 (the last
// term: underflow, flushed or not), its bound within 2^-23 relative, so an
// accepted test has |A - B| > (r - 2^-13) (|d_i| + |d_j|) + 2^-101 in real
// numbers, and a face test whose product underflowed to +-0 against its true
// sign has |d_i| < 2^-126: the point moves < 2^-106 on that axis while t <=
// 2^20.  Either way the real ray misses the cube of half-size r - 2^-13 >
// 1 + m + 2^-11 for t in [0, 2^20].  Every comparison is false for a NaN, and
// the two sums reject infinities and origins beyond 2^10; an origin inside the
// cube fails every test.
#pragma once

#if defined(__HIPCC__) || defined(__HIPCC_RTC__) || defined(__HIP__)
#define RM_FS_HD __host__ __device__
#else
#define RM_FS_HD
#endif

namespace rmfs {

constexpr float kFarSkyM = 0.25f;                         // m: every step of an accepted ray is >= m
constexpr float kFarSkyR = 1.0f + kFarSkyM + 0x1p-10f;    // the tested cube's half-size (exact in f32)
constexpr int kFarSkyN0 = 208;                            // max_steps >= N0: the escaping march returns ZFAR
constexpr float kFarSkyFar = 4.1f;                        // max|q| at depth ZFAR: 3 (clamp) + 1 (box) + 0.031 + slack
constexpr float kFarSkyDepth = 50.0f;                     // ZFAR (rm_device.h static_asserts the two equal)

// true only if o + d t, t in [0, 2^20], stays outside the cube max|q| <= r - 2^-13
RM_FS_HD inline bool ray_misses_cube(float ox, float oy, float oz, float dx, float dy, float dz, float r) {
    const float ax = __builtin_fabsf(ox), ay = __builtin_fabsf(oy), az = __builtin_fabsf(oz);
    const float bx = __builtin_fabsf(dx), by = __builtin_fabsf(dy), bz = __builtin_fabsf(dz);
    const float sxy = bx + by, syz = by + bz, szx = bz + bx;
    // finite, |o_i| <= 2^10, |d_i| <= 4 (a NaN or an infinity fails the comparisons)
    const bool ok = (ax + ay + az <= 1024.0f) & (sxy + bz <= 4.0f);
    const float tiny = 0x1p-100f;
    const bool cz = __builtin_fabsf(__builtin_fmaf(ox, dy, -(oy * dx))) > __builtin_fmaf(r, sxy, tiny);
    const bool cx = __builtin_fabsf(__builtin_fmaf(oy, dz, -(oz * dy))) > __builtin_fmaf(r, syz, tiny);
    const bool cy = __builtin_fabsf(__builtin_fmaf(oz, dx, -(ox * dz))) > __builtin_fmaf(r, szx, tiny);
    const bool fx = (ax > r) & (ox * dx >= 0.0f);
    const bool fy = (ay > r) & (oy * dy >= 0.0f);
    const bool fz = (az > r) & (oz * dz >= 0.0f);
    return ok & (cx | cy | cz | fx | fy | fz);
}

// condition 2 above at the primary ray's far point, fmaf(d, ZFAR, o) per axis (rm_device.h at())
RM_FS_HD inline bool far_point_clear(float ox, float oy, float oz, float dx, float dy, float dz) {
    const float qx = __builtin_fmaf(dx, kFarSkyDepth, ox), qy = __builtin_fmaf(dy, kFarSkyDepth, oy);
    const float qz = __builtin_fmaf(dz, kFarSkyDepth, oz);
    return __builtin_fmaxf(__builtin_fabsf(qx), __builtin_fmaxf(__builtin_fabsf(qy), __builtin_fabsf(qz))) >= kFarSkyFar;
}

// both: the lane's primary march returns ZFAR and its reflection factor is 1
RM_FS_HD inline bool far_sky_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
    const bool miss = ray_misses_cube(ox, oy, oz, dx, dy, dz, kFarSkyR);
    const bool clear = far_point_clear(ox, oy, oz, dx, dy, dz);
    return miss & clear;  // (both evaluated: no per-lane branch)
}

}  // namespace rmfs
