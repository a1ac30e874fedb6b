// rm_far_sky.h -- scene T's far-sky shortcut: the two per-ray
// conditions under which render_T_from (rm_render_direct.h) knows the result of
// the primary march and of the reflection march without taking a step.  Shared
// by the device and by the host (rm_render_host.cpp sets FrameConst.far_sky from
// kFarSkyN0 and FrameConst.near_r from the ladder of 3. below).
// Plain C++ on the host, no HIP and no library call: tests/host/far_sky_test.cpp
// and tests/host/near_sky_test.cpp include this file alone.
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
//
// 3. The near-sky ladder: the same two conditions with a smaller
//    m, for sky rays that pass close to the cube.  Only the step count of 1.
//    changes: "every step >= m" bounds it by 50 / m, far above any usable step
//    cap; the count N(m) below follows the ray instead.
//    What is given.  The ray passes ray_misses_cube with r = 1 + m + 2^-10, so in
//    real numbers g(t) = max_i |o_i + d_i t| - 1 >= m + 2^-11 on [0, 2^20].  Its
//    direction has D = |d|_2 in [kUnitLo, kUnitHi]: the callers' directions are
//    unit within 5.1e-5 (camera_ray normalizes; rm_shade.h shade_ray_ok) and go
//    through at most four plane rotations, each of which scales by sqrt(c^2 +
//    s^2) -- the host offers a rung only when every (c, s) pair of the launch
//    has |c^2 + s^2 - 1| <= 1e-4 (unit_rotation below; rm_render_host.cpp), and
//    otherwise keeps to m = 0.25 and N0, whose proof uses no property of |d|.
//    Let t* be where the real line is nearest the cube's centre and u = D (t -
//    t*): |q(t)|_2 >= |u|, so g(t) >= |u| / sqrt3 - 1.
//    The step.  Every marched point has |q_i| <= 1024 + 4 * 50 < 2048: its fmaf
//    and the box term's subtraction round by <= 2^-14 each, and depth, below 50
//    while the march runs, by <= 2^-19 per addition.  With dist >= box (1.), the
//    depth of an accepted ray grows per step by
//        >= max(m, |u| / sqrt3 - (1 + e)),  e = 2^-12   (2^-11 - 2^-13 - 2^-19 > 0),
//    so no step hits (m >= 0.02 > 0.001) and u grows by >= D times that.  With
//    c = kUnitLo / sqrt3, a = sqrt3 (1 + e + m) and v = |u| - sqrt3 (1 + e) the
//    steps taken at a depth < 50 fall into three runs, in this order:
//    A. u < -a.  There v > sqrt3 m and u grows by >= c v: v shrinks by the
//       factor (1 - c) per step, from v <= |q(ZNEAR)|_2 <= 1024.1.  At most nA
//       steps, nA the first k with 1025 (1 - c)^k <= sqrt3 m.
//    B. |u| <= a.  u grows by >= kUnitLo m per step over a span of 2 a: at most
//       nB = floor(2 a / (kUnitLo m)) + 1 steps.
//    C. u > a, depth < 50, so u - u(ZNEAR) < 49.98 D.  There v > sqrt3 m grows by
//       the factor (1 + c) per step.  Whether the march began before C (then v <
//       sqrt3 m + 49.98 D at every such step) or in it (then v - v0 < 49.98 D,
//       v0 > sqrt3 m), its j-th step in C has ((1 + c)^j - 1) sqrt3 m < 49.98 D:
//       at most nC steps, nC the first j with ((1 + c)^j - 1) sqrt3 m >= 50 kUnitHi.
//    N(m) = nA + nB + nC (near_sky_bound, computed from the rung's own radius).
//    After at most N(m) steps depth >= ZFAR, and with max_steps >= N(m) the
//    march returns ZFAR as in 1.  Run B is what the count pays for: the bound
//    g >= |u| / sqrt3 - 1 grants the cube its diagonal, 2 sqrt3 (1 + m), where a
//    ray in a face's plane along the face's diagonal, the slowest there is, really
//    has 2 sqrt2 (1 + m) at g = m.  The longest
//    march tests/host/near_sky_test.cpp meets is reported there beside N(m):
//    N(m) is proven, not tight.
//    Condition 2 is unchanged: it uses the far point alone, and max_steps >= 1.
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

// ---- the near-sky ladder (3. above)

constexpr double kUnitLo = 0.999, kUnitHi = 1.001;  // |d|_2 of a ray the ladder is offered to
constexpr float kUnitRotTol = 1.0e-4f;              // |c^2 + s^2 - 1| of a rotation the ladder is offered under

// N(m) of 3. for the tested half-size r = 1 + m + 2^-10 (m taken from r as it is in float, so the two agree)
constexpr int near_sky_bound(float r) {
    const double m = (double)r - 1.0 - 0x1p-10, e = 0x1p-12;
    const double s3lo = 1.7320508075, s3hi = 1.7320508076;  // sqrt3 from below and above
    const double c = kUnitLo / s3hi, vmin = s3lo * m;
    if (!(m >= 0.015625)) return 0x7fffffff;  // (the proof asks m > 0.001 and 2^-11; no rung this small fits 256 steps)
    int nA = 0;
    for (double v = 1025.0; v > vmin; v *= 1.0 - c) nA++;
    const int nB = (int)(2.0 * s3hi * (1.0 + e + m) / (kUnitLo * m)) + 1;
    int nC = 0;
    for (double g = 1.0; (g - 1.0) * vmin < 50.0 * kUnitHi; g *= 1.0 + c) nC++;
    return nA + nB + nC;
}

struct NearSkyRung {
    float m;  // every step of an accepted ray is >= m
    float r;  // the tested cube's half-size, 1 + m + 2^-10 in float
    int n;    // max_steps >= n: the escaping march returns ZFAR
};
constexpr NearSkyRung near_sky_rung(float m) {
    const float r = 1.0f + m + 0x1p-10f;
    return NearSkyRung{m, r, near_sky_bound(r)};
}
// widest first: every rung admits the rays of the rungs before it
constexpr int kNearSkyRungs = 4;
constexpr NearSkyRung kNearSkyLadder[kNearSkyRungs] = {near_sky_rung(0.25f), near_sky_rung(0.1f), near_sky_rung(0.05f),
                                                       near_sky_rung(0.02f)};
static_assert(kNearSkyLadder[0].r == kFarSkyR && kNearSkyLadder[0].n <= kFarSkyN0, "the first rung is the far-sky cube");
static_assert(kNearSkyLadder[0].n < kNearSkyLadder[1].n && kNearSkyLadder[1].n < kNearSkyLadder[2].n &&
                  kNearSkyLadder[2].n < kNearSkyLadder[3].n,
              "a smaller m needs more steps");
static_assert(kNearSkyLadder[2].n <= 128 && kNearSkyLadder[3].n <= kFarSkyN0, "m = 0.05 under 128 steps, m = 0.02 under N0");

// a plane rotation (c, s) that keeps a direction's length within 5.01e-5 (a NaN fails)
inline bool unit_rotation(float c, float s) {
    const float n = c * c + s * s - 1.0f;
    return n <= kUnitRotTol && n >= -kUnitRotTol;
}

// The smallest admissible tested half-size for a launch with this step cap, or 0: none (march every ray).
// unit_dirs: the launch's directions have |d|_2 in [kUnitLo, kUnitHi] (3. above); without it only the far-sky
// cube itself is offered, from N0 steps on.
inline float near_sky_radius(int max_steps, bool unit_dirs) {
    float r = 0.0f;
    if (unit_dirs) {
        for (int i = 0; i < kNearSkyRungs; i++)
            if (max_steps >= kNearSkyLadder[i].n) r = kNearSkyLadder[i].r;
    } else if (max_steps >= kFarSkyN0) {
        r = kFarSkyR;
    }
    return r;
}

// far_sky_ray with the launch's radius (FrameConst.near_r): the vote of the timed kernels
RM_FS_HD inline bool near_sky_ray(float ox, float oy, float oz, float dx, float dy, float dz, float r) {
    const bool miss = ray_misses_cube(ox, oy, oz, dx, dy, dz, r);
    const bool clear = far_point_clear(ox, oy, oz, dx, dy, dz);
    return miss & clear;  // (both evaluated: no per-lane branch)
}

}  // namespace rmfs
