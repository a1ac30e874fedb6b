// rm_refl_clear.h -- scene T's reflection certificate: the
// per-ray condition under which render_T_from (rm_render_direct.h) knows that
// the reflection march of getColorReflect contributes the factor
// clamp(length(pr - p) / 3, 0, 1) = 1.0f exactly, without taking a step.  Plain
// C++ on the host, no HIP and no library call: tests/host/refl_clear_test.cpp
// includes this file alone and restates the march.
//
// The ray is the reflection march's own sponge-space ray o + d t (sponge_ray of
// ror = p + 0.01 rdir and rdir), marched by cast_ray_T from t = ZNEAR = 0.02
// (t is the march's depth).  The test, for some axis i, with a = |o_i|,
// u = d_i sign(o_i) (the slope away from the face on o_i's side), b0 = a - 1:
//     u >= kRatio   and   fma(u, ZNEAR, b0) >= kRatio ZNEAR,
// plus the sanity terms: a finite sum |o| <= 2^10, max|d_i| <= 1 + 2^-10 and
// dot(d, d) >= 1 - 2^-10.  It is rm_shadow_clear.h's bound with a much weaker
// claim: no penumbra condition, only "no hit" and "depth 3 within the step cap".
//
// 0. The bound.  box(t) = max_i |o_i + d_i t| - 1 (sponge_box) is >=
//    sign(o_i)(o_i + d_i t) - 1 = g(t) = b0 + u t, and g(t) / t = b0 / t + u.
//    With b0 >= 0 that is >= u >= kRatio; with b0 < 0 it grows with t, so for
//    t >= ZNEAR it is >= b0 / ZNEAR + u >= kRatio by the second condition.  The
//    march's distance is sponge_folds' result, which is >= its box term in the
//    exact and in the fast form, so at every depth t >= ZNEAR
//        dist >= box(t) >= g(t) >= kRatio t >= kRatio ZNEAR = 0.004.
//    In floats: a and u are exact; b0 = a - 1 is exact for a in [1/2, 2] (below
//    1/2 the second condition fails, b0 + u ZNEAR <= -0.5 + 0.0201; above 2
//    b0 >= 1 - 2^-22 and the bound holds by far).  The test's one FMA rounds
//    within 2^-24 of 0.041 at most near the threshold.  at()'s one FMA per axis
//    rounds q_i within 2^-24 |q_i|, and the box term's subtraction is exact for
//    max|q| in [1/2, 2] and within 2^-24 max|q| above: with |q_i| = 1 + g(t),
//        box >= g(t) (1 - 2^-22) - 2^-22,
//    and 2^-22 = 2.4e-7 is 6e-5 of 0.004.  The margins below are 10 % and more.
// (a) No hit.  dist >= 0.004 - 2.4e-7 at every step, four times cast_ray_T's hit
//    threshold of 0.001: `dist < 0.001` never holds.  The shading point p may
//    lie up to 0.001 inside or outside the face (the primary march stops at
//    dist < 0.001): b0 is then as low as -0.001 + 0.01 u, and the second
//    condition, which reads b0 itself, decides.
// (b) Depth 3 within kSteps steps.  depth' = RN(depth + dist) with dist >=
//    kRatio depth (1 - 2^-21): depth never decreases and grows by a factor
//    >= (1 + kRatio)(1 - 2^-20) per step.  From 0.02 it is >= 3 after
//        N = ceil(log(150) / log(1 + kRatio)) = ceil(27.48) = 28 steps:
//    0.02 * 1.2^28 = 3.297, 10 % above 3, against 28 * 2^-20 of roundings; and
//    0.02 * 1.2^27 = 2.747 < 3: a ray leaving a face at u = kRatio exactly, over
//    solid wall, needs all 28 (tests/host/refl_clear_test.cpp shows one).  So the
//    claim needs max_steps >= kSteps; the kernels test F.max_steps themselves and
//    march as before under a smaller cap.  The reference march (RS = 0) then goes
//    on to depth >= ZFAR or to its step cap without a hit, by (a); the timed one
//    (RS = 1) leaves at depth >= 3.  Either way the returned depth is in [3, 50].
// (c) The factor.  pr = ror + rdir depth and ror = p + 0.01 rdir, so pd = pr - p
//    is rdir (0.01 + depth) within 2^-22 (|p| + 50) per component, and
//    |pd| >= |rdir| 3.01 - 4e-5.  rdir's sponge-space image d is rdir rotated
//    (sponge_rot, |d| = |rdir| within 2^-21), so dot(d, d) >= 1 - 2^-10 gives
//    |rdir| >= 1 - 2^-10: |pd| >= 3.007.  v_sqrt_f32 (1 ulp) and the multiply by
//    RN(1/3) give >= 1.002, and the clamp returns the bits of 1.0f, as the stop
//    at depth 3 already relies on.  |pd| <= 52 (1 + 2^-9): no
//    overflow, no NaN.
//
// kRatio = 0.2: the bound 0.004 stands four times above the hit threshold, N is
// 28, and on the benchmark pose no smaller ratio clears more lanes (DESIGN.md
// 2.25).  A NaN fails every comparison, the sum rejects infinities and origins
// beyond 2^10, and an origin inside the cube by more than (u - kRatio) ZNEAR <=
// 0.016 fails the second condition on every axis: inner walls always march.
#pragma once

#if defined(__HIPCC__) || defined(__HIPCC_RTC__) || defined(__HIP__)
#define RM_RC_HD __host__ __device__
#else
#define RM_RC_HD
#endif

namespace rmrc {

#ifndef RM_REFL_CLEAR_RATIO  // (tests/host/refl_clear_test.cpp builds once with 0.02 and must fail)
#define RM_REFL_CLEAR_RATIO 0.2f
#endif
constexpr float kRatio = RM_REFL_CLEAR_RATIO;
constexpr float kNear = 0.02f;               // ZNEAR: cast_ray_T's first depth (rm_device.h static_asserts the two equal)
constexpr float kMaxDir = 1.0f + 0x1p-10f;   // max|d_i|: a rotated unit vector
constexpr float kMinLen2 = 1.0f - 0x1p-10f;  // dot(d, d): (c)'s |pr - p| >= 3.007
// (b)'s N = ceil(log(150) / log(1 + kRatio)): the certificate holds for max_steps >= kSteps only
constexpr int refl_steps(double ratio) {
    int n = 0;
    for (double depth = 0.02; depth < 3.0 && n < (1 << 20); n++) depth *= 1.0 + ratio;
    return n;
}
constexpr int kSteps = refl_steps((double)kRatio);
static_assert(RM_REFL_CLEAR_RATIO != 0.2f || kSteps == 28, "the header's proof states N = 28 for kRatio = 0.2");

// one axis: the outward slope and the bound's value at ZNEAR
RM_RC_HD inline bool axis_clear(float o, float d) {
    const float u = o < 0.0f ? -d : d;  // d_i sign(o_i) (o = 0: a = 0 fails below)
    const float b0 = __builtin_fabsf(o) - 1.0f;
    return (u >= kRatio) & (__builtin_fmaf(u, kNear, b0) >= kRatio * kNear);
}

// true only if cast_ray_T(o + d t) meets nothing and returns a depth >= 3 under every step cap >= kSteps
RM_RC_HD inline bool refl_clear(float ox, float oy, float oz, float dx, float dy, float dz) {
    const float ax = __builtin_fabsf(ox), ay = __builtin_fabsf(oy), az = __builtin_fabsf(oz);
    const float bx = __builtin_fabsf(dx), by = __builtin_fabsf(dy), bz = __builtin_fabsf(dz);
    // finite, |o_i| <= 2^10, max|d_i| <= 1 + 2^-10, |d|^2 >= 1 - 2^-10 (a NaN or an infinity fails the comparisons)
    const float len2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    const bool ok = (ax + ay + az <= 1024.0f) & (bx <= kMaxDir) & (by <= kMaxDir) & (bz <= kMaxDir) & (len2 >= kMinLen2);
    const bool cx = axis_clear(ox, dx), cy = axis_clear(oy, dy), cz = axis_clear(oz, dz);
    return ok & (cx | cy | cz);  // (every axis evaluated: no per-lane branch)
}

}  // namespace rmrc
