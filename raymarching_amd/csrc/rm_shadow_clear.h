// rm_shadow_clear.h -- scene T's soft-shadow certificate: the
// per-ray condition under which render_T_from (rm_render_direct.h) knows that
// soft_shadow2_T_loop returns exactly 1.0f without taking a step.  Plain C++
// on the host, no HIP and no library call: tests/host/shadow_clear_test.cpp
// includes this file alone and restates the loop.
//
// The ray is the shadow march's own sponge-space ray o + d t (sponge_ray of the
// shading point and the light direction), marched from t = mint.  The test, for
// some axis i, with a = |o_i|, u = d_i sign(o_i) (the slope away from the face
// on o_i's side) and b0 = a - 1:
//     u >= kRatio   and   b0 + u mint >= kRatio mint,
// plus the sanity terms (finite input, |o_i| <= 2^10, max|d_i| <= 1 + 2^-10,
// 0.01 <= mint <= 1; the kernels march from mint = 0.01).
//
// 0. The bound.  box(t) = max_i |o_i + d_i t| - 1 (sponge_box) is >=
//    sign(o_i)(o_i + d_i t) - 1 = g(t) = b0 + u t, and g(t) / t = b0 / t + u.
//    With b0 >= 0 that is >= u >= kRatio; with b0 < 0 it grows with t, so for
//    t >= mint it is >= b0 / mint + u >= kRatio by the second condition.  The
//    march's t starts at mint and only grows: at every step
//        h >= box >= g(t) >= kRatio t >= kRatio mint = 0.0035
//    (sponge_folds returns >= its box term, in the exact and the fast form).
//    In floats: a is exact, u is exact, b0 = a - 1 is exact for a in [1/2, 2]
//    (outside it the second condition fails, a < 1/2, or holds by far, a > 2);
//    the test's one FMA and at()'s one FMA per axis round within 2^-24
//    relative, and the box term's subtraction is exact below |q| = 2 and within
//    2^-24 above it: box >= g(t) - 2^-22, which is 2^-13 of 0.0035.  The
//    margins below are 5 % and more.
// 1. No occlusion.  h >= 0.0035 - 2^-22 > 0.001 at every step: `h < 0.001`
//    never holds, the march never returns 0.
// 2. The Lipschitz bound.  Every term of the distance is piecewise linear with
//    slope +-1 in one coordinate: the box term is |q_i| - 1, and fold m is
//    (|1 - 6 |x SH[m] - 1/2 - k|| - 1) / S3[m] in one coordinate x, slope
//    6 SH[m] / S3[m] = 1 (SH = 1/2, 3/2, 9/2; S3 = 3, 9, 27); max and med3
//    pick one of their arguments.  So |h(q) - h(q')| <= max_i |q_i - q'_i|, and
//    along the ray, whose step is 0.1 ph + 0.001 after a distance ph,
//        h' <= ph + max|d_i| (0.1 ph + 0.001),
//        rho = h' / (2 ph) <= 0.5 + (1 + 2^-10)(0.05 + 0.0005 / 0.0035) < 0.694.
//    (The folds act only where box < 1/3, |q| < 4/3: their roundings are ~1e-6,
//    against 0.006 * 2 ph >= 4e-5 of room below rho = 0.70.)
// 3. No candidate lowers res.  res^2 / 16 is kept as num / den = (1/16) / 1.
//    The first step's candidate (Q = 1, D = t) replaces it iff h^2 < t^2 / 16,
//    h < t / 4: not with h >= 0.35 t.  A later step has P = 2 ph, Q = P^2 -
//    h^2, D = t P - h^2 and updates iff Q >= 0, D > 0 and 16 h^2 Q < D^2, which
//    with rho = h / P is h (4 sqrt(1 - rho^2) + rho) < t.  The bracket is
//    concave in rho: on (0, 0.70] it is >= min(4, 3.556) > 3.55, and h >=
//    0.35 t, so the left side is >= 1.24 t.  It stays >= 1.05 t up to rho =
//    0.80 and for h down to 0.296 t: far above every rounding.  (rho >= 1 has
//    Q < 0: no update either.)  num and den keep their initial values.
// 4. The return value.  The loop ends by t >= maxt, by the settle exit, by a
//    step cap, or does not run (mint >= maxt, or a NaN maxt); in every case
//    num = 1/16, den = 1 and the last h is >= 0.001 (1.0f if no step ran), so
//    the result is v_sqrt(16 * (1/16) * v_rcp(1)) = 1.0f: v_rcp_f32(1) and
//    v_sqrt_f32(1) are exact, as render_T_from's shadow_pow branch already
//    relies on.
//
// kRatio = 0.35.  In a brute-force run of a million rays leaving a face, a
// candidate lowered res only below 0.26; the proof above carries to 0.30.
// A NaN fails every comparison, the sum rejects infinities and origins beyond
// 2^10, and an origin inside the cube by more than (u - kRatio) mint <= 0.0066
// fails the second condition on every axis.
#pragma once

#if defined(__HIPCC__) || defined(__HIPCC_RTC__) || defined(__HIP__)
#define RM_SC_HD __host__ __device__
#else
#define RM_SC_HD
#endif

namespace rmsc {

#ifndef RM_SHADOW_CLEAR_RATIO  // (tests/host/shadow_clear_test.cpp builds once with 0.2 and must fail)
#define RM_SHADOW_CLEAR_RATIO 0.35f
#endif
constexpr float kRatio = RM_SHADOW_CLEAR_RATIO;
constexpr float kMaxDir = 1.0f + 0x1p-10f;  // max|d_i|: a rotated unit vector

// one axis: the outward slope and the bound's value at mint
RM_SC_HD inline bool axis_clear(float o, float d, float mint) {
    const float u = o < 0.0f ? -d : d;  // d_i sign(o_i) (o = 0: a = 0 fails below)
    const float b0 = __builtin_fabsf(o) - 1.0f;
    return (u >= kRatio) & (__builtin_fmaf(u, mint, b0) >= kRatio * mint);
}

// true only if soft_shadow2_T_loop(o + d t, mint, maxt) returns exactly 1.0f, for any maxt and step cap
RM_SC_HD inline bool shadow_clear(float ox, float oy, float oz, float dx, float dy, float dz, float mint) {
    const float ax = __builtin_fabsf(ox), ay = __builtin_fabsf(oy), az = __builtin_fabsf(oz);
    const float bx = __builtin_fabsf(dx), by = __builtin_fabsf(dy), bz = __builtin_fabsf(dz);
    // finite, |o_i| <= 2^10, max|d_i| <= 1 + 2^-10 (a NaN or an infinity fails the comparisons)
    // and mint in [0.01, 1]: the proof's ph >= kRatio mint >= 0.0035 (the kernels pass the constant 0.01f)
    const bool ok = (ax + ay + az <= 1024.0f) & (bx <= kMaxDir) & (by <= kMaxDir) & (bz <= kMaxDir) & (mint >= 0.01f) &
                    (mint <= 1.0f);
    const bool cx = axis_clear(ox, dx, mint), cy = axis_clear(oy, dy, mint), cz = axis_clear(oz, dz, mint);
    return ok & (cx | cy | cz);  // (every axis evaluated: no per-lane branch)
}

}  // namespace rmsc
