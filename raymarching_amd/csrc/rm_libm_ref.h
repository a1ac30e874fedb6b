// rm_libm_ref.h -- sinf(x) and powf(x, y) as the GNU C library computes them
// (its single-precision routines since 2.28: double-precision polynomials after
// a table-driven reduction; the algorithms and constants are those of Arm's
// optimized-routines, published under MIT / Apache-2.0), restated with explicit
// fused multiply-adds so that the device returns the float the host's libm
// returns.
//
// Why a GPU library restates libm: the CPU restatement of the reference
// (oracle/rm_oracle.c) evaluates floorMat's sin(pi x) and pow(|p|, 1.3)
// (output_shader.frag:16-28) with the C library, and the colour of a floor
// point inside the tiles' blur band depends on their last bit.  A ray query
// returns a material to a caller who compares it, not a pixel, so rm_cast_rays
// forms scene O's floor material with these (rm_rays.h ray_mat); the render
// kernels keep floor_mat's hardware forms (rm_device.h).
// tests/test_libm_ref.py builds this file for the host and compares it with
// the C library's functions on a million arguments.
//
// Domain: sin_ref any float; pow_ref x > 0 finite and normal, y * log2(x)
// within float range (floorMat: x = |p| < 1e3, y = 1.3); x = 0 returns 0.
#pragma once
#if defined(__HIPCC_RTC__)
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
#define RM_LIBM_FN __device__ __forceinline__
#elif defined(__HIPCC__)
#include <stdint.h>
#define RM_LIBM_FN __host__ __device__ __forceinline__
#else
#include <stdint.h>
#define RM_LIBM_FN inline
#endif

namespace rm {
namespace libm {

RM_LIBM_FN uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }
RM_LIBM_FN double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the sine (n even) or cosine (n odd) polynomial on [-pi/4, pi/4]; neg: the negated cosine
RM_LIBM_FN float sin_poly(double x, double x2, bool neg, int n) {
    if ((n & 1) == 0) {
        const double x3 = x * x2;
        const double s1 = fma_(x2, -0x1.994eb3774cf24p-13, 0x1.1107605230bc4p-7);
        const double x7 = x3 * x2;
        const double s = fma_(x3, -0x1.555545995a603p-3, x);
        return (float)fma_(x7, s1, s);
    }
    const double g = neg ? -1.0 : 1.0;
    const double x4 = x2 * x2;
    const double c2 = fma_(x2, g * 0x1.99343027bf8c3p-16, g * -0x1.6c087e89a359dp-10);
    const double c1 = fma_(x2, g * -0x1.ffffffd0c621cp-2, g);
    const double x6 = x4 * x2;
    const double c = fma_(x4, g * 0x1.55553e1068f19p-5, c1);
    return (float)fma_(x6, c2, c);
}

RM_LIBM_FN float sin_ref(float y) {
    double x = y;
    const uint32_t xi = bits(y), top = (xi >> 20) & 0x7ffu;
    if (top < (0x3f490fdbu >> 20)) {  // |y| < pi/4
        if (top < (0x39800000u >> 20)) return y;  // |y| < 2^-12
        return sin_poly(x, x * x, false, 0);
    }
    if (top < (0x42f00000u >> 20)) {  // |y| < 120: n = round(x / (pi/2)), x -= n pi/2
        const double r = x * 0x1.45F306DC9C883p+23;
        const int n = ((int)r + 0x800000) >> 24;
        x = fma_(-(double)n, 0x1.921FB54442D18p0, x);
        const double s = ((n + 1) & 2) ? -1.0 : 1.0;  // {1, -1, -1, 1}[n & 3]
        return sin_poly(x * s, x * x, (n & 2) != 0, n);
    }
    if (top >= 0x7f8u) return y - y;  // inf, NaN
    // large arguments: 192 bits of 4/pi from the window the exponent selects
    // (word k of the table is bits [8k - 24, 8k + 8) of 4/pi)
    constexpr uint32_t inv_pio4[24] = {0xa2u,       0xa2f9u,     0xa2f983u,   0xa2f9836eu, 0xf9836e4eu, 0x836e4e44u,
                                       0x6e4e4415u, 0x4e441529u, 0x441529fcu, 0x1529fc27u, 0x29fc2757u, 0xfc2757d1u,
                                       0x2757d1f5u, 0x57d1f534u, 0xd1f534ddu, 0xf534ddc0u, 0x34ddc0dbu, 0xddc0db62u,
                                       0xc0db6295u, 0xdb629599u, 0x6295993cu, 0x95993c43u, 0x993c4390u, 0x3c439041u};
    const int sign = (int)(xi >> 31), i = (int)((xi >> 26) & 15u), shift = (int)((xi >> 23) & 7u);
    const uint32_t m = ((xi & 0xffffffu) | 0x800000u) << shift;
    uint64_t res0 = (uint32_t)(m * inv_pio4[i]);
    const uint64_t res1 = (uint64_t)m * inv_pio4[i + 4], res2 = (uint64_t)m * inv_pio4[i + 8];
    res0 = (res2 >> 32) | (res0 << 32);
    res0 += res1;
    const uint64_t nn = (res0 + (1ull << 61)) >> 62;
    res0 -= nn << 62;
    x = (double)(long long)res0 * 0x1.921FB54442D18p-62;
    const int n = (int)nn, q = n + sign;
    const double s = ((q + 1) & 2) ? -1.0 : 1.0;
    return sin_poly(x * s, x * x, (q & 2) != 0, n);
}

// x^y = 2^(y log2 x): log2 x = k + log2(c_i) + log2(z / c_i) with a 16-entry
// table {1 / c_i, log2 c_i} and a degree-5 polynomial; 2^t from a 32-entry table
// of 2^(j/32) and a cubic.  Everything is scaled by 32 as in the library.
RM_LIBM_FN float pow_ref(float xf, float yf) {
    if (xf == 0.0f) return 0.0f;
    constexpr double LT[16][2] = {
        {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
        {0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2},  {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
        {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3},
        {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
        {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
        {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3},
        {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
        {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2}};
    // bits of 2^(j/32), minus j << 47
    constexpr uint64_t ET[32] = {
        0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
        0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
        0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
        0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
        0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
        0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
        0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
        0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};
    const uint32_t ix = bits(xf), tmp = ix - 0x3f330000u, topb = tmp & 0xff800000u;
    const int i = (int)((tmp >> 19) & 15u), k = (int)topb >> 18;  // (k: the exponent times 32)
    const double z = (double)__builtin_bit_cast(float, ix - topb);
    const double r = fma_(z, LT[i][0], -1.0), y0 = LT[i][1] * 32.0 + (double)k;
    const double r2 = r * r, r4 = r2 * r2;
    double a = fma_(0x1.27616c9496e0bp-2 * 32.0, r, -0x1.71969a075c67ap-2 * 32.0);
    const double p = fma_(0x1.ec70a6ca7baddp-2 * 32.0, r, -0x1.7154748bef6c8p-1 * 32.0);
    double q = fma_(0x1.71547652ab82bp0 * 32.0, r, y0);
    q = fma_(p, r2, q);
    a = fma_(a, r4, q);  // 32 log2 x
    const double xd = (double)yf * a;
    double kd = xd + 0x1.8p+52;
    const uint64_t ki = __builtin_bit_cast(uint64_t, kd);
    kd -= 0x1.8p+52;
    const double rr = xd - kd;
    const double s = __builtin_bit_cast(double, ET[ki & 31u] + (ki << 47));
    const double zz = fma_(0x1.c6af84b912394p-5 / 32768.0, rr, 0x1.ebfce50fac4f3p-3 / 1024.0);
    double w = fma_(0x1.62e42ff0c52d6p-1 / 32.0, rr, 1.0);
    w = fma_(zz, rr * rr, w);
    return (float)(w * s);
}

}  // namespace libm
}  // namespace rm
