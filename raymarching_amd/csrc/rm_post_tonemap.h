// rm_post_tonemap.h -- the tonemap operators of post.frag:63-109 as the
// epilogue of a post pass (rm_post_frag.hip, rm_fxaa.hip): tonemap<TM>(c) is
// `color.rgb = tonemap_X(color.rgb)`, operation for operation in float.  The
// including translation units are built without FMA contraction and with
// correctly rounded division, so every '*', '+', '/' below rounds once, as
// tests/post_frag_ref.py restates it.  Inputs are unorm8 texels or blends of
// them (in [0, 1]), so every denominator is positive and nothing is NaN.
#pragma once
#include <type_traits>

#include "rm_post_common.h"

namespace rm {

// post.frag:90-99.  C*B, D*E, D*F and E/F are float products / a float quotient
// of the float constants (folded here as the GLSL compiler folds them).
__host__ __device__ constexpr float u2_partial(float x) {
    constexpr float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    constexpr float CB = C * B, DE = D * E, DF = D * F, EF = E / F;
    return ((x * (A * x + CB) + DE) / (x * (A * x + B) + DF)) - EF;
}

template <int TM>
__device__ __forceinline__ float tonemap1(float x) {
    if constexpr (TM == kTonemapAces) {  // post.frag:67-75
        const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
        return (x * (a * x + b)) / (x * (c * x + d) + e);
    } else if constexpr (TM == kTonemapReinhard) {  // :77-80
        return x / (x + 1.0f);
    } else if constexpr (TM == kTonemapUncharted2) {  // :101-109: exposure_bias 2, white point 11.2
        constexpr float white_scale = 1.0f / u2_partial(11.2f);
        return u2_partial(x * 2.0f) * white_scale;
    } else {
        return x;
    }
}

template <int TM>
__device__ __forceinline__ RGB tonemap(RGB c) {
    static_assert(TM >= 0 && TM < kTonemapCount, "rm_tonemap value");
    if constexpr (TM == kTonemapJodie) {  // post.frag:82-88: mix(c / (l + 1), tc, tc), mix(x, y, a) = x + (y - x) a
        const float l = (c.r * 0.2126f + c.g * 0.7152f) + c.b * 0.0722f;
        const float l1 = l + 1.0f;
        auto ch = [&](float v) {
            const float tc = v / (v + 1.0f), x = v / l1;
            return x + (tc - x) * tc;
        };
        return RGB{ch(c.r), ch(c.g), ch(c.b)};
    } else {
        return RGB{tonemap1<TM>(c.r), tonemap1<TM>(c.g), tonemap1<TM>(c.b)};
    }
}

// gl_FragColor's RGBA8 store of a finite colour whose alpha is the byte of
// texel `t` ((b / 255) * 255 rounds back to b for all 256 bytes)
__device__ __forceinline__ uint32_t pack_rgb_alpha_of(RGB c, uint32_t t) {
    return unorm8_finite(c.r) | (unorm8_finite(c.g) << 8) | (unorm8_finite(c.b) << 16) | (t & 0xff000000u);
}

// tonemap value -> instantiation
template <typename F>
__host__ inline hipError_t with_tonemap(int tonemap, F&& f) {
    switch (tonemap) {
        case kTonemapNone: return f(std::integral_constant<int, kTonemapNone>{});
        case kTonemapAces: return f(std::integral_constant<int, kTonemapAces>{});
        case kTonemapReinhard: return f(std::integral_constant<int, kTonemapReinhard>{});
        case kTonemapJodie: return f(std::integral_constant<int, kTonemapJodie>{});
        case kTonemapUncharted2: return f(std::integral_constant<int, kTonemapUncharted2>{});
    }
    return hipErrorInvalidValue;
}

}  // namespace rm
