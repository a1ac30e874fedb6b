// rm_post_frag.hip -- post.frag's main() (:135-144) with the sample its one
// statement takes generalised to the other two a user of the reference picks
// by editing it:
//   texel      color = texture(u_main_tex, uv)
//   chromatic  color = vec4(chromaticAberration(u_main_tex, uv), texture(u_main_tex, uv).a)
// followed by one of post.frag's tonemap operators (rm_post_tonemap.h) and the
// RGBA8 store.  (The FXAA sample is rm_fxaa.hip's kernel with the same
// epilogue.)  The sampler is rm_fxaa's: NEAREST, CLAMP_TO_EDGE, texel index
// clamp(floor(u W)) in float, uv = (tc.x, 1 - tc.y) with the exact pixel-centre
// tc, so the output is the input flipped vertically.
//
// Built with rm_post.o's flags: no FMA contraction, correctly rounded
// division, so the float path equals tests/post_frag_ref.py bit for bit.
//
// chromaticAberration (post.frag:113-131) is 8 steps of one tap per channel at
// 0.5 - 0.5 ((1 - 2 UV) k) for the channel's factor k: a scaling about the frame
// centre by k, with k running 1 .. 0.9806 (red), 1 .. 0.9861 (green) and
// 1 .. 1.0084 (blue).  A tap's column depends on the pixel's column only and
// its row on the pixel's row only, and nothing depends on a loaded value, so
// the taps are plain global loads, all in flight at once; along a wave's
// 64-pixel row a tap's texels are a shifted, almost contiguous row (the
// displacement changes by about one texel across it): about one cache line
// per tap and wave, served by the TCP / L2.  Staging the tile's tap bounding
// box in LDS instead measured 2.5 times slower.
//
// The kernels are rm_post_frag_kernels.h's text (which rm_post_batch.hip
// compiles into the batch forms as well); this file holds their single-frame
// launch.
#include "rm_post_frag_kernels.h"

namespace rm {

hipError_t launch_post_frag(const uint32_t* in, uint32_t* out, int W, int H, int sample, int tonemap, hipStream_t s) {
    if (W <= 0 || H <= 0) return hipSuccess;
    if (sample == kSampleFxaa) return launch_fxaa_tonemap(in, out, W, H, tonemap, s);
    if (sample != kSampleTexel && sample != kSampleChromatic) return hipErrorInvalidValue;
    const bool chroma = sample == kSampleChromatic;
    const int tiles_x = (W + (chroma ? CA_TX : TS_TX) - 1) / (chroma ? CA_TX : TS_TX);
    const int tiles_y = (H + (chroma ? CA_TY : TS_TY) - 1) / (chroma ? CA_TY : TS_TY);
    const dim3 grid((unsigned)(tiles_x * tiles_y)), block(256);
    static_assert(64 * CA_NW == 256 && TS_TX * TS_TY == 256, "block size");
    return with_tonemap(tonemap, [&](auto tm) {
        constexpr int TM = decltype(tm)::value;
        if (chroma) hipLaunchKernelGGL(rm_post_chromatic_kernel<TM>, grid, block, 0, s, in, out, W, H, tiles_x);
        else hipLaunchKernelGGL(rm_post_texel_kernel<TM>, grid, block, 0, s, in, out, W, H, tiles_x);
        return hipGetLastError();
    });
}

}  // namespace rm
