// rm_fxaa.hip -- the FXAA post pass of the reference (post.frag:16-61, main
// :135-144) as a gfx950 stencil kernel over the RGBA8 frame the ray-march
// pass produced (it consumes the hot path's
// framebuffer directly).
//
// The reference samples u_main_tex with texture() on an sf::RenderTexture
// that was never setSmooth()ed or setRepeated(): GL_NEAREST, CLAMP_TO_EDGE;
// unorm8 texels become c * (1/255) floats and gl_FragColor is stored to an
// RGBA8 target with round-to-nearest.  post.frag flips the frame vertically
// (uv = (tc.x, 1 - tc.y)); that is part of the pass and is kept.
//
// Built without FMA contraction and with correctly rounded division (like
// rm_kernels_o.hip) so the float path is bit-identical to the restatement in
// oracle/rm_oracle.c; the nearest-texel choices then agree exactly too.
// Four pixels per lane, 64x16-pixel workgroups (neighbour texels are re-read
// from L1/L2; 4 B in + 4 B out of HBM per pixel).
//
// Blocks whose span is short output their centre texel without the span taps
// (proof at the test, tests/test_fxaa_claims.py::
// test_short_span_outputs_centre_texel): 0.069-0.072 -> 0.052-0.053 ms on the C3 frame, same
// bits (profiles/r05/fxaa_flat/); with 8x8-pixel blocks per wave pass instead
// of rows, 0.046-0.047 (profiles/r05/fxaa_blocks/); a halo of 4 (its rows are
// then 72 words, 8 banks apart: a block's 8 x 8 reads hit 64 distinct banks)
// 0.041 -> 0.039 (round 6, profiles/r06/fxaa_halo4_ab.log).
// Its own translation unit (split from rm_post.hip in round 5) so that it can
// be scheduled with LLVM's max-ilp strategy, which shortens the latency-bound
// FXAA kernel (0.0721-0.0729 -> 0.0697-0.0706 ms) but slows bloom's
// (profiles/r05/post_ilp_ab.log).
//
// The kernels are rm_fxaa_kernels.h's text (which rm_post_batch.hip compiles
// into the batch forms as well); this file holds their single-frame launches.
#include "rm_fxaa_kernels.h"

namespace rm {

template <int TM>
static hipError_t launch_fxaa_tm(const uint32_t* in, uint32_t* out, int W, int H, hipStream_t s) {
    if (W <= 0 || H <= 0) return hipSuccess;
    if (W <= FXL_MAX_DIM && H <= FXL_MAX_DIM) {
        dim3 grid((W + FXL_TX - 1) / FXL_TX, (H + FXL_TY - 1) / FXL_TY);
        hipLaunchKernelGGL(rm_fxaa_lds_kernel<TM>, grid, dim3(FXL_NT), 0, s, in, out, W, H);
        return hipGetLastError();
    }
    dim3 grid((W + FXAA_TX - 1) / FXAA_TX, (H + FXAA_TY - 1) / FXAA_TY);
    hipLaunchKernelGGL(rm_fxaa_kernel<TM>, grid, dim3(256), 0, s, in, out, W, H);
    return hipGetLastError();
}

hipError_t launch_fxaa(const uint32_t* in, uint32_t* out, int W, int H, hipStream_t s) {
    return launch_fxaa_tm<kTonemapNone>(in, out, W, H, s);
}

hipError_t launch_fxaa_tonemap(const uint32_t* in, uint32_t* out, int W, int H, int tonemap, hipStream_t s) {
    return with_tonemap(tonemap, [&](auto tm) { return launch_fxaa_tm<decltype(tm)::value>(in, out, W, H, s); });
}

}  // namespace rm
