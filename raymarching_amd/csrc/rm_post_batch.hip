// rm_post_batch.hip -- the post passes over a batch of n equally sized RGBA8
// frames packed one after the other (include/rm.h rm_post_frag_batch,
// rm_bloom_batch, rm_post_chain_batch): the batch forms of the
// FXAA, texel, chromatic, mip, bloom, polynomial and strip kernels, and their
// launches, whose number does not grow with n.
//
// The kernels are the single-frame kernels' own text (rm_fxaa_kernels.h,
// rm_post_frag_kernels.h, rm_bloom_kernels.h), compiled here with RM_POST_BATCH
// (rm_post_view.h): each takes a trailing ViewStride and advances its pointers
// to the view the grid names -- blockIdx.z, or blockIdx.y where z names the
// level (polynomials) or x numbers the tiles (texel, chromatic) -- before it
// reads anything.  Everything inside a view is indexed as in a lone frame, so
// CLAMP_TO_EDGE, the FXAA halo, the vertical flip, the resampling and the
// strips' tails cannot leave the view.  The run tables depend on W x H only:
// one set for all views, built by the single-frame kernel (rm_post.hip
// launch_bloom_runs).
//
// Built with rm_post.o's flags (no FMA contraction, correctly rounded
// division): the float paths are the single-frame kernels' bit for bit.  (FXAA's
// unit has LLVM's max-ilp schedule besides, which orders instructions and
// changes no value.)
#define RM_POST_BATCH 1
#include "rm_bloom_kernels.h"
#include "rm_fxaa_kernels.h"
#include "rm_post_batch_plan.h"
#include "rm_post_frag_kernels.h"

namespace rm {

hipError_t launch_post_frag_batch(const uint32_t* in, uint32_t* out, int W, int H, int n, int sample, int tonemap,
                                  hipStream_t s) {
    if (W <= 0 || H <= 0 || n <= 0) return hipSuccess;
    if (sample < 0 || sample >= kSampleCount) return hipErrorInvalidValue;
    const ViewStride vs{(uint64_t)W * (uint64_t)H, 0, 0, 0};
    return with_tonemap(tonemap, [&](auto tm) {
        constexpr int TM = decltype(tm)::value;
        if (sample == kSampleFxaa) {  // (rm_fxaa.hip launch_fxaa_tm's two grids, the views along z)
            if (W <= FXL_MAX_DIM && H <= FXL_MAX_DIM) {
                const dim3 grid((W + FXL_TX - 1) / FXL_TX, (H + FXL_TY - 1) / FXL_TY, n);
                hipLaunchKernelGGL(rm_fxaa_lds_batch_kernel<TM>, grid, dim3(FXL_NT), 0, s, in, out, W, H, vs);
            } else {
                const dim3 grid((W + FXAA_TX - 1) / FXAA_TX, (H + FXAA_TY - 1) / FXAA_TY, n);
                hipLaunchKernelGGL(rm_fxaa_batch_kernel<TM>, grid, dim3(256), 0, s, in, out, W, H, vs);
            }
            return hipGetLastError();
        }
        // (rm_post_frag.hip launch_post_frag's grid: the tiles along x; the views along y)
        const bool chroma = sample == kSampleChromatic;
        const int tiles_x = (W + (chroma ? CA_TX : TS_TX) - 1) / (chroma ? CA_TX : TS_TX);
        const int tiles_y = (H + (chroma ? CA_TY : TS_TY) - 1) / (chroma ? CA_TY : TS_TY);
        const dim3 grid((unsigned)(tiles_x * tiles_y), n), block(256);
        if (chroma) hipLaunchKernelGGL(rm_post_chromatic_batch_kernel<TM>, grid, block, 0, s, in, out, W, H, tiles_x, vs);
        else hipLaunchKernelGGL(rm_post_texel_batch_kernel<TM>, grid, block, 0, s, in, out, W, H, tiles_x, vs);
        return hipGetLastError();
    });
}

// rm_post.hip launch_bloom's sequence with every grid extended by the views.
// Level k >= 1 of view v is at views + v * L.view_words + p.offset[k]; level 0
// is the view's frame.
hipError_t launch_bloom_batch(const uint32_t* in, uint32_t* out, int n, uint32_t* tables, uint32_t* views,
                              const BloomPlan& p, const PostBatchViewLayout& L, hipStream_t s) {
    const int W = p.w[0], H = p.h[0];
    if (W <= 0 || H <= 0 || n <= 0) return hipSuccess;
    const uint64_t frame = (uint64_t)W * (uint64_t)H, view = L.view_words;
    auto level = [&](int k) -> const uint32_t* { return k == 0 ? in : views + p.offset[k]; };
    auto stride = [&](int k) -> uint64_t { return k == 0 ? frame : view; };
    const BloomMips mp = bloom_mips(p);
    for (int k = 1; k <= mp.downs; k++) {
        const int w = p.w[k - 1], h = p.h[k - 1], w1 = p.w[k], h1 = p.h[k];
        hipLaunchKernelGGL(rm_mip_down_batch_kernel, dim3((w1 + 15) / 16, (h1 + 15) / 16, n), dim3(256), 0, s,
                           level(k - 1), views + p.offset[k], w, h, w1, h1, (float)w / (float)w1, (float)h / (float)h1,
                           ViewStride{stride(k - 1), view, 0, 0});
    }
    if (mp.pyramid) {
        const int s0 = mp.s0, nl = p.d2 - s0, lgb = nl - 5, T = 32 << lgb;
        const dim3 g(p.w[s0] / T, p.h[s0] / T, n);
        uint32_t *oa = views + p.offset[p.d1], *ob = views + p.offset[p.d2];  // (d1 > s0 >= 0: never the frame)
        const int ja = p.d1 - s0, jb = p.d2 - s0;
        const ViewStride vs{stride(s0), view, 0, 0};
        switch (lgb) {
            case 0: hipLaunchKernelGGL(rm_mip_pyramid_batch_kernel<0>, g, dim3(1024), 0, s, level(s0), p.w[s0], oa, ja, ob, jb, vs); break;
            case 1: hipLaunchKernelGGL(rm_mip_pyramid_batch_kernel<1>, g, dim3(1024), 0, s, level(s0), p.w[s0], oa, ja, ob, jb, vs); break;
            case 2: hipLaunchKernelGGL(rm_mip_pyramid_batch_kernel<2>, g, dim3(1024), 0, s, level(s0), p.w[s0], oa, ja, ob, jb, vs); break;
            default: hipLaunchKernelGGL(rm_mip_pyramid_batch_kernel<3>, g, dim3(1024), 0, s, level(s0), p.w[s0], oa, ja, ob, jb, vs); break;
        }
    }
    if (p.lod <= 0.0f) {
        hipLaunchKernelGGL(rm_bloom_batch_kernel, dim3((W + 15) / 16, (H + 15) / 16, n), dim3(256), 0, s, Level{in, W, H},
                           out, W, H, ViewStride{frame, 0, 0, 0});
        return hipGetLastError();
    }
    const BloomSetup b = bloom_setup(p, tables, level(p.d1), level(p.d2), views + L.tab[0], views + L.tab[1]);
    hipLaunchKernelGGL(rm_bloom_poly_batch_kernel, dim3(bloom_poly_blocks(b.T), n, 2), dim3(256), 0, s, b.ax, b.T,
                       ViewStride{stride(p.d1), stride(p.d2), view, 0});
    hipLaunchKernelGGL(rm_bloom_min_batch_kernel, dim3((W + 255) / 256, (H + kBloomRows - 1) / kBloomRows, n), dim3(256),
                       0, s, in, b.P, out, W, H, ViewStride{frame, view, 0, 0});
    return hipGetLastError();
}

}  // namespace rm
