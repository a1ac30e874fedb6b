// rm_post.hip -- the bloom post pass of the reference (shaders/post/bloom.frag
// with the mip chain of main.cpp:212-214) over an RGBA8 frame (SURVEY.md
// 8(f), rank 3).  The FXAA pass is rm_fxaa.hip; the helpers both use are in
// rm_post_common.h.
//
// Built without FMA contraction and with correctly rounded division (like
// rm_kernels_o.hip) so the float path is bit-identical to the restatement in
// oracle/rm_oracle.c.
//
// The kernels are rm_bloom_kernels.h's text (which rm_post_batch.hip compiles
// into the batch forms as well); this file holds their single-frame launches.
#include "rm_bloom_kernels.h"

namespace rm {

hipError_t launch_bloom(const uint32_t* in, uint32_t* out, uint32_t* mips, const BloomPlan& p, hipStream_t s,
                        bool runs_cached) {
    const int W = p.w[0], H = p.h[0];
    if (W <= 0 || H <= 0) return hipSuccess;
    const uint32_t* lv[40] = {in};
    // levels 1..d2 (rm_bloom_plan.h bloom_mips: one pyramid launch over level
    // s0 where every level is an exact halving, one launch per level otherwise)
    const BloomMips mp = bloom_mips(p);
    const int s0 = mp.s0;
    const bool pyramid = mp.pyramid;
    for (int k = 1; k <= mp.downs; k++) {
        uint32_t* dst = mips + p.offset[k];
        const int w = p.w[k - 1], h = p.h[k - 1], w1 = p.w[k], h1 = p.h[k];
        hipLaunchKernelGGL(rm_mip_down_kernel, dim3((w1 + 15) / 16, (h1 + 15) / 16), dim3(256), 0, s, lv[k - 1], dst,
                           w, h, w1, h1, (float)w / (float)w1, (float)h / (float)h1);
        lv[k] = dst;
    }
    if (pyramid) {
        const int nl = p.d2 - s0, lgb = nl - 5, T = 32 << lgb;
        for (int k = s0 + 1; k <= p.d2; k++) lv[k] = mips + p.offset[k];  // (only d1, d2 written)
        const dim3 g(p.w[s0] / T, p.h[s0] / T);
        uint32_t *oa = mips + p.offset[p.d1], *ob = mips + p.offset[p.d2];
        const int ja = p.d1 - s0, jb = p.d2 - s0;
        switch (lgb) {
            case 0: hipLaunchKernelGGL(rm_mip_pyramid_kernel<0>, g, dim3(1024), 0, s, lv[s0], p.w[s0], oa, ja, ob, jb); break;
            case 1: hipLaunchKernelGGL(rm_mip_pyramid_kernel<1>, g, dim3(1024), 0, s, lv[s0], p.w[s0], oa, ja, ob, jb); break;
            case 2: hipLaunchKernelGGL(rm_mip_pyramid_kernel<2>, g, dim3(1024), 0, s, lv[s0], p.w[s0], oa, ja, ob, jb); break;
            default: hipLaunchKernelGGL(rm_mip_pyramid_kernel<3>, g, dim3(1024), 0, s, lv[s0], p.w[s0], oa, ja, ob, jb); break;
        }
    }
    const Level L0{in, W, H};
    if (p.lod <= 0.0f) {
        hipLaunchKernelGGL(rm_bloom_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, s, L0, out, W, H);
        return hipGetLastError();
    }
    const BloomSetup b = bloom_setup(p, mips, lv[p.d1], lv[p.d2], mips + p.poly_tab[0], mips + p.poly_tab[1]);
    if (!runs_cached) hipLaunchKernelGGL(rm_bloom_runs_kernel, dim3(6), dim3(1024), 0, s, b.ax, b.R);
    hipLaunchKernelGGL(rm_bloom_poly_kernel, dim3(bloom_poly_blocks(b.T), 1, 2), dim3(256), 0, s, b.ax, b.T);
    hipLaunchKernelGGL(rm_bloom_min_kernel, dim3((W + 255) / 256, (H + kBloomRows - 1) / kBloomRows), dim3(256), 0, s,
                       in, b.P, out, W, H);
    return hipGetLastError();
}

hipError_t launch_bloom_runs(uint32_t* mips, const BloomPlan& p, hipStream_t s) {
    const BloomSetup b = bloom_setup(p, mips, nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(rm_bloom_runs_kernel, dim3(6), dim3(1024), 0, s, b.ax, b.R);
    return hipGetLastError();
}

}  // namespace rm
