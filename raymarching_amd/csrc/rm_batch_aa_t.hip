// rm_batch_aa_t.hip -- adaptive supersampling of a view batch (rm_batch_aa.h):
// the refine kernels of scenes S0 and T, built with rm_kernels_t.o's flags so
// that a refined sample is the frame kernel's pixel bit for bit, and the
// scene-independent detect and plan kernels (integer code).  Not one of the
// render objects (raymarching_amd/Makefile RENDER_OBJS): rm_render_code_hash()
// names the frame kernels only.
#define RM_AA_KERNELS
#define RM_BATCH_AA_KERNELS
#include <cstdlib>
#include <cstring>

#include "rm_batch_aa.h"

namespace rm {

// blockIdx.y is the view: rm_aa.h's detect on the view's frame, mask, counter and queue segment
__global__ __launch_bounds__(64) void rm_batch_aa_detect(const uint32_t* __restrict__ frames, int W, int H, int tiles_x,
                                                         int threshold, uint8_t* __restrict__ mask,
                                                         uint32_t* __restrict__ counters, uint32_t cstride,
                                                         uint32_t* __restrict__ queue) {
    const size_t off = (size_t)blockIdx.y * ((size_t)W * (size_t)H);
    aa_detect_tile(frames + off, W, H, tiles_x, threshold, mask ? mask + off : nullptr,
                   counters + (size_t)blockIdx.y * cstride, queue + off);
}

// One workgroup.  Thread t takes the views [t * chunk, (t + 1) * chunk): it
// sums their group counts and counts, the workgroup scans the 256 sums, and the
// thread writes its views' exclusive prefixes from its own.  prefix[n] is the
// total of the groups, prefix[n + 1] the total of the counts (<= 2^31).
constexpr int kPlanThreads = 256;
__global__ __launch_bounds__(kPlanThreads) void rm_batch_aa_plan(const uint32_t* __restrict__ counters, uint32_t cstride,
                                                                 uint32_t n, int kshift, uint32_t* __restrict__ prefix,
                                                                 uint32_t* __restrict__ refined) {
    __shared__ uint32_t sg[kPlanThreads], sc[kPlanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + kPlanThreads - 1u) / kPlanThreads;
    const uint32_t v0 = min(t * chunk, n), v1 = min(v0 + chunk, n);
    uint32_t g = 0, c = 0;
    for (uint32_t v = v0; v < v1; v++) {
        const uint32_t cnt = counters[(size_t)v * cstride];
        g += rmbaa::groups_of(cnt, kshift);
        c += cnt;
    }
    sg[t] = g;
    sc[t] = c;
    __syncthreads();
    for (uint32_t o = 1; o < (uint32_t)kPlanThreads; o <<= 1) {  // inclusive scan
        const uint32_t ag = t >= o ? sg[t - o] : 0u, ac = t >= o ? sc[t - o] : 0u;
        __syncthreads();
        sg[t] += ag;
        sc[t] += ac;
        __syncthreads();
    }
    uint32_t run = sg[t] - g;
    for (uint32_t v = v0; v < v1; v++) {
        const uint32_t cnt = counters[(size_t)v * cstride];
        prefix[v] = run;
        if (refined) refined[v] = cnt;
        run += rmbaa::groups_of(cnt, kshift);
    }
    if (t == (uint32_t)kPlanThreads - 1u) {
        prefix[n] = sg[t];
        prefix[n + 1u] = sc[t];
    }
}

// counters a 128-byte line apart unless RM_BATCH_AA_COUNTERS=packed (DESIGN.md 2.28 has both measured)
uint32_t batch_aa_counter_stride() {
    const char* e = std::getenv("RM_BATCH_AA_COUNTERS");
    return e && std::strcmp(e, "packed") == 0 ? rmbaa::kCountersPacked : rmbaa::kCountersLine;
}

hipError_t launch_batch_aa_detect(const uint32_t* frames, int W, int H, int n, int threshold, uint8_t* mask,
                                  uint32_t* counters, uint32_t cstride, uint32_t* queue, hipStream_t s) {
    if (!batch_size_ok(W, H, n) || (int64_t)W * H >= rmaa::kMaxPixels) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const int tx = (W + 7) / 8, ty = (H + 7) / 8;  // (tx * ty <= 2^27: the grid's x; n <= 65535: its y)
    hipLaunchKernelGGL(rm_batch_aa_detect, dim3((unsigned)(tx * ty), (unsigned)n), dim3(64), 0, s, frames, W, H, tx,
                       threshold, mask, counters, cstride, queue);
    return hipGetLastError();
}

hipError_t launch_batch_aa_plan(const uint32_t* counters, uint32_t cstride, int n, int samples, uint32_t* prefix,
                                uint32_t* refined, hipStream_t s) {
    if (n <= 0 || n > kBatchMaxViews || !rmaa::samples_ok(samples)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rm_batch_aa_plan, dim3(1), dim3(kPlanThreads), 0, s, counters, cstride, (uint32_t)n,
                       rmaa::samples_shift(samples), prefix, refined);
    return hipGetLastError();
}

hipError_t launch_batch_aa_refine_t(int scene, const FrameConst& F, const void* views, int n, int samples,
                                    const uint32_t* counters, uint32_t cstride, const uint32_t* prefix,
                                    const uint32_t* queue, uint32_t* frames, hipStream_t s) {
    if (scene == SCENE_S0)
        return launch_batch_aa_refine_scene<SCENE_S0>(F, views, n, samples, counters, cstride, prefix, queue, frames, s);
    if (scene == SCENE_T)
        return launch_batch_aa_refine_scene<SCENE_T>(F, views, n, samples, counters, cstride, prefix, queue, frames, s);
    return hipErrorInvalidValue;
}

}  // namespace rm
