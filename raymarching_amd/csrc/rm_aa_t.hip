// rm_aa_t.hip -- adaptive supersampling (rm_aa.h): the refine kernels of scenes
// S0 and T, built with rm_kernels_t.o's flags so that a refined sample is the
// frame kernel's pixel bit for bit, and the scene-independent detect kernel
// (integer code).  Not one of the render objects (raymarching_amd/Makefile
// RENDER_OBJS): rm_render_code_hash() names the frame kernels only.
#define RM_AA_KERNELS
#include <cstdlib>
#include <cstring>

#include "rm_aa.h"

namespace rm {

__global__ __launch_bounds__(64) void rm_aa_detect(const uint32_t* __restrict__ frame, int W, int H, int tiles_x,
                                                   int threshold, uint8_t* __restrict__ mask,
                                                   uint32_t* __restrict__ count, uint32_t* __restrict__ queue) {
    aa_detect_tile(frame, W, H, tiles_x, threshold, mask, count, queue);
}

// lane = (queue entry, sample) unless RM_AA_LAYOUT=pixel (DESIGN.md 2.20 has both measured)
int aa_layout() {
    const char* e = std::getenv("RM_AA_LAYOUT");
    return e && std::strcmp(e, "pixel") == 0 ? AA_LANE_PIXEL : AA_LANE_SAMPLE;
}

hipError_t launch_aa_detect(const uint32_t* frame, int W, int H, int threshold, uint8_t* mask, uint32_t* count,
                            uint32_t* queue, hipStream_t s) {
    if (W <= 0 || H <= 0 || (int64_t)W * H >= rmaa::kMaxPixels) return hipErrorInvalidValue;
    const int tx = (W + 7) / 8, ty = (H + 7) / 8;  // (tx * ty <= 2^27: a one-dimensional grid)
    hipLaunchKernelGGL(rm_aa_detect, dim3((unsigned)(tx * ty)), dim3(64), 0, s, frame, W, H, tx, threshold, mask, count,
                       queue);
    return hipGetLastError();
}

hipError_t launch_aa_refine_t(int scene, const FrameConst& F, int samples, int layout, const uint32_t* count,
                              const uint32_t* queue, uint32_t* frame, hipStream_t s) {
    if (scene == SCENE_S0) return launch_aa_refine_scene<SCENE_S0>(F, samples, layout, count, queue, frame, s);
    if (scene == SCENE_T) return launch_aa_refine_scene<SCENE_T>(F, samples, layout, count, queue, frame, s);
    return hipErrorInvalidValue;
}

}  // namespace rm
