// rm_rays.hip -- the ray-query kernels of the built-in scenes (rm_rays.h):
// rm_cast_rays' march for S0, T, O and OG, and rm_camera_rays' kernel.
//
// One translation unit, built with scene O's flags (no FMA contraction,
// correctly rounded division and sqrt: raymarching_amd/Makefile), so that
// ro + rd * depth and every scene's exact-form distance round as the GLSL
// restatement does.  It is not one of the render kernels' objects: their code,
// and rm_render_code_hash(), do not change with it.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "rm_rays.h"
#include "rm_shade.h"

namespace rm {

// One lane per ray.  The workgroup size is the launch's (cast_block_size): 64
// threads, so that a wave that has finished its rays frees its slot, the render
// kernels' reason for one-wave tiles (measured against 256: DESIGN.md 2.19).
template <int SC>
__global__ __launch_bounds__(256) void rm_cast_rays_kernel(FrameConst F, RayQuery Q, int inside) {
    cast_rays_one<SC>(F, Q, inside);
}

// (the exact forms: scenes O, OG and plugins)
__global__ __launch_bounds__(256) void rm_camera_rays_kernel(FrameConst F, float* __restrict__ origin3,
                                                              float* __restrict__ directions) {
    camera_rays_one<false>(F, origin3, directions);
}

// 64 threads; RM_CAST_BLOCK=256 selects four-wave workgroups, read at every
// call so that tools/ray_query_probe.py can alternate the two in one process
// (DESIGN.md 2.19 has both columns)
int cast_block_size() {
    const char* e = std::getenv("RM_CAST_BLOCK");
    return e && std::atoi(e) == 256 ? 256 : 64;
}

template <int SC>
static hipError_t launch_cast(const FrameConst& F, const RayQuery& Q, int inside, hipStream_t s) {
    const unsigned block = (unsigned)cast_block_size();
    hipLaunchKernelGGL((rm_cast_rays_kernel<SC>), dim3((unsigned)((Q.n + block - 1) / block)), dim3(block), 0, s, F, Q,
                       inside);
    return hipGetLastError();
}

hipError_t launch_cast_rays(int scene, const FrameConst& F, const RayQuery& Q, int inside, hipStream_t s) {
    if (Q.n <= 0) return hipSuccess;
    switch (scene) {
    case SCENE_S0: return launch_cast<SCENE_S0>(F, Q, inside, s);
    case SCENE_T: return launch_cast<SCENE_T>(F, Q, inside, s);
    case SCENE_O: return launch_cast<SCENE_O>(F, Q, inside, s);
    case SCENE_OG: return launch_cast<SCENE_OG>(F, Q, inside, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_camera_rays(bool fast, const FrameConst& F, float* origin3, float* directions, hipStream_t s) {
    // the hardware forms (scenes S0/T) under the flags of those scenes' frame kernels, which contract within
    // expressions (rm_shade_t.hip): the rays are then the frame's own in every bit, and rm_shade_rays of them
    // its pixels
    if (fast) return launch_camera_rays_hw(F, origin3, directions, s);
    const long long n = (long long)F.W * F.H;
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(rm_camera_rays_kernel, grid, block, 0, s, F, origin3, directions);
    return hipGetLastError();
}

}  // namespace rm
