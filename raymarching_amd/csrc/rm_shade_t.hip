// rm_shade_t.hip -- rm_shade_rays (rm_shade.h): the shade kernels of scenes S0
// and T, built with rm_kernels_t.o's flags so that a shaded camera ray is the
// frame kernel's pixel bit for bit, and the camera-ray kernel of these scenes
// under the same flags (that translation unit contracts within expressions:
// built with rm_rays.o's flags, camera_ray's rotation and dot product rounded
// differently from the frame kernels').  Not one of the render objects
// (raymarching_amd/Makefile RENDER_OBJS): rm_render_code_hash() names the frame
// kernels only.
#define RM_SHADE_KERNELS
#include "rm_rays.h"
#include "rm_shade.h"

namespace rm {

__global__ __launch_bounds__(256) void rm_camera_rays_hw_kernel(FrameConst F, float* __restrict__ origin3,
                                                                float* __restrict__ directions) {
    camera_rays_one<true>(F, origin3, directions);
}

hipError_t launch_camera_rays_hw(const FrameConst& F, float* origin3, float* directions, hipStream_t s) {
    const long long n = (long long)F.W * F.H;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_camera_rays_hw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, F, origin3,
                       directions);
    return hipGetLastError();
}

hipError_t launch_shade_rays_t(int scene, const FrameConst& F, const ShadeRays& Q, hipStream_t s) {
    if (scene == SCENE_S0) return launch_shade_scene<SCENE_S0>(F, Q, s);
    if (scene == SCENE_T) return launch_shade_scene<SCENE_T>(F, Q, s);
    return hipErrorInvalidValue;
}

}  // namespace rm
