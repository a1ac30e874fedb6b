// rm_kernels_t.hip -- render kernels of scenes S0 and T (FMA contraction on).
#include "rm_kernels_impl.h"

namespace rm {

hipError_t launch_scene_s0(const FrameConst& F, void* out, bool rgba8, unsigned long long* evals, int kernel,
                           hipStream_t s) {
    return launch_scene<SCENE_S0>(F, out, rgba8, evals, kernel, s);
}
hipError_t launch_scene_t(const FrameConst& F, void* out, bool rgba8, unsigned long long* evals, int kernel,
                           hipStream_t s) {
    return launch_scene<SCENE_T>(F, out, rgba8, evals, kernel, s);
}

hipError_t launch_eval_s0(const FrameConst& F, const float* pts, long long n, float* dist, float* mat,
                          hipStream_t s) {
    return launch_eval<SCENE_S0>(F, pts, n, dist, mat, s);
}
hipError_t launch_eval_t(const FrameConst& F, const float* pts, long long n, float* dist, float* mat,
                          hipStream_t s) {
    return launch_eval<SCENE_T>(F, pts, n, dist, mat, s);
}

hipError_t launch_eval_form_s0(const FrameConst& F, const float* pts, long long n, int form, float* dist,
                               float* mat, float* aux, hipStream_t s) {
    return launch_eval_form<SCENE_S0>(F, pts, n, form, dist, mat, aux, s);
}
hipError_t launch_eval_form_t(const FrameConst& F, const float* pts, long long n, int form, float* dist,
                              float* mat, float* aux, hipStream_t s) {
    return launch_eval_form<SCENE_T>(F, pts, n, form, dist, mat, aux, s);
}

// FrameConst.rcp_*: v_rcp_f32 of the frame size and of u_resolution.y, the floats camera_ray<FAST> divided by in
// every wave before they were members (one thread; the host keeps them per resolution, rm_render_host.cpp frame_rcp)
__global__ __launch_bounds__(64) void rm_resolution_rcp(int W, int H, float res_y, float* __restrict__ out3) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out3[0] = __builtin_amdgcn_rcpf((float)W);
    out3[1] = __builtin_amdgcn_rcpf((float)H);
    out3[2] = __builtin_amdgcn_rcpf(res_y);
}
hipError_t launch_resolution_rcp(int W, int H, float res_y, float* out3, hipStream_t s) {
    hipLaunchKernelGGL(rm_resolution_rcp, dim3(1), dim3(64), 0, s, W, H, res_y, out3);
    return hipGetLastError();
}

hipError_t launch_wire_s0(const FrameConst& F, WireTile* slots, unsigned long long* evals, hipStream_t s) {
    return launch_scene_wire<SCENE_S0>(F, slots, evals, s);
}
hipError_t launch_wire_t(const FrameConst& F, WireTile* slots, unsigned long long* evals, hipStream_t s) {
    return launch_scene_wire<SCENE_T>(F, slots, evals, s);
}

}  // namespace rm
