// rm_batch_t.hip -- view batches (rm_batch.h): the batch kernels of scenes S0
// and T, built with rm_kernels_t.o's flags so that a view's frame is the frame
// kernel's bit for bit.  Not one of the render objects
// (raymarching_amd/Makefile RENDER_OBJS): rm_render_code_hash() names the frame
// kernels only.
#define RM_BATCH_KERNELS
#include "rm_batch.h"

namespace rm {

hipError_t launch_batch_t(int scene, const FrameConst& F, const void* views, int n, void* out, bool rgba8,
                          hipStream_t s) {
    if (scene == SCENE_S0) return launch_batch_scene<SCENE_S0>(F, views, n, out, rgba8, s);
    if (scene == SCENE_T) return launch_batch_scene<SCENE_T>(F, views, n, out, rgba8, s);
    return hipErrorInvalidValue;
}

}  // namespace rm
