// rm_batch_o.hip -- view batches (rm_batch.h): the batch kernels of scenes O
// and OG, built with rm_kernels_o.o's flags (no FMA contraction, correctly
// rounded '/' and sqrtf) so that a view's frame is the frame kernel's bit for
// bit.  Not one of the render objects (raymarching_amd/Makefile RENDER_OBJS).
#define RM_BATCH_KERNELS
#include "rm_batch.h"

namespace rm {

hipError_t launch_batch_o(int scene, const FrameConst& F, const void* views, int n, void* out, bool rgba8,
                          hipStream_t s) {
    if (scene == SCENE_O) return launch_batch_scene<SCENE_O>(F, views, n, out, rgba8, s);
    if (scene == SCENE_OG) return launch_batch_scene<SCENE_OG>(F, views, n, out, rgba8, s);
    return hipErrorInvalidValue;
}

}  // namespace rm
