// rm_batch_aa_o.hip -- adaptive supersampling of a view batch (rm_batch_aa.h):
// the refine kernels of scene O and its glass test variant OG, built with
// rm_kernels_o.o's flags (no FMA contraction, correctly rounded division and
// sqrt) so that a refined sample is the frame kernel's pixel bit for bit.  Not
// one of the render objects (raymarching_amd/Makefile RENDER_OBJS).
#define RM_AA_KERNELS
#define RM_BATCH_AA_KERNELS
#include "rm_batch_aa.h"

namespace rm {

hipError_t launch_batch_aa_refine_o(int scene, const FrameConst& F, const void* views, int n, int samples,
                                    const uint32_t* counters, uint32_t cstride, const uint32_t* prefix,
                                    const uint32_t* queue, uint32_t* frames, hipStream_t s) {
    if (scene == SCENE_O)
        return launch_batch_aa_refine_scene<SCENE_O>(F, views, n, samples, counters, cstride, prefix, queue, frames, s);
    if (scene == SCENE_OG)
        return launch_batch_aa_refine_scene<SCENE_OG>(F, views, n, samples, counters, cstride, prefix, queue, frames, s);
    return hipErrorInvalidValue;
}

}  // namespace rm
