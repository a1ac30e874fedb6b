// rm_aa_o.hip -- adaptive supersampling (rm_aa.h): the refine kernels of scene O
// and its glass test variant OG, built with rm_kernels_o.o's flags (no FMA
// contraction, correctly rounded division and sqrt) so that a refined sample is
// the frame kernel's pixel bit for bit.  Not one of the render objects
// (raymarching_amd/Makefile RENDER_OBJS).
#define RM_AA_KERNELS
#include "rm_aa.h"

namespace rm {

hipError_t launch_aa_refine_o(int scene, const FrameConst& F, int samples, int layout, const uint32_t* count,
                              const uint32_t* queue, uint32_t* frame, hipStream_t s) {
    if (scene == SCENE_O) return launch_aa_refine_scene<SCENE_O>(F, samples, layout, count, queue, frame, s);
    if (scene == SCENE_OG) return launch_aa_refine_scene<SCENE_OG>(F, samples, layout, count, queue, frame, s);
    return hipErrorInvalidValue;
}

}  // namespace rm
