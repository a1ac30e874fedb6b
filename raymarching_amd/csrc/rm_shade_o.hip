// rm_shade_o.hip -- rm_shade_rays (rm_shade.h): the shade kernels of scene O and
// its glass test variant OG, built with rm_kernels_o.o's flags (no FMA
// contraction, correctly rounded division and sqrt) so that a shaded camera ray
// is the frame kernel's pixel bit for bit.  Not one of the render objects
// (raymarching_amd/Makefile RENDER_OBJS).
#define RM_SHADE_KERNELS
#include "rm_shade.h"

namespace rm {

hipError_t launch_shade_rays_o(int scene, const FrameConst& F, const ShadeRays& Q, hipStream_t s) {
    if (scene == SCENE_O) return launch_shade_scene<SCENE_O>(F, Q, s);
    if (scene == SCENE_OG) return launch_shade_scene<SCENE_OG>(F, Q, s);
    return hipErrorInvalidValue;
}

}  // namespace rm
