// rm_post_view.h -- how one text of the post kernels serves a frame and a batch
// of frames.  rm_fxaa_kernels.h, rm_post_frag_kernels.h and
// rm_bloom_kernels.h define every kernel as RM_PK(name): in the single-frame
// translation units (rm_fxaa.hip, rm_post_frag.hip, rm_post.hip) that is
// name_kernel with exactly the arguments and code it had as plain text there;
// rm_post_batch.hip defines RM_POST_BATCH first, and the same text becomes
// name_batch_kernel with a trailing ViewStride argument, whose RM_PV(...)
// statements advance the frame, level and table pointers to the view the grid
// names before anything is read.  The offsets are wave-uniform 64-bit word
// counts, so all the indexing inside a view (32-bit byte offsets, __umul24 row
// offsets, CLAMP_TO_EDGE) stays per frame, and the arithmetic is one text: a
// batch's bytes are the single call's by construction.
#pragma once
#include <stdint.h>

namespace rm {

// words from one view to the next of up to four of a kernel's pointers (each
// kernel says which)
struct ViewStride {
    uint64_t a, b, c, d;
};

}  // namespace rm

#ifdef RM_POST_BATCH
#define RM_PK(name) name##_batch_kernel
#define RM_PV_ARG , ViewStride vs
#define RM_PV(...) __VA_ARGS__
#else
#define RM_PK(name) name##_kernel
#define RM_PV_ARG
#define RM_PV(...)
#endif
