// rm_post_batch_plan.h -- the arithmetic of the batched post passes
// (include/rm.h rm_post_chain_batch, rm_post_batch_plan): the
// size rule, what of bloom's scratch every view needs and what the views share,
// how many views a group holds under a scratch limit, and how many kernel
// launches a chain makes.  Shared by the host entry points
// (rm_post_host.cpp) and the launch code (rm_post_batch.hip), so that
// rm_post_batch_plan reports what a call really allocates and launches.  Plain
// C++ on the host, no HIP: tests/host/post_batch_plan_test.cpp includes this
// header alone.
//
// The scratch buffer, in 32-bit words:
//   shared   bloom_plan(W, H).texels   the single-frame layout of rm_bloom, of
//            which a batch uses the run tables only (they depend on W x H
//            alone and sit where rm_bloom keeps them, so that a batch and a
//            single call of one size reuse each other's tables; the levels and
//            polynomials in it are left to rm_bloom)
//   views    group_views * view_words  per view: levels 1..d2 at the plan's
//            offsets, rounded up to 16 bytes, then the two levels' run-pair
//            polynomials (12 floats per (column run, row run) pair)
// lod <= 0 (H <= 20): bloom reads the frame alone, and both parts are empty.
#pragma once
#include <cstdint>

#include "rm_bloom_plan.h"

namespace rm {

constexpr int64_t kPostBatchDefaultLimit = (int64_t)512 << 20;  // rm.h RM_POST_BATCH_SCRATCH_DEFAULT
constexpr int kPostBatchMaxViews = 65535;                        // gridDim.z (and the view batch's rule)
constexpr int64_t kPostBatchMaxPixels = (int64_t)1 << 31, kPostBatchMaxFrame = (int64_t)1 << 30;

// include/rm.h's size rule of the batched post calls
inline bool post_batch_size_ok(int W, int H, int n) {
    if (W <= 0 || H <= 0 || n < 0 || n > kPostBatchMaxViews) return false;
    const int64_t px = (int64_t)W * H;  // (< 2^62)
    if (px >= kPostBatchMaxFrame) return false;
    return n == 0 || px <= kPostBatchMaxPixels / n;  // (n * px compared by division: no overflow)
}

// one view's part of the scratch, in words from the view's base
struct PostBatchViewLayout {
    uint64_t tab[2];      // the polynomials of levels d1, d2 (levels 1..d2 are at BloomPlan.offset[k])
    uint64_t view_words;  // a multiple of 4
};
inline PostBatchViewLayout post_batch_view_layout(const BloomPlan& p) {
    PostBatchViewLayout L{};
    L.tab[0] = p.level_words;
    L.tab[1] = L.tab[0] + p.poly_words[0];
    L.view_words = L.tab[1] + p.poly_words[1];  // (12 floats per pair: a multiple of 4 words)
    return L;
}

struct PostBatchPlan {  // rm.h rm_post_batch_plan
    int64_t per_view_bytes, shared_bytes;
    int32_t group_views, groups;
    int64_t scratch_bytes;
    int32_t launches;
};

// limit_bytes <= 0: the default.  The caller has applied the size rule.
//   group_views = max(1, min(n, (limit - shared) / per_view))    (all n where a view needs nothing)
//   groups      = ceil(n / group_views)
//   scratch     = shared + group_views * per_view                (0 for n = 0: nothing is allocated)
//   launches    = groups * (1 + bloom_launches) + (lod > 0: the run tables' one launch)
inline PostBatchPlan post_batch_plan(int W, int H, int n, int64_t limit_bytes) {
    const BloomPlan p = bloom_plan(W, H);
    const PostBatchViewLayout L = post_batch_view_layout(p);
    const int64_t limit = limit_bytes > 0 ? limit_bytes : kPostBatchDefaultLimit;
    PostBatchPlan r{};
    r.per_view_bytes = (int64_t)(L.view_words * sizeof(uint32_t));
    r.shared_bytes = (int64_t)(p.texels * sizeof(uint32_t));
    int64_t g = n;
    if (r.per_view_bytes > 0) {
        const int64_t room = limit > r.shared_bytes ? (limit - r.shared_bytes) / r.per_view_bytes : 0;
        g = room < n ? room : n;
    }
    r.group_views = (int32_t)(g < 1 ? 1 : g);
    r.groups = (int32_t)(((int64_t)n + r.group_views - 1) / r.group_views);
    r.scratch_bytes = n == 0 ? 0 : r.shared_bytes + r.group_views * r.per_view_bytes;
    r.launches = n == 0 ? 0 : r.groups * (1 + bloom_launches(p)) + (p.lod > 0.0f ? 1 : 0);
    return r;
}

}  // namespace rm
