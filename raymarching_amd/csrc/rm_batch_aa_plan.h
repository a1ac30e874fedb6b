// rm_batch_aa_plan.h -- the index arithmetic of adaptive supersampling over a
// view batch (include/rm.h rm_render_batch_aa_rgba8): how many
// refine groups a view's count of edge pixels makes, which view a global group
// index belongs to, and where the counters, the plan and the queue lie in the
// context's scratch buffer.  Shared by the host (rm_batch_aa_host.cpp) and the
// device (rm_batch_aa.h), so that both state one rule.  Plain C++ on the host,
// no HIP: tests/host/batch_aa_plan_test.cpp includes this header alone.
//
// A refine group is the work of one wave pass: 64 >> kshift queue entries of one
// view, K = 1 << kshift lanes each.  A group never spans two views, so a view's
// last group is partial unless its count is a multiple of 64 / K.
//
// The scratch buffer, in 32-bit words (every part starts on a 128-byte line):
//   counters  32 * n               view v's count of edge pixels at word
//                                  v * stride, stride = 1 (packed) or 32 (a line
//                                  apart); the region holds either layout
//   plan      roundup32(n + 2)     prefix[0 .. n]: the groups of the views before
//                                  v, prefix[n] the total; then the sum of the counts
//   queue     n * W * H            view v's entries (y * W + x) from v * W * H
#pragma once
#ifndef __HIPCC_RTC__  // (a scene plugin's batch-AA form takes group_entries through rm_aa.h)
#include <cstdint>
#endif

#if defined(__HIPCC__)
#define RM_BAA_HD __host__ __device__
#else
#define RM_BAA_HD
#endif

namespace rmbaa {

constexpr uint32_t kLineWords = 32;  // a 128-byte line
constexpr uint32_t kCountersPacked = 1, kCountersLine = kLineWords;  // the counters' stride in words

// queue entries (pixels) per group of K = 1 << kshift samples
RM_BAA_HD inline uint32_t group_entries(int kshift) { return 64u >> kshift; }

// ceil(count / (64 >> kshift)); count <= 2^30: no wrap
RM_BAA_HD inline uint32_t groups_of(uint32_t count, int kshift) {
    return (count + group_entries(kshift) - 1u) >> (6 - kshift);
}

// The view of global group g < prefix[n]: the v with prefix[v] <= g < prefix[v + 1]
// (views without groups repeat their successor's prefix and are never found).
// Binary search; prefix has n + 1 words, prefix[0] = 0, non-decreasing.
RM_BAA_HD inline uint32_t view_of_group(const uint32_t* prefix, uint32_t n, uint32_t g) {
    uint32_t lo = 0, hi = n;  // prefix[lo] <= g < prefix[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

RM_BAA_HD inline uint64_t round_line(uint64_t words) { return (words + (kLineWords - 1u)) & ~(uint64_t)(kLineWords - 1u); }

struct Layout {
    uint64_t counters, plan, queue, words;  // word offsets of the three parts, and the buffer's size in words
};
// n >= 0 views of W x H; the caller has applied the size rule (n * W * H <= 2^31)
RM_BAA_HD inline Layout layout(int W, int H, int n) {
    Layout l;
    l.counters = 0;
    l.plan = (uint64_t)kLineWords * (uint64_t)n;
    l.queue = l.plan + round_line((uint64_t)n + 2u);
    l.words = l.queue + (uint64_t)n * (uint64_t)W * (uint64_t)H;
    return l;
}

}  // namespace rmbaa
