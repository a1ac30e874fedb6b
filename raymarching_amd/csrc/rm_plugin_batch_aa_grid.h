// rm_plugin_batch_aa_grid.h -- the grid of a scene plugin's batch refine
// (include/rm.h rm_refine_batch_ex_rgba8): dim3(G, 1, n)
// one-wave workgroups, G columns for each of the n views (rm_plugin_kernels.h
// rm_plugin_batch_aa_refine).  A column strides over its view's refine groups,
// so any G >= 1 gives the same bytes; G decides only how the work spreads.
// Plain C++ on the host, no HIP: tests/host/plugin_batch_aa_grid_test.cpp
// includes this header alone.
//
//     G = clamp(ceil(c * waves / n), 1, ceil(W * H / (64 >> kshift)))
//
// waves: the one-wave workgroups the device holds at once (CUs x the kernel's
// occupancy).  c = 1 just fills the device, and views that differ in their
// counts of edge pixels then leave waves idle at the tail; a larger c lets the
// dispatcher fill in behind the views that finish early.  The upper bound is
// the most groups a view can have: every pixel queued.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace rmpbaa {

constexpr uint32_t kOversubscribe = 4;  // c (DESIGN.md 2.32 has 1, 2, 4 and 8 measured; none wins everywhere)
constexpr uint32_t kMaxColumns = 65535;  // of an override: a grid dimension of any launch stays small

// the most refine groups of one view of W x H: ceil(W * H / (64 >> kshift)); W * H < 2^30
inline uint32_t max_groups(int W, int H, int kshift) {
    const uint64_t ppw = 64u >> kshift;
    return (uint32_t)(((uint64_t)W * (uint64_t)H + ppw - 1u) / ppw);
}

// n >= 1 views of W x H >= 1 pixels, K = 1 << kshift samples, kshift 1..3; never 0
inline uint32_t columns(int W, int H, int n, int kshift, uint32_t waves, uint32_t c = kOversubscribe) {
    const uint64_t nn = n > 0 ? (uint64_t)n : 1u;
    const uint64_t want = ((uint64_t)c * (uint64_t)waves + nn - 1u) / nn;
    const uint64_t hi = max_groups(W, H, kshift) > 0u ? max_groups(W, H, kshift) : 1u;
    return (uint32_t)(want < 1u ? 1u : want > hi ? hi : want);
}

// RM_PLUGIN_BATCH_AA_COLUMNS=<G>: the text of an override, or null.  A decimal number >= 1 replaces g (bounded by
// kMaxColumns, not by the view's groups: columns past them leave at once); anything else leaves g.
inline uint32_t columns_override(const char* text, uint32_t g) {
    if (!text || *text < '0' || *text > '9') return g;  // (no sign, no blank)
    char* end = nullptr;
    const unsigned long long v = std::strtoull(text, &end, 10);
    if (end == text || *end != '\0' || v < 1u) return g;
    return (uint32_t)(v > kMaxColumns ? kMaxColumns : v);
}

}  // namespace rmpbaa
