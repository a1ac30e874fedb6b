// rm_aa_rule.h -- adaptive supersampling's two rules (include/rm.h,
// rm_refine_rgba8): which pixels of an RGBA8 frame are edge pixels, and where
// the K samples of a refined pixel lie.  Shared by the host (rm_aa_rule.cpp:
// rm_aa_edge_mask, rm_aa_offsets) and the device (rm_aa.h: the detect and
// refine kernels), so that both state one rule.  Plain C++ on the host, no HIP:
// tests/host/aa_rule_test.cpp links rm_aa_rule.cpp alone.
//
// Edge rule, on RGBA8 words (R in the low byte, alpha ignored): pixel (x, y) is
// an edge pixel iff for some channel c of R, G, B the largest byte of c over
// the pixel's 3x3 neighbourhood minus the smallest is >= threshold (0..255),
// neighbour coordinates clamped to the frame.  Integer arithmetic: exact
// everywhere.
//
// Sample offsets, in pixels from the pixel centre, in lane order:
//   K = 2  (4, 4) (-4, -4)                                           / 16
//   K = 4  (-2, -6) (6, -2) (-6, 2) (2, 6)           (rotated grid)  / 16
//   K = 8  (1, -3) (-1, 3) (5, 1) (-3, -5) (-5, 5) (-7, -1) (3, 7) (7, -7)  / 16
// Every offset o and o + 0.5 is exact in f32, so u_seed1 = o + 0.5 makes
// rm_render_accumulate render exactly that sample.
#pragma once
#ifdef __HIPCC_RTC__  // compiled by hiprtc (a scene plugin's AA form, rm_plugin_kernels.h)
using __hip_internal::int64_t;
using __hip_internal::uint32_t;
#else
#include <cstdint>
#endif

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define RM_AA_HD __host__ __device__
#else
#define RM_AA_HD
#endif

namespace rmaa {

constexpr int kMaxSamples = 8;
constexpr int64_t kMaxPixels = (int64_t)1 << 30;  // W * H below it: 32-bit pixel indices and byte offsets

RM_AA_HD inline bool samples_ok(int K) { return K == 2 || K == 4 || K == 8; }
RM_AA_HD inline bool threshold_ok(int t) { return t >= 0 && t <= 255; }
// log2 K of a valid K
RM_AA_HD inline int samples_shift(int K) { return K == 2 ? 1 : K == 4 ? 2 : 3; }

// The tables above as nibbles (sixteenths + 8, sample i in bits [4 i, 4 i + 4)):
// one constant per axis and K, the same integer arithmetic on host and device
// and no table in memory.
RM_AA_HD inline void sample_offset(int K, int i, float& ox, float& oy) {
    const uint32_t xs = K == 2 ? 0x4Cu : K == 4 ? 0xA2E6u : 0xFB135D79u;
    const uint32_t ys = K == 2 ? 0x4Cu : K == 4 ? 0xEA62u : 0x1F7D39B5u;
    ox = (float)((int)((xs >> (4 * i)) & 15u) - 8) * 0.0625f;
    oy = (float)((int)((ys >> (4 * i)) & 15u) - 8) * 0.0625f;
}

RM_AA_HD inline int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the edge rule at pixel (x, y) of the W x H frame
RM_AA_HD inline bool edge_pixel(const uint32_t* frame, int W, int H, int x, int y, int threshold) {
    uint32_t lo[3] = {255u, 255u, 255u}, hi[3] = {0u, 0u, 0u};
    for (int dy = -1; dy <= 1; dy++) {
        const uint32_t* row = frame + (int64_t)clampi(y + dy, H - 1) * W;
        for (int dx = -1; dx <= 1; dx++) {
            const uint32_t w = row[clampi(x + dx, W - 1)];
            for (int c = 0; c < 3; c++) {
                const uint32_t b = (w >> (8 * c)) & 255u;
                lo[c] = b < lo[c] ? b : lo[c];
                hi[c] = b > hi[c] ? b : hi[c];
            }
        }
    }
    bool edge = false;
    for (int c = 0; c < 3; c++) edge = edge || (int)(hi[c] - lo[c]) >= threshold;
    return edge;
}

}  // namespace rmaa
