// rm_aa_rule.cpp -- the host-only calls of adaptive supersampling (include/rm.h):
// rm_aa_offsets and rm_aa_edge_mask, the rules of rm_aa_rule.h on host memory.
// Plain C++, no HIP (as rm_uniform_decl.cpp): tests/host/aa_rule_test.cpp links
// this file alone, under the sanitizers.
#include "rm_aa_rule.h"

#include "../../include/rm.h"

extern "C" {

rm_status rm_aa_offsets(int samples, float *xy) {
    if (!rmaa::samples_ok(samples) || !xy) return RM_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < samples; i++) rmaa::sample_offset(samples, i, xy[2 * i], xy[2 * i + 1]);
    return RM_OK;
}

rm_status rm_aa_edge_mask(int W, int H, int threshold, const uint32_t *frame, uint8_t *mask) {
    if (W <= 0 || H <= 0 || (int64_t)W * H >= rmaa::kMaxPixels || !rmaa::threshold_ok(threshold) || !frame || !mask)
        return RM_ERR_INVALID_ARGUMENT;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            mask[(int64_t)y * W + x] = rmaa::edge_pixel(frame, W, H, x, y, threshold) ? 1 : 0;
    return RM_OK;
}

}  // extern "C"
