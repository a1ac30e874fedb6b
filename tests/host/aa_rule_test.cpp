// aa_rule_test.cpp -- adaptive supersampling's host-only calls
// (csrc/rm_aa_rule.cpp: rm_aa_edge_mask, rm_aa_offsets) on the CPU.
// Stand-alone: tests/test_aa_host.py builds it with the host compiler under the
// address and undefined-behaviour sanitizers, linked with rm_aa_rule.cpp only.
// The frames are heap vectors of exactly W * H words, so a neighbour read
// outside the frame is an error the sanitizer reports.  Exits non-zero at the
// first failed check, naming it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/rm.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAILED %s (line %d): %s\n", __func__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static const uint32_t kWhite = 0x00ffffffu;  // (alpha 0: alpha is ignored)

static std::vector<uint8_t> mask_of(const std::vector<uint32_t> &f, int W, int H, int threshold) {
    std::vector<uint8_t> m((size_t)W * H, 7);
    CHECK(rm_aa_edge_mask(W, H, threshold, f.data(), m.data()) == RM_OK);
    return m;
}

// one bright pixel on black: exactly the clamped 3x3 block around it
static void lone_pixel(int W, int H, int px, int py) {
    std::vector<uint32_t> f((size_t)W * H, 0u);
    f[(size_t)py * W + px] = kWhite;
    const std::vector<uint8_t> m = mask_of(f, W, H, 32);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const bool near = x >= px - 1 && x <= px + 1 && y >= py - 1 && y <= py + 1;
            CHECK(m[(size_t)y * W + x] == (near ? 1 : 0));
        }
}

static void lone_pixels() {
    const int sizes[][2] = {{61, 37}, {5, 3}, {9, 1}, {1, 9}, {8, 8}, {2, 2}};
    for (const auto &s : sizes) {
        const int W = s[0], H = s[1];
        lone_pixel(W, H, 0, 0);
        lone_pixel(W, H, W - 1, H - 1);
        lone_pixel(W, H, W - 1, 0);
        lone_pixel(W, H, 0, H - 1);
        lone_pixel(W, H, W / 2, H / 2);
    }
}

// the spread is per channel, max - min, compared with >=
static void thresholds_and_channels() {
    const int W = 4, H = 1;
    for (int c = 0; c < 3; c++) {
        std::vector<uint32_t> f = {0u, 0u, 0u, 0u};
        f[0] = 40u << (8 * c);
        CHECK(mask_of(f, W, H, 40)[0] == 1 && mask_of(f, W, H, 40)[1] == 1);
        CHECK(mask_of(f, W, H, 41)[0] == 0 && mask_of(f, W, H, 41)[1] == 0);
        CHECK(mask_of(f, W, H, 40)[2] == 0 && mask_of(f, W, H, 40)[3] == 0);
    }
    // 20 in three channels is not 60 in one; alpha does not count
    std::vector<uint32_t> g = {0x00141414u, 0u, 0u, 0u};
    CHECK(mask_of(g, W, H, 21)[0] == 0);
    CHECK(mask_of(g, W, H, 20)[0] == 1);
    std::vector<uint32_t> a = {0xff000000u, 0u, 0u, 0u};
    CHECK(mask_of(a, W, H, 1)[0] == 0);
    // the spread is over the neighbourhood, not against the centre: 0 | 100 | 200
    std::vector<uint32_t> r = {0u, 100u, 200u, 200u};
    CHECK(mask_of(r, W, H, 200)[1] == 1 && mask_of(r, W, H, 200)[0] == 0 && mask_of(r, W, H, 101)[2] == 0);
    CHECK(mask_of(r, W, H, 255)[1] == 0);
}

static void flat_frames() {
    // threshold 0: every pixel; a flat frame has no edge pixel above it; 1x1 frames
    for (int t : {0, 1, 255}) {
        std::vector<uint32_t> f((size_t)7 * 5, 0x80402010u);
        for (uint8_t v : mask_of(f, 7, 5, t)) CHECK(v == (t == 0 ? 1 : 0));
        std::vector<uint32_t> one = {0xffffffffu};
        CHECK(mask_of(one, 1, 1, t)[0] == (t == 0 ? 1 : 0));
    }
    // a full-range frame at 255
    std::vector<uint32_t> f = {0u, 0xffu, 0u};
    for (uint8_t v : mask_of(f, 3, 1, 255)) CHECK(v == 1);
}

static void bad_arguments() {
    std::vector<uint32_t> f(4, 0u);
    std::vector<uint8_t> m(4, 0);
    CHECK(rm_aa_edge_mask(0, 2, 1, f.data(), m.data()) == RM_ERR_INVALID_ARGUMENT);
    CHECK(rm_aa_edge_mask(2, -1, 1, f.data(), m.data()) == RM_ERR_INVALID_ARGUMENT);
    CHECK(rm_aa_edge_mask(1 << 15, 1 << 15, 1, f.data(), m.data()) == RM_ERR_INVALID_ARGUMENT);  // 2^30 pixels
    CHECK(rm_aa_edge_mask(2, 2, -1, f.data(), m.data()) == RM_ERR_INVALID_ARGUMENT);
    CHECK(rm_aa_edge_mask(2, 2, 256, f.data(), m.data()) == RM_ERR_INVALID_ARGUMENT);
    CHECK(rm_aa_edge_mask(2, 2, 1, nullptr, m.data()) == RM_ERR_INVALID_ARGUMENT);
    CHECK(rm_aa_edge_mask(2, 2, 1, f.data(), nullptr) == RM_ERR_INVALID_ARGUMENT);
}

static void offsets() {
    const int want2[][2] = {{4, 4}, {-4, -4}};
    const int want4[][2] = {{-2, -6}, {6, -2}, {-6, 2}, {2, 6}};
    const int want8[][2] = {{1, -3}, {-1, 3}, {5, 1}, {-3, -5}, {-5, 5}, {-7, -1}, {3, 7}, {7, -7}};
    struct Case {
        int K;
        const int (*want)[2];
    };
    for (const Case &c : {Case{2, want2}, Case{4, want4}, Case{8, want8}}) {
        std::vector<float> xy((size_t)2 * c.K, 99.0f);  // exactly 2 K floats
        CHECK(rm_aa_offsets(c.K, xy.data()) == RM_OK);
        for (int i = 0; i < c.K; i++) {
            CHECK(xy[2 * i] == (float)c.want[i][0] / 16.0f);
            CHECK(xy[2 * i + 1] == (float)c.want[i][1] / 16.0f);
        }
    }
    float one[2] = {5.0f, 5.0f};
    for (int K : {0, 1, 3, 5, 16, -4}) {
        CHECK(rm_aa_offsets(K, one) == RM_ERR_INVALID_ARGUMENT);
        CHECK(one[0] == 5.0f && one[1] == 5.0f);
    }
    CHECK(rm_aa_offsets(4, nullptr) == RM_ERR_INVALID_ARGUMENT);
}

int main() {
    lone_pixels();
    thresholds_and_channels();
    flat_frames();
    bad_arguments();
    offsets();
    std::printf("all checks passed\n");
    return 0;
}
