// plugin_batch_aa_grid_test.cpp -- raymarching_amd/csrc/rm_plugin_batch_aa_grid.h
// alone, on the host: the number of columns G of a scene plugin's batch refine,
//     G = clamp(ceil(c * waves / n), 1, ceil(W * H / (64 >> kshift))),
// against the same rule in 64-bit arithmetic written out here, at the edges of
// the sizes the calls admit, and the override's parsing.  Built by
// tests/test_plugin_batch_aa_host.py with the host compiler under
// -fsanitize=address,undefined; nothing of it is loaded into Python.
#include <cstdint>
#include <cstdio>

#include "../../raymarching_amd/csrc/rm_plugin_batch_aa_grid.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

// the rule, term by term
static uint64_t want(uint64_t W, uint64_t H, uint64_t n, int kshift, uint64_t waves, uint64_t c) {
    const uint64_t ppw = 64u >> kshift;
    const uint64_t hi = (W * H + ppw - 1) / ppw;
    uint64_t g = (c * waves + n - 1) / n;
    if (g < 1) g = 1;
    if (g > hi) g = hi;
    return g;
}

int main() {
    using rmpbaa::columns;
    const uint32_t waves_of[] = {1, 7, 256, 2048, 4096, 1u << 20};  // (an MI355X: 256 CUs x up to 8 one-wave workgroups)
    const int ns[] = {1, 2, 3, 5, 255, 256, 257, 300, 4096, 8191, 8192, 8193, 16384, 65534, 65535};
    const int sizes[][2] = {{1, 1}, {8, 8}, {5, 3}, {61, 37}, {64, 64}, {256, 256}, {1920, 1080}, {4096, 4096},
                            {32768, 32767}, {1, (1 << 30) - 1}, {(1 << 30) - 1, 1}};  // (W * H < 2^30)
    const uint32_t cs[] = {1, 2, 4, 8};
    for (uint32_t waves : waves_of)
        for (int n : ns)
            for (auto& s : sizes)
                for (int kshift = 1; kshift <= 3; kshift++)  // K = 2, 4, 8
                    for (uint32_t c : cs) {
                        const uint32_t g = columns(s[0], s[1], n, kshift, waves, c);
                        CHECK(g == want((uint64_t)s[0], (uint64_t)s[1], (uint64_t)n, kshift, waves, c));
                        CHECK(g >= 1u && (uint64_t)g * (uint64_t)n >= 1u);            // G * n never 0
                        CHECK(g <= rmpbaa::max_groups(s[0], s[1], kshift));            // no column without a group to start on
                        CHECK((uint64_t)g * 64u < (1ull << 32));                       // a launch's threads in x
                    }
    // the default c
    CHECK(rmpbaa::kOversubscribe == 4u);
    CHECK(columns(256, 256, 256, 2, 2048) == columns(256, 256, 256, 2, 2048, rmpbaa::kOversubscribe));
    // by hand: one view takes c * waves columns, until its groups run out
    CHECK(columns(4096, 4096, 1, 2, 2048, 4) == 8192u);
    CHECK(columns(64, 64, 1, 2, 2048, 4) == 256u);   // 4096 pixels / 16 per group
    CHECK(columns(64, 64, 1, 1, 2048, 4) == 128u);   // K = 2: 32 per group
    CHECK(columns(64, 64, 1, 3, 2048, 4) == 512u);   // K = 8: 8 per group
    CHECK(columns(64, 64, 4096, 2, 2048, 4) == 2u);  // 8192 / 4096
    CHECK(columns(64, 64, 4097, 2, 2048, 4) == 2u);  // (rounded up)
    CHECK(columns(256, 256, 65535, 2, 2048, 4) == 1u);
    // n >= c * waves: one column per view
    CHECK(columns(256, 256, 8192, 2, 2048, 4) == 1u);
    CHECK(columns(256, 256, 8193, 2, 2048, 4) == 1u);
    CHECK(columns(256, 256, 8191, 2, 2048, 4) == 2u);
    // one-pixel frames: the upper bound is 1 whatever the device holds
    for (int kshift = 1; kshift <= 3; kshift++) {
        CHECK(rmpbaa::max_groups(1, 1, kshift) == 1u);
        CHECK(columns(1, 1, 1, kshift, 1u << 20, 8) == 1u);
        CHECK(columns(1, 1, 65535, kshift, 2048, 4) == 1u);
    }
    // W * H just under 2^30: the bound in 64 bits, no wrap
    CHECK(rmpbaa::max_groups(1, (1 << 30) - 1, 3) == (1u << 27));
    CHECK(rmpbaa::max_groups(32768, 32767, 1) == (uint32_t)((32768ull * 32767ull + 31u) / 32u));
    CHECK(columns(32768, 32767, 1, 3, 1u << 20, 8) == (8u << 20));
    // a device that reports nothing still gets a column
    CHECK(columns(64, 64, 3, 2, 0, 4) == 1u);

    // the override's text
    using rmpbaa::columns_override;
    CHECK(columns_override(nullptr, 37) == 37u);
    CHECK(columns_override("", 37) == 37u);
    CHECK(columns_override("1", 37) == 1u);
    CHECK(columns_override("512", 37) == 512u);
    CHECK(columns_override("0", 37) == 37u);
    CHECK(columns_override("-3", 37) == 37u);
    CHECK(columns_override("+3", 37) == 37u);
    CHECK(columns_override(" 3", 37) == 37u);
    CHECK(columns_override("12x", 37) == 37u);
    CHECK(columns_override("x", 37) == 37u);
    CHECK(columns_override("65535", 37) == 65535u);
    CHECK(columns_override("65536", 37) == rmpbaa::kMaxColumns);
    CHECK(columns_override("99999999999999999999999999", 37) == rmpbaa::kMaxColumns);

    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
