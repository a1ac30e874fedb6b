// batch_aa_plan_test.cpp -- raymarching_amd/csrc/rm_batch_aa_plan.h alone, on
// the host: the group count of a view's edge pixels, the exclusive prefix and
// the view lookup by binary search against a linear scan for every group index,
// and the scratch layout.  Built by tests/test_batch_aa_host.py with the host
// compiler under -fsanitize=address,undefined; nothing of it is loaded into
// Python.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../raymarching_amd/csrc/rm_batch_aa_plan.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

// the plan kernel's arithmetic, serially: prefix[0 .. n] from the counts
static std::vector<uint32_t> prefix_of(const std::vector<uint32_t>& counts, int kshift) {
    std::vector<uint32_t> p(counts.size() + 1, 0u);
    for (size_t v = 0; v < counts.size(); v++) p[v + 1] = p[v] + rmbaa::groups_of(counts[v], kshift);
    return p;
}

// every group index of the batch: the binary search against a linear scan
static void check_lookup(const std::vector<uint32_t>& counts, int kshift) {
    const std::vector<uint32_t> p = prefix_of(counts, kshift);
    const uint32_t n = (uint32_t)counts.size(), total = p[n];
    uint64_t want_total = 0;
    for (uint32_t c : counts) want_total += ((uint64_t)c + rmbaa::group_entries(kshift) - 1) / rmbaa::group_entries(kshift);
    CHECK((uint64_t)total == want_total);
    uint32_t scan = 0;  // the linear scan's view: the first with groups left
    for (uint32_t g = 0; g < total; g++) {
        while (p[scan + 1] <= g) scan++;
        const uint32_t v = rmbaa::view_of_group(p.data(), n, g);
        if (v != scan || !(p[v] <= g && g < p[v + 1]) || counts[v] == 0) {
            std::printf("FAILED lookup: kshift %d group %u: view %u, scan %u\n", kshift, g, v, scan);
            failures++;
            return;
        }
        // the group's entries lie inside the view's count, and the last group reaches its end
        const uint32_t gl = g - p[v], first = gl * rmbaa::group_entries(kshift);
        CHECK(first < counts[v]);
        if (g + 1 == p[v + 1]) CHECK(first + rmbaa::group_entries(kshift) >= counts[v]);
    }
}

int main() {
    // ---- group counts: 0, 1, ppw - 1, ppw, ppw + 1 and W * H, for K = 2, 4, 8
    for (int kshift = 1; kshift <= 3; kshift++) {
        const uint32_t ppw = 64u >> kshift;
        CHECK(rmbaa::group_entries(kshift) == ppw);
        CHECK(rmbaa::groups_of(0, kshift) == 0);
        CHECK(rmbaa::groups_of(1, kshift) == 1);
        CHECK(rmbaa::groups_of(ppw - 1, kshift) == 1);
        CHECK(rmbaa::groups_of(ppw, kshift) == 1);
        CHECK(rmbaa::groups_of(ppw + 1, kshift) == 2);
        for (uint32_t px : {61u * 37u, 4096u * 4096u, (1u << 30) - 1u}) {  // (W * H < 2^30)
            CHECK((uint64_t)rmbaa::groups_of(px, kshift) == ((uint64_t)px + ppw - 1) / ppw);
        }
        for (uint32_t c = 0; c < 200; c++) CHECK(rmbaa::groups_of(c, kshift) == (c + ppw - 1) / ppw);
    }

    // ---- prefix and view lookup on hand-made counts
    for (int kshift = 1; kshift <= 3; kshift++) {
        const uint32_t ppw = 64u >> kshift;
        check_lookup(std::vector<uint32_t>(7, 0u), kshift);  // all zero: no group, nothing to look up
        CHECK(prefix_of(std::vector<uint32_t>(7, 0u), kshift)[7] == 0);
        check_lookup({0, 5, 0, 0, 0, ppw, ppw + 1, 0, 0, 1, 3 * ppw - 1, 0}, kshift);  // zero first, last and in runs
        check_lookup({0, 0, 0, 9}, kshift);
        check_lookup({9, 0, 0, 0}, kshift);
        check_lookup({1}, kshift);  // one view
        check_lookup({61 * 37}, kshift);
        check_lookup({0}, kshift);
        check_lookup(std::vector<uint32_t>(65535, 1u), kshift);  // 65535 views of one entry each
        std::vector<uint32_t> mixed(300);
        for (size_t v = 0; v < mixed.size(); v++) mixed[v] = (uint32_t)((v * 37u) % 11u == 0 ? 0u : (v * 53u) % 200u);
        check_lookup(mixed, kshift);
    }
    {  // the exclusive prefix by hand, K = 4 (16 entries per group)
        const std::vector<uint32_t> p = prefix_of({0, 16, 17, 0, 1}, 2);
        const uint32_t want[6] = {0, 0, 1, 3, 3, 4};
        for (int i = 0; i < 6; i++) CHECK(p[i] == want[i]);
        CHECK(rmbaa::view_of_group(p.data(), 5, 0) == 1);
        CHECK(rmbaa::view_of_group(p.data(), 5, 1) == 2);
        CHECK(rmbaa::view_of_group(p.data(), 5, 2) == 2);
        CHECK(rmbaa::view_of_group(p.data(), 5, 3) == 4);
    }
    {  // a total near 2^28 fits: the largest batch, every pixel of every view an edge pixel, K = 8 (8 entries per
       // group): 2^31 / 8 = 2^28 groups; and two views of the largest single frame
        const uint32_t n = 2048, px = 1u << 20;  // n * px = 2^31
        std::vector<uint32_t> p(n + 1, 0u);
        for (uint32_t v = 0; v < n; v++) p[v + 1] = p[v] + rmbaa::groups_of(px, 3);
        CHECK(p[n] == 1u << 28);
        for (uint32_t g : {0u, 1u, (1u << 17) - 1u, 1u << 17, (1u << 28) - 1u, (1u << 27) + 12345u}) {
            const uint32_t v = rmbaa::view_of_group(p.data(), n, g);
            CHECK(v == g >> 17 && p[v] <= g && g < p[v + 1]);
        }
        const uint32_t big = (1u << 30) - 1u;
        const std::vector<uint32_t> q = prefix_of({big, big}, 3);
        CHECK(q[2] == 2u * (1u << 27));
        CHECK(rmbaa::view_of_group(q.data(), 2, (1u << 27) - 1u) == 0);
        CHECK(rmbaa::view_of_group(q.data(), 2, 1u << 27) == 1);
    }

    // ---- the scratch layout
    {
        const rmbaa::Layout l = rmbaa::layout(61, 37, 6);
        CHECK(l.counters == 0 && l.plan == 6 * 32 && l.queue == 6 * 32 + 32 && l.words == 6 * 32 + 32 + 6 * 61 * 37);
        CHECK(rmbaa::layout(8, 8, 0).words == 32);  // (n + 2 = 2 words, rounded up to a line)
        for (int n : {1, 29, 30, 31, 62, 63, 4096, 65535}) {
            const rmbaa::Layout m = rmbaa::layout(8, 8, n);
            // the plan's n + 2 words fit before the queue, every part starts on a line, the strided counters fit
            CHECK(m.plan + (uint64_t)n + 2 <= m.queue && m.queue - m.plan < (uint64_t)n + 2 + 32);
            CHECK(m.plan % 32 == 0 && m.queue % 32 == 0);
            CHECK((uint64_t)(n - 1) * rmbaa::kCountersLine < m.plan && (uint64_t)(n - 1) * rmbaa::kCountersPacked < m.plan);
            CHECK(m.words == m.queue + (uint64_t)n * 64);
        }
        // the largest batch: no 32-bit overflow
        const rmbaa::Layout big = rmbaa::layout(1 << 10, 1 << 10, 1 << 11);
        CHECK(big.words == (uint64_t)32 * 2048 + 2080 + ((uint64_t)1 << 31));
    }

    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
