// post_batch_plan_test.cpp -- raymarching_amd/csrc/rm_post_batch_plan.h (and
// the rm_bloom_plan.h it includes) alone, on the host: the size rule, a view's
// layout against bloom's single-frame layout, and the group arithmetic of
// include/rm.h under the default limit, a limit of 1 byte, one view's worth and
// exactly shared + 3 views.  Built by tests/test_post_batch_host.py with the
// host compiler under -fsanitize=address,undefined; nothing of it is loaded
// into Python.
#include <cstdint>
#include <cstdio>

#include "../../raymarching_amd/csrc/rm_post_batch_plan.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

// include/rm.h's relations, restated with plain integers
static void check_plan(int W, int H, int n, int64_t limit) {
    const rm::BloomPlan b = rm::bloom_plan(W, H);
    const rm::PostBatchViewLayout L = rm::post_batch_view_layout(b);
    const rm::PostBatchPlan p = rm::post_batch_plan(W, H, n, limit);
    const int64_t lim = limit > 0 ? limit : ((int64_t)512 << 20);
    // a view: its levels, then its two polynomial tables, nothing else, 16-byte aligned
    uint64_t levels = 0;
    for (int k = 1; k <= b.d2; k++) {
        CHECK(b.offset[k] == levels);
        levels += (uint64_t)b.w[k] * b.h[k];
    }
    if (b.lod > 0.0f) {
        CHECK(b.level_words == ((levels + 3) & ~(uint64_t)3) && b.level_words == b.base_ent[0]);
        for (int l = 0; l < 2; l++) CHECK(b.poly_words[l] == 12ull * b.nruns[2 * l] * b.nruns[2 * l + 1]);
        CHECK(L.tab[0] == b.level_words && L.tab[1] == L.tab[0] + b.poly_words[0]);
        CHECK(L.view_words == L.tab[1] + b.poly_words[1] && L.view_words % 4 == 0 && L.view_words > 0);
        // the single-frame layout ends with the same two tables: shared holds what a view holds, and the run tables
        CHECK(b.texels == b.poly_tab[1] + b.poly_words[1] && b.poly_tab[1] == b.poly_tab[0] + b.poly_words[0]);
        CHECK(b.texels > L.view_words && b.texels % 4 == 0);
    } else {
        CHECK(b.d2 == 0 && b.texels == 0 && L.view_words == 0);
    }
    CHECK(p.per_view_bytes == (int64_t)L.view_words * 4 && p.shared_bytes == (int64_t)b.texels * 4);
    int64_t g = n;
    if (p.per_view_bytes > 0) {
        const int64_t room = (lim - p.shared_bytes) / p.per_view_bytes;  // (may be negative)
        g = room < n ? room : n;
    }
    if (g < 1) g = 1;
    CHECK(p.group_views == g);
    CHECK(p.groups == (n + g - 1) / g);
    CHECK((int64_t)p.groups * p.group_views >= n && (int64_t)(p.groups - 1) * p.group_views < (n > 0 ? n : 1));
    CHECK(p.scratch_bytes == (n == 0 ? 0 : p.shared_bytes + g * p.per_view_bytes));
    if (g > 1) CHECK(p.scratch_bytes <= lim);  // (only a group of one view may exceed the limit)
    const rm::BloomMips m = rm::bloom_mips(b);
    const int per_group = 1 + m.downs + (m.pyramid ? 1 : 0) + (b.lod > 0.0f ? 2 : 1);
    CHECK(p.launches == (n == 0 ? 0 : p.groups * per_group + (b.lod > 0.0f ? 1 : 0)));
    CHECK(m.pyramid ? m.downs == m.s0 && b.d2 - m.s0 >= 5 && b.d2 - m.s0 <= 8 : m.downs == b.d2);
}

int main() {
    const int shapes[][3] = {{61, 37, 7},     {64, 64, 4096}, {256, 256, 256}, {1920, 1080, 8}, {4096, 4096, 1},
                             {40, 16, 3},     {8, 8, 65535},  {512, 7168, 2},  {64, 448, 3},    {200, 150, 4},
                             {33, 20, 300},   {1, 21, 5},     {8, 8, 0},       {1 << 20, 1023, 2}};
    for (const auto& s : shapes) {
        const rm::PostBatchPlan p = rm::post_batch_plan(s[0], s[1], s[2], 0);
        const int64_t limits[] = {0, 1, p.shared_bytes + p.per_view_bytes, p.shared_bytes + 3 * p.per_view_bytes,
                                  p.shared_bytes + 3 * p.per_view_bytes - 1, p.shared_bytes, (int64_t)1 << 40};
        for (int64_t lim : limits) check_plan(s[0], s[1], s[2], lim);
    }
    // by hand: 64 x 64 -- lod = log2(3.2), levels 1 (32 x 32) and 2 (16 x 16), 64 runs on every axis
    {
        const rm::PostBatchPlan p = rm::post_batch_plan(64, 64, 4096, 0);
        CHECK(p.per_view_bytes == 4 * (1024 + 256 + 2 * 12 * 64 * 64));
        CHECK(p.group_views == (((int64_t)512 << 20) - p.shared_bytes) / p.per_view_bytes && p.group_views < 4096);
        CHECK(p.groups == (4096 + p.group_views - 1) / p.group_views);
        CHECK(p.launches == p.groups * 5 + 1);  // post.frag, two levels, polynomials, strips; the run tables once
        const rm::PostBatchPlan q = rm::post_batch_plan(64, 64, 4096, p.shared_bytes + 3 * p.per_view_bytes);
        CHECK(q.group_views == 3 && q.groups == 1366 && q.launches == 1366 * 5 + 1);
        CHECK(rm::post_batch_plan(64, 64, 4096, 1).group_views == 1);
        CHECK(rm::post_batch_plan(64, 64, 4096, (int64_t)1 << 40).groups == 1);
    }
    // 4096 x 4096: one pyramid launch builds levels 7 and 8
    CHECK(rm::post_batch_plan(4096, 4096, 1, 0).launches == 1 + 1 + 2 + 1);
    // 40 x 16: lod <= 0, no scratch, post.frag and rm_bloom_kernel
    {
        const rm::PostBatchPlan p = rm::post_batch_plan(40, 16, 3, 1);
        CHECK(p.per_view_bytes == 0 && p.shared_bytes == 0 && p.scratch_bytes == 0 && p.group_views == 3 &&
              p.groups == 1 && p.launches == 2);
    }
    // the size rule
    using rm::post_batch_size_ok;
    CHECK(post_batch_size_ok(8, 8, 65535) && !post_batch_size_ok(8, 8, 65536) && !post_batch_size_ok(8, 8, -1));
    CHECK(post_batch_size_ok(1 << 10, 1 << 10, 1 << 11) && !post_batch_size_ok(1 << 10, 1 << 10, (1 << 11) + 1));
    CHECK(post_batch_size_ok((1 << 30) - 1, 1, 1) && post_batch_size_ok((1 << 30) - 1, 1, 2));
    CHECK(!post_batch_size_ok((1 << 30) - 1, 1, 3) && !post_batch_size_ok(1 << 30, 1, 1));
    CHECK(!post_batch_size_ok(1 << 15, 1 << 15, 1) && !post_batch_size_ok(1 << 15, 1 << 15, 0));
    CHECK(post_batch_size_ok(32769, 32767, 2) && !post_batch_size_ok(32769, 32767, 3));
    CHECK(!post_batch_size_ok(0x7FFFFFFF, 0x7FFFFFFF, 65535));  // (no overflow in the product)
    CHECK(!post_batch_size_ok(0, 8, 1) && !post_batch_size_ok(8, 0, 0) && !post_batch_size_ok(-1, 8, 1) &&
          !post_batch_size_ok(8, -1, 1));
    CHECK(post_batch_size_ok(1, 65535 * 8 + 1, 1));  // (no tile-row cap: the views are not rendered here)
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
