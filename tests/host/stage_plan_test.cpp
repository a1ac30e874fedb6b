// stage_plan_test.cpp -- raymarching_amd/csrc/rm_stage_plan.h alone, on the
// host: where the staged host buffers of a call go in their one allocation.
// Offsets are multiples of 256 in declaration order and the buffers do not
// overlap, unused buffers take no space, the total is the sum of the rounded
// sizes, and a sum that does not fit a size_t is reported.  Built by
// tests/test_stage_host.py with the host compiler under
// -fsanitize=address,undefined; nothing of it is loaded into Python.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../raymarching_amd/csrc/rm_stage_plan.h"

using rmstage::Item;
using rmstage::plan;

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

static size_t rounded(size_t b) { return (b + 255) / 256 * 256; }

// the rules, restated with plain integers, for one list
static void check_list(const std::vector<Item>& items) {
    std::vector<size_t> off(items.size() + 1, ~(size_t)0);
    size_t total = ~(size_t)0;
    CHECK(plan(items.data(), (int)items.size(), off.data(), total));
    CHECK(off[items.size()] == ~(size_t)0);  // (nothing written past the list)
    size_t next = 0, sum = 0;
    for (size_t i = 0; i < items.size(); i++) {
        if (!items[i].used) continue;
        CHECK(off[i] % 256 == 0);
        CHECK(off[i] == next);  // declaration order, the one before it rounded up: no overlap, no gap
        CHECK(off[i] + items[i].bytes <= total);
        next = off[i] + rounded(items[i].bytes);
        sum += rounded(items[i].bytes);
    }
    CHECK(total == sum && total == next && total % 256 == 0);
    for (size_t i = 0; i < items.size(); i++)
        for (size_t j = i + 1; j < items.size(); j++)
            if (items[i].used && items[j].used && items[i].bytes > 0)
                CHECK(off[i] + items[i].bytes <= off[j]);
}

int main() {
    // a single 1-byte buffer, an empty list, a list of unused buffers
    {
        const Item one = {1, true};
        size_t off = 7, total = 7;
        CHECK(plan(&one, 1, &off, total) && off == 0 && total == 256);
        CHECK(plan(nullptr, 0, nullptr, total) && total == 0);
        const Item none[2] = {{4096, false}, {1, false}};
        size_t offs[2] = {7, 7};
        CHECK(plan(none, 2, offs, total) && total == 0);
    }
    // by hand: the eight buffers of a ray query of 100 rays with a shared origin, status and normal left out
    {
        const size_t f = sizeof(float), N = 100;
        const Item q[8] = {{3 * f, true},      {N * 3 * f, true}, {N * f, true},      {N * f, false},
                           {N * f, true},      {N * 3 * f, true}, {N * 3 * f, false}, {N * 16 * f, true}};
        size_t off[8], total = 0;
        CHECK(plan(q, 8, off, total));
        CHECK(off[0] == 0 && off[1] == 256 && off[2] == 256 + 1280 && off[4] == off[2] + 512);
        CHECK(off[5] == off[4] + 512 && off[7] == off[5] + 1280 && total == off[7] + 6400);
    }
    // sizes around the alignment, used and unused mixed, a buffer of no bytes
    const size_t sizes[] = {0, 1, 255, 256, 257, 511, 512, 4096, 61 * 37 * 4, 61 * 37, (size_t)1 << 32, 12345677};
    for (size_t a : sizes)
        for (size_t b : sizes)
            for (int mask = 0; mask < 8; mask++)
                check_list({{a, (mask & 1) != 0}, {b, (mask & 2) != 0}, {a + b, (mask & 4) != 0}});
    check_list({});
    // overflow near SIZE_MAX: of one buffer's rounding, and of the sum; an unused buffer of any size is no overflow
    {
        size_t off[3], total = 0;
        const Item big = {SIZE_MAX, true};
        CHECK(!plan(&big, 1, off, total));
        const Item edge = {SIZE_MAX - 254, true};  // (rounds past SIZE_MAX)
        CHECK(!plan(&edge, 1, off, total));
        const Item fits = {SIZE_MAX - 255, true};  // (a multiple of 256 itself)
        CHECK(plan(&fits, 1, off, total) && total == SIZE_MAX - 255);
        const Item sum[3] = {{SIZE_MAX / 2, true}, {1, false}, {SIZE_MAX / 2 + 2, true}};
        CHECK(!plan(sum, 3, off, total));
        const Item after[2] = {{SIZE_MAX - 255, true}, {1, true}};
        CHECK(!plan(after, 2, off, total));
        const Item unused[2] = {{SIZE_MAX, false}, {1, true}};
        CHECK(plan(unused, 2, off, total) && off[1] == 0 && total == 256);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
