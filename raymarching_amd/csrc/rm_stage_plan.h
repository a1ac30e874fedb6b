// rm_stage_plan.h -- where the host buffers of a call go in its one staging
// allocation (rm_stage.h): the arithmetic alone, no HIP in it
// (tests/host/stage_plan_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace rmstage {

constexpr size_t kAlign = 256;  // every buffer starts on a multiple of it

struct Item {
    size_t bytes;
    bool used;  // an unused buffer takes no space
};

// offset[i]: where buffer i starts (an unused one: where the next used one does); total: the allocation's bytes,
// the sum of the used buffers' sizes, each rounded up to kAlign.  False if that sum does not fit a size_t.
inline bool plan(const Item *items, int n, size_t *offset, size_t &total) {
    total = 0;
    for (int i = 0; i < n; i++) {
        offset[i] = total;
        if (!items[i].used) continue;
        if (items[i].bytes > SIZE_MAX - (kAlign - 1)) return false;
        const size_t rounded = (items[i].bytes + kAlign - 1) & ~(kAlign - 1);
        if (rounded > SIZE_MAX - total) return false;
        total += rounded;
    }
    return true;
}

}  // namespace rmstage
