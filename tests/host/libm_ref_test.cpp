// libm_ref_test.cpp -- raymarching_amd/csrc/rm_libm_ref.h on the host against
// the C library's sinf and powf (tests/test_libm_ref.py builds and runs it):
// prints the number of arguments on which the floats differ.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../raymarching_amd/csrc/rm_libm_ref.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main() {
    // a 64-bit LCG (Knuth's MMIX constants), top 24 bits -> [0, 1)
    uint64_t state = 20261020;
    auto uniform = [&]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (float)(state >> 40) * (1.0f / 16777216.0f);
    };
    const long n = 1000000;
    long sin_small = 0, sin_mid = 0, sin_large = 0, pow_bad = 0;
    for (long i = 0; i < n; i++) {
        volatile float a = (uniform() * 2.0f - 1.0f) * 0.8f;              // |x| < pi/4 (and tiny ones below)
        volatile float b = (uniform() * 2.0f - 1.0f) * 56.0f * 3.1416f;   // floorMat's range: pos.x * PI, |pos.x| <= 56
        volatile float c = (uniform() * 2.0f - 1.0f) * 1.0e6f;            // the large-argument reduction
        volatile float l = uniform() * 70.0f + 1.0e-3f;                   // |p|
        const float as = i % 16 ? a : a * 1.0e-4f;
        sin_small += bits(std::sin(as)) != bits(rm::libm::sin_ref(as));
        sin_mid += bits(std::sin(b)) != bits(rm::libm::sin_ref(b));
        sin_large += bits(std::sin(c)) != bits(rm::libm::sin_ref(c));
        pow_bad += bits(std::pow(l, 1.3f)) != bits(rm::libm::pow_ref(l, 1.3f));
    }
    std::printf("{\"n\": %ld, \"sin_small\": %ld, \"sin_mid\": %ld, \"sin_large\": %ld, \"pow\": %ld}\n", n, sin_small,
                sin_mid, sin_large, pow_bad);
    return 0;
}
