// rm_bloom_plan.h -- where bloom's mip levels, run tables and run-pair
// polynomials lie in the context's scratch buffer, and which launches build the
// levels (rm_post.hip launch_bloom; rm_post_batch.hip for a batch of frames).
// Plain C++ on the host, no HIP: rm_post_batch_plan.h and through it
// tests/host/post_batch_plan_test.cpp include this header alone.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rm {

// bloom.frag's textureLod level pair and the mip levels 1..d2 it needs,
// packed one after the other in a scratch buffer of `texels` 32-bit words
struct BloomPlan {
    float lod = 0.0f, fr = 0.0f;
    int d1 = 0, d2 = 0;
    int w[40] = {}, h[40] = {};
    size_t offset[40] = {}, texels = 0;
    // lod > 0 (words from the buffer start): the base level's bilinear axes
    // (per column, per row); per axis (d1 x, d1 y, d2 x, d2 y) the pixels' run
    // entries, the runs' cell tuples and the run counts; per level the run-pair
    // polynomials (rm_post.hip).  All but the polynomials depend on W x H only.
    size_t base_ent[2] = {}, run_ent[4] = {}, run_tup[4] = {}, run_count = 0, poly_tab[2] = {};
    int nruns[4] = {};  // most runs an axis can have
    // the words of levels 1..d2 rounded up to 16 bytes (lod > 0: base_ent[0]), and of each level's polynomials
    size_t level_words = 0, poly_words[2] = {};
};

inline BloomPlan bloom_plan(int W, int H) {
    BloomPlan p{};
    int q = 0;
    for (int m = W > H ? W : H; m > 1; m >>= 1) q++;
    p.lod = log2f(0.05f * (float)H);  // bloom.frag:22 (u_resolution = the image, post_bloom.cpp:6)
    if (p.lod > 0.0f) {
        p.d1 = (int)floorf(p.lod);
        p.d1 = p.d1 > q ? q : p.d1;
        p.d2 = p.d1 + 1 > q ? q : p.d1 + 1;
    }
    p.fr = p.lod - floorf(p.lod);
    int w = W, h = H;
    p.w[0] = W;
    p.h[0] = H;
    for (int k = 1; k <= p.d2; k++) {
        w = w > 1 ? w >> 1 : 1;
        h = h > 1 ? h >> 1 : 1;
        p.w[k] = w;
        p.h[k] = h;
        p.offset[k] = p.texels;
        p.texels += (size_t)w * h;
    }
    if (p.lod > 0.0f) {  // the runs and run-pair polynomials of levels d1, d2, 16-byte aligned
        auto al = [](size_t o) { return (o + 3) & ~(size_t)3; };
        const int n[4] = {W, H, W, H}, lw[4] = {p.w[p.d1], p.h[p.d1], p.w[p.d2], p.h[p.d2]};
        size_t o = al(p.texels);
        p.level_words = o;
        for (int a = 0; a < 2; a++) {
            p.base_ent[a] = o;
            o = al(o + 2 * (size_t)n[a]);
        }
        for (int a = 0; a < 4; a++) {
            p.run_ent[a] = o;
            o = al(o + 2 * (size_t)n[a]);
        }
        for (int a = 0; a < 4; a++) {
            const long long m = 5LL * lw[a] + 1;  // distinct cell tuples along the axis
            p.nruns[a] = (int)(n[a] < m ? n[a] : m);
            p.run_tup[a] = o;
            o = al(o + 5 * (size_t)p.nruns[a]);
        }
        p.run_count = o;
        o += 4;
        for (int l = 0; l < 2; l++) {
            p.poly_tab[l] = o;
            p.poly_words[l] = 12 * (size_t)p.nruns[2 * l] * p.nruns[2 * l + 1];
            o += p.poly_words[l];
        }
        p.texels = o;
    }
    return p;
}

// How launch_bloom builds levels 1..d2: when W and H are multiples of 2^d2
// every level is an exact halving, and the last 5..8 levels come from one
// rm_mip_pyramid_kernel launch over level s0 = max(d2 - 8, 0) (only d1, d2
// written); otherwise, and for levels 1..s0, one rm_mip_down_kernel launch per
// level.
struct BloomMips {
    bool pyramid;
    int s0;
    int downs;  // rm_mip_down_kernel launches
};
inline BloomMips bloom_mips(const BloomPlan& p) {
    const int W = p.w[0], H = p.h[0];
    const long long T2 = 1LL << (p.d2 < 62 ? p.d2 : 62);
    const int s0 = p.d2 > 8 ? p.d2 - 8 : 0;
    const bool pyramid = p.lod > 0.0f && p.d2 - s0 >= 5 && W % T2 == 0 && H % T2 == 0;
    return BloomMips{pyramid, s0, pyramid ? s0 : p.d2};
}
// the kernel launches of one bloom whose run tables are in place: the levels, then rm_bloom_kernel (lod <= 0)
// or rm_bloom_poly_kernel and rm_bloom_min_kernel
inline int bloom_launches(const BloomPlan& p) {
    const BloomMips m = bloom_mips(p);
    return m.downs + (m.pyramid ? 1 : 0) + (p.lod > 0.0f ? 2 : 1);
}

}  // namespace rm
