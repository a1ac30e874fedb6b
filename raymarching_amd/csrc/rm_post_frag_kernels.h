// rm_post_frag_kernels.h -- the kernels of post.frag's texel and
// chromaticAberration samples (rm_post_frag.hip tells the pass).  One text for
// two translation units (rm_post_view.h): rm_post_frag.hip compiles it into the
// single-frame kernels, rm_post_batch.hip into the batch forms, which first
// advance `in` and `out` to the frame of the view blockIdx.y names (grid x
// numbers the tiles).
#pragma once
#include "rm_post_common.h"
#include "rm_post_view.h"
#include "rm_post_tonemap.h"

namespace rm {

// the 8 x 3 channel factors: rf *= 0.9972, gf *= 0.998, bf /= 0.9988, iterated
// in float as the shader's loop does
struct ChromaFactors {
    float k[8][3];
};
constexpr ChromaFactors chroma_factors() {
    ChromaFactors f{};
    float rf = 1.0f, gf = 1.0f, bf = 1.0f;
    for (int i = 0; i < 8; i++) {
        f.k[i][0] = rf;
        f.k[i][1] = gf;
        f.k[i][2] = bf;
        rf *= 0.9972f;
        gf *= 0.998f;
        bf /= 0.9988f;
    }
    return f;
}
__device__ const ChromaFactors kChroma = chroma_factors();  // (the same values, indexed by lane)

// texture()'s texel index on an axis of n texels (rm_post_common.h texel())
__device__ __forceinline__ int texel_index(float u, int n) { return clamp_med3((int)floorf(u * (float)n), n - 1); }
// a chromaticAberration tap's: 0.5 - 0.5 (uv k) with uv = 1 - 2 UV (post.frag:115,122-124)
__device__ __forceinline__ int tap_index(float uv, float k, int n) { return texel_index(0.5f - 0.5f * (uv * k), n); }

__device__ __forceinline__ uint32_t load_texel(const uint32_t* __restrict__ in, uint32_t index) {
    // (a 32-bit byte offset from the uniform base: frames < 2^30 texels)
    return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(in) + index * 4u);
}

// The tiles of a frame numbered row-major along grid x (a frame of W*H < 2^30
// pixels has fewer than 2^31 tiles whatever its shape; grid y would cap H).
struct Tile {
    int x0, y0;
};
__device__ __forceinline__ Tile tile_of_block(int tiles_x, int tw, int th) {
    const int ty = blockIdx.x / tiles_x;
    return Tile{(int)(blockIdx.x - ty * tiles_x) * tw, ty * th};
}

// The chromatic sample: 64x32-pixel tiles, a wave per row, a lane per column,
// 8 rows per lane.  A lane forms its 24 tap columns once per tile.  A row's 24
// tap rows are the same for the whole wave: lane t < 24 forms tap t's (first
// texel of the row, iy W), and every lane reads it as a wave-uniform scalar.
constexpr int CA_TX = 64, CA_TY = 32, CA_NW = 4;
template <int TM>
__global__ __launch_bounds__(64 * CA_NW) void RM_PK(rm_post_chromatic)(const uint32_t* __restrict__ in,
                                                                       uint32_t* __restrict__ out, int W, int H,
                                                                       int tiles_x RM_PV_ARG) {
    RM_PV(in += blockIdx.y * vs.a; out += blockIdx.y * vs.a;)  // (view blockIdx.y's frame)
    constexpr ChromaFactors F = chroma_factors();
    const Tile t = tile_of_block(tiles_x, CA_TX, CA_TY);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // (columns and rows past the frame are computed on the clamped pixel and not
    // stored: no lane leaves before the wave-uniform reads below)
    const int x = min(t.x0 + lane, W - 1);
    // post.frag:140: uv = vec2(gl_TexCoord.x, 1 - gl_TexCoord.y)
    const float fx = ((float)x + 0.5f) / (float)W;
    const float ux = 1.0f - 2.0f * fx;
    int ix[8][3];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) ix[i][ch] = tap_index(ux, F.k[i][ch], W);
    const int ixc = texel_index(fx, W);
    const int tap = lane < 24 ? lane : 0;
    const float k_lane = kChroma.k[tap / 3][tap % 3];
    // c += f texel.ch with f = 1/8, texel.ch = byte (1/255): byte ((1/255) / 8)
    // has the same bits (a power of two scales exactly).  c and the term are
    // never negative, so clamp(c, 0, 1) is min(c, 1).
    const float fk = (1.0f / 255.0f) * (1.0f / 8.0f);
    for (int j = 0; j < CA_TY / CA_NW; j++) {
        const int yy = t.y0 + wv + CA_NW * j;
        const int y = min(yy, H - 1);
        const float fy = 1.0f - ((float)y + 0.5f) / (float)H;
        const int row_lane = tap_index(1.0f - 2.0f * fy, k_lane, H) * W;
        const uint32_t tM = load_texel(in, (uint32_t)(texel_index(fy, H) * W + ixc));
        uint32_t tx[8][3];
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
                tx[i][ch] = load_texel(in, (uint32_t)(__builtin_amdgcn_readlane(row_lane, 3 * i + ch) + ix[i][ch]));
        RGB c{0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < 8; i++) {
            c.r = gmin_(c.r + (float)(tx[i][0] & 255u) * fk, 1.0f);
            c.g = gmin_(c.g + (float)((tx[i][1] >> 8) & 255u) * fk, 1.0f);
            c.b = gmin_(c.b + (float)((tx[i][2] >> 16) & 255u) * fk, 1.0f);
        }
        if (yy < H && t.x0 + lane < W) out[(size_t)yy * W + x] = pack_rgb_alpha_of(tonemap<TM>(c), tM);
    }
}

// The texel sample: one pixel per lane, 64x4-pixel workgroups.
constexpr int TS_TX = 64, TS_TY = 4;
template <int TM>
__global__ __launch_bounds__(TS_TX* TS_TY) void RM_PK(rm_post_texel)(const uint32_t* __restrict__ in,
                                                                    uint32_t* __restrict__ out, int W, int H,
                                                                    int tiles_x RM_PV_ARG) {
    RM_PV(in += blockIdx.y * vs.a; out += blockIdx.y * vs.a;)  // (view blockIdx.y's frame)
    const Tile t = tile_of_block(tiles_x, TS_TX, TS_TY);
    const int x = t.x0 + (threadIdx.x & 63), y = t.y0 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float fx = ((float)x + 0.5f) / (float)W;
    const float fy = 1.0f - ((float)y + 0.5f) / (float)H;
    const uint32_t tM = texel(in, W, H, fx, fy);
    out[(size_t)y * W + x] = pack_rgb_alpha_of(tonemap<TM>(rgb(tM)), tM);
}


}  // namespace rm
