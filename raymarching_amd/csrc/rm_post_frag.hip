// rm_post_frag.hip -- post.frag's main() (:135-144) with the sample its one
// statement takes generalised to the other two a user of the reference picks
// by editing it:
//   texel      color = texture(u_main_tex, uv)
//   chromatic  color = vec4(chromaticAberration(u_main_tex, uv), texture(u_main_tex, uv).a)
// followed by one of post.frag's tonemap operators (rm_post_tonemap.h) and the
// RGBA8 store.  (The FXAA sample is rm_fxaa.hip's kernel with the same
// epilogue.)  The sampler is rm_fxaa's: NEAREST, CLAMP_TO_EDGE, texel index
// clamp(floor(u W)) in float, uv = (tc.x, 1 - tc.y) with the exact pixel-centre
// tc, so the output is the input flipped vertically.
//
// Built with rm_post.o's flags: no FMA contraction, correctly rounded
// division, so the float path equals tests/post_frag_ref.py bit for bit.
//
// chromaticAberration (post.frag:113-131) is 8 steps of one tap per channel at
// 0.5 - 0.5 ((1 - 2 UV) k) for the channel's factor k: a scaling about the frame
// centre by k, with k running 1 .. 0.9806 (red), 1 .. 0.9861 (green) and
// 1 .. 1.0084 (blue).  A tap's column depends on the pixel's column only and
// its row on the pixel's row only, and nothing depends on a loaded value, so
// the taps are plain global loads, all in flight at once; along a wave's
// 64-pixel row a tap's texels are a shifted, almost contiguous row (the
// displacement changes by about one texel across it): about one cache line
// per tap and wave, served by the TCP / L2.  Staging the tile's tap bounding
// box in LDS instead measured 2.5 times slower.
#include "rm_post_common.h"
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
__global__ __launch_bounds__(64 * CA_NW) void rm_post_chromatic_kernel(const uint32_t* __restrict__ in,
                                                                       uint32_t* __restrict__ out, int W, int H,
                                                                       int tiles_x) {
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
__global__ __launch_bounds__(TS_TX* TS_TY) void rm_post_texel_kernel(const uint32_t* __restrict__ in,
                                                                    uint32_t* __restrict__ out, int W, int H,
                                                                    int tiles_x) {
    const Tile t = tile_of_block(tiles_x, TS_TX, TS_TY);
    const int x = t.x0 + (threadIdx.x & 63), y = t.y0 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float fx = ((float)x + 0.5f) / (float)W;
    const float fy = 1.0f - ((float)y + 0.5f) / (float)H;
    const uint32_t tM = texel(in, W, H, fx, fy);
    out[(size_t)y * W + x] = pack_rgb_alpha_of(tonemap<TM>(rgb(tM)), tM);
}

hipError_t launch_post_frag(const uint32_t* in, uint32_t* out, int W, int H, int sample, int tonemap, hipStream_t s) {
    if (W <= 0 || H <= 0) return hipSuccess;
    if (sample == kSampleFxaa) return launch_fxaa_tonemap(in, out, W, H, tonemap, s);
    if (sample != kSampleTexel && sample != kSampleChromatic) return hipErrorInvalidValue;
    const bool chroma = sample == kSampleChromatic;
    const int tiles_x = (W + (chroma ? CA_TX : TS_TX) - 1) / (chroma ? CA_TX : TS_TX);
    const int tiles_y = (H + (chroma ? CA_TY : TS_TY) - 1) / (chroma ? CA_TY : TS_TY);
    const dim3 grid((unsigned)(tiles_x * tiles_y)), block(256);
    static_assert(64 * CA_NW == 256 && TS_TX * TS_TY == 256, "block size");
    return with_tonemap(tonemap, [&](auto tm) {
        constexpr int TM = decltype(tm)::value;
        if (chroma) hipLaunchKernelGGL(rm_post_chromatic_kernel<TM>, grid, block, 0, s, in, out, W, H, tiles_x);
        else hipLaunchKernelGGL(rm_post_texel_kernel<TM>, grid, block, 0, s, in, out, W, H, tiles_x);
        return hipGetLastError();
    });
}

}  // namespace rm
