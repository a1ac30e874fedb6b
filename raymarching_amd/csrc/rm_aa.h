// rm_aa.h -- adaptive supersampling of an RGBA8 frame (include/rm.h
// rm_refine_rgba8, rm_render_aa_rgba8): the detect kernel, which
// applies the edge rule (rm_aa_rule.h) and queues the edge pixels, and the
// refine kernels, which render the K jittered samples of every queued pixel
// with the frame kernels' own render_pixel and overwrite the pixel with their
// mean.
//
// The refine kernels must produce the frame kernels' bits, so they are built
// in translation units of their own with the flags of the scene's frame
// kernels: rm_aa_t.hip (S0, T; rm_kernels_t.o's flags) and rm_aa_o.hip (O, OG;
// rm_kernels_o.o's).  Neither is one of the render objects: the frame kernels'
// code and rm_render_code_hash() do not change with them.
//
// Nothing waits inside a launch: detect appends to the queue (one atomic add
// per wave), the stream orders refine after it, and refine reads the count the
// detect launch left in device memory (the host never does, between the two).
//
// A scene plugin's refine kernel (rm_plugin_kernels.h rm_plugin_aa_refine, the
// AA form of the plugin's translation unit) is compiled by
// hiprtc from this header's device part: aa_sample, aa_pack, aa_inv and
// aa_refine_lane_sample, and the batch forms' batch_aa_refine_group.  Under
// __HIPCC_RTC__ everything else -- the standard
// headers, the launchers, the detect kernel and the lane = pixel layout -- is
// left out.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#endif

#include "rm_aa_rule.h"
#include "rm_batch_aa_plan.h"
#include "rm_render_direct.h"

namespace rm {

// The context's scratch buffer: the queue's count in word 0 of a 128-byte line
// of its own, then W * H words of pixel indices (y * W + x).
constexpr int kAaHeadWords = 32;

// The lanes of a refine wave.  AA_LANE_SAMPLE: lane = (queue entry, sample), K
// adjacent lanes per pixel and 64 / K pixels per wave, the samples summed with
// lane shuffles.  AA_LANE_PIXEL: lane = queue entry, a serial loop over the K
// wave-uniform jitters.  Both sum the same tree (DESIGN.md 2.20 has both
// measured); RM_AA_LAYOUT=pixel|sample selects one, read at every call so that
// tools/aa_probe.py can alternate the two in one process.
enum AaLayout : int { AA_LANE_SAMPLE = 0, AA_LANE_PIXEL = 1 };
#ifndef __HIPCC_RTC__
int aa_layout();

// rm_aa_t.hip (the detect kernel is scene-independent integer code)
hipError_t launch_aa_detect(const uint32_t* frame, int W, int H, int threshold, uint8_t* mask, uint32_t* count,
                            uint32_t* queue, hipStream_t s);
// scene S0 / T (rm_aa_t.hip), O / OG (rm_aa_o.hip); any other: hipErrorInvalidValue
hipError_t launch_aa_refine_t(int scene, const FrameConst& F, int samples, int layout, const uint32_t* count,
                              const uint32_t* queue, uint32_t* frame, hipStream_t s);
hipError_t launch_aa_refine_o(int scene, const FrameConst& F, int samples, int layout, const uint32_t* count,
                              const uint32_t* queue, uint32_t* frame, hipStream_t s);

#endif  // __HIPCC_RTC__

// the kernels' translation units (the host file takes the launchers above only), and a plugin's AA form
#if defined(RM_AA_KERNELS) || defined(__HIPCC_RTC__)

#ifndef __HIPCC_RTC__

// One wave per 8x8 tile of the frame (tile = blockIdx.x, row-major on a
// tiles_x-wide grid).  The tile's edge pixels go to the queue in lane order
// from one base: a ballot, one atomic add per wave (lane 0, a vector atomic),
// each lane's place from the ballot's bits below it.  Every pixel is appended
// at most once, so the queue's W * H words cannot overflow.
__device__ __forceinline__ void aa_detect_tile(const uint32_t* __restrict__ frame, int W, int H, int tiles_x,
                                               int threshold, uint8_t* __restrict__ mask, uint32_t* __restrict__ count,
                                               uint32_t* __restrict__ queue) {
    const int lane = threadIdx.x & 63;
    const int by = (int)blockIdx.x / tiles_x, bx = (int)blockIdx.x - by * tiles_x;
    const int x = bx * 8 + (lane & 7), y = by * 8 + (lane >> 3);
    const bool in = x < W && y < H;
    const bool edge = in && rmaa::edge_pixel(frame, W, H, x, y, threshold);
    if (in && mask) mask[(size_t)y * W + x] = edge ? 1 : 0;
    const uint64_t b = __builtin_amdgcn_ballot_w64(edge);
    if (b == 0) return;  // (wave-uniform)
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(b));
    base = __builtin_amdgcn_readfirstlane(base);
    if (edge) queue[base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)(y * W + x);
}

#endif  // __HIPCC_RTC__

// One sample of pixel (x, y): the frame kernels' pixel (render_tile_at,
// rm_render_direct.h; a scene plugin's: plugin_render_tile<false>,
// rm_plugin_kernels.h, whose timed form of render_pixel is 1, as in
// rm_shade.h) with the fragment moved by (ox, oy) as
// rm_render_accumulate moves it -- camera_ray reads the offset from its
// FrameConst, so it gets a copy with jit_x / jit_y set -- in the timed forms
// (the exact skips), after post_colour.
template <int SC>
__device__ __forceinline__ V3 aa_sample(const FrameConst& F, int x, int y, float ox, float oy) {
    using P = ScenePolicy<SC>;
    FrameConst G = F;  // (only camera_ray reads it: scalars, no table)
    G.jit_x = ox;
    G.jit_y = oy;
    float tcx, tcy;
    V3 ro, rd;
    camera_ray<P::kHwMath>(G, x, y, tcx, tcy, ro, rd);
    const float vig = vignette(tcx, tcy);
    Tally cnt;
    V3 c;
    if constexpr (SC == SCENE_T) c = render_pixel<SC, 3, 1, 1>(F, ro, rd, cnt);
    else c = render_pixel<SC, 3, (P::kSettleO || SC == SCENE_PLUGIN) ? 1 : 0>(F, ro, rd, cnt);
    return post_colour<P::kTrim>(c, vig);
}

template <int SC>
__device__ __forceinline__ uint32_t aa_pack(V3 c) {
    return ScenePolicy<SC>::kTrim ? pack_rgb8_opaque(c.x, c.y, c.z) : pack_rgba8(c.x, c.y, c.z, 1.0f);
}

// 1 / K of K = 1 << kshift
__device__ __forceinline__ float aa_inv(int kshift) { return kshift == 1 ? 0.5f : kshift == 2 ? 0.25f : 0.125f; }

// Persistent one-wave workgroups striding over the queue up to the count in
// device memory.  The mean of a pixel's samples is the pairwise tree in sample
// order, ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)), times 1 / K, in f32
// without contraction: rm_aa_rule.h's order, which the host restatement
// (tests/aa_ref.py) sums too.
//
// AA_LANE_SAMPLE: the K lanes of a pixel are adjacent, so the tree is log2 K
// xor-shuffles (an add is commutative: every lane of the pixel ends with the
// same sum); the pixel's first lane stores.  The shuffles run outside the
// branch of the active lanes; the K lanes of an entry are active together.
template <int SC>
__device__ __forceinline__ void aa_refine_lane_sample(const FrameConst& F, int kshift,
                                                      const uint32_t* __restrict__ count,
                                                      const uint32_t* __restrict__ queue, uint32_t* __restrict__ frame) {
    const int lane = threadIdx.x & 63;
    const uint32_t n = *count;
    const int K = 1 << kshift;
    const uint32_t ppw = 64u >> kshift;  // pixels per wave
    const int sample = lane & (K - 1);
    float ox, oy;
    rmaa::sample_offset(K, sample, ox, oy);
    for (uint32_t g = blockIdx.x; g * ppw < n; g += gridDim.x) {  // (n < 2^30: no wrap)
        const uint32_t e = g * ppw + (uint32_t)(lane >> kshift);
        const bool active = e < n;
        uint32_t pix = 0;
        V3 c = v3s(0.0f);
        if (active) {
            pix = queue[e];
            const int y = (int)(pix / (uint32_t)F.W), x = (int)(pix - (uint32_t)y * (uint32_t)F.W);
            c = aa_sample<SC>(F, x, y, ox, oy);
        }
        float sx = c.x, sy = c.y, sz = c.z;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int o = 1; o < rmaa::kMaxSamples; o <<= 1) {
                if (o < K) {  // (wave-uniform)
                    const float tx = __shfl_xor(sx, o, 64), ty = __shfl_xor(sy, o, 64), tz = __shfl_xor(sz, o, 64);
                    sx = sx + tx;
                    sy = sy + ty;
                    sz = sz + tz;
                }
            }
            const float inv = aa_inv(kshift);
            sx = sx * inv;
            sy = sy * inv;
            sz = sz * inv;
        }
        if (active && sample == 0) frame[pix] = aa_pack<SC>(v3(sx, sy, sz));
    }
}

// One refine group of a view batch (rm_batch_aa.h; a scene plugin's batch-AA
// form, rm_plugin_kernels.h rm_plugin_batch_aa_refine): entries gl * ppw .. of a
// view's queue segment, lane = (entry, sample).  aa_refine_lane_sample's loop
// body with the view's constants, count, queue and frame.
template <int SC>
__device__ __forceinline__ void batch_aa_refine_group(const FrameConst& G, int kshift, uint32_t count, uint32_t gl,
                                                      const uint32_t* __restrict__ queue,
                                                      uint32_t* __restrict__ frame, float ox, float oy) {
    const int lane = threadIdx.x & 63;
    const int K = 1 << kshift;
    const uint32_t e = gl * rmbaa::group_entries(kshift) + (uint32_t)(lane >> kshift);
    const bool active = e < count;
    uint32_t pix = 0;
    V3 c = v3s(0.0f);
    if (active) {
        pix = queue[e];
        const int y = (int)(pix / (uint32_t)G.W), x = (int)(pix - (uint32_t)y * (uint32_t)G.W);
        c = aa_sample<SC>(G, x, y, ox, oy);
    }
    float sx = c.x, sy = c.y, sz = c.z;
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int o = 1; o < rmaa::kMaxSamples; o <<= 1) {
            if (o < K) {  // (wave-uniform)
                const float tx = __shfl_xor(sx, o, 64), ty = __shfl_xor(sy, o, 64), tz = __shfl_xor(sz, o, 64);
                sx = sx + tx;
                sy = sy + ty;
                sz = sz + tz;
            }
        }
        const float inv = aa_inv(kshift);
        sx = sx * inv;
        sy = sy * inv;
        sz = sz * inv;
    }
    if (active && (lane & (K - 1)) == 0) frame[pix] = aa_pack<SC>(v3(sx, sy, sz));
}

#ifndef __HIPCC_RTC__
// AA_LANE_PIXEL: the samples of a pixel one after the other on its lane; the
// tree as a binary counter over three partial sums (sample k closes the
// subtrees its low one bits name).
template <int SC>
__device__ __forceinline__ void aa_refine_lane_pixel(const FrameConst& F, int kshift,
                                                     const uint32_t* __restrict__ count,
                                                     const uint32_t* __restrict__ queue, uint32_t* __restrict__ frame) {
    const int lane = threadIdx.x & 63;
    const uint32_t n = *count;
    const int K = 1 << kshift;
    for (uint32_t g = blockIdx.x; g * 64u < n; g += gridDim.x) {
        const uint32_t e = g * 64u + (uint32_t)lane;
        if (e >= n) continue;
        const uint32_t pix = queue[e];
        const int y = (int)(pix / (uint32_t)F.W), x = (int)(pix - (uint32_t)y * (uint32_t)F.W);
        float p0x = 0.0f, p0y = 0.0f, p0z = 0.0f, p1x = 0.0f, p1y = 0.0f, p1z = 0.0f, p2x = 0.0f, p2y = 0.0f, p2z = 0.0f;
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll 1
        for (int k = 0; k < K; k++) {
            float ox, oy;
            rmaa::sample_offset(K, k, ox, oy);  // (wave-uniform)
            const V3 c = aa_sample<SC>(F, x, y, ox, oy);
            {
#pragma clang fp contract(off)
                sx = c.x; sy = c.y; sz = c.z;
                if (k & 1) {
                    sx = p0x + sx; sy = p0y + sy; sz = p0z + sz;
                    if (k & 2) {
                        sx = p1x + sx; sy = p1y + sy; sz = p1z + sz;
                        if (k & 4) {
                            sx = p2x + sx; sy = p2y + sy; sz = p2z + sz;
                        } else {
                            p2x = sx; p2y = sy; p2z = sz;
                        }
                    } else {
                        p1x = sx; p1y = sy; p1z = sz;
                    }
                } else {
                    p0x = sx; p0y = sy; p0z = sz;
                }
            }
        }
        {
#pragma clang fp contract(off)
            const float inv = aa_inv(kshift);
            sx = sx * inv;
            sy = sy * inv;
            sz = sz * inv;
        }
        frame[pix] = aa_pack<SC>(v3(sx, sy, sz));
    }
}

// (the frame kernels' register budget: ScenePolicy<SC>::kWavesPerEU)
template <int SC, int LAYOUT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ScenePolicy<SC>::kWavesPerEU)))
void rm_aa_refine(FrameConst F, int kshift, const uint32_t* __restrict__ count, const uint32_t* __restrict__ queue,
                  uint32_t* __restrict__ frame) {
    if constexpr (LAYOUT == AA_LANE_SAMPLE) aa_refine_lane_sample<SC>(F, kshift, count, queue, frame);
    else aa_refine_lane_pixel<SC>(F, kshift, count, queue, frame);
}

// The grid is fixed from the device, as launch_persist's (rm_kernels_impl.h):
// as many one-wave workgroups as the device holds at once.
template <int SC, int LAYOUT>
hipError_t launch_aa_refine_as(const FrameConst& F, int samples, const uint32_t* count, const uint32_t* queue,
                               uint32_t* frame, hipStream_t s) {
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rm_aa_refine<SC, LAYOUT>, 64, 0);
    if (e != hipSuccess) return e;
    const int waves = std::max(1, cus * std::max(per_cu, 1));
    hipLaunchKernelGGL((rm_aa_refine<SC, LAYOUT>), dim3(waves), dim3(64), 0, s, F, rmaa::samples_shift(samples), count,
                       queue, frame);
    return hipGetLastError();
}

template <int SC>
hipError_t launch_aa_refine_scene(const FrameConst& F, int samples, int layout, const uint32_t* count,
                                  const uint32_t* queue, uint32_t* frame, hipStream_t s) {
    if (!rmaa::samples_ok(samples)) return hipErrorInvalidValue;
    if (layout == AA_LANE_PIXEL) return launch_aa_refine_as<SC, AA_LANE_PIXEL>(F, samples, count, queue, frame, s);
    return launch_aa_refine_as<SC, AA_LANE_SAMPLE>(F, samples, count, queue, frame, s);
}

#endif  // __HIPCC_RTC__

#endif  // RM_AA_KERNELS || __HIPCC_RTC__

}  // namespace rm
