// rm_batch_aa.h -- adaptive supersampling of every view of a batch (include/rm.h
// rm_refine_batch_rgba8, rm_render_batch_aa_rgba8): three launches
// for n frames of W x H, with no host round trip between them.
//   detect  one wave per 8x8 tile of one view (blockIdx.y): rm_aa.h's
//           aa_detect_tile on the view's frame, mask, counter and queue segment
//   plan    one workgroup: the exclusive prefix of the views' group counts, the
//           totals, and the per-view counts for the caller (rm_batch_aa_plan.h)
//   refine  persistent one-wave workgroups striding over the global group
//           indices; a group lies in one view, which the wave finds from the
//           prefix table at a wave-uniform address, so the view's constants are
//           scalar operands as the frame kernels' are (a wave never mixes views)
// A refined pixel is rm_aa.h's: aa_sample per (entry, sample) lane, the pairwise
// tree by xor-shuffles, aa_pack; rm_refine_rgba8's bytes for the view's pose.
//
// The view records are rm_batch.h's (ViewConst put into a copy of the launch's
// FrameConst for scenes S0/T, the view's whole FrameConst in place for O/OG),
// and the translation units take the flags of the scene's frame kernels as
// rm_aa_*.hip do: rm_batch_aa_t.hip (S0, T, and the integer detect and plan
// kernels) and rm_batch_aa_o.hip (O, OG).  Neither is one of the render objects.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rm_aa.h"
#include "rm_batch.h"
#include "rm_batch_aa_plan.h"

namespace rm {

// the counters' stride in words (rmbaa::kCountersPacked or kCountersLine): RM_BATCH_AA_COUNTERS=packed|line,
// read at every call so that tools/batch_aa_probe.py can alternate the two in one process
uint32_t batch_aa_counter_stride();

// scratch: the context's buffer (rmbaa::layout); frames, mask (or null): n frames of W x H
hipError_t launch_batch_aa_detect(const uint32_t* frames, int W, int H, int n, int threshold, uint8_t* mask,
                                  uint32_t* counters, uint32_t cstride, uint32_t* queue, hipStream_t s);
// prefix: n + 2 words; refined: n words in device memory, or null
hipError_t launch_batch_aa_plan(const uint32_t* counters, uint32_t cstride, int n, int samples, uint32_t* prefix,
                                uint32_t* refined, hipStream_t s);
// F, views: as launch_batch_t / launch_batch_o take them (rm_batch.h)
// scene S0 / T (rm_batch_aa_t.hip), O / OG (rm_batch_aa_o.hip); any other: hipErrorInvalidValue
hipError_t launch_batch_aa_refine_t(int scene, const FrameConst& F, const void* views, int n, int samples,
                                    const uint32_t* counters, uint32_t cstride, const uint32_t* prefix,
                                    const uint32_t* queue, uint32_t* frames, hipStream_t s);
hipError_t launch_batch_aa_refine_o(int scene, const FrameConst& F, const void* views, int n, int samples,
                                    const uint32_t* counters, uint32_t cstride, const uint32_t* prefix,
                                    const uint32_t* queue, uint32_t* frames, hipStream_t s);

#ifdef RM_BATCH_AA_KERNELS  // the kernels' translation units (they define RM_AA_KERNELS too)

// (one refine group, batch_aa_refine_group: rm_aa.h's device part, which a scene plugin's batch-AA form shares)

// Scenes S0 / T: the launch's FrameConst with the view's short record put in,
// as rm_batch.h's rm_render_batch does.  The record's address is wave-uniform
// (v comes from blockIdx and scalar loads of the prefix table).
template <int SC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ScenePolicy<SC>::kWavesPerEU)))
void rm_batch_aa_refine(FrameConst F, const ViewConst* __restrict__ views, uint32_t n, int kshift,
                        const uint32_t* __restrict__ counters, uint32_t cstride, const uint32_t* __restrict__ prefix,
                        const uint32_t* __restrict__ queue, uint32_t* __restrict__ frames) {
    const uint32_t total = prefix[n];
    const size_t px = (size_t)F.W * (size_t)F.H;
    float ox, oy;
    rmaa::sample_offset(1 << kshift, (int)(threadIdx.x & 63u) & ((1 << kshift) - 1), ox, oy);
    for (uint32_t g = blockIdx.x; g < total; g += gridDim.x) {
        const uint32_t vi = (uint32_t)__builtin_amdgcn_readfirstlane((int)rmbaa::view_of_group(prefix, n, g));
        const ViewConst& v = views[vi];
        FrameConst G = F;
        G.pos_x = v.pos_x; G.pos_y = v.pos_y; G.pos_z = v.pos_z;
        G.cam1_c = v.cam1_c; G.cam1_s = v.cam1_s; G.cam2_c = v.cam2_c; G.cam2_s = v.cam2_s;
        G.ry_c = v.ry_c; G.ry_s = v.ry_s; G.rx_c = v.rx_c; G.rx_s = v.rx_s;
        G.camq_x = v.camq_x; G.camq_y = v.camq_y; G.camq_z = v.camq_z;
        G.time = v.time; G.mouse_x = v.mouse_x; G.mouse_y = v.mouse_y;
        batch_aa_refine_group<SC>(G, kshift, counters[(size_t)vi * cstride], g - prefix[vi], queue + vi * px,
                                  frames + vi * px, ox, oy);
    }
}

// Scenes O / OG: the view's whole FrameConst where it lies (rm_batch.h batch_whole_record).
template <int SC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ScenePolicy<SC>::kWavesPerEU)))
void rm_batch_aa_refine_whole(const FrameConst* __restrict__ views, uint32_t n, int kshift,
                              const uint32_t* __restrict__ counters, uint32_t cstride,
                              const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ queue,
                              uint32_t* __restrict__ frames) {
    const uint32_t total = prefix[n];
    float ox, oy;
    rmaa::sample_offset(1 << kshift, (int)(threadIdx.x & 63u) & ((1 << kshift) - 1), ox, oy);
    for (uint32_t g = blockIdx.x; g < total; g += gridDim.x) {
        const uint32_t vi = (uint32_t)__builtin_amdgcn_readfirstlane((int)rmbaa::view_of_group(prefix, n, g));
        const FrameConst& G = views[vi];
        const size_t px = (size_t)G.W * (size_t)G.H;
        batch_aa_refine_group<SC>(G, kshift, counters[(size_t)vi * cstride], g - prefix[vi], queue + vi * px,
                                  frames + vi * px, ox, oy);
    }
}

// The grid is fixed from the device, as launch_aa_refine_as's (rm_aa.h).
template <int SC>
hipError_t launch_batch_aa_refine_scene(const FrameConst& F, const void* views, int n, int samples,
                                        const uint32_t* counters, uint32_t cstride, const uint32_t* prefix,
                                        const uint32_t* queue, uint32_t* frames, hipStream_t s) {
    if (!rmaa::samples_ok(samples) || !batch_size_ok(F.W, F.H, n) || (int64_t)F.W * F.H >= rmaa::kMaxPixels ||
        (cstride != rmbaa::kCountersPacked && cstride != rmbaa::kCountersLine))
        return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    constexpr bool whole = SC == SCENE_O || SC == SCENE_OG;  // (batch_whole_record)
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if constexpr (whole) {
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rm_batch_aa_refine_whole<SC>, 64, 0);
    } else {
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rm_batch_aa_refine<SC>, 64, 0);
    }
    if (e != hipSuccess) return e;
    const int waves = std::max(1, cus * std::max(per_cu, 1));
    const int kshift = rmaa::samples_shift(samples);
    if constexpr (whole)
        hipLaunchKernelGGL((rm_batch_aa_refine_whole<SC>), dim3(waves), dim3(64), 0, s,
                           static_cast<const FrameConst*>(views), (uint32_t)n, kshift, counters, cstride, prefix, queue,
                           frames);
    else
        hipLaunchKernelGGL((rm_batch_aa_refine<SC>), dim3(waves), dim3(64), 0, s, F,
                           static_cast<const ViewConst*>(views), (uint32_t)n, kshift, counters, cstride, prefix, queue,
                           frames);
    return hipGetLastError();
}

#endif  // RM_BATCH_AA_KERNELS

}  // namespace rm
