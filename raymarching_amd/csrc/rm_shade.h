// rm_shade.h -- rm_shade_rays (include/rm.h): the pass's colour,
// render(ro, rd) of output_shader.frag:348-385 and template.frag:45-76, along
// caller-supplied rays, one lane per ray.
//
// Each lane calls the frame kernels' own render_pixel in the timed forms (the
// exact skips), as the refine kernels of rm_aa.h do, then main()'s tonemap ->
// contrast (-> vignette) when the display colour is asked for, and stores with
// the scene's pack.  The kernels must give the frame kernels' bits, so the
// built-in scenes' are built in translation units of their own with the flags
// of the scene's frame kernels: rm_shade_t.hip (S0, T; rm_kernels_t.o's flags)
// and rm_shade_o.hip (O, OG; rm_kernels_o.o's).  Neither is one of the render
// objects: rm_render_code_hash() does not change with them.  A scene plugin's
// kernel is rm_plugin_shade (rm_plugin_kernels.h).
//
// Layout: origins and directions are tightly packed xyz triples, read as
// rm_rays.h reads them (three dwords per lane at stride 12 B, no LDS staging).
// Two lane layouts: a ray image of `width` columns is shaded in 8x8 tiles, one
// wave per tile, lane -> pixel as render_tile_at's; a list puts 64 consecutive
// rays in a wave.
//
// The render kernels' shortcuts rest on unit rays with finite components, so
// each lane tests its own ray before anything is marched (shade_ray_ok); a
// rejected ray stores zeros and no loop ever sees it.  Nothing indexes memory
// by ray data.
#pragma once
#include "rm_render_direct.h"

namespace rm {

// One launch's rays and target (device pointers).
struct ShadeRays {
    const float* origins;     // n xyz triples, or null: every ray starts at the launch's u_pos (F.pos_*)
    const float* directions;  // n xyz triples, unit length
    long long n;
    int width;        // > 0: a width x (n / width) ray image in 8x8 tiles; 0: a list
    int display;      // 0: render()'s colour; 1: post_colour of it
    int vignette;     // display, width > 0: pixel (x, y)'s vignette for F.W = width, F.H = n / width; else factor 1
    float4* rgba;     // n, alpha 1; or
    uint32_t* rgba8;  // n words of the scene's pack (display only)
};

// |d|^2 within 1e-4 of 1 and every component finite (a NaN or an infinity fails
// the comparisons)
__device__ __forceinline__ bool shade_ray_ok(V3 ro, V3 rd) {
    const float big = 3.0e38f;
    const bool o = fabsf(ro.x) <= big && fabsf(ro.y) <= big && fabsf(ro.z) <= big;
    const float d2 = rd.x * rd.x + rd.y * rd.y + rd.z * rd.z;
    return o && fabsf(d2 - 1.0f) <= 1.0e-4f;
}

// render(ro, rd) in the timed forms of the scene's frame kernel (render_tile_at,
// plugin_render_tile).  OWN: the ray has an origin of its own, which scene T's
// primary march takes in sponge space per lane: sponge_space<false>, the form
// camera_sponge_origin (rm_device.h) mirrors on the host for u_pos.
template <int SC, bool OWN>
__device__ __forceinline__ V3 shade_render(const FrameConst& F, V3 ro, V3 rd, Tally& cnt) {
    using P = ScenePolicy<SC>;
    if constexpr (SC == SCENE_T) {
        if constexpr (OWN) {
            const LinRay prim{sponge_space<false>(F, ro), sponge_rot<P::kExactMarch>(F, rd.x, rd.y, rd.z)};
            return render_T_from<3, 1, 1>(F, prim, ro, rd, cnt);
        } else {
            return render_pixel<SC, 3, 1, 1>(F, ro, rd, cnt);
        }
    } else {
        return render_pixel<SC, 3, (P::kSettleO || SC == SCENE_PLUGIN) ? 1 : 0>(F, ro, rd, cnt);
    }
}

template <int SC>
__device__ __forceinline__ uint32_t shade_pack(V3 c) {  // (store_pixel's rule)
    return ScenePolicy<SC>::kTrim ? pack_rgb8_opaque(c.x, c.y, c.z) : pack_rgba8(c.x, c.y, c.z, 1.0f);
}

// The body of a shade launch of one-wave workgroups.  TILED: workgroup
// blockIdx.x is tile (bx, by) of the ray image, row-major on a ceil(width / 8)
// wide grid, ragged right and bottom tiles masked; else ray blockIdx.x * 64 +
// lane.  OWN: Q.origins holds an origin per ray.  Each is 0, 1, or
// SHADE_PER_LAUNCH: read from Q (wave-uniform), for the scene plugins' one kernel.
constexpr int SHADE_PER_LAUNCH = -1;
template <int SC, int TILED, int OWN>
__device__ __forceinline__ void shade_rays_one(const FrameConst& F, const ShadeRays& Q) {
    using P = ScenePolicy<SC>;
    static_assert(SC != SCENE_T || OWN >= 0, "scene T's primary ray is built at compile time");
    const bool tiled = TILED < 0 ? Q.width > 0 : TILED != 0;
    const bool own = OWN < 0 ? Q.origins != nullptr : OWN != 0;
    const int lane = threadIdx.x & 63;
    long long i;
    int x = 0, y = 0;
    if (tiled) {
        const int gx = (Q.width + 7) >> 3;
        const int by = (int)(blockIdx.x / (unsigned)gx), bx = (int)(blockIdx.x - (unsigned)by * (unsigned)gx);
        x = bx * 8 + (lane & 7);
        y = by * 8 + (lane >> 3);
        i = (long long)y * Q.width + x;
        if (x >= Q.width) return;
    } else {
        i = (long long)blockIdx.x * 64 + lane;
    }
    if (i >= Q.n) return;
    const V3 rd = v3(Q.directions[3 * i], Q.directions[3 * i + 1], Q.directions[3 * i + 2]);
    V3 ro = v3(F.pos_x, F.pos_y, F.pos_z);
    if (own) ro = v3(Q.origins[3 * i], Q.origins[3 * i + 1], Q.origins[3 * i + 2]);
    if (!shade_ray_ok(ro, rd)) {
        if (Q.rgba8) Q.rgba8[i] = 0u;
        else Q.rgba[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float vig = 1.0f;  // (vignette(0.5, 0.5))
    if (tiled && Q.vignette) {  // (wave-uniform) the frame's texcoords; the ray camera_ray builds is not used
        float tcx, tcy;
        V3 o_, d_;
        camera_ray<P::kHwMath>(F, x, y, tcx, tcy, o_, d_);
        vig = vignette(tcx, tcy);
    }
    Tally cnt;
    V3 c = shade_render<SC, OWN == 1>(F, ro, rd, cnt);
    if (Q.display) c = post_colour<P::kTrim>(c, vig);  // (wave-uniform)
    if (Q.rgba8) Q.rgba8[i] = shade_pack<SC>(c);
    else Q.rgba[i] = make_float4(c.x, c.y, c.z, 1.0f);
}

// a launch's grid of one-wave workgroups (n <= 2^30: at most 2^27 tiles of a
// one-column image, 2^24 waves of a list)
__host__ inline unsigned shade_grid(const ShadeRays& Q) {
    if (Q.width > 0) return (unsigned)((Q.width + 7) / 8) * (unsigned)((Q.n / Q.width + 7) / 8);
    return (unsigned)((Q.n + 63) / 64);
}

#ifndef __HIPCC_RTC__
// scene S0 / T (rm_shade_t.hip), O / OG (rm_shade_o.hip); any other: hipErrorInvalidValue
hipError_t launch_shade_rays_t(int scene, const FrameConst& F, const ShadeRays& Q, hipStream_t s);
hipError_t launch_shade_rays_o(int scene, const FrameConst& F, const ShadeRays& Q, hipStream_t s);
// rm_shade_t.hip: rm_camera_rays' kernel for the scenes whose frame kernels use
// the hardware forms (S0, T), under their flags, so that these rays are the
// frame's own in every bit
hipError_t launch_camera_rays_hw(const FrameConst& F, float* origin3, float* directions, hipStream_t s);

#ifdef RM_SHADE_KERNELS  // the kernels' translation units (the host file takes the launchers above only)

// (the frame kernels' register budget: ScenePolicy<SC>::kWavesPerEU)
template <int SC, int TILED, int OWN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ScenePolicy<SC>::kWavesPerEU)))
void rm_shade_rays_kernel(FrameConst F, ShadeRays Q) {
    shade_rays_one<SC, TILED, OWN>(F, Q);
}

template <int SC>
hipError_t launch_shade_scene(const FrameConst& F, const ShadeRays& Q, hipStream_t s) {
    if (Q.n <= 0) return hipSuccess;
    const dim3 grid(shade_grid(Q)), block(64);
    const bool own = Q.origins != nullptr;
    if (Q.width > 0) {
        if (own) hipLaunchKernelGGL((rm_shade_rays_kernel<SC, 1, 1>), grid, block, 0, s, F, Q);
        else hipLaunchKernelGGL((rm_shade_rays_kernel<SC, 1, 0>), grid, block, 0, s, F, Q);
    } else {
        if (own) hipLaunchKernelGGL((rm_shade_rays_kernel<SC, 0, 1>), grid, block, 0, s, F, Q);
        else hipLaunchKernelGGL((rm_shade_rays_kernel<SC, 0, 0>), grid, block, 0, s, F, Q);
    }
    return hipGetLastError();
}

#endif  // RM_SHADE_KERNELS
#endif  // __HIPCC_RTC__

}  // namespace rm
