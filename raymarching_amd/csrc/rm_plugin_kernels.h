// rm_plugin_kernels.h -- epilogue of a scene plugin's translation unit
// (rm_plugin.h): binds the scene's sceneSDF to the render pipeline and defines
// the plugin's kernels, looked up by name (rm_plugin_host.cpp).  The first
// argument of every kernel is the FrameConst the uniforms are bound from; a
// scene that declares uniforms of its own has their block as the second
// (rm_plugin.h UniformBlock: read from the kernel-argument segment, so the
// parameter itself is never named), loaded once at the top of each kernel.
#pragma once
#include "rm_rays.h"
#include "rm_shade.h"
#if defined(RM_PLUGIN_AA) || defined(RM_PLUGIN_BATCH_AA)
#include "rm_aa.h"
#endif

#ifdef RM_UNIFORM_SLOTS
#define RM_UNIFORM_PARAM rm::glsl::UniformBlock,
#else
#define RM_UNIFORM_PARAM
#define RM_UNIFORM_PRELOAD()
#endif

template <>
struct rm::PluginScene<rm::SCENE_PLUGIN> {
#ifdef RM_SCENE_FLOP
    static constexpr uint32_t flop = RM_SCENE_FLOP;  // per-ray-step FLOP, when the scene states it
#else
    static constexpr uint32_t flop = 0;
#endif
    __device__ __forceinline__ static float dist(rm::V3 p) { return rm::glsl::sceneSDF(p).dist; }
    // the probe form: the scene compiled against the library's probe instance
    __device__ __forceinline__ static float dist_probe(rm::V3 p) { return rm::glsl::probe::sceneSDF(p).dist; }
    __device__ __forceinline__ static rm::Mat mat(rm::V3 p) { return rm::glsl::sceneSDF(p).mat; }
    // the probe instance's material: rm_plugin_eval_probe alone reads it (renders shade with mat)
    __device__ __forceinline__ static rm::Mat mat_probe(rm::V3 p) { return rm::glsl::probe::sceneSDF(p).mat; }
};

#ifndef RM_PLUGIN_EVAL_ONLY
// output_shader.frag's pass over 8x8-pixel one-wave tiles, as two kernels: the
// timed one (rm_plugin_render) and the instrumented one (rm_plugin_render_count:
// ray-step tallies and step maps).  One kernel serving both paid the
// instrumented pipeline's registers in every timed launch (occupancy 5).  The
// output format is a run-time argument.
namespace rm {
template <bool COUNT>
__device__ __forceinline__ void plugin_render_tile(const FrameConst& F, void* out, int rgba8,
                                                   unsigned long long* evals) {
    using P = ScenePolicy<SCENE_PLUGIN>;
    const uint64_t t_start = F.tile_cost ? clock64() : 0;
    const int lane = threadIdx.x;
    int bx = blockIdx.x, by = blockIdx.y;
    if (F.tile_order) {  // costliest tiles first (rm_params.schedule, rm_set_tile_order; as render_tile_at)
        const uint32_t t = F.tile_order[by * gridDim.x + bx];
        by = div_by((int)t, F.gx_magic, (int)gridDim.x);
        bx = (int)t - by * (int)gridDim.x;
    }
    const int x = bx * 8 + (lane & 7), j = by * 8 + (lane >> 3);
    Tally cnt;
    if (x < F.W && j < F.nrows) {
        const int y = shard_row(F, F.row0 + j);
        float tcx, tcy;
        V3 ro, rd;
        camera_ray<P::kHwMath>(F, x, y, tcx, tcy, ro, rd);
        const float vig = vignette(tcx, tcy);
        // the exact skips of scene O's pipeline that hold for any scene (the soft
        // shadows of points facing away from the light): taken
        // by the timed launches, counted by the instrumented ones
        V3 c = render_pixel<SCENE_PLUGIN, 3, COUNT ? 2 : 1>(F, ro, rd, cnt);
        c = post_colour<P::kTrim>(c, vig);
        const size_t i = (size_t)j * F.W + x;
        if (rgba8) store_pixel<P::kTrim>(F, static_cast<uint32_t*>(out), i, c);
        else store_pixel<P::kTrim>(F, static_cast<float4*>(out), i, c);
    }
    if (F.tile_cost && lane == 0) F.tile_cost[by * gridDim.x + bx] = tile_clocks(t_start);
    if constexpr (COUNT) store_tally(F, evals, cnt, x, j, lane);
}
}  // namespace rm
#ifdef RM_PLUGIN_BATCH
// The batch form of the translation unit (rm_plugin.h; include/rm.h rm_render_batch_ex) has this
// kernel alone: one 8x8 wave tile of view blockIdx.z, by the timed kernel's own code, with F bound to the view's
// record -- which the scene's functions read through rm_plugin.h's accessors, so `records` is named here only to
// be the first parameter.  The pass's uniforms a scene may read, and the scene's own, are loaded at the top (as
// RM_UNIFORM_PRELOAD's are in the frame form), so that their reads inside the march loops are copies of these.
extern "C" __global__ __launch_bounds__(64) void rm_plugin_render_batch(const void* records, void* out, int rgba8) {
    const rm::glsl::KernargFrame K = rm::glsl::plugin_frame();
    asm volatile("" ::"s"(K->time), "s"(K->pos_x), "s"(K->pos_y), "s"(K->pos_z), "s"(K->mouse_x), "s"(K->mouse_y),
                 "s"(K->res_x), "s"(K->res_y));
    RM_UNIFORM_PRELOAD();
    const rm::FrameConst& G = *(const rm::FrameConst*)K;
    // what every record of a batch holds (rm_batch.h launch_batch_scene's rule, which rm_batch_host.cpp's
    // records keep): no dispatch order, no tile durations, no accumulation -- said here so that those paths of
    // plugin_render_tile are not compiled in
    __builtin_assume(G.tile_order == nullptr);
    __builtin_assume(G.tile_cost == nullptr);
    __builtin_assume(G.accumulate == 0);
    const size_t frame = (size_t)G.W * (size_t)G.H * (rgba8 ? sizeof(uint32_t) : sizeof(float4));
    rm::plugin_render_tile<false>(G, static_cast<char*>(out) + (size_t)blockIdx.z * frame, rgba8, nullptr);
}
#elif defined(RM_PLUGIN_AA)
// The AA form of the translation unit (include/rm.h rm_refine_ex_rgba8) has this kernel alone:
// rm_aa.h's refine in the lane = (queue entry, sample) layout -- one-wave workgroups striding over the queue of
// edge pixels the compiled-in detect kernel left, each sample the timed kernel's pixel (aa_sample calls what
// plugin_render_tile<false> calls) with the fragment moved by the lane's offset.  F and the uniform block are the
// first two parameters, where the scene's functions read them (rm_plugin.h).
extern "C" __global__ __launch_bounds__(64) void rm_plugin_aa_refine(rm::FrameConst F, RM_UNIFORM_PARAM int kshift,
                                                                     const uint32_t* count, const uint32_t* queue,
                                                                     uint32_t* frame) {
    RM_UNIFORM_PRELOAD();
    rm::aa_refine_lane_sample<rm::SCENE_PLUGIN>(F, kshift, count, queue, frame);
}
#elif defined(RM_PLUGIN_BATCH_AA)
// The batch-AA form of the translation unit (include/rm.h rm_refine_batch_ex_rgba8) has this
// kernel alone: the refine of every view of a batch.  A scene's functions find their view's record from the
// workgroup's index alone (rm_plugin.h plugin_bytes), so a workgroup serves one view, blockIdx.z, as in the batch
// form: gridDim.x one-wave workgroups per view stride over the groups of that view's queue segment, each group
// rm_aa.h's batch_aa_refine_group, the body of the compiled-in batch kernels.  No workgroup waits for another; the
// workgroups of a view that queued nothing leave after one scalar load.  `records` is the first parameter, where
// plugin_bytes reads it; the uniforms are loaded at the top as rm_plugin_render_batch loads them.
extern "C" __global__ __launch_bounds__(64) void rm_plugin_batch_aa_refine(const void* records, int kshift,
                                                                           const uint32_t* counters, uint32_t cstride,
                                                                           const uint32_t* queue, uint32_t* frames) {
    const uint32_t count = counters[(size_t)blockIdx.z * cstride];
    const uint32_t ppw = rmbaa::group_entries(kshift);
    if ((uint32_t)blockIdx.x * ppw >= count) return;  // (wave-uniform: before any record is read)
    const rm::glsl::KernargFrame K = rm::glsl::plugin_frame();
    asm volatile("" ::"s"(K->time), "s"(K->pos_x), "s"(K->pos_y), "s"(K->pos_z), "s"(K->mouse_x), "s"(K->mouse_y),
                 "s"(K->res_x), "s"(K->res_y));
    RM_UNIFORM_PRELOAD();
    const rm::FrameConst& G = *(const rm::FrameConst*)K;
    const size_t px = (size_t)G.W * (size_t)G.H * (size_t)blockIdx.z;
    float ox, oy;
    rmaa::sample_offset(1 << kshift, (int)(threadIdx.x & 63u) & ((1 << kshift) - 1), ox, oy);
    for (uint32_t gl = blockIdx.x; gl * ppw < count; gl += gridDim.x)  // (count < 2^30: no wrap)
        rm::batch_aa_refine_group<rm::SCENE_PLUGIN>(G, kshift, count, gl, queue + px, frames + px, ox, oy);
}
#else
extern "C" __global__ __launch_bounds__(64) void rm_plugin_render(rm::FrameConst F, RM_UNIFORM_PARAM void* out,
                                                                  int rgba8, unsigned long long* evals) {
    RM_UNIFORM_PRELOAD();
    rm::plugin_render_tile<false>(F, out, rgba8, evals);
}
extern "C" __global__ __launch_bounds__(64) void rm_plugin_render_count(rm::FrameConst F, RM_UNIFORM_PARAM void* out,
                                                                         int rgba8, unsigned long long* evals) {
    RM_UNIFORM_PRELOAD();
    rm::plugin_render_tile<true>(F, out, rgba8, evals);
}

// the pass's colour along caller-supplied rays (rm_shade_rays, rm_shade.h): one
// kernel (one more copy of the pipeline to compile per scene, not four), the
// lane layout and the origins' kind read from the launch, wave-uniform
extern "C" __global__ __launch_bounds__(64) void rm_plugin_shade(rm::FrameConst F, RM_UNIFORM_PARAM rm::ShadeRays Q) {
    RM_UNIFORM_PRELOAD();
    rm::shade_rays_one<rm::SCENE_PLUGIN, rm::SHADE_PER_LAUNCH, rm::SHADE_PER_LAUNCH>(F, Q);
}
#endif  // RM_PLUGIN_BATCH, RM_PLUGIN_AA, RM_PLUGIN_BATCH_AA
#elif defined(RM_PLUGIN_BATCH)
#error "the scene defines RM_PLUGIN_EVAL_ONLY (no render kernel): it has no batch form"
#elif defined(RM_PLUGIN_AA)
#error "the scene defines RM_PLUGIN_EVAL_ONLY (no render kernel): it has no AA form"
#elif defined(RM_PLUGIN_BATCH_AA)
#error "the scene defines RM_PLUGIN_EVAL_ONLY (no render kernel): it has no batch-AA form"
#endif

#if !defined(RM_PLUGIN_BATCH) && !defined(RM_PLUGIN_AA) && !defined(RM_PLUGIN_BATCH_AA)
// sceneSDF(p) at explicit points (rm_scene_eval)
extern "C" __global__ __launch_bounds__(256) void rm_plugin_eval(rm::FrameConst F, RM_UNIFORM_PARAM const float* pts,
                                                                 long long n, float* dist, float* mat) {
    RM_UNIFORM_PRELOAD();
    rm::scene_eval_one<rm::SCENE_PLUGIN>(F, pts, n, dist, mat);
}

// the probe instance's sceneSDF(p) at explicit points (rm_scene_eval_form's
// probe forms: distance and material of rm::glsl::probe; aux receives 0).
// Only for a scene that defines RM_PLUGIN_EVAL_PROBE: one more copy of the
// scene to compile (the plugin section's compile times), which
// tests and tools ask for and a scene that is only rendered does not need.
#ifdef RM_PLUGIN_EVAL_PROBE
extern "C" __global__ __launch_bounds__(256) void rm_plugin_eval_probe(rm::FrameConst F,
                                                                       RM_UNIFORM_PARAM const float* pts, long long n,
                                                                       float* dist, float* mat, float* aux) {
    RM_UNIFORM_PRELOAD();
    rm::scene_eval_one<rm::SCENE_PLUGIN, rm::kFormProbe>(F, pts, n, dist, mat, aux);
}
#endif

// castRayD / castRayDI over caller-supplied rays (rm_cast_rays, rm_rays.h)
extern "C" __global__ __launch_bounds__(256) void rm_plugin_cast(rm::FrameConst F, RM_UNIFORM_PARAM rm::RayQuery Q,
                                                                 int inside) {
    RM_UNIFORM_PRELOAD();
    rm::cast_rays_one<rm::SCENE_PLUGIN>(F, Q, inside);
}
#endif  // RM_PLUGIN_BATCH, RM_PLUGIN_AA
