// rm_shade_host.cpp -- rm_shade_rays (include/rm.h): its argument checks, the
// staging of host buffers and the launch (kernels: rm_shade.h, rm_shade_t.hip,
// rm_shade_o.hip; a scene plugin's: rm_plugin_kernels.h).
#include <cstring>

#include "rm_ctx.h"
#include "rm_shade.h"
#include "rm_stage.h"
#include "rm_trace.h"

using rm::FrameConst;
using rm::RowPart;
using namespace rmhost;

namespace {

constexpr int64_t kMaxRays = (int64_t)1 << 30;

// the launch on the context's stream; device pointers
rm_status shade_dev(rm_ctx *ctx, const FrameConst &F, const rm::ShadeRays &Q, rm_stats *stats) {
    rm::TraceRange range("rm_shade_rays");
    if (stats) RM_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    const hipError_t e = ctx->scene == rm::SCENE_PLUGIN
                             ? rmplugin::launch_shade(ctx->plugin, F, ctx->uniform_values, Q, ctx->stream)
                         : ctx->scene == rm::SCENE_S0 || ctx->scene == rm::SCENE_T
                             ? rm::launch_shade_rays_t(ctx->scene, F, Q, ctx->stream)
                             : rm::launch_shade_rays_o(ctx->scene, F, Q, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "shade kernel launch");
    mark_done(ctx);
    if (stats) {
        RM_HIP(hipEventRecord(ctx->ev1, ctx->stream));
        RM_HIP(hipEventSynchronize(ctx->ev1));
        float ms = 0.0f;
        RM_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        std::memset(stats, 0, sizeof(*stats));
        stats->pixels = (uint64_t)Q.n;
        ctx->last_certified = 0;  // (rm_certified_steps: the shade kernels are not instrumented)
        ctx->last_refl_cleared = 0;
        ctx->last_near_sky = 0;
        stats->kernel_ms = ms;
        stats->scene = ctx->scene;
    }
    return RM_OK;
}

}  // namespace

extern "C" {

rm_status rm_shade_rays(rm_ctx *ctx, const float *origins, int shared_origin, const float *directions, int64_t n,
                        const rm_shade_params *params, float *out_rgba, uint32_t *out_rgba8, rm_stats *stats) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (n < 0 || n > kMaxRays || (n > 0 && (!params || !origins || !directions)) ||
        (out_rgba != nullptr) == (out_rgba8 != nullptr))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_shade_rays: bad arguments");
    if (params) {
        const rm_shade_params &p = *params;
        if ((p.output != RM_SHADE_LINEAR && p.output != RM_SHADE_DISPLAY) || (p.vignette != 0 && p.vignette != 1))
            return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_shade_rays: output or vignette out of range");
        if (p.width < 0 || (p.width > 0 && n % p.width != 0))
            return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_shade_rays: n is not a multiple of width");
        if (p.output == RM_SHADE_LINEAR && (out_rgba8 || p.vignette))
            return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_shade_rays: RM_SHADE_LINEAR has a float target and no vignette");
        if (p.vignette && p.width == 0)
            return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_shade_rays: vignette = 1 needs a ray image (width > 0)");
    }
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    if (ctx->scene == rm::SCENE_PLUGIN && !ctx->plugin.shade)
        return fail(ctx, RM_ERR_SCENE, "rm_shade_rays: the scene plugin has no render kernels (RM_PLUGIN_EVAL_ONLY)");
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(ctx->device));
    // the buffers in use (a shared origin is a host triple of its own kind)
    struct Buf {
        const void *p;
        size_t bytes;
        bool input;
    };
    const size_t f = sizeof(float), N = (size_t)n;
    void *const out = out_rgba ? static_cast<void *>(out_rgba) : static_cast<void *>(out_rgba8);
    const Buf bufs[3] = {{shared_origin ? nullptr : origins, N * 3 * f, true},
                         {directions, N * 3 * f, true},
                         {out, out_rgba ? N * 4 * f : N * sizeof(uint32_t), false}};
    int ndev = 0, nused = 0;
    for (const Buf &b : bufs) {
        if (!b.p) continue;
        nused++;
        ndev += is_device_ptr(b.p) ? 1 : 0;
    }
    if (ndev != 0 && ndev != nused)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_shade_rays: host and device pointers mixed");
    if (shared_origin && is_device_ptr(origins))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_shade_rays: the shared origin is a host pointer");
    // the ray image's size reaches the kernels for the vignette's texcoords only
    const int W = params->width > 0 ? params->width : 1, H = params->width > 0 ? (int)(n / params->width) : 1;
    FrameConst F = frame_const(ctx, W, H, RowPart{1, 0, 1}, H);
    if (rm_status st = frame_rcp(ctx, F)) return st;
    if (shared_origin) {  // the launch's u_pos; scene T's primary rays start from its sponge-space image, as a frame's
        F.pos_x = origins[0];
        F.pos_y = origins[1];
        F.pos_z = origins[2];
        rm::camera_sponge_origin(F);
    }
    rm::ShadeRays Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.n = n;
    Q.width = params->width;
    Q.display = params->output == RM_SHADE_DISPLAY ? 1 : 0;
    Q.vignette = params->vignette;
    // host buffers: staged, and the call returns when the results are written
    Stage stage;
    void *dev[3];  // the buffers' device views
    for (int k = 0; k < 3; k++) {
        dev[k] = const_cast<void *>(bufs[k].p);
        if (!ndev) stage.add(bufs[k].p, bufs[k].bytes, bufs[k].input, !bufs[k].input);
    }
    rm_status st = stage.begin(ctx, "rm_shade_rays: staging");
    for (int k = 0; k < 3 && !ndev; k++) dev[k] = stage.dev<void>(k);
    Q.origins = static_cast<const float *>(dev[0]);
    Q.directions = static_cast<const float *>(dev[1]);
    Q.rgba = out_rgba ? static_cast<float4 *>(dev[2]) : nullptr;
    Q.rgba8 = out_rgba8 ? static_cast<uint32_t *>(dev[2]) : nullptr;
    if (st == RM_OK) st = shade_dev(ctx, F, Q, stats);
    return stage.end(ctx, st, "rm_shade_rays");
}

}  // extern "C"
