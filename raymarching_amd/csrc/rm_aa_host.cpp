// rm_aa_host.cpp -- rm_refine_rgba8, rm_render_aa_rgba8, their _ex forms that
// take any scene and rm_aa_prepare (include/rm.h):
// their argument checks, the context's queue, the staging of host buffers
// (rm_stage.h) and the launch sequence (kernels: rm_aa.h, rm_aa_t.hip,
// rm_aa_o.hip; a scene plugin's refine: the AA form of its translation unit,
// rm_plugin_host.cpp aa_ready).
#include <cstring>

#include "rm_aa.h"
#include "rm_ctx.h"
#include "rm_stage.h"
#include "rm_trace.h"

using rm::FrameConst;
using rm::RowPart;
using namespace rmhost;

namespace {

// detect, then refine, on the context's stream; device pointers
rm_status refine_dev(rm_ctx *ctx, int W, int H, const rm_aa_params &p, uint32_t *frame, uint8_t *mask,
                     rm_aa_stats *stats) {
    rm::TraceRange range("rm_refine");
    rm_ctx::Scratch &sc = ctx->scratch[rm_ctx::kScratchAa];  // the queue for a W x H frame
    if (rm_status st = scratch_acquire(ctx, sc, ((size_t)rm::kAaHeadWords + (size_t)W * H) * sizeof(uint32_t))) return st;
    uint32_t *count = sc.as<uint32_t>(), *queue = count + rm::kAaHeadWords;
    RowPart part;
    (void)rm::band_part(H, 1, 0, part);  // the whole frame, as rm_render_rgba8's launch
    FrameConst F = frame_const(ctx, W, H, part, H);
    if (rm_status st = frame_rcp(ctx, F)) return st;
    if (stats && !ctx->aa_ev2) RM_HIP(hipEventCreate(&ctx->aa_ev2));
    RM_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), ctx->stream));
    if (stats) RM_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    hipError_t e = rm::launch_aa_detect(frame, W, H, p.threshold, mask, count, queue, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "supersampling detect launch");
    scratch_used(ctx, sc);
    mark_done(ctx);
    if (stats) RM_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    const int layout = rm::aa_layout();  // (a plugin has the lane = (entry, sample) layout alone)
    e = ctx->scene == rm::SCENE_PLUGIN
            ? rmplugin::launch_aa_refine(ctx->plugin, F, ctx->uniform_values, rmaa::samples_shift(p.samples), count,
                                         queue, frame, ctx->stream)
        : ctx->scene == rm::SCENE_S0 || ctx->scene == rm::SCENE_T
            ? rm::launch_aa_refine_t(ctx->scene, F, p.samples, layout, count, queue, frame, ctx->stream)
            : rm::launch_aa_refine_o(ctx->scene, F, p.samples, layout, count, queue, frame, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "supersampling refine launch");
    return stats ? refine_stats(ctx, count, stats) : RM_OK;
}

// what the _ex calls and rm_aa_prepare ask of a loaded plugin: it must have render kernels
rm_status aa_plugin_scene(rm_ctx *ctx) {
    if (!ctx->plugin.render)
        return fail(ctx, RM_ERR_SCENE, "scene plugin was compiled with RM_PLUGIN_EVAL_ONLY (no render kernel)");
    return RM_OK;
}

// the loaded plugin's refine kernel, compiled and loaded if it is not yet
rm_status aa_plugin_ready(rm_ctx *ctx) {
    std::string err;
    hipError_t e = hipSuccess;
    if (rmplugin::aa_ready(ctx->plugin, err, e)) return RM_OK;
    if (e != hipSuccess) return hip_fail(ctx, e, "scene plugin AA module load");
    return fail(ctx, RM_ERR_SCENE, "scene plugin \"" + ctx->plugin.file + "\": the AA form failed to compile:\n" + err);
}

// the checks of the calls, before any pointer is used; any_scene: the _ex calls, which take a scene plugin
rm_status aa_check(rm_ctx *ctx, const char *what, int W, int H, const rm_aa_params *p, const uint32_t *frame,
                   bool any_scene) {
    if (W <= 0 || H <= 0 || (int64_t)W * H >= rmaa::kMaxPixels || !p || !frame)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(what) + ": bad arguments");
    if (!rmaa::samples_ok(p->samples) || !rmaa::threshold_ok(p->threshold))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(what) + ": samples must be 2, 4 or 8 and threshold 0..255");
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    if (ctx->scene == rm::SCENE_PLUGIN)
        return any_scene ? aa_plugin_scene(ctx) : fail(ctx, RM_ERR_SCENE, "adaptive supersampling: built-in scenes only");
    return RM_OK;
}

// render: rm_render_rgba8 into the frame first (rm_render_aa_rgba8)
rm_status aa_run(rm_ctx *ctx, const char *what, int W, int H, const rm_aa_params *p, uint32_t *frame, uint8_t *mask,
                 rm_aa_stats *stats, bool render, bool any_scene) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (rm_status st = aa_check(ctx, what, W, H, p, frame, any_scene)) return st;
    RM_HIP(hipSetDevice(ctx->device));
    const bool dev = is_device_ptr(frame);
    if (mask && is_device_ptr(mask) != dev)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(what) + ": host and device pointers mixed");
    if (ctx->scene == rm::SCENE_PLUGIN)  // (before anything is written: a form that fails to compile leaves the frame)
        if (rm_status st = aa_plugin_ready(ctx)) return st;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const size_t px = (size_t)W * H, frame_bytes = px * sizeof(uint32_t);
    Stage stage;  // host buffers: staged
    if (!dev) {
        stage.add(frame, frame_bytes, !render, true);
        stage.add(mask, px, false, true);
    }
    rm_status st = stage.begin(ctx, "supersampling: staging");
    uint32_t *frame_d = dev ? frame : stage.dev<uint32_t>(0);
    uint8_t *mask_d = dev ? mask : stage.dev<uint8_t>(1);
    if (st == RM_OK && render) {
        rm_stats base;
        st = render_any(ctx, W, H, H, 1, 0, 0, -1, frame_d, true, stats ? &base : nullptr);
        if (st == RM_OK && stats) stats->base_ms = base.kernel_ms;
    }
    if (st == RM_OK) st = refine_dev(ctx, W, H, *p, frame_d, mask_d, stats);
    return stage.end(ctx, st, what);
}

}  // namespace

namespace rmhost {

rm_status refine_stats(rm_ctx *ctx, const uint32_t *count, rm_aa_stats *stats) {
    RM_HIP(hipEventRecord(ctx->aa_ev2, ctx->stream));
    RM_HIP(hipEventSynchronize(ctx->aa_ev2));
    uint32_t n = 0;
    RM_HIP(hipMemcpy(&n, count, sizeof(n), hipMemcpyDeviceToHost));
    stats->refined = (int64_t)n;
    RM_HIP(hipEventElapsedTime(&stats->detect_ms, ctx->ev0, ctx->ev1));
    RM_HIP(hipEventElapsedTime(&stats->refine_ms, ctx->ev1, ctx->aa_ev2));
    return RM_OK;
}

}  // namespace rmhost

extern "C" {

rm_status rm_refine_rgba8(rm_ctx *ctx, int W, int H, const rm_aa_params *params, uint32_t *frame, uint8_t *mask,
                          rm_aa_stats *stats) {
    return aa_run(ctx, "rm_refine_rgba8", W, H, params, frame, mask, stats, false, false);
}

rm_status rm_render_aa_rgba8(rm_ctx *ctx, int W, int H, const rm_aa_params *params, uint32_t *out, uint8_t *mask,
                             rm_aa_stats *stats) {
    return aa_run(ctx, "rm_render_aa_rgba8", W, H, params, out, mask, stats, true, false);
}

rm_status rm_refine_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_aa_params *params, uint32_t *frame, uint8_t *mask,
                             rm_aa_stats *stats) {
    return aa_run(ctx, "rm_refine_ex_rgba8", W, H, params, frame, mask, stats, false, true);
}

rm_status rm_render_aa_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_aa_params *params, uint32_t *out, uint8_t *mask,
                                rm_aa_stats *stats) {
    return aa_run(ctx, "rm_render_aa_ex_rgba8", W, H, params, out, mask, stats, true, true);
}

rm_status rm_aa_prepare(rm_ctx *ctx) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    if (ctx->scene != rm::SCENE_PLUGIN) return RM_OK;  // (compiled in)
    if (rm_status st = aa_plugin_scene(ctx)) return st;
    RM_HIP(hipSetDevice(ctx->device));
    return aa_plugin_ready(ctx);
}

}  // extern "C"
