// rm_batch_aa_host.cpp -- rm_batch_aa_scratch_bytes, rm_refine_batch_rgba8 and
// rm_render_batch_aa_rgba8 (include/rm.h), and what their _ex forms
// (rm_plugin_batch_host.cpp) share with them: their argument checks, the context's
// scratch (counters, plan, queue), the staging of host buffers and the launch
// sequence -- record upload, batch launch, count memset, detect, plan, refine
// (kernels: rm_batch_aa.h, rm_batch_aa_t.hip, rm_batch_aa_o.hip; a scene plugin's
// refine: the batch-AA form of its translation unit; the records
// and the batch launch are rm_batch_host.cpp's).
#include <cstring>
#include <vector>

#include "rm_batch_aa.h"
#include "rm_ctx.h"
#include "rm_stage.h"
#include "rm_trace.h"

using rm::FrameConst;
using namespace rmhost;

namespace {

// include/rm.h's size rule of the three calls
bool size_ok(int W, int H, int n) { return rm::batch_size_ok(W, H, n) && (int64_t)W * H < rmaa::kMaxPixels; }

// count memset, detect, plan, refine, on the context's stream; device pointers
rm_status refine_batch_dev(rm_ctx *ctx, const FrameConst &F, const void *rec_d, int n, const rm_aa_params &p,
                           uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats) {
    rm::TraceRange range("rm_refine_batch");
    const rmbaa::Layout l = rmbaa::layout(F.W, F.H, n);
    rm_ctx::Scratch &sc = ctx->scratch[rm_ctx::kScratchBatchAa];  // the scratch for n views of W x H
    if (rm_status st = scratch_acquire(ctx, sc, (size_t)l.words * sizeof(uint32_t))) return st;
    uint32_t *counters = sc.as<uint32_t>() + l.counters, *prefix = sc.as<uint32_t>() + l.plan,
             *queue = sc.as<uint32_t>() + l.queue;
    const uint32_t cstride = rm::batch_aa_counter_stride();
    if (stats && !ctx->aa_ev2) RM_HIP(hipEventCreate(&ctx->aa_ev2));
    RM_HIP(hipMemsetAsync(counters, 0, (size_t)n * cstride * sizeof(uint32_t), ctx->stream));
    if (stats) RM_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    hipError_t e = rm::launch_batch_aa_detect(frames, F.W, F.H, n, p.threshold, mask, counters, cstride, queue, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch supersampling detect launch");
    scratch_used(ctx, sc);
    mark_done(ctx);
    e = rm::launch_batch_aa_plan(counters, cstride, n, p.samples, prefix, refined, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch supersampling plan launch");
    if (stats) RM_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    // (a plugin's refine reads the plan's per-view counts and total only through the counters: no prefix)
    e = ctx->scene == rm::SCENE_PLUGIN
            ? rmplugin::launch_batch_aa_refine(ctx->plugin, rec_d, F.W, F.H, n, rmaa::samples_shift(p.samples), counters,
                                               cstride, queue, frames, ctx->stream)
        : ctx->scene == rm::SCENE_S0 || ctx->scene == rm::SCENE_T
            ? rm::launch_batch_aa_refine_t(ctx->scene, F, rec_d, n, p.samples, counters, cstride, prefix, queue, frames,
                                           ctx->stream)
            : rm::launch_batch_aa_refine_o(ctx->scene, F, rec_d, n, p.samples, counters, cstride, prefix, queue, frames,
                                           ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch supersampling refine launch");
    // (the count: the plan's sum of the views' counts, after the groups' total)
    return stats ? refine_stats(ctx, prefix + n + 1, stats) : RM_OK;
}

// the checks of the calls, before any pointer is used, in the single calls' order; ex: the _ex calls, which take a
// scene plugin and its list of per-view uniforms (include/rm.h states the order)
rm_status batch_aa_check(rm_ctx *ctx, const char *what, int W, int H, const rm_view *views, int n,
                         const rm_aa_params *p, const uint32_t *frames, const BatchEx *ex) {
    if (!size_ok(W, H, n))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT,
                    std::string(what) + ": W, H > 0, 0 <= n <= 65535, ceil(H / 8) <= 65535, n * W * H <= 2^31 and W * H < 2^30");
    if (!p || (n > 0 && (!views || !frames)))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(what) + ": null params, views or frames");
    if (!rmaa::samples_ok(p->samples) || !rmaa::threshold_ok(p->threshold))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(what) + ": samples must be 2, 4 or 8 and threshold 0..255");
    for (int v = 0; v < n; v++)
        if (!(views[v].offset[0] == 0.0f && views[v].offset[1] == 0.0f))  // (a NaN fails the compare)
            return fail(ctx, RM_ERR_INVALID_ARGUMENT,
                        std::string(what) + ": a view's offset is not (0, 0) (the samples' offsets take its place)");
    if (ex && (ex->n_uniforms < 0 || (ex->n_uniforms > 0 && !ex->uniforms)))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(what) + ": n_uniforms < 0, or a null list of uniforms");
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    if (ex) return batch_ex_scene(ctx, *ex);
    if (ctx->scene == rm::SCENE_PLUGIN) return fail(ctx, RM_ERR_SCENE, "batch supersampling: built-in scenes only");
    return RM_OK;
}

}  // namespace

namespace rmhost {

rm_status batch_aa_run(rm_ctx *ctx, const char *what, int W, int H, const rm_view *views, int n, const rm_aa_params *p,
                       uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats, bool render,
                       const BatchEx *ex) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (rm_status st = batch_aa_check(ctx, what, W, H, views, n, p, frames, ex)) return st;
    // (the calls without a list zero the stats here, as they always have; the _ex calls after every check)
    if (stats && !ex) std::memset(stats, 0, sizeof(*stats));
    const bool plugin = ctx->scene == rm::SCENE_PLUGIN;
    std::vector<uint32_t> blocks;  // (a plugin's uniform blocks, one per view)
    if (plugin)
        if (rm_status st = batch_ex_blocks(ctx, *ex, n, blocks)) return st;
    if (n == 0) {  // nothing to launch
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return RM_OK;
    }
    RM_HIP(hipSetDevice(ctx->device));
    const bool dev = is_device_ptr(frames);
    if ((mask && is_device_ptr(mask) != dev) || (refined && is_device_ptr(refined) != dev))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(what) + ": host and device pointers mixed");
    if (plugin) {  // (before anything is written: a form that fails to compile leaves the frames)
        if (render)
            if (rm_status st = batch_ex_ready(ctx)) return st;
        if (rm_status st = batch_aa_ex_ready(ctx)) return st;
    }
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const size_t px = (size_t)n * (size_t)W * (size_t)H, frame_bytes = px * sizeof(uint32_t);
    const size_t refined_bytes = (size_t)n * sizeof(uint32_t);
    Stage stage;  // host buffers: staged (frames | refined | mask)
    if (!dev) {
        stage.add(frames, frame_bytes, !render, true);
        stage.add(refined, refined_bytes, false, true);
        stage.add(mask, px, false, true);
    }
    rm_status st = stage.begin(ctx, "batch supersampling: staging");
    uint32_t *frames_d = dev ? frames : stage.dev<uint32_t>(0);
    uint32_t *refined_d = dev ? refined : stage.dev<uint32_t>(1);
    uint8_t *mask_d = dev ? mask : stage.dev<uint8_t>(2);
    FrameConst F;
    const void *rec_d = nullptr;
    if (st == RM_OK) st = batch_records(ctx, W, H, views, n, F, rec_d, blocks.data());
    if (st == RM_OK && render) {
        rm_stats base;
        st = batch_launch(ctx, F, rec_d, n, frames_d, true, stats ? &base : nullptr);
        if (st == RM_OK && stats) stats->base_ms = base.kernel_ms;
    }
    if (st == RM_OK) st = refine_batch_dev(ctx, F, rec_d, n, *p, frames_d, mask_d, refined_d, stats);
    return stage.end(ctx, st, what);
}

}  // namespace rmhost

extern "C" {

rm_status rm_batch_aa_scratch_bytes(int W, int H, int n, int64_t *bytes) {
    if (!size_ok(W, H, n)) return RM_ERR_INVALID_ARGUMENT;
    if (bytes) *bytes = (int64_t)(rmbaa::layout(W, H, n).words * sizeof(uint32_t));
    return RM_OK;
}

rm_status rm_refine_batch_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n, const rm_aa_params *params,
                                uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats) {
    return batch_aa_run(ctx, "rm_refine_batch_rgba8", W, H, views, n, params, frames, mask, refined, stats, false, nullptr);
}

rm_status rm_render_batch_aa_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n, const rm_aa_params *params,
                                   uint32_t *out, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats) {
    return batch_aa_run(ctx, "rm_render_batch_aa_rgba8", W, H, views, n, params, out, mask, refined, stats, true, nullptr);
}

}  // extern "C"
