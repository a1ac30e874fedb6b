// rm_batch_aa_host.cpp -- rm_batch_aa_scratch_bytes, rm_refine_batch_rgba8 and
// rm_render_batch_aa_rgba8 (include/rm.h): their argument checks, the context's
// scratch (counters, plan, queue), the staging of host buffers and the launch
// sequence -- record upload, batch launch, count memset, detect, plan, refine
// (kernels: rm_batch_aa.h, rm_batch_aa_t.hip, rm_batch_aa_o.hip; the records and
// the batch launch are rm_batch_host.cpp's).
#include <cstring>

#include "rm_batch_aa.h"
#include "rm_ctx.h"
#include "rm_trace.h"

using rm::FrameConst;
using namespace rmhost;

namespace {

// include/rm.h's size rule of the three calls
bool size_ok(int W, int H, int n) { return rm::batch_size_ok(W, H, n) && (int64_t)W * H < rmaa::kMaxPixels; }

// The scratch for n views of W x H on the context's stream.  One buffer per
// context (bloom's rule, as rm_aa_host.cpp aa_scratch): a call on another
// stream than the last one first waits, on the device, for that one, marked
// when the context left its stream (rm_ctx_streams.cpp set_stream).
rm_status batch_aa_scratch(rm_ctx *ctx, const rmbaa::Layout &l) {
    if (ctx->baa_ev && ctx->baa_stream != ctx->stream) RM_HIP(hipStreamWaitEvent(ctx->stream, ctx->baa_ev, 0));
    if (l.words > ctx->baa_words) {
        if (ctx->baa_scratch) RM_HIP(hipFree(ctx->baa_scratch));  // (waits for the launches that use it)
        ctx->baa_scratch = nullptr;
        ctx->baa_words = 0;
        RM_HIP(hipMalloc(&ctx->baa_scratch, (size_t)l.words * sizeof(uint32_t)));
        ctx->baa_words = (size_t)l.words;
    }
    return RM_OK;
}

// count memset, detect, plan, refine, on the context's stream; device pointers
rm_status refine_batch_dev(rm_ctx *ctx, const FrameConst &F, const void *rec_d, int n, const rm_aa_params &p,
                           uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats) {
    rm::TraceRange range("rm_refine_batch");
    const rmbaa::Layout l = rmbaa::layout(F.W, F.H, n);
    if (rm_status st = batch_aa_scratch(ctx, l)) return st;
    uint32_t *counters = ctx->baa_scratch + l.counters, *prefix = ctx->baa_scratch + l.plan,
             *queue = ctx->baa_scratch + l.queue;
    const uint32_t cstride = rm::batch_aa_counter_stride();
    if (stats && !ctx->aa_ev2) RM_HIP(hipEventCreate(&ctx->aa_ev2));
    RM_HIP(hipMemsetAsync(counters, 0, (size_t)n * cstride * sizeof(uint32_t), ctx->stream));
    if (stats) RM_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    hipError_t e = rm::launch_batch_aa_detect(frames, F.W, F.H, n, p.threshold, mask, counters, cstride, queue, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch supersampling detect launch");
    ctx->baa_stream = ctx->stream;
    ctx->baa_pending = true;
    mark_done(ctx);
    e = rm::launch_batch_aa_plan(counters, cstride, n, p.samples, prefix, refined, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch supersampling plan launch");
    if (stats) RM_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    e = ctx->scene == rm::SCENE_S0 || ctx->scene == rm::SCENE_T
            ? rm::launch_batch_aa_refine_t(ctx->scene, F, rec_d, n, p.samples, counters, cstride, prefix, queue, frames,
                                           ctx->stream)
            : rm::launch_batch_aa_refine_o(ctx->scene, F, rec_d, n, p.samples, counters, cstride, prefix, queue, frames,
                                           ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch supersampling refine launch");
    if (stats) {
        RM_HIP(hipEventRecord(ctx->aa_ev2, ctx->stream));
        RM_HIP(hipEventSynchronize(ctx->aa_ev2));
        uint32_t total = 0;  // (the plan's sum of the counts, after the groups' total)
        RM_HIP(hipMemcpy(&total, prefix + n + 1, sizeof(total), hipMemcpyDeviceToHost));
        stats->refined = (int64_t)total;
        RM_HIP(hipEventElapsedTime(&stats->detect_ms, ctx->ev0, ctx->ev1));
        RM_HIP(hipEventElapsedTime(&stats->refine_ms, ctx->ev1, ctx->aa_ev2));
    }
    return RM_OK;
}

// the checks of both calls, before any pointer is used, in the single calls' order
rm_status batch_aa_check(rm_ctx *ctx, const char *what, int W, int H, const rm_view *views, int n,
                         const rm_aa_params *p, const uint32_t *frames) {
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
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    if (ctx->scene == rm::SCENE_PLUGIN) return fail(ctx, RM_ERR_SCENE, "batch supersampling: built-in scenes only");
    return RM_OK;
}

// render: rm_render_batch_rgba8 into the frames first (rm_render_batch_aa_rgba8)
rm_status batch_aa_run(rm_ctx *ctx, const char *what, int W, int H, const rm_view *views, int n, const rm_aa_params *p,
                       uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats, bool render) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (rm_status st = batch_aa_check(ctx, what, W, H, views, n, p, frames)) return st;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return RM_OK;  // nothing to launch
    RM_HIP(hipSetDevice(ctx->device));
    const bool dev = is_device_ptr(frames);
    if ((mask && is_device_ptr(mask) != dev) || (refined && is_device_ptr(refined) != dev))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(what) + ": host and device pointers mixed");
    const size_t px = (size_t)n * (size_t)W * (size_t)H, frame_bytes = px * sizeof(uint32_t);
    const size_t refined_bytes = (size_t)n * sizeof(uint32_t);
    char *tmp = nullptr;  // host buffers: staged (frames | refined | mask)
    if (!dev) RM_HIP(hipMalloc(&tmp, frame_bytes + (refined ? refined_bytes : 0) + (mask ? px : 0)));
    uint32_t *frames_d = dev ? frames : reinterpret_cast<uint32_t *>(tmp);
    uint32_t *refined_d = dev || !refined ? refined : reinterpret_cast<uint32_t *>(tmp + frame_bytes);
    uint8_t *mask_d =
        dev || !mask ? mask : reinterpret_cast<uint8_t *>(tmp + frame_bytes + (refined ? refined_bytes : 0));
    FrameConst F;
    const void *rec_d = nullptr;
    rm_status st = batch_records(ctx, W, H, views, n, F, rec_d);
    hipError_t e = hipSuccess;
    if (st == RM_OK && render) {
        rm_stats base;
        st = batch_launch(ctx, F, rec_d, n, frames_d, true, stats ? &base : nullptr);
        if (st == RM_OK && stats) stats->base_ms = base.kernel_ms;
    } else if (st == RM_OK && !dev) {
        e = hipMemcpyAsync(frames_d, frames, frame_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) st = hip_fail(ctx, e, "batch supersampling: staging");
    }
    if (st == RM_OK) st = refine_batch_dev(ctx, F, rec_d, n, *p, frames_d, mask_d, refined_d, stats);
    if (!dev) {
        if (st == RM_OK) {
            e = hipMemcpyAsync(frames, frames_d, frame_bytes, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && refined)
                e = hipMemcpyAsync(refined, refined_d, refined_bytes, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess && mask) e = hipMemcpyAsync(mask, mask_d, px, hipMemcpyDeviceToHost, ctx->stream);
            if (e != hipSuccess) st = hip_fail(ctx, e, "batch supersampling: staging");
        }
        e = hipStreamSynchronize(ctx->stream);  // (also after a failure: tmp may be in use)
        if (st == RM_OK && e != hipSuccess) st = hip_fail(ctx, e, what);
        (void)hipFree(tmp);
    }
    return st;
}

}  // namespace

extern "C" {

rm_status rm_batch_aa_scratch_bytes(int W, int H, int n, int64_t *bytes) {
    if (!size_ok(W, H, n)) return RM_ERR_INVALID_ARGUMENT;
    if (bytes) *bytes = (int64_t)(rmbaa::layout(W, H, n).words * sizeof(uint32_t));
    return RM_OK;
}

rm_status rm_refine_batch_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n, const rm_aa_params *params,
                                uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats) {
    return batch_aa_run(ctx, "rm_refine_batch_rgba8", W, H, views, n, params, frames, mask, refined, stats, false);
}

rm_status rm_render_batch_aa_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n, const rm_aa_params *params,
                                   uint32_t *out, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats) {
    return batch_aa_run(ctx, "rm_render_batch_aa_rgba8", W, H, views, n, params, out, mask, refined, stats, true);
}

}  // extern "C"
