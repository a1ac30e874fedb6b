// rm_batch_host.cpp -- rm_batch_bytes, rm_render_batch and rm_render_batch_rgba8
// (include/rm.h), and what rm_render_batch_ex (rm_plugin_batch_host.cpp) shares
// with them: their argument checks, the per-view records and their upload,
// the staging of a host target and the one launch (kernels: rm_batch.h,
// rm_batch_t.hip, rm_batch_o.hip).  Compiled with -ffp-contract=off as every
// host file; the pose-dependent constants come from rm_render_host.cpp's
// pose_const, the single-frame path's own code.
#include <cmath>
#include <cstring>

#include "rm_batch.h"
#include "rm_ctx.h"
#include "rm_trace.h"

using rm::FrameConst;
using rm::RowPart;
using namespace rmhost;

namespace {

int64_t pixel_bytes(bool rgba8) { return rgba8 ? (int64_t)sizeof(uint32_t) : (int64_t)sizeof(float4); }

// A pinned block of at least `bytes` that no copy still reads: the blocks in
// turn (rm_ctx::BatchSlot), each waited for by the event recorded after its
// last upload.
rm_status batch_host_block(rm_ctx *ctx, size_t bytes, rm_ctx::BatchSlot *&slot) {
    slot = &ctx->batch_slot[ctx->batch_next];
    ctx->batch_next = (ctx->batch_next + 1) % rm_ctx::kBatchSlots;
    if (slot->used) RM_HIP(hipEventSynchronize(slot->copied));
    slot->used = false;
    if (!slot->copied) RM_HIP(hipEventCreateWithFlags(&slot->copied, hipEventDisableTiming));
    if (slot->bytes < bytes) {
        if (slot->host) (void)hipHostFree(slot->host);
        slot->host = nullptr;
        slot->bytes = 0;
        RM_HIP(hipHostMalloc(&slot->host, bytes, hipHostMallocDefault));
        slot->bytes = bytes;
    }
    return RM_OK;
}

}  // namespace

namespace rmhost {

// The launch's shared constants and the upload of the per-view records, on the
// context's stream (rm_ctx.h): what a view batch and its supersampling
// (rm_batch_aa_host.cpp) both start with.
rm_status batch_records(rm_ctx *ctx, int W, int H, const rm_view *views, int n, FrameConst &F, const void *&rec_d,
                        const uint32_t *blocks) {
    RowPart part;
    (void)rm::band_part(H, 1, 0, part);  // the whole frame, as rm_render's launch
    F = frame_const(ctx, W, H, part, H);
    if (rm_status st = frame_rcp(ctx, F)) return st;  // (one lookup per call: the resolution is shared)
    F.row0 = 0;
    F.tile_run = rm::wave_row_mode(part, 0, 8, F.run_magic != 0);
    F.lat_tiles = 0;  // (row-major: no ordered launch, no latency tiles)

    // a record per view: the short one, or the view's whole FrameConst (rm_batch.h batch_whole_record); a scene
    // plugin's: the whole FrameConst, then the view's uniform block (rm_plugin.h, the batch form)
    const bool plugin = ctx->scene == rm::SCENE_PLUGIN;
    const int slots = ctx->plugin.uniform_slots;
    const size_t stride = plugin ? rmplugin::batch_record_stride(slots) : rm::batch_record_bytes(ctx->scene);
    const size_t bytes = (size_t)n * stride;
    rm_ctx::BatchSlot *slot = nullptr;
    if (rm_status st = batch_host_block(ctx, bytes, slot)) return st;
    FrameConst V = F;  // (pose_const writes the pose-dependent members only)
    for (int v = 0; v < n; v++) {
        pose_const(V, views[v].pos, views[v].mouse, views[v].time);
        // the fragment moves as rm_render_accumulate moves it for u_seed1 = offset + 0.5
        V.jit_x = seed_jitter(views[v].offset[0] + 0.5f);
        V.jit_y = seed_jitter(views[v].offset[1] + 0.5f);
        if (plugin) {
            char *rec = static_cast<char *>(slot->host) + (size_t)v * stride;
            std::memset(rec, 0, stride);
            std::memcpy(rec, &V, sizeof(V));
            if (slots > 0)
                std::memcpy(rec + rmplugin::kBatchUniformOffset, blocks + (size_t)v * 4 * (size_t)slots, 16 * (size_t)slots);
        } else {
            rm::batch_record_write(ctx->scene, slot->host, v, V);
        }
    }
    F.near_r = V.near_r;  // (shared by the views: pose_const withdraws the ladder's radius if any view's pose asks it)
    rm_ctx::Scratch &sc = ctx->scratch[rm_ctx::kScratchBatch];  // the device buffer for n records
    if (rm_status st = scratch_acquire(ctx, sc, bytes)) return st;
    rec_d = sc.ptr;
    RM_HIP(hipMemcpyAsync(sc.ptr, slot->host, bytes, hipMemcpyHostToDevice, ctx->stream));
    RM_HIP(hipEventRecord(slot->copied, ctx->stream));
    slot->used = true;
    scratch_used(ctx, sc);
    mark_done(ctx);
    return RM_OK;
}

// the one launch over views x tiles; F, rec_d: batch_records'; `out` a device pointer
rm_status batch_launch(rm_ctx *ctx, const FrameConst &F, const void *rec_d, int n, void *out, bool rgba8,
                       rm_stats *stats) {
    ctx->last_certified = 0;  // (of the last render launch alone; this one counts nothing)
    ctx->last_refl_cleared = 0;
    ctx->last_near_sky = 0;
    if (stats) RM_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    const hipError_t e =
        ctx->scene == rm::SCENE_PLUGIN
            ? rmplugin::launch_render_batch(ctx->plugin, rec_d, F.W, F.H, n, out, rgba8, ctx->stream)
        : ctx->scene == rm::SCENE_S0 || ctx->scene == rm::SCENE_T
            ? rm::launch_batch_t(ctx->scene, F, rec_d, n, out, rgba8, ctx->stream)
            : rm::launch_batch_o(ctx->scene, F, rec_d, n, out, rgba8, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "view batch launch");
    if (stats) {
        RM_HIP(hipEventRecord(ctx->ev1, ctx->stream));
        RM_HIP(hipEventSynchronize(ctx->ev1));
        float ms = 0.0f;
        RM_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        std::memset(stats, 0, sizeof(*stats));
        stats->pixels = (uint64_t)n * (uint64_t)F.W * (uint64_t)F.H;
        stats->kernel_ms = ms;
        stats->scene = ctx->scene;
        stats->dispatch = RM_DISPATCH_ROW_MAJOR;
    }
    return RM_OK;
}

}  // namespace rmhost

namespace {

// the upload and the one launch, on the context's stream; `out` a device pointer
rm_status batch_dev(rm_ctx *ctx, int W, int H, const rm_view *views, int n, void *out, bool rgba8, rm_stats *stats,
                    const uint32_t *blocks) {
    FrameConst F;
    const void *rec_d = nullptr;
    if (rm_status st = batch_records(ctx, W, H, views, n, F, rec_d, blocks)) return st;
    return batch_launch(ctx, F, rec_d, n, out, rgba8, stats);
}

}  // namespace

namespace rmhost {

rm_status batch_run(rm_ctx *ctx, int W, int H, const rm_view *views, int n, void *out, bool rgba8, rm_stats *stats,
                    const BatchEx *ex) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    rm::TraceRange range("rm_render_batch");
    if (!rm::batch_size_ok(W, H, n))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT,
                    "view batch: W, H > 0, 0 <= n <= 65535, ceil(H / 8) <= 65535 and n * W * H <= 2^31");
    if (n > 0 && (!views || !out)) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "view batch: null views or output");
    if (ex && (ex->n_uniforms < 0 || (ex->n_uniforms > 0 && !ex->uniforms)))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "view batch: n_uniforms < 0, or a null list of uniforms");
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    const bool plugin = ctx->scene == rm::SCENE_PLUGIN;
    if (plugin && !ex) return fail(ctx, RM_ERR_SCENE, "view batches: built-in scenes only");
    if (ex)
        if (rm_status st = batch_ex_scene(ctx, *ex)) return st;
    for (int v = 0; v < n; v++)
        for (int k = 0; k < 2; k++) {
            const float o = views[v].offset[k];
            if (!(o >= -0.5f && o < 0.5f))  // (a NaN fails both compares)
                return fail(ctx, RM_ERR_INVALID_ARGUMENT, "view batch: a view's offset is outside [-0.5, 0.5)");
        }
    std::vector<uint32_t> blocks;  // (a plugin's uniform blocks, one per view)
    if (plugin)
        if (rm_status st = batch_ex_blocks(ctx, *ex, n, blocks)) return st;
    if (n == 0) {  // nothing to launch
        if (stats) {
            std::memset(stats, 0, sizeof(*stats));
            stats->scene = ctx->scene;
            stats->dispatch = RM_DISPATCH_ROW_MAJOR;
        }
        return RM_OK;
    }
    RM_HIP(hipSetDevice(ctx->device));
    if (plugin)
        if (rm_status st = batch_ex_ready(ctx)) return st;
    if (is_device_ptr(out)) return batch_dev(ctx, W, H, views, n, out, rgba8, stats, blocks.data());
    // a host target goes through the staging buffer
    const size_t bytes = (size_t)n * (size_t)W * (size_t)H * (size_t)pixel_bytes(rgba8);
    if (rm_status st = ensure_staging(ctx, bytes)) return st;
    if (rm_status st = batch_dev(ctx, W, H, views, n, ctx->staging, rgba8, stats, blocks.data())) return st;
    RM_HIP(hipMemcpyAsync(out, ctx->staging, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RM_HIP(hipStreamSynchronize(ctx->stream));
    return RM_OK;
}

}  // namespace rmhost

extern "C" {

rm_status rm_batch_bytes(int W, int H, int n, int rgba8, int64_t *frame_bytes, int64_t *total_bytes) {
    if (!rm::batch_size_ok(W, H, n)) return RM_ERR_INVALID_ARGUMENT;
    const int64_t frame = (int64_t)W * H * pixel_bytes(rgba8 != 0);
    if (frame_bytes) *frame_bytes = frame;
    if (total_bytes) *total_bytes = frame * n;
    return RM_OK;
}

rm_status rm_render_batch(rm_ctx *ctx, int W, int H, const rm_view *views, int n, float *out, rm_stats *stats) {
    return batch_run(ctx, W, H, views, n, out, false, stats, nullptr);
}

rm_status rm_render_batch_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n, uint32_t *out,
                                rm_stats *stats) {
    return batch_run(ctx, W, H, views, n, out, true, stats, nullptr);
}

}  // extern "C"
