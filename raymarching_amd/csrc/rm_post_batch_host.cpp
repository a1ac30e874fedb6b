// rm_post_batch_host.cpp -- the post passes over a batch of frames
// (include/rm.h rm_post_frag_batch, rm_bloom_batch, rm_post_chain_batch,
// rm_post_batch_plan, rm_set_post_batch_scratch_limit): their
// argument checks, bloom's scratch buffer -- which the single-frame calls of
// rm_capi.cpp share -- and the launch sequence over the groups of views that
// fit the scratch limit (kernels and launches: rm_post_batch.hip; the
// arithmetic: rm_post_batch_plan.h).
#include <initializer_list>

#include "rm_ctx.h"
#include "rm_post_batch_plan.h"
#include "rm_trace.h"

using namespace rmhost;

static_assert(rm::kPostBatchDefaultLimit == RM_POST_BATCH_SCRATCH_DEFAULT, "rm.h's constant and the plan's");

namespace rmhost {

rm_status bloom_scratch(rm_ctx *ctx, size_t words, int W, int H, bool &cached) {
    if (ctx->bloom_ev && ctx->bloom_stream != ctx->stream)  // the last bloom ran on another stream
        RM_HIP(hipStreamWaitEvent(ctx->stream, ctx->bloom_ev, 0));
    if (words > ctx->mips_texels) {
        if (ctx->mips) RM_HIP(hipFree(ctx->mips));  // (waits for the launches that use it)
        ctx->mips = nullptr;
        ctx->mips_texels = 0;
        ctx->bloom_runs_w = 0;
        RM_HIP(hipMalloc(&ctx->mips, words * sizeof(uint32_t)));
        ctx->mips_texels = words;
    }
    cached = ctx->bloom_runs_w == W && ctx->bloom_runs_h == H && ctx->bloom_runs_stream == ctx->stream;
    ctx->bloom_runs_w = 0;
    return RM_OK;
}

void bloom_done(rm_ctx *ctx, int W, int H) {
    ctx->bloom_stream = ctx->stream;
    ctx->bloom_pending = true;
    ctx->bloom_runs_w = W;
    ctx->bloom_runs_h = H;
    ctx->bloom_runs_stream = ctx->stream;
}

}  // namespace rmhost

namespace {

// [a, a + words) and [b, b + words) share a word
bool overlap(const uint32_t *a, const uint32_t *b, uint64_t words) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    const uint64_t bytes = words * sizeof(uint32_t);
    return x < y ? y - x < bytes : x - y < bytes;
}

// The checks of the three calls, in rm.h's order; nothing is launched or written before they pass.
rm_status batch_args(rm_ctx *ctx, const char *who, int W, int H, int n, int sample, int tonemap,
                     std::initializer_list<const uint32_t *> bufs) {
    auto bad = [&](const char *what) { return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
    if (!rm::post_batch_size_ok(W, H, n)) return bad("W, H > 0, 0 <= n <= 65535, n * W * H <= 2^31 and W * H < 2^30");
    if (sample < 0 || sample >= rm::kSampleCount) return bad("unknown sample (rm_post_sample)");
    if (tonemap < 0 || tonemap >= rm::kTonemapCount) return bad("unknown tonemap (rm_tonemap)");
    if (n == 0) return RM_OK;
    for (const uint32_t *p : bufs)
        if (!p) return bad("null buffer");
    const uint64_t words = (uint64_t)n * (uint64_t)W * (uint64_t)H;
    for (const uint32_t *const *a = bufs.begin(); a != bufs.end(); ++a)
        for (const uint32_t *const *b = a + 1; b != bufs.end(); ++b)
            if (overlap(*a, *b, words)) return bad("the buffers' n * W * H words overlap");
    for (const uint32_t *p : bufs)
        if (!is_device_ptr(p)) return bad("device pointers required");
    return RM_OK;
}

// frag: rm_post_frag_batch(in -> mid); bloom: rm_bloom_batch(mid -> out); both: the chain, group by group
rm_status run(rm_ctx *ctx, const char *who, int W, int H, int n, int sample, int tonemap, const uint32_t *in,
              uint32_t *mid, uint32_t *out, bool frag, bool bloom) {
    RM_HIP(hipSetDevice(ctx->device));
    rm::TraceRange range(who);
    const size_t frame = (size_t)W * (size_t)H;
    hipError_t e = hipSuccess;
    if (!bloom) {
        e = rm::launch_post_frag_batch(in, mid, W, H, n, sample, tonemap, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "post batch: post_frag launch");
        mark_done(ctx);
        return RM_OK;
    }
    const rm::BloomPlan plan = rm::bloom_plan(W, H);
    const rm::PostBatchViewLayout L = rm::post_batch_view_layout(plan);
    const rm::PostBatchPlan bp = rm::post_batch_plan(W, H, n, ctx->post_batch_limit);
    bool cached = false;
    if (rm_status st = bloom_scratch(ctx, (size_t)(bp.scratch_bytes / (int64_t)sizeof(uint32_t)), W, H, cached)) return st;
    uint32_t *tables = ctx->mips, *views = ctx->mips + plan.texels;
    if (plan.lod > 0.0f && !cached) {
        e = rm::launch_bloom_runs(tables, plan, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "post batch: bloom runs launch");
    }
    for (int v0 = 0; v0 < n; v0 += bp.group_views) {  // (the groups share the views' part: one after the other)
        const int g = n - v0 < bp.group_views ? n - v0 : bp.group_views;
        if (frag) {
            e = rm::launch_post_frag_batch(in + v0 * frame, mid + v0 * frame, W, H, g, sample, tonemap, ctx->stream);
            if (e != hipSuccess) return hip_fail(ctx, e, "post batch: post_frag launch");
        }
        e = rm::launch_bloom_batch(mid + v0 * frame, out + v0 * frame, g, tables, views, plan, L, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "post batch: bloom launch");
    }
    bloom_done(ctx, W, H);
    mark_done(ctx);
    return RM_OK;
}

}  // namespace

extern "C" {

rm_status rm_post_batch_plan(int W, int H, int n, int64_t limit_bytes, struct rm_post_batch_plan *out) {
    if (!rm::post_batch_size_ok(W, H, n) || limit_bytes < 0) return RM_ERR_INVALID_ARGUMENT;
    if (out) {
        const rm::PostBatchPlan p = rm::post_batch_plan(W, H, n, limit_bytes);
        out->per_view_bytes = p.per_view_bytes;
        out->shared_bytes = p.shared_bytes;
        out->group_views = p.group_views;
        out->groups = p.groups;
        out->scratch_bytes = p.scratch_bytes;
        out->launches = p.launches;
        out->reserved = 0;
    }
    return RM_OK;
}

rm_status rm_set_post_batch_scratch_limit(rm_ctx *ctx, int64_t bytes) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (bytes < 0) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_set_post_batch_scratch_limit: a negative limit");
    ctx->post_batch_limit = bytes;
    return RM_OK;
}

rm_status rm_post_frag_batch(rm_ctx *ctx, int W, int H, int n, int sample, int tonemap, const uint32_t *in,
                             uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (rm_status st = batch_args(ctx, "rm_post_frag_batch", W, H, n, sample, tonemap, {in, out})) return st;
    if (n == 0) return RM_OK;
    return run(ctx, "rm_post_frag_batch", W, H, n, sample, tonemap, in, out, nullptr, true, false);
}

rm_status rm_bloom_batch(rm_ctx *ctx, int W, int H, int n, const uint32_t *in, uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (rm_status st = batch_args(ctx, "rm_bloom_batch", W, H, n, 0, 0, {in, out})) return st;
    if (n == 0) return RM_OK;
    return run(ctx, "rm_bloom_batch", W, H, n, 0, 0, nullptr, const_cast<uint32_t *>(in), out, false, true);
}

rm_status rm_post_chain_batch(rm_ctx *ctx, int W, int H, int n, int sample, int tonemap, const uint32_t *in,
                              uint32_t *mid, uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (rm_status st = batch_args(ctx, "rm_post_chain_batch", W, H, n, sample, tonemap, {in, mid, out})) return st;
    if (n == 0) return RM_OK;
    return run(ctx, "rm_post_chain_batch", W, H, n, sample, tonemap, in, mid, out, true, true);
}

}  // extern "C"
