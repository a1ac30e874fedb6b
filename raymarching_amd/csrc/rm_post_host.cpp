// rm_post_host.cpp -- the post passes (include/rm.h): rm_fxaa, rm_post_frag,
// rm_bloom, rm_post_chain and rm_post_chain_ex of one frame, and their forms
// over a batch of frames (rm_post_frag_batch, rm_bloom_batch,
// rm_post_chain_batch, rm_post_batch_plan, rm_set_post_batch_scratch_limit;
// DESIGN.md 2.29): their argument checks, bloom's scratch buffer and its
// run-table cache, which all of them share, and the batch's launch sequence
// over the groups of views that fit the scratch limit (kernels and launches:
// rm_post.hip, rm_fxaa.hip, rm_post_frag.hip, rm_post_batch.hip; the
// arithmetic: rm_bloom_plan.h, rm_post_batch_plan.h).
#include <initializer_list>

#include "rm_ctx.h"
#include "rm_post_batch_plan.h"
#include "rm_trace.h"

using namespace rmhost;

static_assert(rm::kPostBatchDefaultLimit == RM_POST_BATCH_SCRATCH_DEFAULT, "rm.h's constant and the plan's");
static_assert(RM_POST_SAMPLE_FXAA == rm::kSampleFxaa && RM_POST_SAMPLE_TEXEL == rm::kSampleTexel &&
                  RM_POST_SAMPLE_CHROMATIC == rm::kSampleChromatic && RM_POST_SAMPLE_CHROMATIC + 1 == rm::kSampleCount,
              "rm_post_sample and the kernels' kSample*");
static_assert(RM_TONEMAP_NONE == rm::kTonemapNone && RM_TONEMAP_ACES == rm::kTonemapAces &&
                  RM_TONEMAP_REINHARD == rm::kTonemapReinhard && RM_TONEMAP_REINHARD_JODIE == rm::kTonemapJodie &&
                  RM_TONEMAP_UNCHARTED2 == rm::kTonemapUncharted2 && RM_TONEMAP_UNCHARTED2 + 1 == rm::kTonemapCount,
              "rm_tonemap and the kernels' kTonemap*");

namespace {

// Bloom's scratch (mip levels, run tables, polynomials) holds at least `words` on the context's stream, for
// rm_bloom, the post chains and their batch forms alike; `cached`: its run tables are W x H's already (the last
// bloom of this context had the same size and stream, and the buffer is the same).
rm_status bloom_scratch(rm_ctx *ctx, size_t words, int W, int H, bool &cached, uint32_t *&mips) {
    rm_ctx::Scratch &sc = ctx->scratch[rm_ctx::kScratchBloom];
    bool grown = false;
    const rm_status st = scratch_acquire(ctx, sc, words * sizeof(uint32_t), &grown);
    if (grown) ctx->bloom_runs_w = 0;
    if (st != RM_OK) return st;
    mips = sc.as<uint32_t>();
    cached = ctx->bloom_runs_w == W && ctx->bloom_runs_h == H && ctx->bloom_runs_stream == ctx->stream;
    ctx->bloom_runs_w = 0;
    return RM_OK;
}

// a bloom of W x H was enqueued on the stream, its run tables at bloom_plan(W, H)'s offsets
void bloom_done(rm_ctx *ctx, int W, int H) {
    scratch_used(ctx, ctx->scratch[rm_ctx::kScratchBloom]);
    ctx->bloom_runs_w = W;
    ctx->bloom_runs_h = H;
    ctx->bloom_runs_stream = ctx->stream;
}

// rm_bloom and the two post chains, after their argument checks: first() enqueues the pass that writes `mid`
// (rm_bloom: none, `mid` is the caller's frame), then bloom of it into `out`
template <class First>
rm_status bloom_after(rm_ctx *ctx, const char *who, int W, int H, const uint32_t *mid, uint32_t *out,
                      const char *first_what, const char *bloom_what, First first) {
    RM_HIP(hipSetDevice(ctx->device));
    rm::TraceRange range(who);
    const rm::BloomPlan plan = rm::bloom_plan(W, H);
    bool cached = false;
    uint32_t *mips = nullptr;
    if (rm_status st = bloom_scratch(ctx, plan.texels, W, H, cached, mips)) return st;
    hipError_t e = first();
    if (e != hipSuccess) return hip_fail(ctx, e, first_what);
    e = rm::launch_bloom(mid, out, mips, plan, ctx->stream, cached);
    if (e != hipSuccess) return hip_fail(ctx, e, bloom_what);
    bloom_done(ctx, W, H);
    mark_done(ctx);
    return RM_OK;
}

// what rm_post_frag and rm_post_chain_ex check alike (`who` names the call)
rm_status post_frag_args(rm_ctx *ctx, const char *who, int W, int H, int sample, int tonemap, bool distinct,
                         std::initializer_list<const uint32_t *> bufs) {
    auto bad = [&](const char *what) { return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
    for (const uint32_t *p : bufs)
        if (!p) return bad("bad arguments");
    if (W <= 0 || H <= 0 || !distinct) return bad("bad arguments");
    if (sample < 0 || sample >= rm::kSampleCount) return bad("unknown sample (rm_post_sample)");
    if (tonemap < 0 || tonemap >= rm::kTonemapCount) return bad("unknown tonemap (rm_tonemap)");
    if ((int64_t)W * H >= ((int64_t)1 << 30))  // the kernels' 32-bit byte offsets
        return bad("frame of 2^30 texels or more");
    for (const uint32_t *p : bufs)
        if (!is_device_ptr(p)) return bad("device pointers required");
    return RM_OK;
}

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
    uint32_t *tables = nullptr;
    if (rm_status st = bloom_scratch(ctx, (size_t)(bp.scratch_bytes / (int64_t)sizeof(uint32_t)), W, H, cached, tables))
        return st;
    uint32_t *views = tables + plan.texels;
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

rm_status rm_fxaa(rm_ctx *ctx, int W, int H, const uint32_t *in, uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!in || !out || W <= 0 || H <= 0 || in == out) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_fxaa: bad arguments");
    if ((int64_t)W * H >= ((int64_t)1 << 30))  // the kernel's 32-bit byte offsets
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_fxaa: frame of 2^30 texels or more");
    if (!is_device_ptr(in) || !is_device_ptr(out))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_fxaa: device pointers required");
    return launch_on(ctx, "fxaa launch", [&] {
        rm::TraceRange range("rm_fxaa");
        return rm::launch_fxaa(in, out, W, H, ctx->stream);
    });
}

rm_status rm_post_frag(rm_ctx *ctx, int W, int H, int sample, int tonemap, const uint32_t *in, uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (rm_status st = post_frag_args(ctx, "rm_post_frag", W, H, sample, tonemap, in != out, {in, out})) return st;
    return launch_on(ctx, "post_frag launch", [&] {
        rm::TraceRange range("rm_post_frag");
        return rm::launch_post_frag(in, out, W, H, sample, tonemap, ctx->stream);
    });
}

rm_status rm_bloom(rm_ctx *ctx, int W, int H, const uint32_t *in, uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!in || !out || W <= 0 || H <= 0 || in == out)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_bloom: bad arguments");
    if (!is_device_ptr(in) || !is_device_ptr(out))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_bloom: device pointers required");
    return bloom_after(ctx, "rm_bloom", W, H, in, out, "", "bloom launch", [] { return hipSuccess; });
}

rm_status rm_post_chain(rm_ctx *ctx, int W, int H, const uint32_t *in, uint32_t *mid, uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!in || !mid || !out || W <= 0 || H <= 0 || in == mid || mid == out || in == out)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_post_chain: bad arguments");
    if ((int64_t)W * H >= ((int64_t)1 << 30))  // the FXAA kernel's 32-bit byte offsets
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_post_chain: frame of 2^30 texels or more");
    if (!is_device_ptr(in) || !is_device_ptr(mid) || !is_device_ptr(out))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_post_chain: device pointers required");
    // main.cpp:209-214: FXAA into postTexture, its mip chain, bloom of it
    // (the mips from FXAA's registers measured slower)
    return bloom_after(ctx, "rm_post_chain", W, H, mid, out, "post chain: fxaa launch", "post chain: bloom launch",
                       [&] { return rm::launch_fxaa(in, mid, W, H, ctx->stream); });
}

rm_status rm_post_chain_ex(rm_ctx *ctx, int W, int H, int sample, int tonemap, const uint32_t *in, uint32_t *mid,
                           uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (rm_status st = post_frag_args(ctx, "rm_post_chain_ex", W, H, sample, tonemap,
                                      in != mid && mid != out && in != out, {in, mid, out}))
        return st;
    // main.cpp:209-214 with the edited post.frag: the pass into postTexture, bloom of it
    return bloom_after(ctx, "rm_post_chain_ex", W, H, mid, out, "post chain: post_frag launch",
                       "post chain: bloom launch",
                       [&] { return rm::launch_post_frag(in, mid, W, H, sample, tonemap, ctx->stream); });
}

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
