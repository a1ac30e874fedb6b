// rm_plugin_batch_host.cpp -- rm_render_batch_ex, rm_render_batch_ex_rgba8 and
// rm_batch_prepare (include/rm.h), and the supersampled forms
// rm_refine_batch_ex_rgba8, rm_render_batch_aa_ex_rgba8 and rm_batch_aa_prepare
// (through rm_batch_aa_host.cpp's batch_aa_run):
// view batches of any scene, a scene plugin's with its uniforms set per view.
// The call itself is rm_batch_host.cpp's batch_run -- the checks, the pinned
// blocks, the records' scratch buffer, the staging and the one launch are
// shared; here is what a plugin adds to it: the list's checks and the per-view
// uniform blocks (rm_plugin_batch_pack.h), and the batch form of the scene's
// code object, compiled on first use (rm_plugin_host.cpp batch_ready).
#include "rm_ctx.h"
#include "rm_plugin_batch_pack.h"

using namespace rmhost;

namespace rmhost {

rm_status batch_ex_scene(rm_ctx *ctx, const BatchEx &ex) {
    if (ctx->scene == rm::SCENE_PLUGIN) {
        if (!ctx->plugin.render)
            return fail(ctx, RM_ERR_SCENE, "scene plugin was compiled with RM_PLUGIN_EVAL_ONLY (no render kernel)");
        return RM_OK;
    }
    if (ex.n_uniforms > 0)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "view batch: a built-in scene declares no uniforms");
    return RM_OK;
}

rm_status batch_ex_blocks(rm_ctx *ctx, const BatchEx &ex, int n, std::vector<uint32_t> &blocks) {
    const std::string err =
        rmpack::pack_view_uniforms(ctx->uniforms, ctx->uniform_values, ex.uniforms, ex.n_uniforms, n, blocks);
    return err.empty() ? RM_OK : fail(ctx, RM_ERR_INVALID_ARGUMENT, err);
}

rm_status batch_ex_ready(rm_ctx *ctx) {
    std::string err;
    hipError_t e = hipSuccess;
    if (rmplugin::batch_ready(ctx->plugin, err, e)) return RM_OK;
    if (e != hipSuccess) return hip_fail(ctx, e, "scene plugin batch module load");
    return fail(ctx, RM_ERR_SCENE, "scene plugin \"" + ctx->plugin.file + "\": the batch form failed to compile:\n" + err);
}

rm_status batch_aa_ex_ready(rm_ctx *ctx) {
    std::string err;
    hipError_t e = hipSuccess;
    if (rmplugin::batch_aa_ready(ctx->plugin, err, e)) return RM_OK;
    if (e != hipSuccess) return hip_fail(ctx, e, "scene plugin batch-AA module load");
    return fail(ctx, RM_ERR_SCENE,
                "scene plugin \"" + ctx->plugin.file + "\": the batch-AA form failed to compile:\n" + err);
}

}  // namespace rmhost

extern "C" {

rm_status rm_render_batch_ex(rm_ctx *ctx, int W, int H, const rm_view *views, int n, const rm_view_uniform *uniforms,
                             int n_uniforms, float *out, rm_stats *stats) {
    const BatchEx ex = {uniforms, n_uniforms};
    return batch_run(ctx, W, H, views, n, out, false, stats, &ex);
}

rm_status rm_render_batch_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n,
                                   const rm_view_uniform *uniforms, int n_uniforms, uint32_t *out, rm_stats *stats) {
    const BatchEx ex = {uniforms, n_uniforms};
    return batch_run(ctx, W, H, views, n, out, true, stats, &ex);
}

rm_status rm_batch_prepare(rm_ctx *ctx) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    const BatchEx none = {nullptr, 0};
    if (rm_status st = batch_ex_scene(ctx, none)) return st;
    if (ctx->scene != rm::SCENE_PLUGIN) return RM_OK;  // (compiled in)
    RM_HIP(hipSetDevice(ctx->device));
    return batch_ex_ready(ctx);
}

rm_status rm_refine_batch_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n,
                                   const rm_view_uniform *uniforms, int n_uniforms, const rm_aa_params *params,
                                   uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats) {
    const BatchEx ex = {uniforms, n_uniforms};
    return batch_aa_run(ctx, "rm_refine_batch_ex_rgba8", W, H, views, n, params, frames, mask, refined, stats, false,
                        &ex);
}

rm_status rm_render_batch_aa_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n,
                                      const rm_view_uniform *uniforms, int n_uniforms, const rm_aa_params *params,
                                      uint32_t *out, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats) {
    const BatchEx ex = {uniforms, n_uniforms};
    return batch_aa_run(ctx, "rm_render_batch_aa_ex_rgba8", W, H, views, n, params, out, mask, refined, stats, true,
                        &ex);
}

rm_status rm_batch_aa_prepare(rm_ctx *ctx) {
    if (rm_status st = rm_batch_prepare(ctx)) return st;  // (its checks, and the batch form)
    if (ctx->scene != rm::SCENE_PLUGIN) return RM_OK;     // (compiled in)
    return batch_aa_ex_ready(ctx);
}

}  // extern "C"
