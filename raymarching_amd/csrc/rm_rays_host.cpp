// rm_rays_host.cpp -- rm_cast_rays and rm_camera_rays (include/rm.h): their
// argument checks, the staging of host buffers and the launches (kernels:
// rm_rays.h, rm_rays.hip; a scene plugin's: rm_plugin_kernels.h).
#include <cstring>

#include "rm_ctx.h"
#include "rm_rays.h"
#include "rm_stage.h"
#include "rm_trace.h"

using rm::FrameConst;
using rm::RowPart;
using namespace rmhost;

static_assert((int)RM_RAY_MISS == (int)rm::RAY_MISS && (int)RM_RAY_HIT == (int)rm::RAY_HIT &&
                  (int)RM_RAY_EXHAUSTED == (int)rm::RAY_EXHAUSTED,
              "rm.h RM_RAY_* and rm_rays.h RAY_*");

namespace {

constexpr int64_t kMaxRays = (int64_t)1 << 30;

// the launch on the context's stream, with the stats of an instrumented one
rm_status cast_dev(rm_ctx *ctx, rm::RayQuery Q, int inside, rm_stats *stats) {
    rm::TraceRange range("rm_cast_rays");
    const FrameConst F = frame_const(ctx, 1, 1, RowPart{1, 0, 1}, 1);
    if (stats) {
        Q.evals = ctx->d_evals;
        RM_HIP(hipMemsetAsync(ctx->d_evals, 0, 6 * sizeof(unsigned long long), ctx->stream));
        RM_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    }
    const hipError_t e =
        ctx->scene == rm::SCENE_PLUGIN
            ? rmplugin::launch_cast(ctx->plugin, F, ctx->uniform_values, Q, inside, rm::cast_block_size(), ctx->stream)
            : rm::launch_cast_rays(ctx->scene, F, Q, inside, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "cast kernel launch");
    mark_done(ctx);
    if (stats) {
        RM_HIP(hipEventRecord(ctx->ev1, ctx->stream));
        RM_HIP(hipEventSynchronize(ctx->ev1));
        float ms = 0.0f;
        RM_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        unsigned long long ev = 0;
        RM_HIP(hipMemcpy(&ev, ctx->d_evals, sizeof(ev), hipMemcpyDeviceToHost));
        std::memset(stats, 0, sizeof(*stats));
        stats->evals = ev;
        ctx->last_certified = 0;  // (rm_certified_steps: a ray query certifies nothing)
        ctx->last_refl_cleared = 0;
        ctx->last_near_sky = 0;
        stats->pixels = (uint64_t)Q.n;
        stats->kernel_ms = ms;
        stats->scene = ctx->scene;
    }
    return RM_OK;
}

}  // namespace

extern "C" {

rm_status rm_cast_rays(rm_ctx *ctx, const float *origins, int shared_origin, const float *directions, int64_t n,
                       int inside, const rm_ray_hits *out, rm_stats *stats) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (n < 0 || n > kMaxRays || (n > 0 && (!origins || !directions || !out || !out->t)))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_cast_rays: bad arguments");
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(ctx->device));
    // the buffers in use, their sizes in floats per ray (origins: per launch when shared)
    struct Buf {
        const void *p;
        size_t bytes;
        bool input;
    };
    const size_t f = sizeof(float), N = (size_t)n;
    const Buf bufs[8] = {{origins, (shared_origin ? 1 : N) * 3 * f, true}, {directions, N * 3 * f, true},
                         {out->t, N * f, false},            {out->status, N * f, false},
                         {out->steps, N * f, false},        {out->position, N * 3 * f, false},
                         {out->normal, N * 3 * f, false},   {out->material, N * 16 * f, false}};
    int ndev = 0, nused = 0;
    for (const Buf &b : bufs) {
        if (!b.p) continue;
        nused++;
        ndev += is_device_ptr(b.p) ? 1 : 0;
    }
    if (ndev != 0 && ndev != nused)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_cast_rays: host and device pointers mixed");
    // host buffers: staged, and the call returns when the results are written
    Stage stage;
    void *dev[8];  // the buffers' device views
    for (int k = 0; k < 8; k++) {
        dev[k] = const_cast<void *>(bufs[k].p);
        if (!ndev) stage.add(bufs[k].p, bufs[k].bytes, bufs[k].input, !bufs[k].input);
    }
    rm_status st = stage.begin(ctx, "rm_cast_rays: staging");
    for (int k = 0; k < 8 && !ndev; k++) dev[k] = stage.dev<void>(k);
    rm::RayQuery Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.n = n;
    Q.shared_origin = shared_origin ? 1 : 0;
    Q.origins = static_cast<const float *>(dev[0]);
    Q.directions = static_cast<const float *>(dev[1]);
    Q.t = static_cast<float *>(dev[2]);
    Q.status = static_cast<int *>(dev[3]);
    Q.steps = static_cast<uint32_t *>(dev[4]);
    Q.position = static_cast<float *>(dev[5]);
    Q.normal = static_cast<float *>(dev[6]);
    Q.material = static_cast<float *>(dev[7]);
    if (st == RM_OK) st = cast_dev(ctx, Q, inside, stats);
    return stage.end(ctx, st, "rm_cast_rays");
}

rm_status rm_camera_rays(rm_ctx *ctx, int W, int H, float *origin3, float *directions) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (W <= 0 || H <= 0 || (int64_t)W * H > kMaxRays || !origin3 || !directions)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_camera_rays: bad arguments");
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    RM_HIP(hipSetDevice(ctx->device));
    rm::TraceRange range("rm_camera_rays");
    const bool dev_o = is_device_ptr(origin3), dev_d = is_device_ptr(directions);
    const size_t bytes = (size_t)W * H * 3 * sizeof(float);
    FrameConst F = frame_const(ctx, W, H, RowPart{1, 0, 1}, H);
    if (rm_status st = frame_rcp(ctx, F)) return st;
    // the form of the loaded scene's render kernel (a plugin's: output_shader.frag's pass)
    const bool fast = ctx->scene == rm::SCENE_S0   ? rm::ScenePolicy<rm::SCENE_S0>::kHwMath
                      : ctx->scene == rm::SCENE_T  ? rm::ScenePolicy<rm::SCENE_T>::kHwMath
                      : ctx->scene == rm::SCENE_O  ? rm::ScenePolicy<rm::SCENE_O>::kHwMath
                      : ctx->scene == rm::SCENE_OG ? rm::ScenePolicy<rm::SCENE_OG>::kHwMath
                                                   : rm::ScenePolicy<rm::SCENE_PLUGIN>::kHwMath;
    Stage stage;  // host directions: staged
    if (!dev_d) stage.add(directions, bytes, false, true);
    if (rm_status st = stage.begin(ctx, "rm_camera_rays")) return st;
    if (!dev_o) {
        origin3[0] = F.pos_x;
        origin3[1] = F.pos_y;
        origin3[2] = F.pos_z;
    }
    const hipError_t e = rm::launch_camera_rays(fast, F, dev_o ? origin3 : nullptr,
                                                dev_d ? directions : stage.dev<float>(0), ctx->stream);
    if (e == hipSuccess) mark_done(ctx);
    return stage.end(ctx, e == hipSuccess ? RM_OK : hip_fail(ctx, e, "rm_camera_rays"), "rm_camera_rays");
}

}  // extern "C"
