// rm_render_host.cpp -- a render launch of a context: the per-frame constant
// block the kernels read (rm_device.h FrameConst) from the state the reference
// keeps inside sf::Shader (rm_ctx.h), the kernel choice, the launch with its
// dispatch order.  Compiled with -ffp-contract=off so that the host-side
// per-frame constants (sin/cos of the camera and sponge rotations, the Hash11
// table) are computed with the same roundings as the GLSL expressions they
// hoist.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rm_ctx.h"
#include "rm_trace.h"

using rm::FrameConst;
using rm::RowPart;

namespace rmhost {
namespace {

inline float fract(float x) { return x - std::floor(x); }

// output_shader.frag:54-59
float hash11(float p) {
    float a = fract(p * 443.897f);
    float x = a, y = a, z = a;
    float dd = x * (y + 19.19f) + y * (z + 19.19f) + z * (x + 19.19f);
    x += dd; y += dd; z += dd;
    return fract((x + y) * z);
}

// (sampleDir * Hash11(i)).y of CalculateThickness (output_shader.frag:75-109)
// at a normal (0, ny, 0): Hash33 (:61-66), GenerateSampleVector, reflectVector
// (:70-80) in GLSL float semantics (no contraction; normalize = x * (1/length))
float sss_floor_term(float ny, int i) {
    const float fi = (float)i, nx = -0.0f, nyn = -ny, nz = -0.0f;  // -norm
    float x = fract((nx + fi) * 443.897f), y = fract((nyn + fi) * 441.423f), z = fract((nz + fi) * 437.195f);
    const float dd = x * (y + 19.19f) + y * (x + 19.19f) + z * (z + 19.19f);  // dot(p3, p3.yxz + 19.19)
    x += dd; y += dd; z += dd;
    const float hx = fract((x + y) * z) - 0.5f, hy = fract((x + x) * y) - 0.5f, hz = fract((y + x) * x) - 0.5f;
    const float r = 1.0f / std::sqrt(hx * hx + hy * hy + hz * hz);
    const float rx = hx * r, ry = hy * r, rz = hz * r;
    const float d = rx * nx + ry * nyn + rz * nz;
    const float dir_y = ry - (nyn * 2.0f) * (d < 0.0f ? d : 0.0f);
    return dir_y * hash11(fi);
}

// Workgroups at the head of an ordered launch that render scene T with the
// latency-optimized folds (FrameConst.lat_tiles) ...
constexpr int kLatTiles = 2048;
// ... in launches short enough for their tail to show: a rank's share, a 1080p
// frame.  The C4 share at N = 8 (32768 tiles) takes 0.077 ms per pipelined
// frame with them and 0.098 without; a whole 4096^2 frame (262144 tiles) runs
// 0.4 % faster without them, an N = 2 half frame (131072) the same either way
// (profiles/r05/knob_lat_r05.log, lat_share_r05.jsonl): launches of more tiles
// than this take none.
constexpr int64_t kLatMaxTiles = 98304;
int lat_tiles_for(int kernel, int W, int nrows) {
    const rm::TileGrid g = rm::tile_grid(kernel, W, nrows);
    return (int64_t)g.x * g.y <= kLatMaxTiles ? kLatTiles : 0;
}

// Launches per dispatch-order sort of a geometry (rm_ctx::Sched): 16 -- an
// order is at most 17 launches old (frame-to-frame coherence keeps it good, the
// dilated key covers a moving camera), and the duration stores, the sort and
// the cross-stream events run on one launch in sixteen.  Round 2 chose 4 (C3
// frame 0.683 -> 0.672 ms against 1); after the round-3 skips the frame is
// shorter and 8 measured 0.7 % (still) and 1.8 % (walking) faster than 4, 16
// the same as 8 (profiles/r03/sched_period_after_skips.jsonl).
// Round 4 sorts on the frame's stream (21 us per sort in the frame's time):
// 16 measured 0.3-0.7 % faster than 8 still, walking and at P1, 4 slower
// (profiles/r04/sched_knobs_final_ab.log, sched_period_walk_p1_ab.log).
constexpr uint64_t kSchedPeriod = 16;

// Dilation radius (tiles) of the sort key (rm_kernels.hip tile_key): 2.  With
// a moving camera (bench.py --walk) the costly regions move between the launch
// that measured the durations and the launches that use the order:
// undilated, C3 walks at 0.457 ms per frame against row-major's 0.440; radius
// 2 0.439, with the still pose unchanged (0.583 ms, row-major 0.633); radius 4
// 0.437 walking but 0.589 still (profiles/r03/sched_walk_dilate.jsonl, DESIGN.md
// 2.6).
constexpr int kSchedDilate = 2;

}  // namespace

rm_status ensure_staging(rm_ctx *ctx, size_t bytes) {
    if (ctx->staging_bytes >= bytes) return RM_OK;
    if (ctx->staging) (void)hipFree(ctx->staging);
    ctx->staging = nullptr;
    ctx->staging_bytes = 0;
    RM_HIP(hipMalloc(&ctx->staging, bytes));
    ctx->staging_bytes = bytes;
    return RM_OK;
}

// rm_params.kernel: 0 auto, 1 = 16x16-pixel workgroups, 2 = 8x8-pixel workgroups
int pick_kernel(const rm_params &p) {
    if (p.kernel == 1) return rm::KERNEL_TILE16;
    if (p.kernel == 3) return rm::KERNEL_TILE16X4;
    if (p.kernel == 4) return rm::KERNEL_PERSIST;
    return rm::KERNEL_TILE8;  // 0 auto, 2: measured fastest on every config
}

// the pose's four plane rotations keep a direction's length (rm_far_sky.h unit_rotation): glsl_cos and glsl_sin
// of one angle do, until the angle is so large that x + pi/2 no longer resolves
static bool pose_keeps_unit(const FrameConst &F) {
    return rmfs::unit_rotation(F.cam1_c, F.cam1_s) && rmfs::unit_rotation(F.cam2_c, F.cam2_s) &&
           rmfs::unit_rotation(F.ry_c, F.ry_s) && rmfs::unit_rotation(F.rx_c, F.rx_s);
}

// The members of F that depend on the pose (u_pos, u_mouse, u_time) and nothing
// else: frame_const below calls it with the context's pose, a view batch
// (rm_batch_host.cpp) once per view with the view's -- one body under this
// file's -ffp-contract=off, so the two paths cannot round differently.
void pose_const(FrameConst &F, const float pos[3], const float mouse[2], float time) {
    F.pos_x = pos[0]; F.pos_y = pos[1]; F.pos_z = pos[2];
    // rot(a) = mat2(cos a, -sin a, sin a, cos a) (common.frag:1088-1092)
    float a1 = -mouse[1], a2 = mouse[0];
    F.cam1_c = rm::glsl_cos(a1); F.cam1_s = rm::glsl_sin(a1);
    F.cam2_c = rm::glsl_cos(a2); F.cam2_s = rm::glsl_sin(a2);
    // transformR(.., vec3(180, u_time * 2, 0)): rotationY(-rot.y), rotationX(-rot.x)
    // with radians(x) = x * pi/180 (common.frag:190-214,434-441)
    float rot_y = time * 2.0f, rot_x = 180.0f;
    float ay = -rot_y * 0.017453292519943295f, ax = -rot_x * 0.017453292519943295f;
    F.ry_c = rm::glsl_cos(ay); F.ry_s = rm::glsl_sin(ay);
    F.rx_c = rm::glsl_cos(ax); F.rx_s = rm::glsl_sin(ax);
    rm::camera_sponge_origin(F);  // (after pos and the sponge rotation)
    // the near-sky ladder is proved for directions of unit length (rm_far_sky.h 3.): a pose whose rotations do not
    // keep it takes the launch's radius back to the far-sky cube's (near_sky_radius; a view batch: any view's)
    if (F.near_r > 0.0f && !pose_keeps_unit(F)) F.near_r = rmfs::near_sky_radius(F.max_steps, false);
    F.time = time;
    F.mouse_x = mouse[0];
    F.mouse_y = mouse[1];
}

// fract(u_seed1) - 0.5 (GLSL fract, x - floor(x)): rm_render_accumulate*'s sub-pixel offset of the fragment
float seed_jitter(float seed) { return (seed - std::floor(seed)) - 0.5f; }

FrameConst frame_const(const rm_ctx *c, int W, int H, const RowPart &part, int nrows) {
    FrameConst F;
    std::memset(&F, 0, sizeof(F));
    F.res_x = c->res_set ? c->res[0] : (float)W;
    F.res_y = c->res_set ? c->res[1] : (float)H;
    // (before pose_const, which withdraws the ladder's radius under a pose it is not proved for)
    F.max_steps = c->params.max_steps;
    F.near_r = c->scene == rm::SCENE_T ? rmfs::near_sky_radius(F.max_steps, true) : 0.0f;
    pose_const(F, c->pos, c->mouse, c->time);
    F.W = W; F.H = H;
    F.cycle = part.cycle; F.offset = part.offset; F.run = part.run; F.nrows = nrows;
    F.run_magic = rm::div_magic((uint32_t)part.run, (uint64_t)H + 1);  // packed rows j < H
    // 0 (unbounded, the reference) travels as INT_MAX: one compare per shadow step
    F.shadow_max_steps = c->params.shadow_max_steps > 0 ? c->params.shadow_max_steps : 0x7fffffff;
    // the far-sky vote of the instrumented kernels, behind rm_stats.skipped: max_steps >= N0 (rm_far_sky.h).  The
    // timed kernels vote at F.near_r (above)
    F.far_sky = c->scene == rm::SCENE_T && F.max_steps >= rmfs::kFarSkyN0 ? 1 : 0;
    F.lat_tiles = lat_tiles_for(pick_kernel(c->params), W, nrows);
    for (int i = 0; i < 32; i++) {
        F.hash11[i] = hash11((float)i);
        F.sss_floor[0][i] = sss_floor_term(1.0f, i);
        F.sss_floor[1][i] = sss_floor_term(0x1.fffffep-1f, i);
    }
    return F;
}

rm_status frame_rcp(rm_ctx *ctx, FrameConst &F) {
    if (ctx->scene != rm::SCENE_S0 && ctx->scene != rm::SCENE_T) return RM_OK;  // (the other scenes divide)
    uint32_t bits;
    std::memcpy(&bits, &F.res_y, sizeof(bits));
    rm_ctx::RcpEntry *hit = nullptr, *lru = &ctx->rcp_cache[0];
    for (int i = 0; i < ctx->rcp_n; i++) {
        rm_ctx::RcpEntry &e = ctx->rcp_cache[i];
        if (e.W == F.W && e.H == F.H && e.res_y_bits == bits) hit = &e;
        if (e.used < lru->used) lru = &e;
    }
    if (!hit) {
        if (!ctx->d_rcp) RM_HIP(hipMalloc(&ctx->d_rcp, 3 * sizeof(float)));
        float v[3];
        hipError_t e = rm::launch_resolution_rcp(F.W, F.H, F.res_y, ctx->d_rcp, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "resolution reciprocal launch");
        RM_HIP(hipMemcpyAsync(v, ctx->d_rcp, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
        RM_HIP(hipStreamSynchronize(ctx->stream));
        hit = ctx->rcp_n < rm_ctx::kRcpEntries ? &ctx->rcp_cache[ctx->rcp_n++] : lru;
        hit->W = F.W; hit->H = F.H; hit->res_y_bits = bits;
        std::memcpy(hit->rcp, v, sizeof(v));
    }
    hit->used = ++ctx->rcp_clock;
    F.rcp_w = hit->rcp[0]; F.rcp_h = hit->rcp[1]; F.rcp_res_y = hit->rcp[2];
    return RM_OK;
}

rm_status render_dev(rm_ctx *ctx, int W, int H, const RowPart &part, int row0, int count, void *out, bool rgba8,
                     rm_stats *stats, uint32_t *evmap, bool accum, const WireOut *wire) {
    rm::TraceRange range("rm_render");
    // the wire's tile code runs in one-wave 8x8 tiles (rm_render_direct.h)
    const int kernel = wire ? (int)rm::KERNEL_TILE8 : pick_kernel(ctx->params);
    FrameConst F = frame_const(ctx, W, H, part, count);
    if (rm_status st = frame_rcp(ctx, F)) return st;
    F.row0 = row0;
    // scenes S0/T: a wave's rows from one scalar division (waves are 8 rows high, 4 in the 16x4 tiling)
    F.tile_run = rm::wave_row_mode(part, row0, kernel == rm::KERNEL_TILE16X4 ? 4 : 8, F.run_magic != 0);

    F.evals_map = evmap;
    if (accum) {  // fract(u_seed1) - 0.5 (GLSL fract, x - floor(x)), per frame
        F.accumulate = 1;
        F.sample_part = ctx->sample_part;
        F.jit_x = seed_jitter(ctx->seed1[0]);
        F.jit_y = seed_jitter(ctx->seed1[1]);
    }
    rm_ctx::Sched *sc = nullptr;
    if (ctx->tile_order) {  // an explicit order wins
        const rm::TileGrid g = rm::tile_grid(ctx->scene == rm::SCENE_PLUGIN ? (int)rm::KERNEL_TILE8 : kernel, W, count);
        if ((int64_t)g.x * g.y == ctx->tile_order_n) F.tile_order = ctx->tile_order;
    } else {
        rm_status st;
        sc = sched_slot(ctx, W, H, part, row0, count, st);
        if (st != RM_OK) return st;
        if (sc) {
            const uint64_t P = kSchedPeriod, k = sc->k;
            // an instrumented launch (count_evals, step maps) takes every reference
            // step, so its tile durations would rank the tiles by work the timed
            // kernels skip: it uses the current order but records no durations and
            // does not advance the geometry's launch count
            if (k % P == 0 && !(ctx->params.count_evals != 0 || evmap))
                F.tile_cost = sc->buf + ((k / P) & 1) * sc->n;  // sort k / P reads them
            if (k >= 1) {  // the newest sort's order (it ran right after launch s * P, same stream)
                const uint64_t s = (k - 1) / P;
                F.tile_order = sc->buf + (2 + (s & 1)) * sc->n;
            }
        }
    }
    rm_ctx::PersistBlock *pb = nullptr;
    if (ctx->scene != rm::SCENE_PLUGIN && kernel == rm::KERNEL_PERSIST) {
        // this stream's counters, zeroed once; each launch leaves them zeroed
        rm_status st = persist_block(ctx, pb);
        if (st != RM_OK) return st;
        F.persist = pb->ctr;
    }
    ctx->last_certified = 0;  // rm_certified_steps(): of this launch alone, set below when it is counted
    ctx->last_refl_cleared = 0;  // rm_reflection_cleared_steps(): likewise
    ctx->last_near_sky = 0;      // rm_near_sky_steps(): likewise
    bool cnt = ctx->params.count_evals != 0 || evmap;
    if (cnt) RM_HIP(hipMemsetAsync(ctx->d_evals, 0, 6 * sizeof(unsigned long long), ctx->stream));
    if (stats) RM_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    hipError_t e =
        wire ? rm::launch_render_wire(ctx->scene, F, static_cast<rm::WireTile *>(out), cnt ? ctx->d_evals : nullptr,
                                      ctx->stream)
        : ctx->scene == rm::SCENE_PLUGIN
            ? rmplugin::launch_render(ctx->plugin, F, ctx->uniform_values, out, rgba8, cnt ? ctx->d_evals : nullptr, ctx->stream)
            : rm::launch_render(ctx->scene, F, out, rgba8, cnt ? ctx->d_evals : nullptr, kernel, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "render kernel launch");
    if (stats) RM_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    if (wire) {  // the offset table, the message size, the payload (rm_wire.hip)
        e = rm::launch_wire_finish(out, W, count, wire->msg, wire->size_out, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "wire scan/compact launch");
    }
    if (pb) RM_HIP(hipEventRecord(pb->last, ctx->stream));
    if (sc && F.tile_cost) {  // sort this launch's durations, on its stream right after it
        const size_t slot = (sc->k / kSchedPeriod) & 1;
        uint32_t *h = sc->buf + 4 * (size_t)sc->n;
        e = rm::launch_tile_order(sc->buf + slot * sc->n, sc->n, sc->gx, kSchedDilate, sc->buf + (2 + slot) * sc->n,
                                  h + 512 * slot, h + 512 * (1 - slot), reinterpret_cast<uint8_t *>(h + 1024),
                                  ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "tile order launch");
    }
    if (sc) {
        sc->dirty = true;  // (marked when the context leaves the stream: rm_set_stream)
        if (!cnt) sc->k++;
    }
    mark_done(ctx);
    if (stats) {
        RM_HIP(hipEventSynchronize(ctx->ev1));
        float ms = 0.0f;
        RM_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        unsigned long long ev[6] = {0, 0, 0, 0, 0, 0};
        if (cnt) RM_HIP(hipMemcpy(ev, ctx->d_evals, sizeof(ev), hipMemcpyDeviceToHost));
        std::memset(stats, 0, sizeof(*stats));
        stats->evals = ev[0];
        stats->flop = ev[1];
        stats->skipped = ev[2];
        ctx->last_certified = ev[3];  // (0 when not counted)
        ctx->last_refl_cleared = ev[4];
        ctx->last_near_sky = ev[5];
        stats->pixels = (uint64_t)W * (uint64_t)count;
        stats->kernel_ms = ms;
        stats->scene = ctx->scene;
        stats->dispatch = !F.tile_order ? RM_DISPATCH_ROW_MAJOR
                          : F.tile_order == ctx->tile_order ? RM_DISPATCH_EXPLICIT
                                                            : RM_DISPATCH_ADAPTIVE;
        // the latency tiles: scene T, an ordered launch of one-wave tiles
        // (rm_render_direct.h render_tile_at)
        if (F.tile_order && ctx->scene == rm::SCENE_T && kernel != rm::KERNEL_TILE16) {
            const rm::TileGrid g = rm::tile_grid(kernel, W, count);
            stats->lat_tiles = std::min(F.lat_tiles, g.x * g.y);
        }
    }
    return RM_OK;
}

// row_count < 0: every packed row from row_begin on; out: float4 or RGBA8 rows
rm_status render_part(rm_ctx *ctx, int W, int H, const RowPart &part, int row_begin, int row_count, void *out,
                      bool rgba8, rm_stats *stats, uint32_t *evmap, bool accum) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (W <= 0 || H <= 0) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "render: bad size");
    if ((long long)W * H > (1LL << 31)) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "render: frame too large");
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    if (ctx->scene == rm::SCENE_PLUGIN && !ctx->plugin.render)
        return fail(ctx, RM_ERR_SCENE, "scene plugin was compiled with RM_PLUGIN_EVAL_ONLY (no render kernel)");
    int n = rows_of_part(H, part);
    if (row_count < 0) row_count = n - row_begin;
    if (row_begin < 0 || row_count < 0 || row_begin + row_count > n)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "render: packed row range outside the shard");
    if (row_count == 0) {  // e.g. more shards than bands: nothing to do
        if (stats) {
            std::memset(stats, 0, sizeof(*stats));
            stats->scene = ctx->scene;
        }
        return RM_OK;
    }
    if (!out) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "render: null output");
    RM_HIP(hipSetDevice(ctx->device));
    const bool dev_out = is_device_ptr(out), dev_map = !evmap || is_device_ptr(evmap);
    if (dev_out && dev_map)
        return render_dev(ctx, W, H, part, row_begin, row_count, out, rgba8, stats, evmap, accum);
    // host buffers go through the staging buffer: the frame, then the step map
    const size_t bytes = dev_out ? 0 : (size_t)W * row_count * (rgba8 ? sizeof(uint32_t) : sizeof(float4));
    const size_t map_bytes = dev_map ? 0 : (size_t)W * row_count * sizeof(uint32_t);
    rm_status s = ensure_staging(ctx, bytes + map_bytes);
    if (s != RM_OK) return s;
    char *st = reinterpret_cast<char *>(ctx->staging);
    uint32_t *map_d = dev_map ? evmap : reinterpret_cast<uint32_t *>(st + bytes);
    if (accum && !dev_out) RM_HIP(hipMemcpyAsync(st, out, bytes, hipMemcpyHostToDevice, ctx->stream));  // u_sample
    s = render_dev(ctx, W, H, part, row_begin, row_count, dev_out ? out : st, rgba8, stats, map_d, accum);
    if (s != RM_OK) return s;
    if (!dev_out) RM_HIP(hipMemcpyAsync(out, st, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (!dev_map) RM_HIP(hipMemcpyAsync(evmap, map_d, map_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RM_HIP(hipStreamSynchronize(ctx->stream));
    return RM_OK;
}

// round-robin bands (band, nshards, shard)
rm_status render_any(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, int row_begin, int row_count,
                     void *out, bool rgba8, rm_stats *stats, uint32_t *evmap, bool accum) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    RowPart part;
    if (W <= 0 || H <= 0 || !band_part(band, nshards, shard, part))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "render: bad size/shard");
    return render_part(ctx, W, H, part, row_begin, row_count, out, rgba8, stats, evmap, accum);
}

}  // namespace rmhost
