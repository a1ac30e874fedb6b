// rm_capi.cpp -- the C ABI declared in include/rm.h: the entry points, their
// argument checks and messages.  The context is rm_ctx.h; a render launch is
// rm_render_host.cpp, stream and event lifetime rm_ctx_streams.cpp, scene-file
// text rm_scene_file.cpp; the post passes are rm_post_host.cpp.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "rm_ctx.h"
#include "rm_internal.h"
#include "rm_scene_file.h"
#include "rm_stage.h"

using rm::cycle_part;
using rm::FrameConst;
using rm::RowPart;
using rm::rows_of_part;
using namespace rmhost;

static_assert(rmscene::kSceneS0 == rm::SCENE_S0 && rmscene::kSceneT == rm::SCENE_T &&
                  rmscene::kSceneO == rm::SCENE_O && rmscene::kSceneOG == rm::SCENE_OG &&
                  rmscene::kScenePlugin == rm::SCENE_PLUGIN,
              "rm_scene_file.h restates rm::SceneId");

namespace {

// The compressed wire's one size rule (include/rm.h), checked by every entry
// point that sizes, writes or reads a message before it touches a pointer: a
// part of nrows rows of W pixels must fit the launches (tile rows in grid.y)
// and the table entry's 27-bit word offset (rm_wire.hip: off << 5 | cnt), for
// a message whose every tile takes all of its kTileWords words.
bool wire_part_ok(int W, int nrows) {
    if (W <= 0 || W > (1 << 18) || nrows < 0 || nrows > 65535) return false;
    const int64_t T = (int64_t)((W + 7) / 8) * ((nrows + 7) / 8);
    const int64_t words = ((int64_t)rm::wire_capacity(W, nrows) - 8 - ((4 * T + 7) & ~(int64_t)7)) / 8;  // kTileWords T
    return words < ((int64_t)1 << 27);
}

}  // namespace

int rm_internal_device(const rm_ctx *ctx) { return ctx->device; }
rm_status rm_internal_mark_done(rm_ctx *ctx) {
    mark_done(ctx);
    return RM_OK;
}
hipStream_t rm_internal_stream(const rm_ctx *ctx) { return ctx->stream; }
int rm_internal_scene(const rm_ctx *ctx) { return ctx->scene; }
void rm_internal_set_error(rm_ctx *ctx, const std::string &msg) { ctx->err = msg; }

extern "C" {

rm_status rm_create(rm_ctx **out, int device) {
    if (!out) return RM_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        (void)hipGetLastError();
        return RM_ERR_DEVICE;
    }
    rm_ctx *ctx = new rm_ctx();
    ctx->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&ctx->d_evals, 6 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev0);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->done, hipEventDisableTiming);
    ctx->persist.reserve(rm_ctx::kPersistBlocks);
    if (e != hipSuccess) {
        rm_destroy(ctx);
        return e == hipErrorOutOfMemory ? RM_ERR_OUT_OF_MEMORY : RM_ERR_DEVICE;
    }
    *out = ctx;
    return RM_OK;
}

rm_status rm_destroy(rm_ctx *ctx) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    (void)hipSetDevice(ctx->device);
    wait_idle(ctx);
    rmplugin::unload(ctx->plugin);
    if (ctx->d_evals) (void)hipFree(ctx->d_evals);
    if (ctx->d_rcp) (void)hipFree(ctx->d_rcp);
    for (auto &b : ctx->persist) {
        if (b.ctr) (void)hipFree(b.ctr);
        if (b.last) (void)hipEventDestroy(b.last);
    }
    if (ctx->staging) (void)hipFree(ctx->staging);
    for (rm_ctx::Scratch &sc : ctx->scratch) scratch_free(sc);
    if (ctx->aa_ev2) (void)hipEventDestroy(ctx->aa_ev2);
    for (auto &b : ctx->batch_slot) {  // (wait_idle above: no upload still reads a block)
        if (b.host) (void)hipHostFree(b.host);
        if (b.copied) (void)hipEventDestroy(b.copied);
    }
    if (ctx->tile_order) (void)hipFree(ctx->tile_order);
    for (rm_ctx::Sched &e : ctx->sched) (void)sched_release(ctx, e);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->done) (void)hipEventDestroy(ctx->done);
    delete ctx;
    return RM_OK;
}

rm_status rm_load_scene(rm_ctx *ctx, const char *file_name) {
    if (!ctx || !file_name) return RM_ERR_INVALID_ARGUMENT;
    std::string file(file_name);
    int sc = rmscene::scene_of(rmscene::base_name(file));
    std::ifstream probe(file);
    bool exists = probe.is_open();
    probe.close();
    rmuniform::Table uniforms;  // what the scene declares (a built-in scene: none)
    if (exists) {
        std::string src, err;
        rm_status st = rmscene::load_scene_file(file, sc, src, err);
        if (st != RM_OK) {
            std::fprintf(stderr, "%s\n", err.c_str());
            return fail(ctx, st, err);
        }
        if (sc == rm::SCENE_PLUGIN) {
            // a scene plugin: compiled like the reference's shader reload; on
            // failure the previous scene stays loaded
            rmplugin::Code code;
            std::string log;
            if (!rmplugin::compile(src, file, code, log, uniforms)) {
                std::fprintf(stderr, "%s\n", log.c_str());
                return fail(ctx, RM_ERR_SCENE, "scene plugin \"" + file + "\" failed to compile:\n" + log);
            }
            RM_HIP(hipSetDevice(ctx->device));
            // kernels of the previous code object may still run on the stream
            RM_HIP(hipStreamSynchronize(ctx->stream));
            hipError_t e = rmplugin::load(code, uniforms.slots, ctx->plugin);
            if (e != hipSuccess) return hip_fail(ctx, e, "scene plugin module load");
            // (what the batch form is compiled from on its first use, rm_render_batch_ex)
            ctx->plugin.src = src;
            ctx->plugin.file = file;
        }
    } else if (sc < 0) {
        std::string err = "ShaderLoader: can't load file \"" + file + "\"";
        std::fprintf(stderr, "%s\n", err.c_str());
        return fail(ctx, RM_ERR_FILE, err);
    }
    ctx->scene = sc;
    ctx->scene_file = file;
    // a loaded scene starts from its declarations' defaults, as a fresh GL
    // program does (the reference's reload makes a new program)
    uniforms.defaults(ctx->uniform_values);
    ctx->uniforms = std::move(uniforms);
    ctx->err.clear();
    return RM_OK;
}

// The seven uniforms of the pass (common.frag:4-11), then the ones the loaded
// scene declares; any other name warns once and is ignored.
struct PassUniform { const char *name; int n; };
static const PassUniform kPassUniforms[] = {{"u_resolution", 2}, {"u_pos", 3}, {"u_mouse", 2}, {"u_time", 1},
                                            {"u_sample_part", 1}, {"u_seed1", 2}, {"u_seed2", 2}};

static rm_status warn_unknown(rm_ctx *ctx, const char *name) {
    if (ctx->warned.insert(name).second) std::fprintf(stderr, "rm: uniform \"%s\" not found in shader\n", name);
    return RM_OK;
}

static rm_status long_name(rm_ctx *ctx, const char *name) {
    return fail(ctx, RM_ERR_INVALID_ARGUMENT, "uniform name of " + std::to_string(std::strlen(name)) +
                                                  " characters (at most " + std::to_string(rmuniform::kMaxName) + ")");
}

static rm_status wrong_type(rm_ctx *ctx, const rmuniform::Decl &d, const std::string &got) {
    return fail(ctx, RM_ERR_INVALID_ARGUMENT,
                "uniform \"" + d.name + "\" is declared " + rmuniform::type_name(d) + ", got " + got);
}

static std::string floats_name(int n, int count = 1) {
    return (n == 1 ? std::string("float") : "vec" + std::to_string(n)) +
           (count > 1 ? "[" + std::to_string(count) + "]" : std::string());
}

static rm_status set_uniform(rm_ctx *ctx, const char *name, int n, float x, float y, float z, float w = 0.0f) {
    if (!ctx || !name) return RM_ERR_INVALID_ARGUMENT;
    if (std::strlen(name) > (size_t)rmuniform::kMaxName) return long_name(ctx, name);
    std::string nm(name);
    for (const PassUniform &u : kPassUniforms) {
        if (nm != u.name) continue;
        if (n != u.n) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "uniform \"" + nm + "\" has " + std::to_string(u.n) +
                                                                    " components, got " +
                                                                    (n ? std::to_string(n) : std::string("an int")));
        if (nm == "u_resolution") { ctx->res[0] = x; ctx->res[1] = y; ctx->res_set = true; }
        else if (nm == "u_pos") { ctx->pos[0] = x; ctx->pos[1] = y; ctx->pos[2] = z; }
        else if (nm == "u_mouse") { ctx->mouse[0] = x; ctx->mouse[1] = y; }
        else if (nm == "u_time") ctx->time = x;
        // u_sample_part, u_seed1, u_seed2: declared, unused by the reference's pass
        // (common.frag:8-11); rm_render_accumulate* reads them
        else if (nm == "u_sample_part") ctx->sample_part = x;
        else if (nm == "u_seed1") { ctx->seed1[0] = x; ctx->seed1[1] = y; }
        else if (nm == "u_seed2") { ctx->seed2[0] = x; ctx->seed2[1] = y; }
        return RM_OK;
    }
    if (const rmuniform::Decl *d = ctx->uniforms.find(nm)) {
        if (d->type != rmuniform::kFloat || d->count || d->components != n) return wrong_type(ctx, *d, floats_name(n));
        const float v[4] = {x, y, z, w};
        std::memcpy(ctx->uniform_values + 4 * d->slot, v, (size_t)n * sizeof(float));
        return RM_OK;
    }
    return warn_unknown(ctx, name);
}

rm_status rm_set_uniform1f(rm_ctx *ctx, const char *name, float x) { return set_uniform(ctx, name, 1, x, 0, 0); }
rm_status rm_set_uniform2f(rm_ctx *ctx, const char *name, float x, float y) {
    return set_uniform(ctx, name, 2, x, y, 0);
}
rm_status rm_set_uniform3f(rm_ctx *ctx, const char *name, float x, float y, float z) {
    return set_uniform(ctx, name, 3, x, y, z);
}
rm_status rm_set_uniform4f(rm_ctx *ctx, const char *name, float x, float y, float z, float w) {
    return set_uniform(ctx, name, 4, x, y, z, w);
}

rm_status rm_set_uniform1i(rm_ctx *ctx, const char *name, int32_t v) {
    if (!ctx || !name) return RM_ERR_INVALID_ARGUMENT;
    if (std::strlen(name) > (size_t)rmuniform::kMaxName) return long_name(ctx, name);
    if (const rmuniform::Decl *d = ctx->uniforms.find(name)) {
        if (d->type == rmuniform::kFloat) return wrong_type(ctx, *d, "int");
        ctx->uniform_values[4 * d->slot] = d->type == rmuniform::kBool ? (uint32_t)(v != 0) : (uint32_t)v;
        return RM_OK;
    }
    return set_uniform(ctx, name, 0, 0, 0, 0);  // a float uniform of the pass (refused), or an unknown name
}

rm_status rm_set_uniformfv(rm_ctx *ctx, const char *name, int components, const float *v, int count) {
    if (!ctx || !name) return RM_ERR_INVALID_ARGUMENT;
    if (!v || components < 1 || components > 4 || count < 1)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_set_uniformfv: bad arguments");
    if (std::strlen(name) > (size_t)rmuniform::kMaxName) return long_name(ctx, name);
    const rmuniform::Decl *d = ctx->uniforms.find(name);
    if (!d || !d->count) {  // not an array: the plain setter of that arity, for one element
        if (count == 1) return set_uniform(ctx, name, components, v[0], components > 1 ? v[1] : 0.0f,
                                           components > 2 ? v[2] : 0.0f, components > 3 ? v[3] : 0.0f);
        if (d) return wrong_type(ctx, *d, floats_name(components, count));
        for (const PassUniform &u : kPassUniforms)
            if (std::strcmp(name, u.name) == 0)
                return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string("uniform \"") + name + "\" is not an array");
        return warn_unknown(ctx, name);
    }
    if (d->components != components || count > d->count) return wrong_type(ctx, *d, floats_name(components, count));
    for (int i = 0; i < count; i++)
        std::memcpy(ctx->uniform_values + 4 * (d->slot + i), v + (size_t)i * components, (size_t)components * sizeof(float));
    return RM_OK;
}

rm_status rm_uniform_count(rm_ctx *ctx, int *n) {
    if (!ctx || !n) return RM_ERR_INVALID_ARGUMENT;
    *n = (int)ctx->uniforms.decls.size();
    return RM_OK;
}

rm_status rm_uniform_info_at(rm_ctx *ctx, int index, rm_uniform_info *out) {
    if (!ctx || !out) return RM_ERR_INVALID_ARGUMENT;
    if (index < 0 || index >= (int)ctx->uniforms.decls.size())
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_uniform_info_at: index outside [0, rm_uniform_count)");
    const rmuniform::Decl &d = ctx->uniforms.decls[(size_t)index];
    static_assert(sizeof(out->name) == rmuniform::kMaxName + 1, "rm_uniform_info.name");
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->name, d.name.c_str(), d.name.size());
    out->type = d.type;
    out->components = d.components;
    out->count = d.count;
    return RM_OK;
}

rm_status rm_get_uniformfv(rm_ctx *ctx, const char *name, float *v, int capacity, int *written) {
    if (!ctx || !name || !v) return RM_ERR_INVALID_ARGUMENT;
    const rmuniform::Decl *d = ctx->uniforms.find(name);
    if (!d) return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string("the loaded scene declares no uniform \"") + name + "\"");
    if (d->type != rmuniform::kFloat) return wrong_type(ctx, *d, "a read of floats");
    const int n = d->components * d->slots();
    if (capacity < n)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "uniform \"" + d->name + "\" (" + rmuniform::type_name(*d) + ") has " +
                                                      std::to_string(n) + " floats, capacity " + std::to_string(capacity));
    for (int i = 0; i < d->slots(); i++)
        std::memcpy(v + (size_t)i * d->components, ctx->uniform_values + 4 * (d->slot + i),
                    (size_t)d->components * sizeof(float));
    if (written) *written = n;
    return RM_OK;
}

rm_status rm_get_uniform1i(rm_ctx *ctx, const char *name, int32_t *v) {
    if (!ctx || !name || !v) return RM_ERR_INVALID_ARGUMENT;
    const rmuniform::Decl *d = ctx->uniforms.find(name);
    if (!d) return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string("the loaded scene declares no uniform \"") + name + "\"");
    if (d->type == rmuniform::kFloat) return wrong_type(ctx, *d, "a read of an int");
    *v = (int32_t)ctx->uniform_values[4 * d->slot];
    return RM_OK;
}

static_assert((int)RM_UNIFORM_FLOAT == (int)rmuniform::kFloat && (int)RM_UNIFORM_INT == (int)rmuniform::kInt &&
                  (int)RM_UNIFORM_BOOL == (int)rmuniform::kBool,
              "rm_uniform_type and rm_uniform_decl.h");

rm_status rm_set_params(rm_ctx *ctx, const rm_params *p) {
    if (!ctx || !p) return RM_ERR_INVALID_ARGUMENT;
    if (p->max_steps < 0 || p->max_steps > (1 << 20) || p->shadow_max_steps < 0 || p->kernel < 0 || p->kernel > 4 ||
        p->schedule < 0 || p->schedule > 1)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_set_params: out of range");
    ctx->params = *p;
    return RM_OK;
}

rm_status rm_get_params(rm_ctx *ctx, rm_params *p) {
    if (!ctx || !p) return RM_ERR_INVALID_ARGUMENT;
    *p = ctx->params;
    return RM_OK;
}

rm_status rm_set_stream(rm_ctx *ctx, void *stream) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    return set_stream(ctx, reinterpret_cast<hipStream_t>(stream));
}

rm_status rm_set_stream_kept(rm_ctx *ctx, void *stream) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!is_kept(ctx, s)) ctx->kept.push_back(s);
    return rm_set_stream(ctx, stream);
}

rm_status rm_synchronize(rm_ctx *ctx) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    RM_HIP(hipStreamSynchronize(ctx->stream));
    return RM_OK;
}

rm_status rm_render(rm_ctx *ctx, int W, int H, float *out, rm_stats *stats) {
    return render_any(ctx, W, H, H > 0 ? H : 1, 1, 0, 0, -1, out, false, stats);
}

rm_status rm_render_step_map(rm_ctx *ctx, int W, int H, float *out, uint32_t *evals_map, rm_stats *stats) {
    if (!evals_map) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_render_step_map: null evals_map");
    return render_any(ctx, W, H, H > 0 ? H : 1, 1, 0, 0, -1, out, false, stats, evals_map);
}

rm_status rm_render_band(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, float *out, rm_stats *stats) {
    return render_any(ctx, W, H, band, nshards, shard, 0, -1, out, false, stats);
}

rm_status rm_render_rows(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, int row_begin, int row_count,
                         float *out, rm_stats *stats) {
    if (row_count < 0) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_render_rows: negative row_count");
    return render_any(ctx, W, H, band, nshards, shard, row_begin, row_count, out, false, stats);
}

rm_status rm_render_rgba8(rm_ctx *ctx, int W, int H, uint32_t *out, rm_stats *stats) {
    return render_any(ctx, W, H, H > 0 ? H : 1, 1, 0, 0, -1, out, true, stats);
}

rm_status rm_render_accumulate(rm_ctx *ctx, int W, int H, float *accum, rm_stats *stats) {
    return render_any(ctx, W, H, H > 0 ? H : 1, 1, 0, 0, -1, accum, false, stats, nullptr, true);
}

rm_status rm_render_accumulate_rgba8(rm_ctx *ctx, int W, int H, uint32_t *accum, rm_stats *stats) {
    return render_any(ctx, W, H, H > 0 ? H : 1, 1, 0, 0, -1, accum, true, stats, nullptr, true);
}

rm_status rm_render_band_rgba8(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, uint32_t *out,
                               rm_stats *stats) {
    return render_any(ctx, W, H, band, nshards, shard, 0, -1, out, true, stats);
}

rm_status rm_render_rows_rgba8(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, int row_begin,
                               int row_count, uint32_t *out, rm_stats *stats) {
    if (row_count < 0) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_render_rows_rgba8: negative row_count");
    return render_any(ctx, W, H, band, nshards, shard, row_begin, row_count, out, true, stats);
}

rm_status rm_cycle_rows(int H, int cycle, int offset, int run, int *nrows) {
    RowPart p;
    if (!nrows || H <= 0 || !cycle_part(cycle, offset, run, p)) return RM_ERR_INVALID_ARGUMENT;
    *nrows = rows_of_part(H, p);
    return RM_OK;
}

rm_status rm_render_cycle_rows(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int row_begin,
                               int row_count, float *out, rm_stats *stats) {
    RowPart p;
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!cycle_part(cycle, offset, run, p) || row_count < 0)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_render_cycle_rows: bad cycle/offset/run/row_count");
    return render_part(ctx, W, H, p, row_begin, row_count, out, false, stats);
}

rm_status rm_render_cycle_rows_rgba8(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int row_begin,
                                     int row_count, uint32_t *out, rm_stats *stats) {
    RowPart p;
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!cycle_part(cycle, offset, run, p) || row_count < 0)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_render_cycle_rows_rgba8: bad cycle/offset/run/row_count");
    return render_part(ctx, W, H, p, row_begin, row_count, out, true, stats);
}

rm_status rm_render_cycle_rows_wire(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int row_begin,
                                    int row_count, uint8_t *msg, void *workspace, int64_t *size_out, rm_stats *stats) {
    RowPart p;
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!wire_part_ok(W, row_count) || !cycle_part(cycle, offset, run, p) || !msg || !workspace)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_render_cycle_rows_wire: bad arguments");
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    if (ctx->scene == rm::SCENE_PLUGIN)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT,
                    "rm_render_cycle_rows_wire: built-in scenes only (a plugin part: rm_render_cycle_rows_rgba8 + "
                    "rm_wire_encode)");
    if (!is_device_ptr(msg) || !is_device_ptr(workspace) || (size_out && !is_device_ptr(size_out)))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_render_cycle_rows_wire: device pointers required");
    const int n = rows_of_part(H, p);
    if (row_begin < 0 || row_begin + row_count > n)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_render_cycle_rows_wire: packed row range outside the part");
    RM_HIP(hipSetDevice(ctx->device));
    const WireOut wo{msg, reinterpret_cast<long long *>(size_out)};
    if (row_count == 0) {  // an empty message (the table of no tiles)
        hipError_t e = rm::launch_wire_finish(workspace, W, 0, msg, wo.size_out, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "wire scan launch");
        if (stats) {
            std::memset(stats, 0, sizeof(*stats));
            stats->scene = ctx->scene;
        }
        mark_done(ctx);
        return RM_OK;
    }
    return render_dev(ctx, W, H, p, row_begin, row_count, workspace, true, stats, nullptr, false, &wo);
}

rm_status rm_deinterleave_cycle_rgb8(rm_ctx *ctx, int W, int H, int cycle, int nparts, const int *offsets,
                                     const int *runs, const int64_t *part_bytes, const uint8_t *gathered,
                                     uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (W <= 0 || H <= 0 || cycle <= 0 || nparts < 1 || nparts > rm::kMaxCycleParts || !offsets || !runs ||
        !part_bytes || !gathered || !out)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_deinterleave_cycle_rgb8: bad arguments");
    rm::CycleParts parts;
    std::memset(&parts, 0, sizeof(parts));
    parts.n = nparts;
    int next = 0;  // the parts, in order, tile [0, cycle)
    for (int i = 0; i < nparts; i++) {
        RowPart p;
        if (offsets[i] != next || !cycle_part(cycle, offsets[i], runs[i], p) || part_bytes[i] < 0)
            return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_deinterleave_cycle_rgb8: parts must tile [0, cycle) in order");
        next += runs[i];
        parts.off[i] = offsets[i];
        parts.run[i] = runs[i];
        parts.base[i] = part_bytes[i];
    }
    if (next != cycle) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_deinterleave_cycle_rgb8: parts must tile [0, cycle)");
    if (!is_device_ptr(gathered) || !is_device_ptr(out))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_deinterleave_cycle_rgb8: device pointers required");
    return launch_on(ctx, "deinterleave launch",
                     [&] { return rm::launch_deinterleave_cycle_rgb8(gathered, out, W, H, cycle, parts, ctx->stream); });
}

int64_t rm_wire_capacity(int W, int nrows) {
    return wire_part_ok(W, nrows) ? (int64_t)rm::wire_capacity(W, nrows) : -1;
}

int64_t rm_wire_workspace_bytes(int W, int nrows) {
    return wire_part_ok(W, nrows) ? (int64_t)rm::wire_workspace(W, nrows) : -1;
}

rm_status rm_wire_encode(rm_ctx *ctx, int W, int nrows, const uint32_t *rows, uint8_t *msg, void *workspace,
                         int64_t *size_out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!wire_part_ok(W, nrows) || !msg || !workspace || (nrows > 0 && !rows))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_wire_encode: bad arguments");
    if (!is_device_ptr(msg) || !is_device_ptr(workspace) || (nrows > 0 && !is_device_ptr(rows)) ||
        (size_out && !is_device_ptr(size_out)))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_wire_encode: device pointers required");
    return launch_on(ctx, "wire encode launch", [&] {
        return rm::launch_wire_encode(rows, W, nrows, msg, workspace, reinterpret_cast<long long *>(size_out), ctx->stream);
    });
}

rm_status rm_wire_decode(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int nrows, const uint8_t *msg,
                         uint32_t *frame) {
    RowPart p;
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!wire_part_ok(W, nrows) || H <= 0 || !cycle_part(cycle, offset, run, p) || nrows > rows_of_part(H, p) ||
        !msg || !frame)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_wire_decode: bad arguments");
    if (!is_device_ptr(msg) || !is_device_ptr(frame))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_wire_decode: device pointers required");
    return launch_on(ctx, "wire decode launch",
                     [&] { return rm::launch_wire_decode(msg, nrows, W, cycle, offset, run, frame, ctx->stream); });
}

rm_status rm_wire_decode_parts(rm_ctx *ctx, int W, int H, int cycle, int nparts, const int *offsets, const int *runs,
                               const int *nrows, const uint8_t *const *msgs, uint32_t *frame) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (W <= 0 || W > (1 << 18) || H <= 0 || nparts < 0 || nparts > rm::kMaxWireParts || !frame ||
        (nparts > 0 && (!offsets || !runs || !nrows || !msgs)))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_wire_decode_parts: bad arguments");
    rm::WireParts parts;
    std::memset(&parts, 0, sizeof(parts));
    parts.n = nparts;
    parts.cycle = cycle;
    for (int i = 0; i < nparts; i++) {
        RowPart p;
        if (!wire_part_ok(W, nrows[i]) || !cycle_part(cycle, offsets[i], runs[i], p) ||
            nrows[i] > rows_of_part(H, p) || !msgs[i] || !is_device_ptr(msgs[i]))
            return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_wire_decode_parts: bad part");
        parts.part[i] = rm::WirePart{msgs[i], nrows[i], offsets[i], runs[i]};
    }
    if (!is_device_ptr(frame)) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_wire_decode_parts: device frame required");
    return launch_on(ctx, "wire decode launch", [&] { return rm::launch_wire_decode_parts(parts, W, frame, ctx->stream); });
}

rm_status rm_scatter_part_rgba8(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int nrows,
                                const uint32_t *rows, uint32_t *frame) {
    RowPart p;
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (W <= 0 || H <= 0 || !cycle_part(cycle, offset, run, p) || nrows < 0 || nrows > rows_of_part(H, p) ||
        !frame || (nrows > 0 && !rows))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_scatter_part_rgba8: bad arguments");
    if (!is_device_ptr(frame) || (nrows > 0 && !is_device_ptr(rows)))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_scatter_part_rgba8: device pointers required");
    return launch_on(ctx, "scatter launch",
                     [&] { return rm::launch_scatter_part(rows, nrows, W, cycle, offset, run, frame, ctx->stream); });
}

rm_status rm_set_tile_order(rm_ctx *ctx, const uint32_t *order, int64_t n) {
    if (!ctx || n < 0 || (n > 0 && !order)) return RM_ERR_INVALID_ARGUMENT;
    RM_HIP(hipSetDevice(ctx->device));
    if (ctx->tile_order) RM_HIP(hipFree(ctx->tile_order));
    ctx->tile_order = nullptr;
    ctx->tile_order_n = 0;
    if (n == 0) return RM_OK;
    std::vector<uint32_t> h((size_t)n);
    RM_HIP(hipMemcpy(h.data(), order, (size_t)n * sizeof(uint32_t), hipMemcpyDefault));
    std::vector<char> seen((size_t)n, 0);  // a permutation of [0, n)
    for (uint32_t t : h) {
        if (t >= (uint64_t)n || seen[t]) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_set_tile_order: not a permutation");
        seen[t] = 1;
    }
    RM_HIP(hipMalloc(&ctx->tile_order, (size_t)n * sizeof(uint32_t)));
    RM_HIP(hipMemcpy(ctx->tile_order, h.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->tile_order_n = n;
    return RM_OK;
}

rm_status rm_tile_grid(const rm_params *p, int W, int rows, int *tiles_x, int *tiles_y) {
    if (!p || !tiles_x || !tiles_y || W <= 0 || rows <= 0) return RM_ERR_INVALID_ARGUMENT;
    const rm::TileGrid g = rm::tile_grid(pick_kernel(*p), W, rows);
    *tiles_x = g.x;
    *tiles_y = g.y;
    return RM_OK;
}

rm_status rm_shard_rows(int H, int band, int nshards, int shard, int *nrows) {
    if (!nrows || H <= 0 || band <= 0 || nshards <= 0 || shard < 0 || shard >= nshards) return RM_ERR_INVALID_ARGUMENT;
    RowPart p;
    *nrows = rm::band_part(band, nshards, shard, p) ? rows_of_part(H, p) : 0;  // (0: band * nshards overflows)
    return RM_OK;
}

// 0: float4, 1: RGBA8 words, 2: RGB8 wire -> RGBA8 words
static rm_status deinterleave_any(rm_ctx *ctx, int W, int H, int band, int nshards, int rows_per_shard,
                                  const void *gathered, void *out, int kind) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!gathered || !out || W <= 0 || H <= 0 || band <= 0 || nshards <= 0)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_deinterleave: bad arguments");
    for (int s = 0; s < nshards; s++) {
        RowPart p;
        if (rm::band_part(band, nshards, s, p) && rows_of_part(H, p) > rows_per_shard)
            return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_deinterleave: rows_per_shard too small");
    }
    if (!is_device_ptr(gathered) || !is_device_ptr(out))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_deinterleave: device pointers required");
    return launch_on(ctx, "deinterleave launch", [&] {
        return kind == 2 ? rm::launch_deinterleave_rgb8(reinterpret_cast<const uint8_t *>(gathered),
                                                       reinterpret_cast<uint32_t *>(out), W, H, band, nshards,
                                                       rows_per_shard, ctx->stream)
               : kind == 1 ? rm::launch_deinterleave_u32(reinterpret_cast<const uint32_t *>(gathered),
                                                         reinterpret_cast<uint32_t *>(out), W, H, band, nshards,
                                                         rows_per_shard, ctx->stream)
                           : rm::launch_deinterleave(reinterpret_cast<const float4 *>(gathered),
                                                     reinterpret_cast<float4 *>(out), W, H, band, nshards,
                                                     rows_per_shard, ctx->stream);
    });
}

rm_status rm_deinterleave(rm_ctx *ctx, int W, int H, int band, int nshards, int rows_per_shard, const float *gathered,
                          float *out) {
    return deinterleave_any(ctx, W, H, band, nshards, rows_per_shard, gathered, out, 0);
}

rm_status rm_deinterleave_rgba8(rm_ctx *ctx, int W, int H, int band, int nshards, int rows_per_shard,
                                const uint32_t *gathered, uint32_t *out) {
    return deinterleave_any(ctx, W, H, band, nshards, rows_per_shard, gathered, out, 1);
}

rm_status rm_deinterleave_rgb8(rm_ctx *ctx, int W, int H, int band, int nshards, int rows_per_shard,
                               const uint8_t *gathered, uint32_t *out) {
    return deinterleave_any(ctx, W, H, band, nshards, rows_per_shard, gathered, out, 2);
}

rm_status rm_pack_rgb8(rm_ctx *ctx, int64_t npixels, const uint32_t *in, uint8_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (npixels == 0) return RM_OK;  // an empty shard (more shards than row bands)
    if (!in || !out || npixels < 0) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_pack_rgb8: bad arguments");
    if (!is_device_ptr(in) || !is_device_ptr(out))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_pack_rgb8: device pointers required");
    return launch_on(ctx, "pack_rgb8 launch", [&] { return rm::launch_pack_rgb8(in, out, (size_t)npixels, ctx->stream); });
}

rm_status rm_pack_rgba8(rm_ctx *ctx, int64_t npixels, const float *in, uint32_t *out) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (!in || !out || npixels < 0) return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_pack_rgba8: bad arguments");
    if (!is_device_ptr(in) || !is_device_ptr(out))
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, "rm_pack_rgba8: device pointers required");
    return launch_on(ctx, "pack launch", [&] {
        return rm::launch_pack_rgba8(reinterpret_cast<const float4 *>(in), out, (size_t)npixels, ctx->stream);
    });
}

// rm_scene_eval and rm_scene_eval_form.  RM_FORM_EXACT launches rm_scene_eval's
// kernel (and, for aux alone, the probe kernel without its other outputs).
static rm_status scene_eval_form(rm_ctx *ctx, const float *points, int64_t n, int form, float *dist, float *material,
                                 float *aux, const char *what) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!points || !dist)) || form < 0 || form >= rm::kFormCount)
        return fail(ctx, RM_ERR_INVALID_ARGUMENT, std::string(what) + ": bad arguments");
    if (ctx->scene < 0) return fail(ctx, RM_ERR_NO_SCENE, "no scene loaded (rm_load_scene)");
    const bool plugin = ctx->scene == rm::SCENE_PLUGIN;
    if (plugin && form != RM_FORM_EXACT && !ctx->plugin.eval_probe)
        return fail(ctx, RM_ERR_SCENE, std::string(what) + ": the scene plugin has no probe-form kernel "
                                                           "(#define RM_PLUGIN_EVAL_PROBE in the scene source)");
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(ctx->device));
    // device views of the four buffers (host ones are staged, each on its own: the call takes a mixture)
    const size_t pb = (size_t)n * 3 * sizeof(float), db = (size_t)n * sizeof(float), mb = (size_t)n * 16 * sizeof(float);
    Stage stage;
    auto view = [&](const float *buf, size_t bytes, bool in) {
        return !buf || is_device_ptr(buf) ? -1 : stage.add(buf, bytes, in, !in);
    };
    const int ip = view(points, pb, true), id = view(dist, db, false), im = view(material, mb, false),
              ia = view(aux, db, false);
    rm_status st = stage.begin(ctx, what);
    const float *p = ip < 0 ? points : stage.dev<float>(ip);
    float *d = id < 0 ? dist : stage.dev<float>(id);
    float *m = im < 0 ? material : stage.dev<float>(im);
    float *a = ia < 0 ? aux : stage.dev<float>(ia);
    hipError_t e = hipSuccess;
    FrameConst F = frame_const(ctx, 1, 1, RowPart{1, 0, 1}, 1);
    auto probe = [&](int f, float *pd, float *pm) {
        return plugin ? rmplugin::launch_eval_probe(ctx->plugin, F, ctx->uniform_values, p, n, pd, pm, a, ctx->stream)
                      : rm::launch_scene_eval_form(ctx->scene, F, p, n, f, pd, pm, a, ctx->stream);
    };
    if (st == RM_OK && form == RM_FORM_EXACT) {
        e = plugin ? rmplugin::launch_eval(ctx->plugin, F, ctx->uniform_values, p, n, d, m, ctx->stream)
                   : rm::launch_scene_eval(ctx->scene, F, p, n, d, m, ctx->stream);
        if (e == hipSuccess && a)  // (a plugin's aux is 0)
            e = plugin ? hipMemsetAsync(a, 0, db, ctx->stream) : probe(RM_FORM_PROBE, nullptr, nullptr);
    } else if (st == RM_OK) {
        e = probe(form, d, m);
    }
    if (e != hipSuccess) st = hip_fail(ctx, e, what);
    if (stage.staged()) return stage.end(ctx, st, what);
    if (st == RM_OK) e = hipStreamSynchronize(ctx->stream);  // (device buffers: the call waits all the same)
    return e != hipSuccess && st == RM_OK ? hip_fail(ctx, e, what) : st;
}

rm_status rm_scene_eval(rm_ctx *ctx, const float *points, int64_t n, float *dist, float *material) {
    return scene_eval_form(ctx, points, n, RM_FORM_EXACT, dist, material, nullptr, "rm_scene_eval");
}

static_assert(RM_FORM_EXACT == rm::kFormExact && RM_FORM_PROBE == rm::kFormProbe &&
                  RM_FORM_PROBE_NB1 == rm::kFormProbeNb1,
              "rm.h's rm_form are scene_eval_one's FORM");

rm_status rm_scene_eval_form(rm_ctx *ctx, const float *points, int64_t n, int form, float *dist, float *material,
                             float *aux) {
    return scene_eval_form(ctx, points, n, form, dist, material, aux, "rm_scene_eval_form");
}

// rm_compile_scene; form: the batch, the AA or the batch-AA form of the code object (rm_compile_scene_batch,
// rm_compile_scene_aa, rm_compile_scene_batch_aa)
static rm_status compile_scene(const char *file_name, char *log, size_t log_size, rmplugin::Form form) {
    if (!file_name) return RM_ERR_INVALID_ARGUMENT;
    std::string src, err, clog;
    int sc = -1;
    rm_status st = rmscene::load_scene_file(file_name, sc, src, err);
    if (st != RM_OK) {
        clog = err;
    } else if (sc != rm::SCENE_PLUGIN) {
        clog = "compiled-in scene " + std::string(sc == rm::SCENE_T ? "T" : sc == rm::SCENE_O ? "O" : "(built-in)");
    } else {
        rmplugin::Code code;
        rmuniform::Table uniforms;
        if (!rmplugin::compile(src, file_name, code, clog, uniforms, form)) st = RM_ERR_SCENE;
    }
    if (log && log_size > 0) {
        size_t k = clog.size() < log_size - 1 ? clog.size() : log_size - 1;
        std::memcpy(log, clog.data(), k);
        log[k] = '\0';
    }
    return st;
}

rm_status rm_compile_scene(const char *file_name, char *log, size_t log_size) {
    return compile_scene(file_name, log, log_size, rmplugin::FORM_FRAME);
}

rm_status rm_compile_scene_batch(const char *file_name, char *log, size_t log_size) {
    return compile_scene(file_name, log, log_size, rmplugin::FORM_BATCH);
}

rm_status rm_compile_scene_aa(const char *file_name, char *log, size_t log_size) {
    return compile_scene(file_name, log, log_size, rmplugin::FORM_AA);
}

rm_status rm_compile_scene_batch_aa(const char *file_name, char *log, size_t log_size) {
    return compile_scene(file_name, log, log_size, rmplugin::FORM_BATCH_AA);
}

int rm_abi_version(void) { return RM_ABI_VERSION; }

rm_status rm_certified_steps(rm_ctx *ctx, uint64_t *steps) {
    if (!ctx || !steps) return RM_ERR_INVALID_ARGUMENT;
    *steps = ctx->last_certified;
    return RM_OK;
}

rm_status rm_reflection_cleared_steps(rm_ctx *ctx, uint64_t *steps) {
    if (!ctx || !steps) return RM_ERR_INVALID_ARGUMENT;
    *steps = ctx->last_refl_cleared;
    return RM_OK;
}

rm_status rm_near_sky_steps(rm_ctx *ctx, uint64_t *steps) {
    if (!ctx || !steps) return RM_ERR_INVALID_ARGUMENT;
    *steps = ctx->last_near_sky;
    return RM_OK;
}

rm_status rm_resolution_cache_info(rm_ctx *ctx, int *entries, int *capacity) {
    if (!ctx) return RM_ERR_INVALID_ARGUMENT;
    if (entries) *entries = ctx->rcp_n;
    if (capacity) *capacity = rm_ctx::kRcpEntries;
    return RM_OK;
}

const char *rm_last_error(rm_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

const char *rm_status_string(rm_status s) {
    switch (s) {
    case RM_OK: return "RM_OK";
    case RM_ERR_INVALID_ARGUMENT: return "RM_ERR_INVALID_ARGUMENT";
    case RM_ERR_FILE: return "RM_ERR_FILE";
    case RM_ERR_SCENE: return "RM_ERR_SCENE";
    case RM_ERR_NO_SCENE: return "RM_ERR_NO_SCENE";
    case RM_ERR_DEVICE: return "RM_ERR_DEVICE";
    case RM_ERR_OUT_OF_MEMORY: return "RM_ERR_OUT_OF_MEMORY";
    }
    return "RM_ERR_UNKNOWN";
}

}  // extern "C"
