// rm_ctx.h -- the context behind the C ABI (include/rm.h) and what the host
// files of librm.so share about it: rm_capi.cpp (entry points),
// rm_render_host.cpp (a render launch), rm_ctx_streams.cpp (stream and event
// lifetime, the scratch buffers' stream rule); the staging of host buffers is
// rm_stage.h.  Internal; other translation units go through rm_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include <set>
#include <string>
#include <vector>

#include "../../include/rm.h"
#include "rm_launch.h"
#include "rm_plugin_host.h"
#include "rm_rows.h"

struct rm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int scene = -1;
    std::string scene_file;
    // uniforms (common.frag:4-11)
    float res[2] = {0.0f, 0.0f};
    bool res_set = false;
    float pos[3] = {0.0f, 0.0f, 0.0f};
    float mouse[2] = {0.0f, 0.0f};
    float time = 0.0f;
    // KERNEL_PERSIST: blocks of self-resetting tile counters, one per stream
    // the context launches on (launches on one stream run one after another, so
    // a block is never shared by two launches in flight).  At most kPersistBlocks:
    // a new stream takes the least recently used block once the event recorded
    // after its last launch has completed (the launch left its counters zeroed).
    struct PersistBlock {
        hipStream_t stream = nullptr;
        uint32_t *ctr = nullptr;
        hipEvent_t last = nullptr;
        uint64_t used = 0;
    };
    static constexpr int kPersistBlocks = 4;
    std::vector<PersistBlock> persist;
    // work this context enqueued: `dirty` is set by each call that enqueues
    // on `stream`; `done` is recorded on the stream only when the context
    // leaves it (rm_set_stream) or is destroyed -- an event recorded after
    // every launch cost a ~11 us gap between consecutive frames on the stream
    // (DESIGN.md 2.14).  A left stream's event stays in `retired` until it
    // completes (rm_destroy waits for these, not the
    // whole device).
    hipEvent_t done = nullptr;
    bool dirty = false;
    std::vector<hipEvent_t> retired;
    // streams bound with rm_set_stream_kept (the caller keeps them alive until
    // rm_destroy): leaving one records nothing; it joins `owed`, and its work
    // is marked only when something waits for it (an entry's release,
    // rm_destroy), on the stream itself
    std::vector<hipStream_t> kept, owed;
    float sample_part = 1.0f;  // u_sample_part, u_seed1, u_seed2: read by rm_render_accumulate*
    float seed1[2] = {0.0f, 0.0f}, seed2[2] = {0.0f, 0.0f};
    rm_params params = {128, 0, 0, 0, 1};
    std::string err;
    std::set<std::string> warned;
    unsigned long long *d_evals = nullptr;
    unsigned long long last_certified = 0;  // rm_certified_steps(): d_evals[3] of the last render launch, 0 unless it was counted and filled an rm_stats
    unsigned long long last_near_sky = 0;  // rm_near_sky_steps(): d_evals[5] of the last render launch, as last_certified
    unsigned long long last_refl_cleared = 0;  // rm_reflection_cleared_steps(): d_evals[4] of the last render launch, as last_certified
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float4 *staging = nullptr;
    size_t staging_bytes = 0;
    // Device scratch buffers, one per use and context, grown on demand and shared by the context's streams:
    // `stream` is the one of the last use (scratch_used); when the context leaves it (set_stream), `ev` is recorded
    // there, and a use on another stream first waits, on the device, for that event (scratch_acquire) -- no marker
    // per frame; one per leave, and only after a use (`pending`: used on `stream` since `ev` was last recorded)
    struct Scratch {
        void *ptr = nullptr;
        size_t bytes = 0;
        hipEvent_t ev = nullptr;  // made on the first leave that needs it
        hipStream_t stream = nullptr;
        bool pending = false;
        template <class T>
        T *as() const { return static_cast<T *>(ptr); }
    };
    enum ScratchId {
        kScratchBloom,    // bloom's mip levels 1..d2, run tables and polynomials (rm_post_host.cpp)
        kScratchAa,       // adaptive supersampling's queue: the count's line, then a word per pixel (rm_aa.h)
        kScratchBatch,    // the device copy of a view batch's per-view records (rm_batch.h ViewConst)
        kScratchBatchAa,  // a batch's supersampling: the counters, the plan and the queue (rm_batch_aa_plan.h)
        kScratchCount
    };
    Scratch scratch[kScratchCount];
    int bloom_runs_w = 0, bloom_runs_h = 0;  // the size whose bloom run tables the bloom scratch holds (0: none)
    hipStream_t bloom_runs_stream = nullptr;
    // rm_set_post_batch_scratch_limit: the most of the bloom scratch a batched bloom may ask for (0: the default,
    // rm_post_batch_plan.h); the batch's views go through the buffer in groups that fit
    int64_t post_batch_limit = 0;
    hipEvent_t aa_ev2 = nullptr;  // a third timing event (rm_aa_stats: detect | refine), made on first use
    // the host side of a view batch's record upload (rm_batch_host.cpp): pinned blocks taken in turn, each with the
    // event recorded after its asynchronous copy.  A call fills a block only once that event has completed, so a
    // batch enqueued while the one before it still runs never overwrites records a copy has yet to read (at most
    // kBatchSlots uploads in flight; the next call waits for the oldest copy, not for its kernel's frames)
    struct BatchSlot {
        void *host = nullptr;
        size_t bytes = 0;
        hipEvent_t copied = nullptr;
        bool used = false;  // `copied` has been recorded
    };
    static constexpr int kBatchSlots = 4;
    BatchSlot batch_slot[kBatchSlots];
    int batch_next = 0;
    // FrameConst.rcp_* of scenes S0/T (rm_render_host.cpp frame_rcp): the device's reciprocals of the frame
    // size and of u_resolution.y, kept per resolution -- the key changes when a window is resized, not per frame
    // (u_time and the pose do not enter it).  A small fixed-size cache, least recently used out, so that callers
    // alternating between a few sizes do not synchronise on every call; a miss runs a one-thread kernel on the
    // context's stream and waits for it.  Per context, so per GPU.
    struct RcpEntry {
        int W = 0, H = 0;
        uint32_t res_y_bits = 0;
        float rcp[3] = {0.0f, 0.0f, 0.0f};
        uint64_t used = 0;
    };
    static constexpr int kRcpEntries = 8;
    RcpEntry rcp_cache[kRcpEntries];
    int rcp_n = 0;
    uint64_t rcp_clock = 0;
    float *d_rcp = nullptr;   // the kernel's three floats (made on the first miss)
    rmplugin::Module plugin;  // the loaded scene plugin (scene == SCENE_PLUGIN)
    // the uniforms the loaded scene declares itself (empty for a built-in
    // scene) and their current values, the block every plugin launch passes by
    // value; a successful rm_load_scene sets the declarations' defaults
    rmuniform::Table uniforms;
    uint32_t uniform_values[rmuniform::kBlockWords] = {};
    uint32_t *tile_order = nullptr;  // rm_set_tile_order (device copy)
    int64_t tile_order_n = 0;
    // adaptive dispatch order (rm_params.schedule): per launch geometry and
    // stream, the tile durations of the last launch and the order they give
    // Every kSchedPeriod-th launch of a geometry (L_s = s * period, s = 0, 1,
    // ...) writes its tile durations into cost[s & 1]; sort s of those
    // durations runs right after it on the same stream and writes order[s & 1],
    // which launches L_s + 1 .. L_{s+1} dispatch.  The other launches write no
    // durations.  (Round 2-4 sorted on a side stream, overlapping the next
    // launch: its kernels only got CUs as that launch drained, and the launch
    // after it waited ~45 us for them)
    struct Sched {
        uint64_t key = 0;
        hipStream_t stream = nullptr;
        int n = 0, gx = 0;         // tiles, tile-grid width
        uint64_t k = 0;            // launches so far
        uint32_t *buf = nullptr;   // cost[2][n] | order[2][n] | 2 x (hist[256] | cursor[256]) | bucket u8[n]
        hipEvent_t last = nullptr;  // after the last launch that read or wrote buf: recorded on `stream`
        bool dirty = false;         // when the entry is released or the context destroyed on `stream`
        // ... or, once the context has left `stream`, the `done` event recorded
        // there as it left (borrowed: one marker per leave instead of one per
        // entry as well; rm_destroy destroys it after the entries are released)
        hipEvent_t left = nullptr;
        uint64_t used = 0;
        size_t bytes = 0;  // buf's size
    };
    Sched sched[8];
    uint64_t sched_clock = 0;
    // buffers of evicted adaptive-order entries, each with the marker of its
    // last use (ev: owned, or a borrowed `done` event); reused by a new entry
    // once the marker has completed, instead of a host wait at the eviction
    // (a marker recorded then on a kept stream covers everything queued there
    // since, e.g. the next pipelined frame)
    struct Spare {
        uint32_t *buf = nullptr;
        size_t bytes = 0;
        hipEvent_t ev = nullptr;
        bool own = false;
    };
    std::vector<Spare> spare;
};

namespace rmhost {

inline rm_status fail(rm_ctx *c, rm_status s, const std::string &msg) {
    if (c) c->err = msg;
    return s;
}

inline rm_status hip_fail(rm_ctx *c, hipError_t e, const char *what) {
    return fail(c, e == hipErrorOutOfMemory ? RM_ERR_OUT_OF_MEMORY : RM_ERR_DEVICE,
                std::string(what) + ": " + hipGetErrorString(e));
}

#define RM_HIP(call)                                          \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); \
    } while (0)

// Note that the context enqueued work on its stream (rm_ctx::dirty).
inline void mark_done(rm_ctx *ctx) { ctx->dirty = true; }

inline bool is_kept(const rm_ctx *ctx, hipStream_t s) {
    for (hipStream_t k : ctx->kept)
        if (k == s) return true;
    return false;
}

inline bool is_device_ptr(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// The tail of a launch-only entry point, after its argument checks:
// launch() enqueues on the ctx stream, `what` names it in the error text.
// (Inlined: the frame loops count host microseconds per call)
template <class Launch>
__attribute__((always_inline)) inline rm_status launch_on(rm_ctx *ctx, const char *what, Launch launch) {
    RM_HIP(hipSetDevice(ctx->device));
    hipError_t e = launch();
    if (e != hipSuccess) return hip_fail(ctx, e, what);
    mark_done(ctx);
    return RM_OK;
}

// ---- rm_ctx_streams.cpp
rm_status persist_block(rm_ctx *ctx, rm_ctx::PersistBlock *&out);
rm_ctx::Sched *sched_slot(rm_ctx *ctx, int W, int H, const rm::RowPart &part, int row0, int count, rm_status &st);
hipError_t sched_release(rm_ctx *ctx, rm_ctx::Sched &e);
rm_status set_stream(rm_ctx *ctx, hipStream_t s);  // rm_set_stream
// A scratch buffer (rm_ctx::Scratch) of at least `bytes` on the context's stream: after the event of a last use on
// another stream, and grown if it is too small (*grown: the old buffer and its contents are gone; a failed
// allocation leaves the scratch empty).  scratch_used: work that uses it was enqueued on the context's stream
rm_status scratch_acquire(rm_ctx *ctx, rm_ctx::Scratch &sc, size_t bytes, bool *grown = nullptr);
void scratch_used(rm_ctx *ctx, rm_ctx::Scratch &sc);
void scratch_free(rm_ctx::Scratch &sc);  // rm_destroy
void wait_idle(rm_ctx *ctx);             // rm_destroy: nothing the context enqueued still runs

// ---- rm_render_host.cpp
int pick_kernel(const rm_params &p);
// the pose-dependent members of F (position, camera and sponge rotations, camq_*, time, mouse): frame_const's own
// code, which a view batch calls once per view (rm_batch_host.cpp).  It also takes F.near_r back to the far-sky
// cube's radius under a pose whose rotations do not keep a direction's length (rm_far_sky.h 3.)
void pose_const(rm::FrameConst &F, const float pos[3], const float mouse[2], float time);
float seed_jitter(float seed);  // fract(seed) - 0.5: FrameConst.jit_* of u_seed1
rm_status ensure_staging(rm_ctx *ctx, size_t bytes);  // ctx->staging holds at least `bytes`
rm::FrameConst frame_const(const rm_ctx *c, int W, int H, const rm::RowPart &part, int nrows);
// F.rcp_* for F's W, H and res_y (scenes S0/T; every launch whose kernel builds camera rays calls it after
// frame_const, which leaves them 0): from the context's per-resolution cache, computed on the device on a miss
rm_status frame_rcp(rm_ctx *ctx, rm::FrameConst &F);
// rm_render_cycle_rows_wire: the compressed wire's message instead of pixels
// (`out` is then the tile-slot workspace, rm_wire_tile.h)
struct WireOut {
    uint8_t *msg;
    long long *size_out;
};
rm_status render_dev(rm_ctx *ctx, int W, int H, const rm::RowPart &part, int row0, int count, void *out, bool rgba8,
                     rm_stats *stats, uint32_t *evmap = nullptr, bool accum = false, const WireOut *wire = nullptr);
rm_status render_part(rm_ctx *ctx, int W, int H, const rm::RowPart &part, int row_begin, int row_count, void *out,
                      bool rgba8, rm_stats *stats, uint32_t *evmap = nullptr, bool accum = false);
rm_status render_any(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, int row_begin, int row_count,
                     void *out, bool rgba8, rm_stats *stats, uint32_t *evmap = nullptr, bool accum = false);


// ---- rm_batch_host.cpp
// a view batch's shared constants F (W x H, row-major) and the upload of its n per-view records (rm_batch.h) on
// the context's stream, then its one launch into the device pointer `out`: rm_render_batch's two halves, which
// rm_batch_aa_host.cpp calls too (a refine alone takes the records without the launch)
// (a scene plugin's records, rm_plugin_host.h batch_record_stride: the view's whole FrameConst, then its uniform
// block, view v's at blocks + v * 4 * slots words -- rm_plugin_batch_pack.h's; built-in scenes take none)
rm_status batch_records(rm_ctx *ctx, int W, int H, const rm_view *views, int n, rm::FrameConst &F, const void *&rec_d,
                        const uint32_t *blocks = nullptr);
rm_status batch_launch(rm_ctx *ctx, const rm::FrameConst &F, const void *rec_d, int n, void *out, bool rgba8,
                       rm_stats *stats);
// rm_render_batch[_rgba8] (ex null: a scene plugin is refused) and rm_render_batch_ex[_rgba8]: the checks in
// include/rm.h's order, the staging of a host target, the records and the launch
struct BatchEx {
    const rm_view_uniform *uniforms;
    int n_uniforms;
};
rm_status batch_run(rm_ctx *ctx, int W, int H, const rm_view *views, int n, void *out, bool rgba8, rm_stats *stats,
                    const BatchEx *ex);

// ---- rm_plugin_batch_host.cpp
// what rm_render_batch_ex asks of the loaded scene before any view is looked at: a plugin must have render kernels,
// a built-in scene takes no uniforms
rm_status batch_ex_scene(rm_ctx *ctx, const BatchEx &ex);
// a plugin's per-view uniform blocks from the list (RM_ERR_INVALID_ARGUMENT with the list's fault in rm_last_error)
rm_status batch_ex_blocks(rm_ctx *ctx, const BatchEx &ex, int n, std::vector<uint32_t> &blocks);
// the loaded plugin's batch kernel, compiled and loaded if it is not yet
rm_status batch_ex_ready(rm_ctx *ctx);

// the loaded plugin's batch refine kernel (the batch-AA form), compiled and loaded if it is not yet
rm_status batch_aa_ex_ready(rm_ctx *ctx);

// ---- rm_batch_aa_host.cpp
// rm_refine_batch_rgba8 / rm_render_batch_aa_rgba8 (ex null: a scene plugin is refused) and their _ex forms: the
// checks in include/rm.h's order, the staging of host buffers, the records, the batch launch when `render`, then
// count memset, detect, plan and the scene's refine; `what` names the call in the messages
rm_status batch_aa_run(rm_ctx *ctx, const char *what, int W, int H, const rm_view *views, int n, const rm_aa_params *p,
                       uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats, bool render,
                       const BatchEx *ex);

// ---- rm_aa_host.cpp
// the stats tail of a refine and of a batch's (rm_batch_aa_host.cpp): aa_ev2 recorded and waited for, the device
// word at `count` into stats->refined, detect_ms = ev0..ev1 and refine_ms = ev1..aa_ev2
rm_status refine_stats(rm_ctx *ctx, const uint32_t *count, rm_aa_stats *stats);

}  // namespace rmhost
