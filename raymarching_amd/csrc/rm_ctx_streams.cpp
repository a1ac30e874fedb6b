// rm_ctx_streams.cpp -- stream and event lifetime of a context (rm_ctx.h): the
// bookkeeping that lets it leave a stream without a marker per frame, and wait
// for its own work alone when buffers are released or it is destroyed; and the
// one rule by which its scratch buffers pass from stream to stream.
#include "rm_ctx.h"

namespace rmhost {
namespace {

// An adaptive-order entry whose last use is not marked yet and whose stream
// can still be recorded on: the ctx stream or a kept one.
bool sched_owed(const rm_ctx *ctx, const rm_ctx::Sched &e) {
    return e.dirty && (e.stream == ctx->stream || is_kept(ctx, e.stream));
}

// The event that marks the last use of an entry's buffers (its last launch: an
// event, since the stream it ran on may belong to the caller and be gone by
// now), and whether the entry owns it.  Still owed: `last`, recorded now.
// Else, if the context left e.stream after e's last launch, the marker recorded
// then (a borrowed `done` event, re-recorded later only once it had completed,
// so a wait on it never returns early; rm_destroy destroys it after the spares
// and the entries).  Else `last` as it was recorded.
struct Marker {
    hipEvent_t ev;
    bool own;
};
hipError_t sched_marker(rm_ctx *ctx, const rm_ctx::Sched &e, Marker &m) {
    if (sched_owed(ctx, e)) {
        m = Marker{e.last, true};
        return hipEventRecord(e.last, e.stream);
    }
    m = e.left ? Marker{e.left, false} : Marker{e.last, true};
    return hipSuccess;
}

void spare_free(rm_ctx::Spare &sp) {
    if (sp.ev) (void)hipEventSynchronize(sp.ev);
    (void)hipFree(sp.buf);
    if (sp.own && sp.ev) (void)hipEventDestroy(sp.ev);
    sp = rm_ctx::Spare();
}

// Evict an entry without a host wait: its buffer joins ctx->spare with the
// marker of its last use.
hipError_t sched_retire(rm_ctx *ctx, rm_ctx::Sched &e, size_t bytes) {
    Marker m;
    if (!e.buf || sched_marker(ctx, e, m) != hipSuccess) return sched_release(ctx, e);
    if (!m.own && e.last) (void)hipEventDestroy(e.last);
    if (ctx->spare.size() >= 8) {  // bounded: the oldest is freed (a host wait, rare)
        spare_free(ctx->spare.front());
        ctx->spare.erase(ctx->spare.begin());
    }
    ctx->spare.push_back(rm_ctx::Spare{e.buf, bytes, m.ev, m.own});
    e = rm_ctx::Sched();
    return hipSuccess;
}

// A spare buffer of at least `bytes` whose last use has completed, or null.
uint32_t *spare_take(rm_ctx *ctx, size_t bytes, size_t &got) {
    for (size_t i = 0; i < ctx->spare.size(); i++) {
        rm_ctx::Spare &sp = ctx->spare[i];
        if (sp.bytes < bytes || (sp.ev && hipEventQuery(sp.ev) != hipSuccess)) continue;
        uint32_t *b = sp.buf;
        got = sp.bytes;
        if (sp.own && sp.ev) (void)hipEventDestroy(sp.ev);
        ctx->spare.erase(ctx->spare.begin() + (long)i);
        (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady
        return b;
    }
    (void)hipGetLastError();
    return nullptr;
}

// Record the adaptive-order entries' `last` events still owed on the ctx
// stream or on a kept stream (before the context is destroyed).
hipError_t record_sched_last(rm_ctx *ctx) {
    for (rm_ctx::Sched &e : ctx->sched)
        if (e.buf && sched_owed(ctx, e)) {
            Marker m;
            hipError_t r = sched_marker(ctx, e, m);
            if (r != hipSuccess) return r;
            e.dirty = false;
            e.left = nullptr;
        }
    return hipSuccess;
}

}  // namespace

// The KERNEL_PERSIST counter block of the ctx stream (rm_ctx::PersistBlock).
// A new block joins ctx->persist only once its event and counters exist (a
// half-built block would match the null stream with a null counter array).
rm_status persist_block(rm_ctx *ctx, rm_ctx::PersistBlock *&out) {
    out = nullptr;
    for (auto &b : ctx->persist)
        if (b.stream == ctx->stream) out = &b;
    if (!out && (int)ctx->persist.size() < rm_ctx::kPersistBlocks) {
        rm_ctx::PersistBlock b{};
        const size_t bytes = (size_t)rm::kPersistWords * sizeof(uint32_t);
        RM_HIP(hipEventCreateWithFlags(&b.last, hipEventDisableTiming));
        hipError_t e = hipMalloc(&b.ctr, bytes);
        if (e == hipSuccess) e = hipMemsetAsync(b.ctr, 0, bytes, ctx->stream);
        if (e != hipSuccess) {
            if (b.ctr) (void)hipFree(b.ctr);
            (void)hipEventDestroy(b.last);
            return hip_fail(ctx, e, "persist_block: counter block");
        }
        b.stream = ctx->stream;
        ctx->persist.push_back(b);
        out = &ctx->persist.back();
    }
    if (!out) {  // recycle the least recently used block once its last launch is done
        out = &ctx->persist[0];
        for (auto &b : ctx->persist)
            if (b.used < out->used) out = &b;
        RM_HIP(hipEventSynchronize(out->last));
        out->stream = ctx->stream;
    }
    out->used = ++ctx->sched_clock;  // per-context LRU clock (shared with the sched entries)
    return RM_OK;
}

// Free an adaptive-order entry once nothing still reads or writes its buffers
// (a host wait for the marker of its last use).
hipError_t sched_release(rm_ctx *ctx, rm_ctx::Sched &e) {
    hipError_t r = hipSuccess;
    if (e.buf) {
        Marker m;
        r = sched_marker(ctx, e, m);
        if (r == hipSuccess && m.ev) r = hipEventSynchronize(m.ev);
        (void)hipFree(e.buf);
    }
    if (e.last) (void)hipEventDestroy(e.last);
    e = rm_ctx::Sched();
    return r;
}

// The adaptive-order state of a launch geometry on the ctx stream (least
// recently used entry recycled), or null when scheduling does not apply.
rm_ctx::Sched *sched_slot(rm_ctx *ctx, int W, int H, const rm::RowPart &part, int row0, int count, rm_status &st) {
    st = RM_OK;
    // plugins always launch one-wave 8x8 tiles (rm_plugin_kernels.h)
    const int kernel = pick_kernel(ctx->params);
    if (!ctx->params.schedule ||
        (ctx->scene != rm::SCENE_PLUGIN && kernel != rm::KERNEL_TILE8 && kernel != rm::KERNEL_PERSIST))
        return nullptr;
    const rm::TileGrid g = rm::tile_grid(rm::KERNEL_TILE8, W, count);
    const int n = g.x * g.y;
    uint64_t key = 0xcbf29ce484222325ULL;
    for (long long v : {(long long)ctx->scene, (long long)W, (long long)H, (long long)part.cycle, (long long)part.offset,
                        (long long)part.run, (long long)row0, (long long)count})
        key = (key ^ (uint64_t)v) * 0x100000001b3ULL;
    rm_ctx::Sched *lru = &ctx->sched[0];
    for (rm_ctx::Sched &e : ctx->sched) {
        if (e.buf && e.key == key && e.stream == ctx->stream && e.n == n) {
            e.used = ++ctx->sched_clock;
            return &e;
        }
        if (e.used < lru->used) lru = &e;
    }
    hipError_t e = hipSuccess;
    // cost[2][n] | order[2][n] | 2 x (hist | cursor) | bucket bytes[n]
    const size_t need = ((size_t)4 * n + 1024 + ((size_t)n + 3) / 4) * sizeof(uint32_t);
    e = sched_retire(ctx, *lru, lru->bytes);
    size_t got = 0;
    if (e == hipSuccess && (lru->buf = spare_take(ctx, need, got)) == nullptr) {
        e = hipMalloc(&lru->buf, need);
        got = need;
    }
    lru->bytes = got;
    if (e == hipSuccess) e = hipMemsetAsync(lru->buf + 4 * (size_t)n, 0, 1024 * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&lru->last, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)sched_release(ctx, *lru);
        st = hip_fail(ctx, e, "schedule buffers");
        return nullptr;
    }
    lru->key = key;
    lru->stream = ctx->stream;
    lru->n = n;
    lru->gx = g.x;
    lru->used = ++ctx->sched_clock;
    return lru;
}

rm_status scratch_acquire(rm_ctx *ctx, rm_ctx::Scratch &sc, size_t bytes, bool *grown) {
    if (sc.ev && sc.stream != ctx->stream) RM_HIP(hipStreamWaitEvent(ctx->stream, sc.ev, 0));
    if (bytes > sc.bytes) {
        if (sc.ptr) RM_HIP(hipFree(sc.ptr));  // (waits for the launches that use it)
        sc.ptr = nullptr;
        sc.bytes = 0;
        if (grown) *grown = true;
        RM_HIP(hipMalloc(&sc.ptr, bytes));
        sc.bytes = bytes;
    }
    return RM_OK;
}

void scratch_used(rm_ctx *ctx, rm_ctx::Scratch &sc) {
    sc.stream = ctx->stream;
    sc.pending = true;
}

void scratch_free(rm_ctx::Scratch &sc) {
    if (sc.ptr) (void)hipFree(sc.ptr);
    if (sc.ev) (void)hipEventDestroy(sc.ev);
    sc = rm_ctx::Scratch();
}

rm_status set_stream(rm_ctx *ctx, hipStream_t s) {
    for (rm_ctx::Scratch &sc : ctx->scratch)
        if (sc.pending && s != ctx->stream && sc.stream == ctx->stream) {
            // a scratch's last use, marked for a use on another stream (scratch_acquire); a kept stream too
            RM_HIP(hipSetDevice(ctx->device));
            if (!sc.ev) RM_HIP(hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming));
            RM_HIP(hipEventRecord(sc.ev, ctx->stream));
            sc.pending = false;
        }
#ifdef RM_ANALYSIS_LEAVE_NO_RECORD
    // analysis builds only (-DRM_ANALYSIS_LEAVE_NO_RECORD, tools/scale_model.py
    // prices the marker with it; unsafe: a later release of a schedule buffer or
    // rm_destroy no longer waits for the old stream's work): leaving a stream
    // records nothing
    ctx->stream = s;
    return RM_OK;
#endif
    if (s != ctx->stream && ctx->dirty && is_kept(ctx, ctx->stream)) {
        // a kept stream: no marker now (its entries stay dirty, rm_ctx::kept)
        bool listed = false;
        for (hipStream_t o : ctx->owed) listed = listed || o == ctx->stream;
        if (!listed) ctx->owed.push_back(ctx->stream);
        ctx->dirty = false;
    }
    if (s != ctx->stream && ctx->dirty) {
        // the old stream's last work, marked now (it may be gone by the time it
        // is waited for): one `done` event, which the adaptive-order entries
        // used there since borrow (a second marker per leave cost ~4 us of
        // every frame on the two-stream pipeline); `done` is
        // kept until it completes, a completed one is reused for the new
        // stream (no host wait here)
        RM_HIP(hipSetDevice(ctx->device));
        RM_HIP(hipEventRecord(ctx->done, ctx->stream));
        for (rm_ctx::Sched &e : ctx->sched)
            if (e.buf && e.dirty && e.stream == ctx->stream) {
                e.left = ctx->done;
                e.dirty = false;
            }
        hipEvent_t next = nullptr;
        for (size_t i = 0; i < ctx->retired.size(); i++)
            if (hipEventQuery(ctx->retired[i]) == hipSuccess) {
                next = ctx->retired[i];
                ctx->retired.erase(ctx->retired.begin() + (long)i);
                break;
            }
        (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady
        if (!next) RM_HIP(hipEventCreateWithFlags(&next, hipEventDisableTiming));
        ctx->retired.push_back(ctx->done);
        ctx->done = next;
        ctx->dirty = false;
    }
    ctx->stream = s;
    return RM_OK;
}

// Nothing this context enqueued still runs: its own events (the streams
// it left may be the caller's and gone by now); other work on the device
// is not waited for.
// The bound stream must still exist: HIP does not validate stream handles,
// and a record on a destroyed one faults inside the runtime (a test saw
// SIGSEGV) instead of returning an error, so the lifetime rule of rm.h
// (rm_set_stream) is the only protection there.  The fallback below covers
// only a record that does return an error (e.g. a device fault): the
// context's work can then not be waited for by event, and the whole device
// is.
void wait_idle(rm_ctx *ctx) {
    bool lost = record_sched_last(ctx) != hipSuccess;
    if (ctx->done && ctx->dirty) {
        if (hipEventRecord(ctx->done, ctx->stream) == hipSuccess) (void)hipEventSynchronize(ctx->done);
        else lost = true;
    }
    for (hipStream_t s : ctx->owed)  // kept streams left with this context's work on them
        if (!lost && ctx->done) {
            if (hipEventRecord(ctx->done, s) == hipSuccess) (void)hipEventSynchronize(ctx->done);
            else lost = true;
        }
    if (lost) {
        (void)hipGetLastError();
        (void)hipDeviceSynchronize();
    }
    for (rm_ctx::Spare &sp : ctx->spare) spare_free(sp);  // (before the borrowed `done` events go)
    ctx->spare.clear();
    for (hipEvent_t ev : ctx->retired) {
        (void)hipEventSynchronize(ev);
        (void)hipEventDestroy(ev);
    }
    for (auto &b : ctx->persist)
        if (b.last) (void)hipEventSynchronize(b.last);
    for (rm_ctx::Sched &e : ctx->sched) {
        if (e.buf && e.last && !e.left) (void)hipEventSynchronize(e.last);
        e.left = nullptr;  // (its `done` event was waited for above and is destroyed)
    }
}

}  // namespace rmhost
