// rm_stage.h -- the staging of a call's host buffers: one device allocation
// that holds them all (rm_stage_plan.h places them), the copies in, the copies
// out, and a wait before the allocation is freed -- also after a failure, since
// work already enqueued may still use it.  Callers check beforehand that their
// pointers are all host or all device ones, with their own messages; a buffer
// that is on the device already is simply not added, and a Stage without
// buffers does nothing at all (no allocation, no wait).
#pragma once
#include "rm_ctx.h"
#include "rm_stage_plan.h"

namespace rmhost {

class Stage {
public:
    static constexpr int kMax = 8;
    // A host buffer of the call (null: one the caller left out, which takes no space and whose dev() is null);
    // in: begin copies it to the device, out: end copies it back.  Returns its index.
    int add(const void *host, size_t bytes, bool in, bool out) {
        host_[n_] = host;
        in_[n_] = in;
        out_[n_] = out;
        items_[n_] = rmstage::Item{bytes, host != nullptr};
        return n_++;
    }
    // The allocation and the copies in, on the context's stream; `what` names a failed copy, here and in end.
    // After a failure, end still has to be called.
    rm_status begin(rm_ctx *ctx, const char *what) {
        what_ = what;
        size_t total = 0;
        if (!rmstage::plan(items_, n_, off_, total))
            return fail(ctx, RM_ERR_OUT_OF_MEMORY, std::string(what) + ": the buffers' sizes overflow");
        if (total == 0) return RM_OK;
        RM_HIP(hipMalloc(&tmp_, total));
        for (int i = 0; i < n_; i++)
            if (items_[i].used && in_[i]) {
                const hipError_t e =
                    hipMemcpyAsync(tmp_ + off_[i], host_[i], items_[i].bytes, hipMemcpyHostToDevice, ctx->stream);
                if (e != hipSuccess) return hip_fail(ctx, e, what);
            }
        return RM_OK;
    }
    bool staged() const { return tmp_ != nullptr; }
    template <class T>
    T *dev(int i) const {
        return tmp_ && items_[i].used ? reinterpret_cast<T *>(tmp_ + off_[i]) : nullptr;
    }
    // The copies out if the call went well so far (st), then the wait and the free; the first failure, `st` first.
    // `what` names a failed wait.
    rm_status end(rm_ctx *ctx, rm_status st, const char *what) {
        if (!tmp_) return st;
        for (int i = 0; i < n_ && st == RM_OK; i++)
            if (items_[i].used && out_[i]) {
                const hipError_t e = hipMemcpyAsync(const_cast<void *>(host_[i]), tmp_ + off_[i], items_[i].bytes,
                                                    hipMemcpyDeviceToHost, ctx->stream);
                if (e != hipSuccess) st = hip_fail(ctx, e, what_);
            }
        const hipError_t e = hipStreamSynchronize(ctx->stream);  // (also after a failure: tmp_ may be in use)
        if (st == RM_OK && e != hipSuccess) st = hip_fail(ctx, e, what);
        (void)hipFree(tmp_);
        tmp_ = nullptr;
        return st;
    }

private:
    const void *host_[kMax] = {};
    bool in_[kMax] = {}, out_[kMax] = {};
    rmstage::Item items_[kMax] = {};
    size_t off_[kMax] = {};
    int n_ = 0;
    char *tmp_ = nullptr;
    const char *what_ = "";
};

}  // namespace rmhost
