// rm_launch.h -- host-side launcher interface between the host files (rm_ctx.h)
// and the kernels (rm_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rm_bloom_plan.h"
#include "rm_render_direct.h"

namespace rm {


// the workgroup grid of a render launch over W x rows pixels
struct TileGrid {
    int x, y;
};
inline TileGrid tile_grid(int kernel, int W, int rows) {
    const int tw = kernel == KERNEL_TILE16 ? 16 : kernel == KERNEL_TILE16X4 ? 16 : 8;
    const int th = kernel == KERNEL_TILE16 ? 16 : kernel == KERNEL_TILE16X4 ? 4 : 8;
    return TileGrid{(W + tw - 1) / tw, (rows + th - 1) / th};
}

// out: W-wide rows of float4 (rgba8 = false) or RGBA8 words (rgba8 = true)
struct WireTile;
// rm_render_cycle_rows_wire: the built-in scenes' render kernel (8x8 one-wave
// tiles) encoding every tile into its wire slot instead of storing pixels
hipError_t launch_render_wire(int scene, const FrameConst& F, WireTile* slots, unsigned long long* evals,
                              hipStream_t s);
hipError_t launch_render(int scene, const FrameConst& F, void* out, bool rgba8, unsigned long long* evals, int kernel,
                         hipStream_t s);
// scenes S0/T: out3 (device) = v_rcp_f32 of (float)W, (float)H, res_y (FrameConst.rcp_*; rm_kernels_t.hip)
hipError_t launch_resolution_rcp(int W, int H, float res_y, float* out3, hipStream_t s);
// sceneSDF(p) of a compiled-in scene at n points (rm_scene_eval)
hipError_t launch_scene_eval(int scene, const FrameConst& F, const float* pts, long long n, float* dist, float* mat,
                             hipStream_t s);
// its probe forms (rm_scene_eval_form: form = kFormProbe or kFormProbeNb1);
// dist, mat and aux (scene O's probe-form slack, 0 elsewhere) may each be null
hipError_t launch_scene_eval_form(int scene, const FrameConst& F, const float* pts, long long n, int form, float* dist,
                                  float* mat, float* aux, hipStream_t s);
hipError_t launch_deinterleave(const float4* gathered, float4* out, int W, int H, int band, int nshards,
                               int rows_per_shard, hipStream_t s);
hipError_t launch_deinterleave_u32(const uint32_t* gathered, uint32_t* out, int W, int H, int band, int nshards,
                                   int rows_per_shard, hipStream_t s);
hipError_t launch_pack_rgba8(const float4* in, uint32_t* out, size_t n, hipStream_t s);
hipError_t launch_pack_rgb8(const uint32_t* in, uint8_t* out, size_t n, hipStream_t s);
hipError_t launch_deinterleave_rgb8(const uint8_t* gathered, uint32_t* out, int W, int H, int band, int nshards,
                                    int rows_per_shard, hipStream_t s);
// cyclic parts of a frame (rm_deinterleave_cycle_rgb8): part p owns the rows y
// with (y mod cycle) - off[p] in [0, run[p]), its packed RGB8 rows from byte base[p]
constexpr int kMaxCycleParts = 64;
struct CycleParts {
    int n;
    int off[kMaxCycleParts], run[kMaxCycleParts];
    long long base[kMaxCycleParts];
};
hipError_t launch_deinterleave_cycle_rgb8(const uint8_t* gathered, uint32_t* out, int W, int H, int cycle,
                                          const CycleParts& parts, hipStream_t s);
// the next launch's tile order (costliest first) from the tile durations
// (hist: 256 counts + 256 cursors, zero on entry); clears `next` (512 words)
// for the following launch
hipError_t launch_tile_order(const uint32_t* cost, int n, int gx, int radius, uint32_t* order, uint32_t* hist,
                             uint32_t* next, uint8_t* bucket, hipStream_t s);
hipError_t launch_fxaa(const uint32_t* in, uint32_t* out, int W, int H, hipStream_t s);
// post.frag's main() with a choice of sample and tonemap operator (rm_post_frag,
// DESIGN.md 2.18); the values are rm.h's rm_post_sample / rm_tonemap
constexpr int kSampleFxaa = 0, kSampleTexel = 1, kSampleChromatic = 2, kSampleCount = 3;
constexpr int kTonemapNone = 0, kTonemapAces = 1, kTonemapReinhard = 2, kTonemapJodie = 3, kTonemapUncharted2 = 4,
              kTonemapCount = 5;
// rm_fxaa.hip: FXAA with the operator applied to its float colour before the store
hipError_t launch_fxaa_tonemap(const uint32_t* in, uint32_t* out, int W, int H, int tonemap, hipStream_t s);
// rm_post_frag.hip: the texel and chromaticAberration samples
hipError_t launch_post_frag(const uint32_t* in, uint32_t* out, int W, int H, int sample, int tonemap, hipStream_t s);
// rm_wire.hip: the compressed RGB wire of RGBA8 row parts
long long wire_capacity(int W, int n);
long long wire_workspace(int W, int n);
hipError_t launch_wire_encode(const uint32_t* rows, int W, int n, uint8_t* msg, void* workspace,
                              long long* size_out, hipStream_t s);
// the scan and compaction of slots already written (rm_wire_tile.h: a render epilogue, or the rows encoder)
hipError_t launch_wire_finish(const void* workspace, int W, int n, uint8_t* msg, long long* size_out, hipStream_t s);
hipError_t launch_wire_decode(const uint8_t* msg, int n, int W, int cycle, int offset, int run, uint32_t* frame,
                              hipStream_t s);
constexpr int kMaxWireParts = 64;
struct WirePart {
    const uint8_t* msg;
    int nrows, offset, run;
};
struct WireParts {
    int n, cycle;
    WirePart part[kMaxWireParts];
};
hipError_t launch_wire_decode_parts(const WireParts& parts, int W, uint32_t* frame, hipStream_t s);
hipError_t launch_scatter_part(const uint32_t* rows, int n, int W, int cycle, int offset, int run, uint32_t* frame,
                               hipStream_t s);

// BloomPlan, bloom_plan(W, H): rm_bloom_plan.h (plain C++).
// runs_cached: the buffer already holds this W x H's run tables, written on
// this stream (only the mip levels and the polynomials are rebuilt)
hipError_t launch_bloom(const uint32_t* in, uint32_t* out, uint32_t* mips, const BloomPlan& p, hipStream_t s,
                        bool runs_cached);
// the run tables alone, at the plan's offsets in `mips` (rm_bloom_runs_kernel; lod > 0)
hipError_t launch_bloom_runs(uint32_t* mips, const BloomPlan& p, hipStream_t s);

// rm_post_batch.hip: the post passes over n frames of W x H packed one after
// the other.  View v's frame is at in / out + v * W * H.
hipError_t launch_post_frag_batch(const uint32_t* in, uint32_t* out, int W, int H, int n, int sample, int tonemap,
                                  hipStream_t s);
// `tables`: the run tables at the plan's offsets, already written on this
// stream (lod > 0); view v's levels and polynomials at views + v * L.view_words
// (rm_post_batch_plan.h view_layout)
struct PostBatchViewLayout;
hipError_t launch_bloom_batch(const uint32_t* in, uint32_t* out, int n, uint32_t* tables, uint32_t* views,
                              const BloomPlan& p, const PostBatchViewLayout& L, hipStream_t s);

}  // namespace rm
