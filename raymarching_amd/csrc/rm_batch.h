// rm_batch.h -- view batches (include/rm.h rm_render_batch, rm_render_batch_rgba8;
// DESIGN.md 2.26): n poses of the loaded scene rendered by one launch over
// views x tiles.  A workgroup is one 8x8 wave tile of one view (blockIdx.z);
// it renders the tile with the frame kernels' own render_tile_at, in the timed
// form, row-major, from the view's constants: scenes S0/T from the launch's
// shared FrameConst with the view's pose-dependent members put in (a short
// record per view), scenes O/OG from the view's whole FrameConst in device
// memory (batch_whole_record below says why).
//
// The batch kernels must produce the frame kernels' bits, so they are built in
// translation units of their own with the flags of the scene's frame kernels:
// rm_batch_t.hip (S0, T; rm_kernels_t.o's flags) and rm_batch_o.hip (O, OG;
// rm_kernels_o.o's).  Neither is one of the render objects: the frame kernels'
// code and rm_render_code_hash() do not change with them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rm_launch.h"
#include "rm_render_direct.h"

namespace rm {

// What differs between the views of a batch: the members of FrameConst that
// depend on u_pos, u_mouse, u_time or the sub-pixel offset (rm_render_host.cpp
// pose_const fills them for the frame path and for this record alike).  One
// record per view in device memory, 16-byte aligned and 80 bytes long, read at
// a wave-uniform address (scalar loads).
struct alignas(16) ViewConst {
    float pos_x, pos_y, pos_z;
    float cam1_c, cam1_s, cam2_c, cam2_s;
    float ry_c, ry_s, rx_c, rx_s;
    float camq_x, camq_y, camq_z;
    float time, mouse_x, mouse_y;
    float jit_x, jit_y;
    float pad_;
};
static_assert(sizeof(ViewConst) == 80, "ViewConst: 20 words");

inline ViewConst view_of(const FrameConst& F) {
    return ViewConst{F.pos_x,  F.pos_y,  F.pos_z,  F.cam1_c, F.cam1_s, F.cam2_c,  F.cam2_s,  F.ry_c,  F.ry_s,  F.rx_c,
                     F.rx_s,   F.camq_x, F.camq_y, F.camq_z, F.time,   F.mouse_x, F.mouse_y, F.jit_x, F.jit_y, 0.0f};
}

// The grid's limits (gridDim.y, gridDim.z <= 65535) and the largest target,
// n * W * H <= 2^31 pixels: include/rm.h's size rule, which rm_batch_bytes and
// both render calls apply before anything else.
constexpr int kBatchMaxViews = 65535;
constexpr int kBatchMaxTileRows = 65535;
constexpr long long kBatchMaxPixels = 1LL << 31;
inline bool batch_size_ok(int W, int H, int n) {
    if (W <= 0 || H <= 0 || n < 0 || n > kBatchMaxViews) return false;
    if (((long long)H + 7) / 8 > kBatchMaxTileRows) return false;
    // (W * H < 2^62; n * (W * H) compared by division: no overflow)
    const long long px = (long long)W * H;
    return n == 0 || px <= kBatchMaxPixels / n;
}

// Scenes O and OG read FrameConst's tables (hash11, sss_floor) at run-time
// indices.  A kernel-local copy of the struct with a view's members put in is
// then not split into registers: it went to scratch whole (608 bytes per lane,
// where the frame kernel has none), and its members would be
// per-lane loads.  Their record is therefore the view's whole FrameConst, read
// in place through the uniform pointer, as the frame kernels read theirs in
// the kernel-argument segment.  Scenes S0 and T index no table and take the
// short record.
inline bool batch_whole_record(int scene) { return scene == SCENE_O || scene == SCENE_OG; }
inline size_t batch_record_bytes(int scene) { return batch_whole_record(scene) ? sizeof(FrameConst) : sizeof(ViewConst); }
// record v of a batch's host block: V is the launch's shared constants with view v's members put in
inline void batch_record_write(int scene, void* records, int v, const FrameConst& V) {
    if (batch_whole_record(scene)) static_cast<FrameConst*>(records)[v] = V;
    else static_cast<ViewConst*>(records)[v] = view_of(V);
}

// F: the launch's shared constants (a whole frame of F.W x F.H, row-major, no
// tile order, no accumulation); views: n records of the scene's kind
// (batch_record_bytes) in device memory; out: n tightly packed frames of float4
// (rgba8 = false) or RGBA8 words.
// scene S0 / T (rm_batch_t.hip), O / OG (rm_batch_o.hip); any other: hipErrorInvalidValue
hipError_t launch_batch_t(int scene, const FrameConst& F, const void* views, int n, void* out, bool rgba8,
                          hipStream_t s);
hipError_t launch_batch_o(int scene, const FrameConst& F, const void* views, int n, void* out, bool rgba8,
                          hipStream_t s);

#ifdef RM_BATCH_KERNELS  // the kernels' translation units (the host file takes the launchers above only)

// blockIdx.z is the view.  Its record's address is wave-uniform and the memory
// is read-only for the launch, so the nineteen words arrive by scalar loads
// and G's members stay SGPR operands, as F's are in the frame kernels
// (render_T moves the operands it wants in VGPRs itself).
// (the frame kernels' register budget: ScenePolicy<SC>::kWavesPerEU)
template <int SC, typename OUT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ScenePolicy<SC>::kWavesPerEU)))
void rm_render_batch(FrameConst F, const ViewConst* __restrict__ views, OUT* __restrict__ out, long long stride) {
    const ViewConst& v = views[blockIdx.z];
    FrameConst G = F;
    G.pos_x = v.pos_x; G.pos_y = v.pos_y; G.pos_z = v.pos_z;
    G.cam1_c = v.cam1_c; G.cam1_s = v.cam1_s; G.cam2_c = v.cam2_c; G.cam2_s = v.cam2_s;
    G.ry_c = v.ry_c; G.ry_s = v.ry_s; G.rx_c = v.rx_c; G.rx_s = v.rx_s;
    G.camq_x = v.camq_x; G.camq_y = v.camq_y; G.camq_z = v.camq_z;
    G.time = v.time; G.mouse_x = v.mouse_x; G.mouse_y = v.mouse_y;
    G.jit_x = v.jit_x; G.jit_y = v.jit_y;
    // what every batch launch holds (launch_batch_scene refuses another F): no dispatch order, no tile durations,
    // no accumulation -- said here so that those paths of render_tile_at are not compiled in
    G.tile_order = nullptr;
    G.tile_cost = nullptr;
    G.accumulate = 0;
    render_tile_at<SC, false, KERNEL_TILE8, OUT>(G, out + (long long)blockIdx.z * stride, nullptr, (int)blockIdx.x,
                                                 (int)blockIdx.y, (int)gridDim.x);
}

// The whole-record form (batch_whole_record): the view's FrameConst where it
// lies, at a wave-uniform address in memory that is read-only for the launch.
template <int SC, typename OUT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ScenePolicy<SC>::kWavesPerEU)))
void rm_render_batch_whole(const FrameConst* __restrict__ views, OUT* __restrict__ out, long long stride) {
    const FrameConst& G = views[blockIdx.z];
    // what every record of a batch holds (launch_batch_scene refuses another F): no dispatch order, no tile
    // durations, no accumulation -- said here so that those paths of render_tile_at are not compiled in
    __builtin_assume(G.tile_order == nullptr);
    __builtin_assume(G.tile_cost == nullptr);
    __builtin_assume(G.accumulate == 0);
    render_tile_at<SC, false, KERNEL_TILE8, OUT>(G, out + (long long)blockIdx.z * stride, nullptr, (int)blockIdx.x,
                                                 (int)blockIdx.y, (int)gridDim.x);
}

template <int SC>
hipError_t launch_batch_scene(const FrameConst& F, const void* views, int n, void* out, bool rgba8, hipStream_t s) {
    if (!batch_size_ok(F.W, F.H, n) || F.nrows != F.H || F.tile_order || F.tile_cost || F.evals_map || F.persist ||
        F.accumulate)
        return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const TileGrid g = tile_grid(KERNEL_TILE8, F.W, F.H);
    const dim3 grid((unsigned)g.x, (unsigned)g.y, (unsigned)n), block(64);
    const long long stride = (long long)F.W * F.H;
    uint32_t* const out8 = static_cast<uint32_t*>(out);
    float4* const out4 = static_cast<float4*>(out);
    if constexpr (SC == SCENE_O || SC == SCENE_OG) {  // (batch_whole_record)
        const FrameConst* const v = static_cast<const FrameConst*>(views);
        if (rgba8) hipLaunchKernelGGL((rm_render_batch_whole<SC, uint32_t>), grid, block, 0, s, v, out8, stride);
        else hipLaunchKernelGGL((rm_render_batch_whole<SC, float4>), grid, block, 0, s, v, out4, stride);
    } else {
        const ViewConst* const v = static_cast<const ViewConst*>(views);
        if (rgba8) hipLaunchKernelGGL((rm_render_batch<SC, uint32_t>), grid, block, 0, s, F, v, out8, stride);
        else hipLaunchKernelGGL((rm_render_batch<SC, float4>), grid, block, 0, s, F, v, out4, stride);
    }
    return hipGetLastError();
}

#endif  // RM_BATCH_KERNELS

}  // namespace rm
