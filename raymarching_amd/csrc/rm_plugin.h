// rm_plugin.h -- prelude of a scene plugin's translation unit.
//
// rm_load_scene("scene.hip") compiles, with hiprtc for gfx950,
//
//     #include "rm_plugin.h"
//     namespace rm { namespace glsl {            // GLSL names win over HIP's
//     #pragma clang force_cuda_host_device begin // GLSL has no __device__
//     <the preprocessed scene source, GLSL spellings translated>
//     #pragma clang force_cuda_host_device end
//     } }
//     #include "rm_plugin_kernels.h"
//
// The scene source defines `SdResult sceneSDF(vec3 p)` with the library of
// rm_sdf_lib.h, as output_shader.frag:12-48 does with common.frag, and may
// read the pass's uniforms u_resolution, u_pos, u_mouse, u_time
// (common.frag:4-7), and uniforms it declares itself (`uniform vec4 u_ball =
// ...;`, rm_uniform_decl.h: the translation unit then starts with
// #define RM_UNIFORM_SLOTS n and wraps the scene in one #define per name, see
// UniformBlock below).  The render pipeline is output_shader.frag's render()
// and main() (rm_render_direct.h render_O), as for the compiled-in scene O.
#pragma once
#include "rm_render_direct.h"
#include "rm_sdf_lib.h"

namespace rm {
namespace glsl {

// The pass's uniforms, read where a scene function needs them from the
// kernel's own FrameConst argument: every plugin kernel takes it first, so it
// sits at offset 0 of the kernel-argument segment, and the scene's functions
// are force-inlined into the kernels (rm_plugin_host.cpp), where that segment
// is addressable.  These are constant-address-space loads, invariant, so a
// uniform read inside a march loop -- transformR's sin and cos of u_time --
// is hoisted out of it.  (Round 4 copied the uniforms to LDS; the LDS read of
// u_time stayed inside the loops, whose volatile asm statements LLVM must
// assume to write memory, and the scene-O plugin evaluated two sin and two
// cos, with two IEEE divisions, on every ray-step.)
//
// The batch form (#define RM_PLUGIN_BATCH at the head of the translation unit;
// include/rm.h rm_render_batch_ex): the views of a batch differ
// in these values, so they cannot be kernel arguments.  Each view has a record
// in device memory -- its whole FrameConst, then at kUniformOffset its uniform
// block: PluginArgsHead's layout -- and plugin_bytes() below is the address of
// the record of the workgroup's view, blockIdx.z: the pointer in the kernel's
// first argument plus blockIdx.z * kRecordStride, wave-uniform.  The memory is
// read-only for the launch and is read through the constant address space too,
// so the loads stay scalar and invariant, and hoist as the frame form's do.
// The batch-AA form (#define RM_PLUGIN_BATCH_AA; rm_render_batch_aa_ex_rgba8,
// DESIGN.md 2.32) reads the same records the same way: its refine workgroups
// have their view in blockIdx.z too.
typedef const __attribute__((address_space(4))) FrameConst* KernargFrame;
typedef const __attribute__((address_space(4))) char* KernargBytes;
constexpr int kUniformOffset = (int)((sizeof(FrameConst) + 15) & ~(size_t)15);
#ifdef RM_UNIFORM_SLOTS
constexpr int kRecordStride = kUniformOffset + 16 * RM_UNIFORM_SLOTS;
#else
constexpr int kRecordStride = kUniformOffset;
#endif
// where the pass's uniforms and the scene's block are read from
__device__ __forceinline__ KernargBytes plugin_bytes() {
#if defined(RM_PLUGIN_BATCH) || defined(RM_PLUGIN_BATCH_AA)
    // (the kernel's first parameter, a pointer to the records)
    typedef const __attribute__((address_space(4))) KernargBytes* KernargPointer;
    const KernargBytes records = *(KernargPointer)__builtin_amdgcn_kernarg_segment_ptr();
    return records + (size_t)blockIdx.z * (size_t)kRecordStride;
#else
    return (KernargBytes)__builtin_amdgcn_kernarg_segment_ptr();
#endif
}
__device__ __forceinline__ KernargFrame plugin_frame() { return (KernargFrame)plugin_bytes(); }

#ifdef RM_UNIFORM_SLOTS
// The uniforms a scene declares itself (`uniform vec4 u_ball = ...;`,
// rm_uniform_decl.h): RM_UNIFORM_SLOTS slots of 16 bytes, the second argument
// of every kernel of such a scene (rm_plugin_kernels.h), read like the
// FrameConst before it: from the kernel-argument segment, in the constant
// address space, at an offset fixed here.  A scene without declarations
// defines no RM_UNIFORM_SLOTS and has the kernels it always had.
struct alignas(16) UniformBlock {
    uint32_t w[4 * RM_UNIFORM_SLOTS];
};
struct PluginArgsHead {  // the kernels' first two parameters, as the kernel-argument segment lays them out
    FrameConst F;
    UniformBlock U;
};
static_assert(__builtin_offsetof(PluginArgsHead, U) == kUniformOffset && alignof(FrameConst) <= 16,
              "the uniform block follows the FrameConst in the kernel-argument segment");
static_assert(RM_UNIFORM_SLOTS >= 1 && RM_UNIFORM_SLOTS <= 64, "rm_uniform_decl.h kMaxSlots");

__device__ __forceinline__ float uniform_f(int byte) {
    return *(const __attribute__((address_space(4))) float*)(plugin_bytes() + kUniformOffset + byte);
}
__device__ __forceinline__ int uniform_i(int byte) {
    return *(const __attribute__((address_space(4))) int*)(plugin_bytes() + kUniformOffset + byte);
}
// a float / vec2 / vec3 / vec4 (of either library instance) at a byte offset of the block
template <class V>
__device__ __forceinline__ V uniform_v(int byte) {
    if constexpr (sizeof(V) == 4) return uniform_f(byte);
    else if constexpr (sizeof(V) == 8) return V(uniform_f(byte), uniform_f(byte + 4));
    else if constexpr (sizeof(V) == 12) return V(uniform_f(byte), uniform_f(byte + 4), uniform_f(byte + 8));
    else return V(uniform_f(byte), uniform_f(byte + 4), uniform_f(byte + 8), uniform_f(byte + 12));
}
// `name[i]` of an array uniform, i any int: wave-uniform indices are scalar
// loads, others vector loads of the same constant memory.  (GLSL leaves an
// index outside [0, N) undefined; here it reads the nearest element, never
// outside the block.)
template <class V, int BYTE, int N>
struct UniformArray {
    __device__ __forceinline__ V operator[](int i) const {
        const int k = i < 0 ? 0 : i > N - 1 ? N - 1 : i;
        return uniform_v<V>(BYTE + 16 * k);
    }
};
// N words of the block, loaded at the top of a kernel and kept by an empty
// asm: the reads of the same words inside the march loops are then copies of
// these loads, and what depends on them alone -- transformR's sin and cos of
// u_time * u_spin -- leaves the loops (without it LLVM kept
// the scalar loads and everything computed from them in every loop body)
template <int BYTE, int N>
__device__ __forceinline__ void uniform_keep() {
    if constexpr (N >= 1) asm volatile("" ::"s"(uniform_f(BYTE)));
    if constexpr (N >= 2) asm volatile("" ::"s"(uniform_f(BYTE + 4)));
    if constexpr (N >= 3) asm volatile("" ::"s"(uniform_f(BYTE + 8)));
    if constexpr (N >= 4) asm volatile("" ::"s"(uniform_f(BYTE + 12)));
}
#endif

}  // namespace glsl
}  // namespace rm

#define u_resolution (::rm::glsl::vec2(::rm::glsl::plugin_frame()->res_x, ::rm::glsl::plugin_frame()->res_y))
#define u_pos                                                                                              \
    (::rm::glsl::vec3(::rm::glsl::plugin_frame()->pos_x, ::rm::glsl::plugin_frame()->pos_y,               \
                      ::rm::glsl::plugin_frame()->pos_z))
#define u_mouse (::rm::glsl::vec2(::rm::glsl::plugin_frame()->mouse_x, ::rm::glsl::plugin_frame()->mouse_y))
#define u_time (::rm::glsl::plugin_frame()->time)
