// rm_plugin_host.h -- host side of scene plugins: hiprtc compilation of a
// scene source into a gfx950 code object, and its module (rm_plugin.h).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "rm_device.h"
#include "rm_rays.h"
#include "rm_shade.h"
#include "rm_uniform_decl.h"

namespace rmplugin {

using Code = std::shared_ptr<const std::vector<char>>;

// The GLSL spellings a scene source may use that C++ reads differently,
// rewritten outside comments and literals: unsuffixed floating literals get
// an f (GLSL float, not C++ double); file-scope `const` becomes `constexpr`
// (GLSL constants are usable everywhere, C++ host constants are not usable
// on the device); parameter qualifiers `in` are dropped and `out`/`inout`
// become references; swizzle reads e.xz / e.xyz / e.xyzw become
// swz2/swz3/swz4<indices>(e).  Swizzle writes are not translated.
std::string glsl_source(const std::string& src);

// Compile a (preprocessed) scene source; code objects are cached by the text
// handed to the compiler.  `uniforms` receives the scene's `uniform`
// declarations (rm_uniform_decl.h), read from `src` on every call: the
// compiler sees the source with the declarations blanked, so two sources that
// differ in a default value share a code object and nothing else.  On failure
// `log` holds the diagnostics.
// `form`: the frame form, or one of the one-kernel forms of the translation
// unit, the frame form's text behind one #define at its head -- the same scene
// text and options: FORM_BATCH (rm_plugin.h RM_PLUGIN_BATCH), whose kernel is
// rm_plugin_render_batch, and FORM_AA (RM_PLUGIN_AA), whose kernel is
// rm_plugin_aa_refine, and FORM_BATCH_AA (RM_PLUGIN_BATCH_AA), whose kernel is
// rm_plugin_batch_aa_refine.  A scene that defines RM_PLUGIN_EVAL_ONLY has none
// of them and fails to compile.
enum Form : int { FORM_FRAME = 0, FORM_BATCH = 1, FORM_AA = 2, FORM_BATCH_AA = 3 };
bool compile(const std::string& src, const std::string& file, Code& code, std::string& log,
             rmuniform::Table& uniforms, Form form = FORM_FRAME);

struct Module {
    hipModule_t mod = nullptr;
    hipFunction_t render = nullptr;        // timed render kernel; null for an RM_PLUGIN_EVAL_ONLY scene
    hipFunction_t render_count = nullptr;  // instrumented render kernel (ray-step counts, step maps)
    hipFunction_t eval = nullptr;
    hipFunction_t eval_probe = nullptr;    // rm_scene_eval_form's probe forms; null unless the scene defines RM_PLUGIN_EVAL_PROBE
    hipFunction_t cast = nullptr;          // rm_cast_rays' march (RM_PLUGIN_EVAL_ONLY scenes have it too)
    hipFunction_t shade = nullptr;         // rm_shade_rays' kernel; null for an RM_PLUGIN_EVAL_ONLY scene
    Code code;
    int uniform_slots = 0;  // > 0: the kernels take the uniform block as their second argument (rm_plugin.h)
    // the batch form (rm_render_batch_ex): a code object and a module of its own, compiled from `src` and loaded
    // by batch_ready on first use, dropped with the module (load, unload)
    std::string src, file;  // the preprocessed scene source rm_load_scene compiled, and its file name
    hipModule_t batch_mod = nullptr;
    hipFunction_t render_batch = nullptr;
    // the AA form (rm_refine_ex_rgba8): as the batch form, by aa_ready; the refine's grid, as many one-wave
    // workgroups as the device holds at once, is fixed when the form is loaded
    hipModule_t aa_mod = nullptr;
    hipFunction_t aa_refine = nullptr;
    unsigned aa_grid = 0;
    // the batch-AA form (rm_refine_batch_ex_rgba8): as the AA form, by batch_aa_ready; `batch_aa_waves`, the one-wave
    // workgroups of its kernel the device holds at once, is what rm_plugin_batch_aa_grid.h's rule starts from
    hipModule_t batch_aa_mod = nullptr;
    hipFunction_t batch_aa_refine = nullptr;
    unsigned batch_aa_waves = 0;
};
// on the current device; m keeps its old module on failure
hipError_t load(const Code& code, int uniform_slots, Module& m);
void unload(Module& m);
// The batch form of m's scene, compiled (cached by text, as compile caches) and loaded on the current device; at
// once if it is loaded already.  False with `err` set: `e` is hipSuccess if the compilation failed.
bool batch_ready(Module& m, std::string& err, hipError_t& e);
// The AA form likewise (rm_plugin_aa_refine and its grid).
bool aa_ready(Module& m, std::string& err, hipError_t& e);
// rm_aa.h's refine launch for m's scene: the queue of `*count` pixel indices at `queue` (device memory, the
// compiled-in detect kernel's), K = 1 << kshift samples per pixel into `frame`; `uniforms` as launch_render's;
// hipErrorInvalidDeviceFunction before aa_ready
hipError_t launch_aa_refine(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, int kshift,
                            const uint32_t* count, const uint32_t* queue, uint32_t* frame, hipStream_t s);
// The batch-AA form likewise (rm_plugin_batch_aa_refine and the device's waves of it).
bool batch_aa_ready(Module& m, std::string& err, hipError_t& e);
// The refine of a batch's n views of W x H for m's scene, on dim3(G, 1, n) one-wave workgroups with G from
// rm_plugin_batch_aa_grid.h (RM_PLUGIN_BATCH_AA_COLUMNS, read here at every call, overrides it): `records` as
// launch_render_batch's; view v's count at counters[v * cstride], its queue segment and its frame at v * W * H
// words of `queue` and `frames` (rm_batch_aa_plan.h); hipErrorInvalidDeviceFunction before batch_aa_ready
hipError_t launch_batch_aa_refine(const Module& m, const void* records, int W, int H, int n, int kshift,
                                  const uint32_t* counters, uint32_t cstride, const uint32_t* queue, uint32_t* frames,
                                  hipStream_t s);
// bytes of one view's record: the FrameConst, then the uniform block at rm_plugin.h's kUniformOffset
constexpr size_t kBatchUniformOffset = (sizeof(rm::FrameConst) + 15) & ~(size_t)15;
static_assert(kBatchUniformOffset == 592, "include/rm.h states a plugin record's bytes");
inline size_t batch_record_stride(int uniform_slots) { return kBatchUniformOffset + 16 * (size_t)uniform_slots; }
// n views of W x H from `records` (device memory, n records of batch_record_stride(m.uniform_slots) bytes) into
// the packed frames at `out`; hipErrorInvalidDeviceFunction before batch_ready
hipError_t launch_render_batch(const Module& m, const void* records, int W, int H, int n, void* out, bool rgba8,
                               hipStream_t s);
// `uniforms`: the context's block of rmuniform::kBlockWords words, copied into
// the kernel arguments by the launch call (its first m.uniform_slots slots)
hipError_t launch_render(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, void* out, bool rgba8,
                         unsigned long long* evals, hipStream_t s);
hipError_t launch_eval(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, const float* pts,
                       long long n, float* dist, float* mat, hipStream_t s);
// the probe instance's distance and material (dist, mat and aux may each be null; aux receives 0);
// hipErrorInvalidDeviceFunction for a scene that does not define RM_PLUGIN_EVAL_PROBE
hipError_t launch_eval_probe(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, const float* pts,
                             long long n, float* dist, float* mat, float* aux, hipStream_t s);
// `block`: threads per workgroup (rm::cast_block_size)
hipError_t launch_cast(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, const rm::RayQuery& Q,
                       int inside, int block, hipStream_t s);
// hipErrorInvalidDeviceFunction for a scene without render kernels (RM_PLUGIN_EVAL_ONLY)
hipError_t launch_shade(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, const rm::ShadeRays& Q,
                        hipStream_t s);

}  // namespace rmplugin
