// rm_plugin_host.cpp -- scene plugins.
//
// The reference reloads its scene by recompiling the preprocessed
// output_shader.frag through sf::Shader::loadFromMemory
// (source/shader_loader.cpp:19; the "Reload scene shader" button,
// main.cpp:134-139).  Here a scene is a source file (".hip") written against
// the reference's scene library (rm_sdf_lib.h, common.frag:37-679):
// rm_load_scene preprocesses it with the reference's #include semantics and
// compiles it with hiprtc for gfx950 into a code object whose kernels are
// output_shader.frag's pass around the scene's sceneSDF (rm_plugin.h,
// rm_plugin_kernels.h).  Code objects are cached per source text, so reloading
// an unchanged scene costs no compilation.
#include "rm_plugin_host.h"

#include "rm_plugin_batch_aa_grid.h"

#include <hip/hiprtc.h>

#include <cstdio>
#include <vector>

#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <fstream>
#include <initializer_list>
#include <map>
#include <mutex>

extern "C" {
extern const int rm_rtc_header_count;
extern const char* const rm_rtc_header_names[];
extern const char* const rm_rtc_header_texts[];
}

namespace rmplugin {

namespace {

bool is_id(char c) { return std::isalnum((unsigned char)c) || c == '_'; }

// component index of a swizzle letter (xyzw / rgba / stpq), -1 otherwise
int swizzle_index(char c, int set) {
    static const char* sets[3] = {"xyzw", "rgba", "stpq"};
    for (int i = 0; i < 4; i++)
        if (sets[set][i] == c) return i;
    return -1;
}

// "xz" -> "swz2<0, 2>", or "" if w is not a 2-4 letter swizzle of one set
std::string swizzle_call(const std::string& w) {
    if (w.size() < 2 || w.size() > 4) return "";
    for (int set = 0; set < 3; set++) {
        std::string idx;
        bool ok = true;
        for (char c : w) {
            int k = swizzle_index(c, set);
            if (k < 0) {
                ok = false;
                break;
            }
            idx += (idx.empty() ? "" : ", ") + std::to_string(k);
        }
        if (ok) return "swz" + std::to_string(w.size()) + "<" + idx + ">";
    }
    return "";
}

// start (in o) of the postfix expression that ends o: identifiers, member
// chains, and bracketed call / index groups
size_t operand_start(const std::string& o) {
    size_t k = o.size();
    for (;;) {
        if (k > 0 && (o[k - 1] == ')' || o[k - 1] == ']')) {
            const char close = o[k - 1], open = close == ')' ? '(' : '[';
            int depth = 0;
            size_t m = k;
            while (m > 0) {
                m--;
                if (o[m] == close) depth++;
                else if (o[m] == open && --depth == 0) break;
            }
            k = m;
            while (k > 0 && is_id(o[k - 1])) k--;  // a call's or an array's name
        } else if (k > 0 && is_id(o[k - 1])) {
            while (k > 0 && is_id(o[k - 1])) k--;
        } else {
            break;
        }
        if (k > 0 && o[k - 1] == '.') {
            k--;
            continue;
        }
        break;
    }
    return k;
}

}  // namespace

std::string glsl_source(const std::string& s) {
    std::string o;
    o.reserve(s.size() + s.size() / 8);
    const size_t n = s.size();
    size_t i = 0;
    int braces = 0, parens = 0;
    while (i < n) {
        const char c = s[i];
        if (c == '/' && i + 1 < n && (s[i + 1] == '/' || s[i + 1] == '*')) {  // comments
            const bool line = s[i + 1] == '/';
            size_t e = line ? s.find('\n', i) : s.find("*/", i + 2);
            e = e == std::string::npos ? n : (line ? e : e + 2);
            o.append(s, i, e - i);
            i = e;
            continue;
        }
        if (c == '"' || c == '\'') {  // string and character literals
            size_t j = i + 1;
            while (j < n && s[j] != c) j += s[j] == '\\' ? 2 : 1;
            j = j < n ? j + 1 : n;
            o.append(s, i, j - i);
            i = j;
            continue;
        }
        if (std::isalpha((unsigned char)c) || c == '_') {  // identifiers and keywords
            size_t j = i;
            while (j < n && is_id(s[j])) j++;
            const std::string w = s.substr(i, j - i);
            i = j;
            if (w == "const" && braces == 0 && parens == 0) {
                o += "constexpr";
            } else if (parens > 0 && (w == "in" || w == "out" || w == "inout")) {
                while (i < n && (s[i] == ' ' || s[i] == '\t')) i++;
                size_t k = i;
                while (k < n && is_id(s[k])) k++;
                o.append(s, i, k - i);  // the parameter's type
                if (w != "in") o += '&';
                i = k;
            } else {
                o += w;
            }
            continue;
        }
        if (std::isdigit((unsigned char)c) || (c == '.' && i + 1 < n && std::isdigit((unsigned char)s[i + 1]))) {
            size_t j = i + 1;  // a preprocessing number
            while (j < n && (is_id(s[j]) || s[j] == '.' ||
                             ((s[j] == '+' || s[j] == '-') && (s[j - 1] == 'e' || s[j - 1] == 'E'))))
                j++;
            const std::string num = s.substr(i, j - i);
            i = j;
            const bool hex = num.size() > 1 && num[0] == '0' && (num[1] == 'x' || num[1] == 'X');
            o += num;
            if (!hex && num.find_first_of(".eE") != std::string::npos && !std::isalpha((unsigned char)num.back()))
                o += 'f';
            continue;
        }
        if (c == '.' && i + 1 < n && std::isalpha((unsigned char)s[i + 1])) {  // member access or swizzle
            size_t j = i + 1;
            while (j < n && is_id(s[j])) j++;
            const std::string w = s.substr(i + 1, j - i - 1);
            size_t k = j;
            while (k < n && (s[k] == ' ' || s[k] == '\t')) k++;
            const std::string call = swizzle_call(w);
            const bool assigned = k < n && s[k] == '=' && !(k + 1 < n && s[k + 1] == '=');
            if (!call.empty() && !(k < n && s[k] == '(') && !assigned) {
                const size_t a = operand_start(o);
                const std::string operand = o.substr(a);
                o.resize(a);
                o += call + "(" + operand + ")";
                i = j;
                continue;
            }
            o += '.';
            o += w;
            i = j;
            continue;
        }
        if (c == '{') braces++;
        else if (c == '}') braces--;
        else if (c == '(') parens++;
        else if (c == ')') parens--;
        o += c;
        i++;
    }
    return o;
}

namespace {

std::mutex g_mu;
std::map<std::string, Code> g_cache;

std::string translation_unit(const std::string& src, const std::string& file, const rmuniform::Table& uniforms,
                             Form form) {
    std::string name;
    for (char c : file) {
        if (c == '"' || c == '\\') name += '\\';
        name += c;
    }
    // the scene twice: against the library's GLSL-rounding instance (rm::glsl:
    // marches, normals, rm_scene_eval) and against its probe instance
    // (rm::glsl::probe, FMA contraction: AO, soft shadows, thickness), as the
    // built-in scenes have exact and probe forms (rm_sdf_lib_body.h)
    const std::string scene = glsl_source(src);
    auto instance = [&](const char* open, const char* close, const char* pre, const char* post) {
        return std::string(open) + "namespace {\n" + pre +
               "#pragma clang force_cuda_host_device begin\n"
               // (every scene function inlined into the kernels: the uniforms are
               // read from the kernel-argument segment, rm_plugin.h; GLSL has no
               // recursion)
               "#pragma clang attribute push (__attribute__((always_inline)), apply_to = function)\n"
               "#line 1 \"" + name + "\"\n" + scene +
               "\n#pragma clang attribute pop\n"
               "#pragma clang force_cuda_host_device end\n" + post + "}  // namespace\n" + close;
    };
    // the scene's own uniforms (rm_uniform_decl.h): each name reads its slot of
    // the kernels' uniform block, in both instances; a scene without any has
    // the text, and so the code object, it had before there were such uniforms
    std::string head, defines, undefs;
    if (!uniforms.decls.empty()) {
        head = "#define RM_UNIFORM_SLOTS " + std::to_string(uniforms.slots) + "\n";
        rmuniform::device_text(uniforms, defines, undefs);
    }
    // the batch form is the frame form's text behind one #define: the same scene text in the same two instances
    // under the same pragmas, so that a view's bytes are the frame kernels' (rm_plugin.h, rm_plugin_kernels.h)
    if (form == FORM_BATCH) head = "#define RM_PLUGIN_BATCH 1\n" + head;
    // (the AA form likewise, so that a refined sample rounds as the frame kernel's pixel does)
    if (form == FORM_AA) head = "#define RM_PLUGIN_AA 1\n" + head;
    // (and the batch-AA form: the AA form's samples from the batch form's records)
    if (form == FORM_BATCH_AA) head = "#define RM_PLUGIN_BATCH_AA 1\n" + head;
    return head + "#include \"rm_plugin.h\"\n" + defines +
           instance("namespace rm {\nnamespace glsl {\n", "}  // namespace glsl\n}  // namespace rm\n", "", "") +
           instance("namespace rm {\nnamespace glsl {\nnamespace probe {\n",
                    "}  // namespace probe\n}  // namespace glsl\n}  // namespace rm\n",
                    "#pragma clang fp contract(fast)\n", "#pragma clang fp contract(off)\n") +
           undefs + "#include \"rm_plugin_kernels.h\"\n";
}

}  // namespace

bool compile(const std::string& src, const std::string& file, Code& code, std::string& log,
             rmuniform::Table& uniforms, Form form) {
    std::string scene;
    if (!rmuniform::parse(src, file, uniforms, scene, log)) return false;
    const std::string tu = translation_unit(scene, file, uniforms, form);
    log.clear();
    // debugging: the TU and its code object (a cached one too), the other forms' beside the frame form's
    auto dump = [&](const Code& c) {
        const char* dir = std::getenv("RM_PLUGIN_DUMP");
        if (!dir) return;
        const std::string stem = std::string(dir) + (form == FORM_BATCH ? "/plugin_batch" : form == FORM_AA ? "/plugin_aa" :
                                                        form == FORM_BATCH_AA ? "/plugin_batch_aa" : "/plugin");
        std::ofstream(stem + "_tu.hip") << tu;
        std::ofstream(stem + ".co", std::ios::binary).write(c->data(), (std::streamsize)c->size());
    };
    {
        std::lock_guard<std::mutex> g(g_mu);
        auto it = g_cache.find(tu);
        if (it != g_cache.end()) {
            code = it->second;
            dump(code);
            return true;
        }
    }
    hiprtcProgram prog = nullptr;
    hiprtcResult r = hiprtcCreateProgram(&prog, tu.c_str(), file.c_str(), rm_rtc_header_count, rm_rtc_header_texts,
                                         rm_rtc_header_names);
    if (r != HIPRTC_SUCCESS) {
        log = std::string("hiprtcCreateProgram: ") + hiprtcGetErrorString(r);
        return false;
    }
    // the flags of scene O's translation unit (raymarching_amd/Makefile), no
    // SLP vectorization (as librm's own device code: DEVFLAGS)
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                          "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-Wno-unused-function",
                          "-Wno-unused-variable"};
    std::vector<const char*> all(opts, opts + sizeof(opts) / sizeof(opts[0]));
    r = hiprtcCompileProgram(prog, (int)all.size(), all.data());
    size_t ls = 0;
    if (hiprtcGetProgramLogSize(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        log.resize(ls);
        hiprtcGetProgramLog(prog, &log[0]);
        while (!log.empty() && (log.back() == '\0' || log.back() == '\n')) log.pop_back();
    }
    if (r != HIPRTC_SUCCESS) {
        if (log.empty()) log = hiprtcGetErrorString(r);
        hiprtcDestroyProgram(&prog);
        return false;
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    auto v = std::make_shared<std::vector<char>>(cs);
    hiprtcGetCode(prog, v->data());
    hiprtcDestroyProgram(&prog);
    code = v;
    dump(code);
    std::lock_guard<std::mutex> g(g_mu);
    g_cache[tu] = v;
    return true;
}

hipError_t load(const Code& code, int uniform_slots, Module& m) {
    Module n;
    hipError_t e = hipModuleLoadData(&n.mod, code->data());
    if (e != hipSuccess) return e;
    if (hipModuleGetFunction(&n.render, n.mod, "rm_plugin_render") != hipSuccess ||
        hipModuleGetFunction(&n.render_count, n.mod, "rm_plugin_render_count") != hipSuccess) {
        (void)hipGetLastError();
        n.render = n.render_count = nullptr;
    }
    if (!n.render || hipModuleGetFunction(&n.shade, n.mod, "rm_plugin_shade") != hipSuccess) {
        (void)hipGetLastError();
        n.shade = nullptr;
    }
    e = hipModuleGetFunction(&n.eval, n.mod, "rm_plugin_eval");
    if (e == hipSuccess) e = hipModuleGetFunction(&n.cast, n.mod, "rm_plugin_cast");
    if (e != hipSuccess) {
        (void)hipModuleUnload(n.mod);
        return e;
    }
    if (hipModuleGetFunction(&n.eval_probe, n.mod, "rm_plugin_eval_probe") != hipSuccess) {
        (void)hipGetLastError();  // a scene without RM_PLUGIN_EVAL_PROBE
        n.eval_probe = nullptr;
    }
    n.code = code;
    n.uniform_slots = uniform_slots;
    unload(m);  // (the batch, AA and batch-AA forms of the scene before with it)
    m = n;
    return hipSuccess;
}

void unload(Module& m) {
    if (m.batch_aa_mod) (void)hipModuleUnload(m.batch_aa_mod);
    if (m.aa_mod) (void)hipModuleUnload(m.aa_mod);
    if (m.batch_mod) (void)hipModuleUnload(m.batch_mod);
    if (m.mod) (void)hipModuleUnload(m.mod);
    m = Module();
}

namespace {

std::string load_error(const char* label, hipError_t e) {
    return std::string("scene plugin ") + label + " module load: " + hipGetErrorString(e);
}

// A one-kernel form of m's scene: compiled (cached by text, as compile caches), loaded on the current device into
// `mod`, its kernel looked up into `fn`; both stay null on failure
bool form_ready(Module& m, Form form, const char* label, const char* kernel, hipModule_t& mod, hipFunction_t& fn,
                std::string& err, hipError_t& e) {
    e = hipSuccess;
    Code code;
    rmuniform::Table uniforms;
    if (!compile(m.src, m.file, code, err, uniforms, form)) return false;
    e = hipModuleLoadData(&mod, code->data());
    if (e == hipSuccess && (e = hipModuleGetFunction(&fn, mod, kernel)) != hipSuccess) (void)hipModuleUnload(mod);
    if (e == hipSuccess) return true;
    mod = nullptr;
    fn = nullptr;
    err = load_error(label, e);
    return false;
}

// One launch of a kernel of m's scene on a grid of `block`-thread workgroups.  Its arguments: F, then -- iff the
// scene declares uniforms -- the uniform block, then `rest` (pointers to the values); a null F: the batch kernel,
// which takes `rest` alone.  (The launch copies each argument by the size the kernel declares: the block's first
// uniform_slots slots, read now -- a later rm_set_uniform* does not reach a launch already enqueued.)
hipError_t launch(hipFunction_t fn, dim3 grid, unsigned block, const Module& m, const rm::FrameConst* F,
                  const uint32_t* uniforms, hipStream_t s, std::initializer_list<const void*> rest) {
    void* args[8];
    int n = 0;
    if (F) args[n++] = const_cast<rm::FrameConst*>(F);
    if (F && m.uniform_slots > 0) args[n++] = const_cast<uint32_t*>(uniforms);
    for (const void* a : rest) args[n++] = const_cast<void*>(a);
    return hipModuleLaunchKernel(fn, grid.x, grid.y, grid.z, block, 1, 1, 0, s, args, nullptr);
}

}  // namespace

bool batch_ready(Module& m, std::string& err, hipError_t& e) {
    e = hipSuccess;
    return m.render_batch ||
           form_ready(m, FORM_BATCH, "batch", "rm_plugin_render_batch", m.batch_mod, m.render_batch, err, e);
}

namespace {

// the one-wave workgroups of `fn` the device holds at once (rm_aa.h's launch_aa_refine_as counts them so)
hipError_t device_waves(hipFunction_t fn, unsigned& waves) {
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, 0);
    if (e == hipSuccess) waves = (unsigned)std::max(1, cus * std::max(per_cu, 1));
    return e;
}

// form_ready, then the device's waves of the form's kernel into `waves`; a failure leaves the form unloaded
bool refine_form_ready(Module& m, Form form, const char* label, const char* kernel, hipModule_t& mod,
                       hipFunction_t& fn, unsigned& waves, std::string& err, hipError_t& e) {
    if (!form_ready(m, form, label, kernel, mod, fn, err, e)) return false;
    e = device_waves(fn, waves);
    if (e == hipSuccess) return true;
    (void)hipModuleUnload(mod);
    mod = nullptr;
    fn = nullptr;
    err = load_error(label, e);
    return false;
}

}  // namespace

bool aa_ready(Module& m, std::string& err, hipError_t& e) {
    e = hipSuccess;
    // the grid, as rm_aa.h's launch_aa_refine_as fixes it: the one-wave workgroups the device holds at once
    return m.aa_refine ||
           refine_form_ready(m, FORM_AA, "AA", "rm_plugin_aa_refine", m.aa_mod, m.aa_refine, m.aa_grid, err, e);
}

bool batch_aa_ready(Module& m, std::string& err, hipError_t& e) {
    e = hipSuccess;
    return m.batch_aa_refine || refine_form_ready(m, FORM_BATCH_AA, "batch-AA", "rm_plugin_batch_aa_refine",
                                                  m.batch_aa_mod, m.batch_aa_refine, m.batch_aa_waves, err, e);
}

hipError_t launch_batch_aa_refine(const Module& m, const void* records, int W, int H, int n, int kshift,
                                  const uint32_t* counters, uint32_t cstride, const uint32_t* queue, uint32_t* frames,
                                  hipStream_t s) {
    if (!m.batch_aa_refine) return hipErrorInvalidDeviceFunction;
    if (n <= 0) return hipSuccess;
    const uint32_t g = rmpbaa::columns_override(std::getenv("RM_PLUGIN_BATCH_AA_COLUMNS"),
                                                rmpbaa::columns(W, H, n, kshift, m.batch_aa_waves));
    return launch(m.batch_aa_refine, dim3(g, 1, (unsigned)n), 64, m, nullptr, nullptr, s,
                  {&records, &kshift, &counters, &cstride, &queue, &frames});
}

hipError_t launch_aa_refine(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, int kshift,
                            const uint32_t* count, const uint32_t* queue, uint32_t* frame, hipStream_t s) {
    if (!m.aa_refine) return hipErrorInvalidDeviceFunction;
    return launch(m.aa_refine, dim3(m.aa_grid), 64, m, &F, uniforms, s, {&kshift, &count, &queue, &frame});
}

hipError_t launch_render_batch(const Module& m, const void* records, int W, int H, int n, void* out, bool rgba8,
                               hipStream_t s) {
    if (!m.render_batch) return hipErrorInvalidDeviceFunction;
    if (n <= 0) return hipSuccess;
    const int r8 = rgba8 ? 1 : 0;
    return launch(m.render_batch, dim3((unsigned)((W + 7) / 8), (unsigned)((H + 7) / 8), (unsigned)n), 64, m, nullptr,
                  nullptr, s, {&records, &out, &r8});
}

hipError_t launch_render(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, void* out, bool rgba8,
                         unsigned long long* evals, hipStream_t s) {
    if (!m.render || !m.render_count) return hipErrorInvalidDeviceFunction;
    rm::FrameConst f = F;
    f.gx_magic = rm::div_magic((uint32_t)((F.W + 7) / 8), (uint64_t)((F.W + 7) / 8) * (uint64_t)((F.nrows + 7) / 8));
    const int r8 = rgba8 ? 1 : 0;
    return launch(evals ? m.render_count : m.render, dim3((unsigned)((F.W + 7) / 8), (unsigned)((F.nrows + 7) / 8)), 64,
                  m, &f, uniforms, s, {&out, &r8, &evals});
}

hipError_t launch_eval(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, const float* pts,
                       long long n, float* dist, float* mat, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    return launch(m.eval, dim3((unsigned)((n + 255) / 256)), 256, m, &F, uniforms, s, {&pts, &n, &dist, &mat});
}

hipError_t launch_eval_probe(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, const float* pts,
                             long long n, float* dist, float* mat, float* aux, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!m.eval_probe) return hipErrorInvalidDeviceFunction;
    return launch(m.eval_probe, dim3((unsigned)((n + 255) / 256)), 256, m, &F, uniforms, s,
                  {&pts, &n, &dist, &mat, &aux});
}

hipError_t launch_cast(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, const rm::RayQuery& Q,
                       int inside, int block, hipStream_t s) {
    if (Q.n <= 0) return hipSuccess;
    if (!m.cast) return hipErrorInvalidDeviceFunction;
    return launch(m.cast, dim3((unsigned)((Q.n + block - 1) / block)), (unsigned)block, m, &F, uniforms, s,
                  {&Q, &inside});
}

hipError_t launch_shade(const Module& m, const rm::FrameConst& F, const uint32_t* uniforms, const rm::ShadeRays& Q,
                        hipStream_t s) {
    if (!m.shade) return hipErrorInvalidDeviceFunction;
    if (Q.n <= 0) return hipSuccess;
    return launch(m.shade, dim3(rm::shade_grid(Q)), 64, m, &F, uniforms, s, {&Q});
}

}  // namespace rmplugin
