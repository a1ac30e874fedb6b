// rm_pass.hpp -- C++ host adapter over the rm.h C ABI that mirrors the SFML
// surface the reference's main.cpp drives its ray-march pass through, so that
// main.cpp:52-54,187-207 port one call for one call:
//
//   reference (SFML)                                   here
//   sf::Shader shader;                                 rm::Shader shader(device);
//   ShaderLoader::loadFromFile(f, sf::Shader::Fragment, rm::ShaderLoader::loadFromFile(f, rm::Shader::Fragment,
//                              shader)  -> bool                                    shader) -> bool
//   shader.setUniform("u_pos", sf::Vector3f)           shader.setUniform("u_pos", rm::Vec3{...})
//   sf::RenderTexture t; t.create(w, h);               rm::RenderTexture t; t.create(w, h);
//   t.draw(sprite, &shader);                           t.draw(shader);
//   t.getTexture()                                     t.textureRGBA8() (device RGBA8) / t.copyToHostRGBA8(...)
//
// and the post passes of main.cpp:56-61,209-214:
//
//   sf::Shader post_shader;                            rm::PostShader post_shader(shader);
//   ShaderLoader::loadFromFile("post.frag", ..., post_shader)   the same call (the name is checked)
//   post_shader.setUniform("u_resolution", Vector2f)   post_shader.setUniform("u_resolution", rm::Vec2{...})
//   post_shader.setUniform("u_main_tex", t.getTexture())   post_shader.setUniform("u_main_tex", t)
//   (an edit of post.frag's main)                      post_shader.setSample(...), setTonemap(...)
//   postTexture.draw(sprite, &post_shader);            postTexture.draw(post_shader);
//   PostBloom post_bloom; post_bloom.init(Vector2f)    rm::PostBloom post_bloom(shader); post_bloom.init(rm::Vec2{...})
//   postTexture.setSmooth(true); generateMipmap();     (part of apply)
//   post_bloom.apply(postTexture.getTexture(), out, sprite)   post_bloom.apply(postTexture, out)
//
// The post objects run on the context (and stream) of the rm::Shader they are
// made from, so a frame's passes are ordered as the reference's GL calls are.
//
// Errors follow the reference: loadFromFile prints and returns false
// (source/shader_loader.cpp:26-30); other calls return false and keep the
// message in lastError().  Header-only; link with librm.so.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rm.h"

namespace rm {

struct Vec2 { float x, y; };
struct Vec3 { float x, y, z; };
struct Vec4 { float x, y, z, w; };

class Shader {
public:
    enum Type { Fragment };

    explicit Shader(int device = 0) : device_(device) {
        // a librm.so of another ABI would read and write these structs with
        // other layouts (include/rm.h RM_ABI_VERSION)
        if (rm_abi_version() != RM_ABI_VERSION) {
            std::fprintf(stderr, "rm::Shader: librm.so has ABI %d, rm.h declares %d\n", rm_abi_version(),
                         RM_ABI_VERSION);
            return;
        }
        if (rm_create(&ctx_, device) != RM_OK) ctx_ = nullptr;
    }
    ~Shader() {
        if (ctx_) rm_destroy(ctx_);
    }
    Shader(const Shader&) = delete;
    Shader& operator=(const Shader&) = delete;

    bool valid() const { return ctx_ != nullptr; }
    rm_ctx* ctx() { return ctx_; }
    int device() const { return device_; }
    std::string lastError() const { return ctx_ ? rm_last_error(ctx_) : "no HIP device"; }

    bool setUniform(const char* name, float x) { return ctx_ && rm_set_uniform1f(ctx_, name, x) == RM_OK; }
    bool setUniform(const char* name, Vec2 v) { return ctx_ && rm_set_uniform2f(ctx_, name, v.x, v.y) == RM_OK; }
    bool setUniform(const char* name, Vec3 v) {
        return ctx_ && rm_set_uniform3f(ctx_, name, v.x, v.y, v.z) == RM_OK;
    }
    // uniforms the loaded scene declares itself (rm.h, rm_load_scene), as
    // sf::Shader names the overloads: Glsl::Vec4, int, bool, and the arrays
    bool setUniform(const char* name, Vec4 v) {
        return ctx_ && rm_set_uniform4f(ctx_, name, v.x, v.y, v.z, v.w) == RM_OK;
    }
    bool setUniform(const char* name, int v) { return ctx_ && rm_set_uniform1i(ctx_, name, v) == RM_OK; }
    bool setUniform(const char* name, bool v) { return ctx_ && rm_set_uniform1i(ctx_, name, v ? 1 : 0) == RM_OK; }
    bool setUniformArray(const char* name, const float* v, std::size_t length) {
        return setArray(name, 1, v, length);
    }
    bool setUniformArray(const char* name, const Vec2* v, std::size_t length) {
        return setArray(name, 2, reinterpret_cast<const float*>(v), length);
    }
    bool setUniformArray(const char* name, const Vec3* v, std::size_t length) {
        return setArray(name, 3, reinterpret_cast<const float*>(v), length);
    }
    bool setUniformArray(const char* name, const Vec4* v, std::size_t length) {
        return setArray(name, 4, reinterpret_cast<const float*>(v), length);
    }
    // The reference's compile-time MAX_MARCHING_STEPS (common.frag:15) and the
    // uncapped soft-shadow loop (common.frag:814) are run-time here.
    bool setMarchSteps(int max_steps, int shadow_max_steps = 0) {
        rm_params p;
        if (!ctx_ || rm_get_params(ctx_, &p) != RM_OK) return false;
        p.max_steps = max_steps;
        p.shadow_max_steps = shadow_max_steps;
        return rm_set_params(ctx_, &p) == RM_OK;
    }

    // Ray queries (rm.h rm_cast_rays, rm_camera_rays; no counterpart in the
    // reference, whose castRayD is only reachable inside a frame's shading):
    // the rays main() builds for a w x h frame, and castRayD along any rays.
    // Buffers are all device or all host pointers, as the C calls take them.
    bool cameraRays(int w, int h, Vec3* origin, Vec3* directions) {
        return ctx_ && rm_camera_rays(ctx_, w, h, reinterpret_cast<float*>(origin),
                                      reinterpret_cast<float*>(directions)) == RM_OK;
    }
    bool castRays(const Vec3* origins, bool sharedOrigin, const Vec3* directions, std::int64_t n,
                  const rm_ray_hits& hits, bool inside = false, rm_stats* stats = nullptr) {
        return ctx_ && rm_cast_rays(ctx_, reinterpret_cast<const float*>(origins), sharedOrigin ? 1 : 0,
                                    reinterpret_cast<const float*>(directions), n, inside ? 1 : 0, &hits,
                                    stats) == RM_OK;
    }
    // rm.h rm_shade_rays: the pass's colour along any unit rays (a fisheye, a
    // cube map, a stereo pair, lens rays); exactly one of rgba (n x 4 floats)
    // and rgba8 (n words) is set.  A shared origin is a host pointer.
    bool shadeRays(const Vec3* origins, bool sharedOrigin, const Vec3* directions, std::int64_t n,
                   const rm_shade_params& params, float* rgba, std::uint32_t* rgba8, rm_stats* stats = nullptr) {
        return ctx_ && rm_shade_rays(ctx_, reinterpret_cast<const float*>(origins), sharedOrigin ? 1 : 0,
                                     reinterpret_cast<const float*>(directions), n, &params, rgba, rgba8,
                                     stats) == RM_OK;
    }
    // rm.h rm_render_batch[_rgba8]: n views of the loaded scene from one launch
    // (a turntable, an animation's frames, thumbnails, a stereo pair), view v's
    // w x h frame at out + v * w * h elements, each what setUniform(u_pos,
    // u_mouse, u_time) + RenderTexture::draw gives.  `views` is a host array;
    // `out` a device pointer (asynchronous unless stats is given) or a host one.
    // Built-in scenes only; the shader's own pose is neither read nor changed.
    bool renderBatch(int w, int h, const rm_view* views, int n, std::uint32_t* out, rm_stats* stats = nullptr) {
        return ctx_ && rm_render_batch_rgba8(ctx_, w, h, views, n, out, stats) == RM_OK;
    }
    bool renderBatch(int w, int h, const rm_view* views, int n, float* out, rm_stats* stats = nullptr) {
        return ctx_ && rm_render_batch(ctx_, w, h, views, n, out, stats) == RM_OK;
    }
    // rm.h rm_render_batch_ex[_rgba8]: renderBatch for any scene, a scene plugin
    // included, with uniforms the scene declares set per view -- view v's frame
    // is what setUniform(pose) + setUniform of view v's values of every listed
    // uniform + RenderTexture::draw gives; an unlisted uniform keeps the value
    // set on the shader, and the shader's own values do not change.  A plugin's
    // batch kernel is compiled on the first call after loadFromFile unless
    // batchPrepare did it before.  With a built-in scene: renderBatch, and a
    // non-empty list fails.
    bool renderBatchEx(int w, int h, const rm_view* views, int n, const rm_view_uniform* uniforms, int nUniforms,
                       std::uint32_t* out, rm_stats* stats = nullptr) {
        return ctx_ && rm_render_batch_ex_rgba8(ctx_, w, h, views, n, uniforms, nUniforms, out, stats) == RM_OK;
    }
    bool renderBatchEx(int w, int h, const rm_view* views, int n, const rm_view_uniform* uniforms, int nUniforms,
                       float* out, rm_stats* stats = nullptr) {
        return ctx_ && rm_render_batch_ex(ctx_, w, h, views, n, uniforms, nUniforms, out, stats) == RM_OK;
    }
    bool batchPrepare() { return ctx_ && rm_batch_prepare(ctx_) == RM_OK; }
    // rm.h rm_aa_prepare: compile and load a scene plugin's refine kernel now, not
    // inside the first RenderTexture::drawAAEx (nothing to do for a built-in scene)
    bool prepareAA() { return ctx_ && rm_aa_prepare(ctx_) == RM_OK; }
    // rm.h rm_render_batch_aa_rgba8: renderBatch's RGBA8 frames with every view's
    // edge pixels supersampled, view v's frame what setUniform(pose) +
    // RenderTexture::drawAA(shader, samples, threshold) gives.  mask (n * w * h
    // bytes) and refined (n words, the views' counts of refined pixels) may be
    // null; they live where `out` does (all device or all host pointers).  Every
    // view's offset must be (0, 0).
    bool renderBatchAA(int w, int h, const rm_view* views, int n, std::uint32_t* out, int samples = 4,
                       int threshold = 32, std::uint8_t* mask = nullptr, std::uint32_t* refined = nullptr,
                       rm_aa_stats* stats = nullptr) {
        const rm_aa_params p{samples, threshold};
        return ctx_ && rm_render_batch_aa_rgba8(ctx_, w, h, views, n, &p, out, mask, refined, stats) == RM_OK;
    }
    // rm.h rm_render_batch_aa_ex_rgba8: renderBatchAA for any scene, a scene
    // plugin included, with uniforms the scene declares set per view as
    // renderBatchEx sets them -- view v's frame is what setUniform(pose) +
    // setUniform of view v's values + RenderTexture::drawAAEx gives.  A plugin's
    // batch and batch-refine kernels are compiled on the first call after
    // loadFromFile unless prepareBatchAA did it before.  With a built-in scene:
    // renderBatchAA, and a non-empty list fails.
    bool renderBatchAAEx(int w, int h, const rm_view* views, int n, const rm_view_uniform* uniforms, int nUniforms,
                         std::uint32_t* out, int samples = 4, int threshold = 32, std::uint8_t* mask = nullptr,
                         std::uint32_t* refined = nullptr, rm_aa_stats* stats = nullptr) {
        const rm_aa_params p{samples, threshold};
        return ctx_ && rm_render_batch_aa_ex_rgba8(ctx_, w, h, views, n, uniforms, nUniforms, &p, out, mask, refined,
                                                   stats) == RM_OK;
    }
    bool prepareBatchAA() { return ctx_ && rm_batch_aa_prepare(ctx_) == RM_OK; }

private:
    bool setArray(const char* name, int components, const float* v, std::size_t length) {
        return ctx_ && length <= 64 && rm_set_uniformfv(ctx_, name, components, v, (int)length) == RM_OK;
    }
    rm_ctx* ctx_ = nullptr;
    int device_ = 0;
};
static_assert(sizeof(Vec2) == 8 && sizeof(Vec3) == 12 && sizeof(Vec4) == 16, "tightly packed floats (rm_set_uniformfv)");

class RenderTexture;

// post.frag as main.cpp:56-58,209-210 drives it: the pass is rm_post_frag on the
// context of the ray-march shader.  The reference's user chooses the sample
// and the tonemap operator by editing post.frag's main(); here they are
// setSample / setTonemap (the defaults are post.frag as shipped: FXAA, none).
class PostShader {
public:
    explicit PostShader(Shader& pass) : pass_(pass) {}
    bool valid() const { return pass_.valid(); }
    rm_ctx* ctx() { return pass_.ctx(); }
    std::string lastError() const { return error_.empty() ? pass_.lastError() : error_; }

    bool setUniform(const char* name, Vec2 v) {
        if (std::strcmp(name, "u_resolution") != 0) return unknown(name);
        resolution_ = v;
        return true;
    }
    bool setUniform(const char* name, RenderTexture& texture) {
        if (std::strcmp(name, "u_main_tex") != 0) return unknown(name);
        main_tex_ = &texture;
        return true;
    }
    void setSample(rm_post_sample s) { sample_ = s; }
    void setTonemap(rm_tonemap t) { tonemap_ = t; }
    rm_post_sample sample() const { return sample_; }
    rm_tonemap tonemap() const { return tonemap_; }
    Vec2 resolution() const { return resolution_; }
    RenderTexture* mainTexture() { return main_tex_; }
    void markLoaded() { loaded_ = true; }
    bool loaded() const { return loaded_; }
    bool fail(const std::string& msg) {
        error_ = msg;
        return false;
    }
    // The pass over n frames of u_resolution packed one after the other in
    // device memory, such as a view batch's (rm_post_frag_batch): view v of
    // `dst` is RenderTexture::draw(post) of view v of `src`.  drawChainBatch:
    // that pass into `mid`, then PostBloom's into `dst` (rm_post_chain_batch),
    // main.cpp:209-214 for every view at once.
    bool drawBatch(const std::uint32_t* src, std::uint32_t* dst, int n) {
        if (!loaded_) return fail("rm::PostShader: not loaded (ShaderLoader::loadFromFile(\"post.frag\", ...))");
        fail("");  // (clear: a failure below is the library's message)
        return rm_post_frag_batch(ctx(), (int)resolution_.x, (int)resolution_.y, n, sample_, tonemap_, src, dst) == RM_OK;
    }
    bool drawChainBatch(const std::uint32_t* src, std::uint32_t* mid, std::uint32_t* dst, int n) {
        if (!loaded_) return fail("rm::PostShader: not loaded (ShaderLoader::loadFromFile(\"post.frag\", ...))");
        fail("");
        return rm_post_chain_batch(ctx(), (int)resolution_.x, (int)resolution_.y, n, sample_, tonemap_, src, mid, dst) ==
               RM_OK;
    }

private:
    bool unknown(const char* name) { return fail(std::string("rm::PostShader: post.frag has no uniform ") + name); }
    Shader& pass_;
    Vec2 resolution_{0.0f, 0.0f};
    RenderTexture* main_tex_ = nullptr;
    rm_post_sample sample_ = RM_POST_SAMPLE_FXAA;
    rm_tonemap tonemap_ = RM_TONEMAP_NONE;
    bool loaded_ = false;
    std::string error_;
};

struct ShaderLoader {
    // source/shader_loader.h:11
    static bool loadFromFile(const char* file_name, Shader::Type, Shader& out_shader) {
        if (!out_shader.valid()) {
            std::fprintf(stderr, "ShaderLoader: no HIP device\n");
            return false;
        }
        return rm_load_scene(out_shader.ctx(), file_name) == RM_OK;  // prints its own message on failure
    }
    // main.cpp:57: the post shader is post.frag (any directory); no file is read,
    // the pass is compiled into librm.so
    static bool loadFromFile(const char* file_name, Shader::Type, PostShader& out_shader) {
        const char* base = std::strrchr(file_name, '/');
        base = base ? base + 1 : file_name;
        if (!out_shader.valid() || std::strcmp(base, "post.frag") != 0) {
            std::fprintf(stderr, "ShaderLoader: can't load file %s (the post shader is post.frag)\n", file_name);
            return false;
        }
        out_shader.markLoaded();
        return true;
    }
};

// A W x H render target resident in device memory (sf::RenderTexture).  RGBA8
// by default, the format the reference's RenderTextures hold (main.cpp:34-50):
// the kernel packs the pixel in its epilogue (rm_render_rgba8, 4 B/px of HBM);
// RGBA32F keeps gl_FragColor unrounded (rm_render, 16 B/px).  A draw is
// asynchronous on the shader's stream; copyToHostRGBA8 waits for it.
class RenderTexture {
public:
    enum Format { RGBA8, RGBA32F };

    ~RenderTexture() { release(); }
    bool create(int w, int h, Format fmt = RGBA8) {
        release();
        w_ = w;
        h_ = h;
        fmt_ = fmt;
        return hipMalloc(&tex_, (size_t)w * h * (fmt == RGBA8 ? 4 : 16)) == hipSuccess;
    }
    // RenderTarget::draw(sprite, &shader) with the full-screen sprite (main.cpp:199,205)
    bool draw(Shader& shader, rm_stats* stats = nullptr) {
        if (!tex_) return false;
        return (fmt_ == RGBA8 ? rm_render_rgba8(shader.ctx(), w_, h_, static_cast<uint32_t*>(tex_), stats)
                              : rm_render(shader.ctx(), w_, h_, static_cast<float*>(tex_), stats)) == RM_OK;
    }
    // The same draw reading the ping-pong plumbing (u_sample = this texture,
    // u_sample_part, u_seed1; main.cpp:192-207): progressive accumulation
    // (rm_render_accumulate[_rgba8]).  In place: each pixel reads only itself.
    bool drawAccumulate(Shader& shader, rm_stats* stats = nullptr) {
        if (!tex_) return false;
        return (fmt_ == RGBA8 ? rm_render_accumulate_rgba8(shader.ctx(), w_, h_, static_cast<uint32_t*>(tex_), stats)
                              : rm_render_accumulate(shader.ctx(), w_, h_, static_cast<float*>(tex_), stats)) ==
               RM_OK;
    }
    // draw() with adaptive supersampling (rm_render_aa_rgba8; the reference's
    // main() is "NO AA"): the frame's edge pixels -- a channel's spread over the
    // 3x3 neighbourhood >= threshold, 0..255 -- are rendered again with
    // `samples` (2, 4 or 8) sub-pixel samples and averaged.  RGBA8 targets and
    // built-in scenes only; the default threshold is a convenience, not tuned.
    bool drawAA(Shader& shader, int samples = 4, int threshold = 32, rm_aa_stats* stats = nullptr) {
        if (!tex_ || fmt_ != RGBA8) return false;
        const rm_aa_params p{samples, threshold};
        return rm_render_aa_rgba8(shader.ctx(), w_, h_, &p, static_cast<uint32_t*>(tex_), nullptr, stats) == RM_OK;
    }
    // drawAA for any scene, a scene plugin included (rm_render_aa_ex_rgba8): with
    // a built-in scene it is drawAA; a plugin's refine kernel is compiled on the
    // first call after loadFromFile unless Shader::prepareAA did it before.
    bool drawAAEx(Shader& shader, int samples = 4, int threshold = 32, rm_aa_stats* stats = nullptr) {
        if (!tex_ || fmt_ != RGBA8) return false;
        const rm_aa_params p{samples, threshold};
        return rm_render_aa_ex_rgba8(shader.ctx(), w_, h_, &p, static_cast<uint32_t*>(tex_), nullptr, stats) == RM_OK;
    }
    // RenderTarget::draw(sprite, &post_shader) (main.cpp:210): post.frag over the
    // shader's u_main_tex into this RGBA8 target (rm_post_frag)
    bool draw(PostShader& post) {
        RenderTexture* src = post.mainTexture();
        if (!post.loaded())
            return post.fail("rm::PostShader: not loaded (ShaderLoader::loadFromFile(\"post.frag\", ...))");
        if (!src || !src->textureRGBA8() || !textureRGBA8())
            return post.fail("rm::PostShader: u_main_tex and the target must be RGBA8 textures");
        if (src->w_ != w_ || src->h_ != h_ || post.resolution().x != (float)w_ || post.resolution().y != (float)h_)
            return post.fail("rm::PostShader: u_resolution, u_main_tex and the target must have one size");
        post.fail("");  // (clear: a failure below is the library's message)
        return rm_post_frag(post.ctx(), w_, h_, post.sample(), post.tonemap(), src->textureRGBA8(), textureRGBA8()) ==
               RM_OK;
    }
    Format format() const { return fmt_; }
    // the device target: RGBA8 words (R in the low byte) or RGBA32F texels;
    // asking for the other format's view returns null and says so once
    uint32_t* textureRGBA8() { return fmt_ == RGBA8 ? static_cast<uint32_t*>(tex_) : mismatch<uint32_t>("RGBA8"); }
    const uint32_t* textureRGBA8() const { return fmt_ == RGBA8 ? static_cast<const uint32_t*>(tex_) : nullptr; }
    float* texture() { return fmt_ == RGBA32F ? static_cast<float*>(tex_) : mismatch<float>("RGBA32F"); }
    int width() const { return w_; }
    int height() const { return h_; }
    // RGBA8 (the reference target's format), row 0 first (looks up).  An
    // RGBA32F target is packed into a device buffer kept for later calls.
    bool copyToHostRGBA8(Shader& shader, std::vector<uint32_t>& out) {
        out.resize((size_t)w_ * h_);
        const uint32_t* src = textureRGBA8();
        if (!src) {
            if (!packed_ && hipMalloc(&packed_, out.size() * sizeof(uint32_t)) != hipSuccess) {
                packed_ = nullptr;
                return false;
            }
            if (rm_pack_rgba8(shader.ctx(), (int64_t)out.size(), static_cast<const float*>(tex_), packed_) != RM_OK)
                return false;
            src = packed_;
        }
        return rm_synchronize(shader.ctx()) == RM_OK &&
               hipMemcpy(out.data(), src, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
    }

private:
    template <typename T>
    T* mismatch(const char* want) {
        if (!warned_) {
            std::fprintf(stderr, "rm::RenderTexture: a %s view of a %s target (create(w, h, RenderTexture::%s))\n",
                         want, fmt_ == RGBA8 ? "RGBA8" : "RGBA32F", want);
            warned_ = true;
        }
        return nullptr;
    }
    void release() {
        if (tex_) (void)hipFree(tex_);
        if (packed_) (void)hipFree(packed_);
        tex_ = nullptr;
        packed_ = nullptr;
    }
    void* tex_ = nullptr;
    uint32_t* packed_ = nullptr;
    int w_ = 0, h_ = 0;
    Format fmt_ = RGBA8;
    bool warned_ = false;
};

// source/post_bloom.h: bloom.frag over a texture's mip chain (rm_bloom), on the
// context of the ray-march shader
class PostBloom {
public:
    explicit PostBloom(Shader& pass) : pass_(pass) {}
    void init(Vec2 resolution) { resolution_ = resolution; }
    // main.cpp:212-214: setSmooth + generateMipmap of `src` are part of the pass
    bool apply(const RenderTexture& src, RenderTexture& dst) {
        if (!src.textureRGBA8() || !dst.textureRGBA8() || src.width() != dst.width() || src.height() != dst.height() ||
            resolution_.x != (float)src.width() || resolution_.y != (float)src.height())
            return false;
        return rm_bloom(pass_.ctx(), src.width(), src.height(), src.textureRGBA8(), dst.textureRGBA8()) == RM_OK;
    }
    // apply() over n frames of init()'s resolution packed one after the other in
    // device memory, such as a view batch's (rm_bloom_batch): view v of `dst` is
    // apply() of view v of `src`
    bool applyBatch(const uint32_t* src, uint32_t* dst, int n) {
        return rm_bloom_batch(pass_.ctx(), (int)resolution_.x, (int)resolution_.y, n, src, dst) == RM_OK;
    }

private:
    Shader& pass_;
    Vec2 resolution_{0.0f, 0.0f};
};

// The multi-GPU form of RenderTexture::draw: a W x H RGBA8 frame whose row
// bands are rendered by one Shader per GPU and gathered over RCCL to the first
// shader's device (rm_comm_init_all + rm_render_sharded_all, one process
// driving N GPUs).  Set the same uniforms on every shader before draw().
class ShardedRenderTexture {
public:
    ~ShardedRenderTexture() { release(); }
    bool create(int w, int h, const std::vector<Shader*>& shaders, int band = 16) {
        release();
        if (shaders.empty()) return false;
        std::vector<rm_ctx*> ctxs;
        for (Shader* s : shaders) {
            if (!s || !s->valid()) return false;
            ctxs.push_back(s->ctx());
        }
        comms_.assign(ctxs.size(), nullptr);
        if (rm_comm_init_all(comms_.data(), ctxs.data(), (int)ctxs.size()) != RM_OK) {
            comms_.clear();
            return false;
        }
        root_ = shaders[0];
        w_ = w;
        h_ = h;
        band_ = band;
        int dev = 0;
        (void)hipGetDevice(&dev);
        bool ok = hipSetDevice(root_->device()) == hipSuccess &&
                  hipMalloc(&frame_, (size_t)w * h * sizeof(uint32_t)) == hipSuccess;
        (void)hipSetDevice(dev);
        return ok;
    }
    // stats: one rm_stats per GPU (or null)
    bool draw(rm_stats* stats = nullptr) {
        return frame_ && rm_render_sharded_all(comms_.data(), (int)comms_.size(), w_, h_, band_, frame_, stats) == RM_OK;
    }
    uint32_t* frame() { return frame_; }
    bool copyToHostRGBA8(std::vector<uint32_t>& out) {
        out.resize((size_t)w_ * h_);
        return rm_synchronize(root_->ctx()) == RM_OK && hipSetDevice(root_->device()) == hipSuccess &&
               hipMemcpy(out.data(), frame_, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
    }

private:
    void release() {
        for (rm_comm* c : comms_)
            if (c) rm_comm_destroy(c);
        comms_.clear();
        if (frame_) (void)hipFree(frame_);
        frame_ = nullptr;
    }
    std::vector<rm_comm*> comms_;
    Shader* root_ = nullptr;
    uint32_t* frame_ = nullptr;
    int w_ = 0, h_ = 0, band_ = 16;
};

}  // namespace rm
