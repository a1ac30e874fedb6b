// raymarch_headless.cpp -- the reference's frame loop (main.cpp:12-226)
// without a window: the ray-march pass runs through rm::Shader /
// rm::RenderTexture (include/rm_pass.hpp -> librm.so) exactly where main.cpp
// calls ShaderLoader / sf::Shader::setUniform / RenderTexture::draw.
//
// Input comes from a script instead of SFML events: one character per frame,
// W/A/S/D/U(p)/N(down) move as the reference's WASD/Space/LShift
// (main.cpp:111-126,155-171), '.' = no key; --mouse dx,dy adds a per-frame
// mouse delta (main.cpp:86-97).  --post runs the reference's post passes after
// each frame (main.cpp:209-214: post.frag into postTexture, bloom of it back
// into outputTexture) through rm::PostShader / rm::PostBloom; --post-sample and
// --tonemap stand for an edit of post.frag's main().  The ImGui overlay stays
// out of scope.  With --post, --ppm writes the frame after the post passes.
//
// Usage: raymarch_headless [--scene output_shader.frag] [--w 1600] [--h 900]
//          [--frames 60] [--script WWWWDD..] [--mouse 3,0] [--time-freeze]
//          [--steps 128] [--ppm out.ppm] [--gpus N] [--band 16] [--accumulate]
//          [--format rgba8|float] [--stats] [--warmup N]
//          [--post] [--post-sample fxaa|chromatic|texel]
//          [--tonemap none|aces|reinhard|jodie|uncharted2]
//          [--uniform name=v[,v...]]... [--pick X,Y] [--aa K[:threshold]]
//          [--fisheye fov_deg] [--views FILE]
// --views FILE renders one view batch instead of the frame loop
// (rm::Shader::renderBatchEx -> rm_render_batch_ex_rgba8: any scene, a .hip
// scene plugin included, its --uniform values shared by the views): FILE holds
// one view per line, px py pz mx my t [ox oy] (u_pos, u_mouse, u_time and an optional
// sub-pixel offset), all rendered at --w x --h by one launch on one GPU.  With
// --ppm NAME it writes NAME.0000.ppm, NAME.0001.ppm, ...; with --stats the JSON
// line carries the launch's kernel_ms.  With --aa K[:threshold] the batch is
// rendered antialiased (rm::Shader::renderBatchAAEx -> rm_render_batch_aa_ex_rgba8,
// any scene again, every view's offset (0, 0)): the JSON line gains "aa": K and "refined": the
// pixels refined over all views, and kernel_ms sums the batch, detect + plan
// and refine launches.  With --post [--post-sample ..] [--tonemap ..] the batch
// (antialiased or not) is rendered into a device target and the post passes run
// over all its views at once (rm::PostShader::drawChainBatch ->
// rm_post_chain_batch): --ppm then writes the post-processed frames and the
// JSON line gains "post": true.
// --fisheye fov_deg writes --ppm from the fisheye camera main() carries
// commented out (output_shader.frag:396-400) instead of the pinhole's frame:
// after the last frame its w x h rays are built here on the host, from the
// last frame's u_pos and u_mouse, and shaded by rm::Shader::shadeRays (rm.h
// rm_shade_rays) as a ray image with the frame's vignette into RGBA8 words.
// One GPU.
// --aa K[:threshold] draws each frame with adaptive supersampling
// (rm::RenderTexture::drawAAEx -> rm_render_aa_ex_rgba8: any scene, a .hip
// scene plugin included): K = 2, 4 or 8 samples at
// the pixels whose 3x3 neighbourhood spreads a colour channel by at least
// threshold (0..255, default 32; 0: every pixel).  One GPU, the RGBA8 target;
// --stats then counts the base frame's, the detect and the refine kernel.
// --uniform sets a uniform the scene declares itself (a scene plugin's
// `uniform vec4 u_ball = ...;`, rm.h rm_load_scene) once the scene is loaded:
// one to four numbers for a float / vec2 / vec3 / vec4, one for an int or a
// bool; repeatable.
// --pick X,Y prints a JSON line about what is under pixel (X, Y) of the last
// frame drawn: the pixel's ray from rm::Shader::cameraRays, cast with
// castRays (rm.h rm_cast_rays): status, t, position, normal and the
// material's diffuse colour.
// Frames are drawn into the RGBA8 target the reference renders into
// (--format float: RGBA32F) and queued without a host synchronization per
// frame; --stats times each frame's kernel (HIP events, which waits for every
// frame) and reports kernel_ms_per_frame.  fps_wall counts the frames after
// --warmup (untimed) frames, up to the completion of the last one.
// --gpus N renders each frame's row bands on GPUs 0..N-1 and gathers them over
// RCCL to GPU 0 (rm::ShardedRenderTexture -> rm_render_sharded_all); --sharded
// takes that path with one GPU too.
#include <chrono>
#include <cmath>
#include <initializer_list>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/rm_pass.hpp"

// a w x h RGBA8 frame (R in the low byte) as a binary PPM
static bool write_ppm(const std::string& name, const uint32_t* px, int w, int h) {
    FILE* fp = std::fopen(name.c_str(), "wb");
    if (!fp) return false;
    std::fprintf(fp, "P6\n%d %d\n255\n", w, h);
    for (size_t i = 0; i < (size_t)w * h; i++) {
        const uint32_t v = px[i];
        unsigned char rgb[3] = {(unsigned char)(v & 255), (unsigned char)((v >> 8) & 255),
                                (unsigned char)((v >> 16) & 255)};
        std::fwrite(rgb, 1, 3, fp);
    }
    return std::fclose(fp) == 0;
}

// --views FILE: one view per line, px py pz mx my t [ox oy]; empty lines and lines starting with '#' are skipped
static bool read_views(const std::string& file, std::vector<rm_view>& views) {
    FILE* fp = std::fopen(file.c_str(), "r");
    if (!fp) {
        std::fprintf(stderr, "--views: cannot open %s\n", file.c_str());
        return false;
    }
    char line[512];
    int lineno = 0;
    bool ok = true;
    while (ok && std::fgets(line, sizeof(line), fp)) {
        lineno++;
        const char* p = line;
        while (*p == ' ' || *p == '\t') p++;
        if (*p == '#' || *p == '\n' || *p == '\r' || *p == '\0') continue;
        rm_view v;
        std::memset(&v, 0, sizeof(v));
        char tail = 0;
        const int got = std::sscanf(p, "%f %f %f %f %f %f %f %f %c", &v.pos[0], &v.pos[1], &v.pos[2], &v.mouse[0],
                                    &v.mouse[1], &v.time, &v.offset[0], &v.offset[1], &tail);
        if (got != 6 && got != 8) {
            std::fprintf(stderr, "--views %s:%d: expected px py pz mx my t [ox oy]\n", file.c_str(), lineno);
            ok = false;
        }
        views.push_back(v);
    }
    std::fclose(fp);
    return ok;
}

int main(int argc, char** argv) {
    std::string scene = "output_shader.frag", script, ppm, views_file;
    int w = 1600, h = 900, frames = 60, steps = 128, gpus = 1, band = 16;
    int mdx = 0, mdy = 0;
    bool time_freeze = false, sharded = false, accumulate = false, stats = false, fmt_float = false;
    int warmup = 0;
    int pick_x = -1, pick_y = -1;
    int aa_samples = 0, aa_threshold = 32;  // --aa (0: off)
    float fisheye_fov = 0.0f;               // --fisheye (0: off)
    bool post = false;
    rm_post_sample post_sample = RM_POST_SAMPLE_FXAA;
    rm_tonemap tonemap = RM_TONEMAP_NONE;
    struct UniformArg {
        std::string name;
        std::vector<double> v;
    };
    std::vector<UniformArg> uniform_args;
    // a name of `names` -> its index, or -1
    auto choice = [](const std::string& v, std::initializer_list<const char*> names) {
        int k = 0;
        for (const char* n : names) {
            if (v == n) return k;
            k++;
        }
        return -1;
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() { return i + 1 < argc ? std::string(argv[++i]) : std::string(); };
        if (a == "--scene") scene = next();
        else if (a == "--w") w = std::atoi(next().c_str());
        else if (a == "--h") h = std::atoi(next().c_str());
        else if (a == "--frames") frames = std::atoi(next().c_str());
        else if (a == "--script") script = next();
        else if (a == "--steps") steps = std::atoi(next().c_str());
        else if (a == "--gpus") gpus = std::atoi(next().c_str());
        else if (a == "--band") band = std::atoi(next().c_str());
        else if (a == "--ppm") ppm = next();
        else if (a == "--views") views_file = next();
        else if (a == "--time-freeze") time_freeze = true;
        else if (a == "--sharded") sharded = true;
        else if (a == "--accumulate") accumulate = true;
        else if (a == "--stats") stats = true;
        else if (a == "--warmup") warmup = std::atoi(next().c_str());
        else if (a == "--format") {
            const std::string f = next();
            if (f != "rgba8" && f != "float") {
                std::fprintf(stderr, "--format rgba8|float\n");
                return 2;
            }
            fmt_float = f == "float";
        }
        else if (a == "--post") post = true;
        else if (a == "--post-sample") {
            const int k = choice(next(), {"fxaa", "texel", "chromatic"});  // rm_post_sample's order
            if (k < 0) {
                std::fprintf(stderr, "--post-sample fxaa|chromatic|texel\n");
                return 2;
            }
            post_sample = (rm_post_sample)k;
        }
        else if (a == "--tonemap") {
            const int k = choice(next(), {"none", "aces", "reinhard", "jodie", "uncharted2"});  // rm_tonemap's order
            if (k < 0) {
                std::fprintf(stderr, "--tonemap none|aces|reinhard|jodie|uncharted2\n");
                return 2;
            }
            tonemap = (rm_tonemap)k;
        }
        else if (a == "--mouse") std::sscanf(next().c_str(), "%d,%d", &mdx, &mdy);
        else if (a == "--pick") {
            if (std::sscanf(next().c_str(), "%d,%d", &pick_x, &pick_y) != 2 || pick_x < 0 || pick_y < 0) {
                std::fprintf(stderr, "--pick X,Y\n");
                return 2;
            }
        }
        else if (a == "--aa") {
            const std::string v = next();
            char tail = 0;
            const int got = std::sscanf(v.c_str(), "%d:%d%c", &aa_samples, &aa_threshold, &tail);
            if ((got != 1 && got != 2) || (got == 1 && v.find(':') != std::string::npos) ||
                (aa_samples != 2 && aa_samples != 4 && aa_samples != 8) || aa_threshold < 0 || aa_threshold > 255) {
                std::fprintf(stderr, "--aa K[:threshold]  (K = 2, 4 or 8; threshold 0..255)\n");
                return 2;
            }
        }
        else if (a == "--fisheye") {
            fisheye_fov = (float)std::atof(next().c_str());
            if (!(fisheye_fov > 0.0f && fisheye_fov <= 360.0f)) {
                std::fprintf(stderr, "--fisheye fov_deg  (0 < fov <= 360)\n");
                return 2;
            }
        }
        else if (a == "--uniform") {
            const std::string u = next();
            const size_t eq = u.find('=');
            UniformArg arg;
            arg.name = u.substr(0, eq);
            const char* p = eq == std::string::npos ? "" : u.c_str() + eq + 1;
            while (*p) {
                char* end = nullptr;
                const double x = std::strtod(p, &end);
                if (end == p || (*end != ',' && *end != '\0')) break;
                arg.v.push_back(x);
                p = *end ? end + 1 : end;
                if (!*end) break;
            }
            if (arg.name.empty() || *p || arg.v.empty() || arg.v.size() > 4) {
                std::fprintf(stderr, "--uniform name=v[,v[,v[,v]]]\n");
                return 2;
            }
            uniform_args.push_back(arg);
        }
        else {
            std::fprintf(stderr, "unknown argument %s\n", a.c_str());
            return 2;
        }
    }
    // main.cpp:14-27
    float wf = (float)w, hf = (float)h;
    int mouseX = w / 2, mouseY = h / 2;
    const float mouseSensitivity = 3.0f, speed = 0.1f;
    rm::Vec3 pos{2.0f, 3.0f, 3.0f};
    int framesStill = 1;

    if (gpus < 1) {
        std::fprintf(stderr, "--gpus must be >= 1\n");
        return 2;
    }
    if (accumulate && (gpus > 1 || sharded)) {
        std::fprintf(stderr, "--accumulate renders on one GPU\n");
        return 2;
    }
    if (post && (gpus > 1 || sharded || accumulate || fmt_float)) {
        std::fprintf(stderr, "--post runs on the one-GPU RGBA8 target, without --accumulate\n");
        return 2;
    }
    if (aa_samples && (gpus > 1 || sharded || accumulate || fmt_float)) {
        std::fprintf(stderr, "--aa draws on the one-GPU RGBA8 target, without --accumulate\n");
        return 2;
    }
    if (fisheye_fov > 0.0f && (gpus > 1 || sharded || ppm.empty())) {
        std::fprintf(stderr, "--fisheye writes --ppm, on one GPU\n");
        return 2;
    }
    // one shader (librm context) per GPU; the first is the reference's `shader`
    std::vector<std::unique_ptr<rm::Shader>> shaders;
    std::vector<rm::Shader*> all;
    for (int g = 0; g < gpus; g++) {
        shaders.emplace_back(new rm::Shader(g));
        rm::Shader& s = *shaders.back();
        if (!s.valid()) {
            std::fprintf(stderr, "no HIP device %d\n", g);
            return 1;
        }
        if (!rm::ShaderLoader::loadFromFile(scene.c_str(), rm::Shader::Fragment, s)) return 1;
        s.setUniform("u_resolution", rm::Vec2{wf, hf});
        s.setMarchSteps(steps);
        for (const UniformArg& u : uniform_args) {
            // the declared type decides between the float and the int call
            rm_uniform_info info;
            int n = 0, type = RM_UNIFORM_FLOAT;
            rm_uniform_count(s.ctx(), &n);
            for (int k = 0; k < n; k++)
                if (rm_uniform_info_at(s.ctx(), k, &info) == RM_OK && u.name == info.name) type = info.type;
            const float x = (float)u.v[0], y = u.v.size() > 1 ? (float)u.v[1] : 0.0f,
                        z = u.v.size() > 2 ? (float)u.v[2] : 0.0f, q = u.v.size() > 3 ? (float)u.v[3] : 0.0f;
            const bool set = type != RM_UNIFORM_FLOAT && u.v.size() == 1 ? s.setUniform(u.name.c_str(), (int)u.v[0])
                             : u.v.size() == 1 ? s.setUniform(u.name.c_str(), x)
                             : u.v.size() == 2 ? s.setUniform(u.name.c_str(), rm::Vec2{x, y})
                             : u.v.size() == 3 ? s.setUniform(u.name.c_str(), rm::Vec3{x, y, z})
                                               : s.setUniform(u.name.c_str(), rm::Vec4{x, y, z, q});
            if (!set) {
                std::fprintf(stderr, "--uniform %s: %s\n", u.name.c_str(), s.lastError().c_str());
                return 1;
            }
        }
        all.push_back(&s);
    }
    rm::Shader& shader = *all[0];
    if (!views_file.empty()) {  // one batch instead of the frame loop
        std::vector<rm_view> views;
        if (!read_views(views_file, views)) return 2;
        const int n = (int)views.size();
        std::vector<uint32_t> px((size_t)n * w * h);  // a host target: staged, written when the call returns
        rm_stats st;
        std::memset(&st, 0, sizeof(st));
        rm_aa_stats aa_st;  // --aa: always taken, for the JSON line's "refined"
        std::memset(&aa_st, 0, sizeof(aa_st));
        // --post: the batch is rendered into a device target, and main.cpp:209-214's post passes run over all
        // its views at once (rm_post_chain_batch); the frames written are the post-processed ones
        uint32_t* dev = nullptr;  // frames | post.frag's output | bloom's output
        if (post && n > 0 && hipMalloc(&dev, 3 * px.size() * sizeof(uint32_t)) != hipSuccess) {
            std::fprintf(stderr, "cannot allocate the device targets of %d %dx%d views\n", n, w, h);
            return 1;
        }
        uint32_t* target = dev ? dev : px.data();
        const auto b0 = std::chrono::steady_clock::now();
        if (aa_samples ? !shader.renderBatchAAEx(w, h, views.data(), n, nullptr, 0, target, aa_samples, aa_threshold,
                                                 nullptr, nullptr, &aa_st)
                       : !shader.renderBatchEx(w, h, views.data(), n, nullptr, 0, target, stats ? &st : nullptr)) {
            std::fprintf(stderr, "--views failed: %s\n", shader.lastError().c_str());
            return 1;
        }
        if (dev) {
            rm::PostShader post_shader(shader);
            if (!rm::ShaderLoader::loadFromFile("post.frag", rm::Shader::Fragment, post_shader)) return 1;
            post_shader.setUniform("u_resolution", rm::Vec2{wf, hf});
            post_shader.setSample(post_sample);
            post_shader.setTonemap(tonemap);
            if (!post_shader.drawChainBatch(dev, dev + px.size(), dev + 2 * px.size(), n) ||
                rm_synchronize(shader.ctx()) != RM_OK ||
                hipMemcpy(px.data(), dev + 2 * px.size(), px.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) !=
                    hipSuccess) {
                std::fprintf(stderr, "--views --post failed: %s\n", post_shader.lastError().c_str());
                return 1;
            }
            (void)hipFree(dev);
        }
        if (aa_samples) st.kernel_ms = aa_st.base_ms + aa_st.detect_ms + aa_st.refine_ms;
        const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b0).count();
        std::printf("{\"views\": %d, \"w\": %d, \"h\": %d, \"scene\": \"%s\", \"format\": \"rgba8\", \"wall_ms\": %.3f", n, w,
                    h, scene.c_str(), wall_ms);
        if (stats) std::printf(", \"kernel_ms\": %.4f", st.kernel_ms);
        if (aa_samples) std::printf(", \"aa\": %d, \"refined\": %lld", aa_samples, (long long)aa_st.refined);
        if (post) std::printf(", \"post\": true");
        std::printf("}\n");
        for (int v = 0; v < n && !ppm.empty(); v++) {
            char suffix[32];
            std::snprintf(suffix, sizeof(suffix), ".%04d.ppm", v);
            if (!write_ppm(ppm + suffix, px.data() + (size_t)v * w * h, w, h)) return 1;
        }
        return 0;
    }
    sharded = sharded || gpus > 1;
    auto setAll = [&](const char* name, auto v) {
        for (rm::Shader* s : all) s->setUniform(name, v);
    };
    rm::RenderTexture outputTexture;
    rm::ShardedRenderTexture shardedTexture;
    if (!sharded ? !outputTexture.create(w, h, fmt_float ? rm::RenderTexture::RGBA32F : rm::RenderTexture::RGBA8)
                 : !shardedTexture.create(w, h, all, band)) {
        std::fprintf(stderr, "cannot allocate the %dx%d target on %d GPU(s): %s\n", w, h, gpus,
                     shader.lastError().c_str());
        return 1;
    }

    // main.cpp:48-50,56-61
    rm::RenderTexture postTexture;
    rm::PostShader post_shader(shader);
    rm::PostBloom post_bloom(shader);
    if (post) {
        if (!postTexture.create(w, h)) {
            std::fprintf(stderr, "cannot allocate the %dx%d post target\n", w, h);
            return 1;
        }
        if (!rm::ShaderLoader::loadFromFile("post.frag", rm::Shader::Fragment, post_shader)) return 1;
        post_shader.setUniform("u_resolution", rm::Vec2{wf, hf});
        post_shader.setSample(post_sample);
        post_shader.setTonemap(tonemap);
        post_bloom.init(rm::Vec2{wf, hf});
    }

    std::mt19937 e2(20261015);
    std::uniform_real_distribution<float> dist(0.0f, 1.0f);
    auto t0 = std::chrono::steady_clock::now();
    auto t_timed = t0;
    double kernel_ms = 0.0;
    rm::Vec2 mouse{0.0f, 0.0f};  // the last frame's u_mouse
    for (int f = 0; f < warmup + frames; f++) {
        if (f == warmup) {  // the timed frames start when the warm-up frames are done
            if (rm_synchronize(shader.ctx()) != RM_OK) return 1;
            t_timed = std::chrono::steady_clock::now();
        }
        bool wasd[6] = {false, false, false, false, false, false};
        char k = f < (int)script.size() ? script[f] : '.';
        const char keys[] = "WASDUN";
        for (int j = 0; j < 6; j++) wasd[j] = (k == keys[j]);
        mouseX += mdx;
        mouseY += mdy;
        if (mdx || mdy) framesStill = 1;
        // main.cpp:153-171: camera angles and a step along the view-rotated axes
        float mx = ((float)mouseX / w - 0.5f) * mouseSensitivity;
        float my = ((float)mouseY / h - 0.5f) * mouseSensitivity;
        float dx = (float)(wasd[3] - wasd[1]), dy = (float)(wasd[4] - wasd[5]), dz = (float)(wasd[2] - wasd[0]);
        float ty = dy * std::cos(-my) - dz * std::sin(-my);
        float tz = dy * std::sin(-my) + dz * std::cos(-my);
        float tx = dx;
        float nx = tx * std::cos(mx) - tz * std::sin(mx);
        float nz = tx * std::sin(mx) + tz * std::cos(mx);
        pos = rm::Vec3{pos.x + nx * speed, pos.y + ty * speed, pos.z + nz * speed};
        for (bool b : wasd)
            if (b) framesStill = 1;
        setAll("u_pos", pos);
        mouse = rm::Vec2{mx, my};
        setAll("u_mouse", mouse);
        if (!time_freeze) {
            float t = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
            setAll("u_time", t);
        }
        setAll("u_sample_part", 1.0f / framesStill);
        const rm::Vec2 seed1{dist(e2) * 999.0f, dist(e2) * 999.0f}, seed2{dist(e2) * 999.0f, dist(e2) * 999.0f};
        setAll("u_seed1", seed1);
        setAll("u_seed2", seed2);
        std::vector<rm_stats> st(gpus);
        rm_stats* stp = stats ? st.data() : nullptr;
        rm_aa_stats aa_st;
        // --accumulate: the pass reads u_sample/u_sample_part/u_seed1 (progressive
        // supersampling while the camera is still; one GPU)
        const bool drawn = sharded      ? shardedTexture.draw(stp)
                           : accumulate ? outputTexture.drawAccumulate(shader, stp)
                           : aa_samples ? outputTexture.drawAAEx(shader, aa_samples, aa_threshold, stats ? &aa_st : nullptr)
                                        : outputTexture.draw(shader, stp);
        if (drawn && aa_samples && stats) st[0].kernel_ms = aa_st.base_ms + aa_st.detect_ms + aa_st.refine_ms;
        if (!drawn) {
            std::fprintf(stderr, "draw failed: %s\n", shader.lastError().c_str());
            return 1;
        }
        if (post) {  // main.cpp:209-214
            post_shader.setUniform("u_main_tex", outputTexture);
            if (!postTexture.draw(post_shader) || !post_bloom.apply(postTexture, outputTexture)) {
                std::fprintf(stderr, "post passes failed: %s\n", post_shader.lastError().c_str());
                return 1;
            }
        }
        float slowest = 0.0f;
        for (const rm_stats& x : st) slowest = x.kernel_ms > slowest ? x.kernel_ms : slowest;
        if (f >= warmup) kernel_ms += slowest;
        framesStill++;
    }
    for (rm::Shader* s : all)
        if (rm_synchronize(s->ctx()) != RM_OK) return 1;
    double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_timed).count();
    std::printf("{\"frames\": %d, \"warmup\": %d, \"w\": %d, \"h\": %d, \"gpus\": %d, \"scene\": \"%s\", "
                "\"format\": \"%s\", \"fps_wall\": %.2f, ",
                frames, warmup, w, h, gpus, scene.c_str(), sharded || !fmt_float ? "rgba8" : "float", frames / wall);
    if (stats) std::printf("\"kernel_ms_per_frame\": %.4f, ", frames ? kernel_ms / frames : 0.0);
    std::printf("\"pos\": [%.4f, %.4f, %.4f]}\n", pos.x, pos.y, pos.z);
    if (pick_x >= 0) {  // the uniforms are the last frame's
        if (pick_x >= w || pick_y >= h) {
            std::fprintf(stderr, "--pick %d,%d outside the %dx%d frame\n", pick_x, pick_y, w, h);
            return 2;
        }
        rm::Vec3 origin{0.0f, 0.0f, 0.0f}, position, normal;
        std::vector<rm::Vec3> dirs((size_t)w * h);
        float t = 0.0f, material[16];
        int32_t status = 0;
        rm_ray_hits hits;
        std::memset(&hits, 0, sizeof(hits));
        hits.t = &t;
        hits.status = &status;
        hits.position = &position.x;
        hits.normal = &normal.x;
        hits.material = material;
        if (!shader.cameraRays(w, h, &origin, dirs.data()) ||
            !shader.castRays(&origin, true, &dirs[(size_t)pick_y * w + pick_x], 1, hits)) {
            std::fprintf(stderr, "--pick failed: %s\n", shader.lastError().c_str());
            return 1;
        }
        std::printf("{\"pick\": [%d, %d], \"status\": \"%s\", \"t\": %.9g, \"position\": [%.9g, %.9g, %.9g], "
                    "\"normal\": [%.9g, %.9g, %.9g], \"diffuse\": [%.9g, %.9g, %.9g]}\n",
                    pick_x, pick_y, status == RM_RAY_HIT ? "hit" : status == RM_RAY_MISS ? "miss" : "exhausted", t,
                    position.x, position.y, position.z, normal.x, normal.y, normal.z, material[0], material[1],
                    material[2]);
    }
    if (!ppm.empty()) {
        std::vector<uint32_t> px;
        if (fisheye_fov > 0.0f) {
            // (0, 0, -1) turned by -uv.y and uv.x times radians(fov) / 2, then by the mouse
            // (output_shader.frag:396-404), in f32; row vector times rot(a) = mat2(c, -s, s, c)
            auto rot = [](float& a, float& b, float angle) {
                const float c = std::cos(angle), s = std::sin(angle);
                const float a1 = a * c + b * -s, b1 = a * s + b * c;
                a = a1;
                b = b1;
            };
            const float coeff = fisheye_fov * 0.017453292519943295f * 0.5f;
            std::vector<rm::Vec3> dirs((size_t)w * h);
            for (int y = 0; y < h; y++) {
                for (int x = 0; x < w; x++) {
                    const float ux = (((float)x + 0.5f) / wf - 0.5f) * wf / hf;
                    const float uy = (((float)y + 0.5f) / hf - 0.5f) * hf / hf;
                    rm::Vec3 d{0.0f, 0.0f, -1.0f};
                    rot(d.y, d.z, -uy * coeff);
                    rot(d.x, d.z, ux * coeff);
                    rot(d.y, d.z, -mouse.y);
                    rot(d.x, d.z, mouse.x);
                    dirs[(size_t)y * w + x] = d;
                }
            }
            px.resize((size_t)w * h);
            const rm_shade_params sp{w, RM_SHADE_DISPLAY, 1};
            if (!shader.shadeRays(&pos, true, dirs.data(), (std::int64_t)w * h, sp, nullptr, px.data())) {
                std::fprintf(stderr, "--fisheye failed: %s\n", shader.lastError().c_str());
                return 1;
            }
        } else if (!sharded ? !outputTexture.copyToHostRGBA8(shader, px) : !shardedTexture.copyToHostRGBA8(px)) {
            return 1;
        }
        if (!write_ppm(ppm, px.data(), w, h)) return 1;
    }
    return 0;
}
