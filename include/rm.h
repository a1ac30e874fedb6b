/*
 * rm.h -- C ABI of librm.so, the MI355X (gfx950) ray-march pass.
 *
 * Drop-in boundary for the reference's full-screen fragment pass
 * (cahekp/Raymarching).  The reference drives that pass through SFML:
 *
 *   ShaderLoader::loadFromFile(file, sf::Shader::Fragment, shader)
 *       source/shader_loader.h:11, source/shader_loader.cpp:8-20
 *   shader.setUniform("u_resolution" | "u_pos" | "u_mouse" | "u_time" | ...)
 *       main.cpp:54,187-194 (include/SFML/Graphics/Shader.hpp:297,306,315)
 *   renderTexture.draw(fullScreenSprite, &shader)
 *       main.cpp:199,205 (include/SFML/Graphics/RenderTarget.hpp:237)
 *
 * and each entry point below replaces one of those calls (see the per-call
 * comments and INTEGRATION.md).  Conventions: every call returns an
 * rm_status (no exceptions cross the ABI); buffers are caller-owned; one
 * rm_ctx per host thread; uniforms/params are state of the ctx, read at the
 * next render call, as GL uniforms are read at the next draw.
 *
 * Pixel convention: out[row*W + col] is the fragment with
 * gl_TexCoord = ((col+0.5)/W, (row+0.5)/H); row 0 is first in memory and
 * looks up.  Pixels are RGBA float32 (gl_FragColor,
 * alpha = 1) or, from the *_rgba8 calls, RGBA8 unorm as the reference's
 * sf::RenderTexture stores them.
 */
#ifndef RM_H_
#define RM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the structs and calls below.  Bumped whenever a struct the
 * library writes grows or a call changes meaning; a caller compiled against
 * one version must not pass its structs to a library of another (check
 * rm_abi_version() == RM_ABI_VERSION once at start-up).
 *   1  round 1-2 (rm_stats without `skipped`)
 *   2  rm_stats.skipped
 *   3  rm_stats.dispatch, rm_stats.lat_tiles; rm_abi_version() */
#define RM_ABI_VERSION 3

typedef enum rm_status {
    RM_OK = 0,
    RM_ERR_INVALID_ARGUMENT = 1, /* bad pointer/size/uniform arity                       */
    RM_ERR_FILE = 2,             /* "can't load file" (source/shader_loader.cpp:26-30)  */
    RM_ERR_SCENE = 3,            /* no scene plugin for this source (cf. GL compile fail) */
    RM_ERR_NO_SCENE = 4,         /* render before a successful rm_load_scene            */
    RM_ERR_DEVICE = 5,           /* HIP runtime error (message in rm_last_error)        */
    RM_ERR_OUT_OF_MEMORY = 6
} rm_status;

typedef struct rm_ctx rm_ctx;

/* Run-time knobs that replace the reference's compile-time constants. */
typedef struct rm_params {
    int32_t max_steps;        /* MAX_MARCHING_STEPS, common.frag:15 (default 128)        */
    int32_t shadow_max_steps; /* softshadow2 cap; 0 = unbounded as common.frag:814       */
    int32_t count_evals;      /* 1: instrumented kernel, rm_stats.evals = sceneSDF calls */
    int32_t kernel;           /* workgroup tiling: 0 auto (= 2), 1 16x16 px (4 waves), 2 8x8 px (1 wave), 3 16x4 px (1 wave),
                                 4 8x8 px tiles pulled by persistent waves from an atomic counter (built-in scenes) */
    int32_t schedule;         /* dispatch order of one-wave tiles: 1 (default) = the costliest tiles of a recent
                                 launch of the same geometry on the same stream first (their measured durations,
                                 counting-sorted on the GPU right after every 16th launch, on its stream,
                                 RM_SCHED_PERIOD; the first launch of a geometry runs row-major); 0 = row-major.
                                 Pixels are the same either way; an rm_set_tile_order order takes precedence. */
} rm_params;

/* rm_stats.dispatch: the order the launch's workgroups rendered tiles in */
enum {
    RM_DISPATCH_ROW_MAJOR = 0, /* workgroup i renders tile i                                    */
    RM_DISPATCH_EXPLICIT = 1,  /* rm_set_tile_order's order                                      */
    RM_DISPATCH_ADAPTIVE = 2   /* sorted durations of an earlier launch (rm_params.schedule = 1)  */
};

typedef struct rm_stats {
    uint64_t evals;  /* sceneSDF calls (ray-steps) of this render, when count_evals   */
    uint64_t pixels; /* pixels rendered                                                */
    float kernel_ms; /* device time of the render kernel (HIP events on the ctx stream) */
    int32_t scene;   /* scene id that ran                                              */
    uint64_t flop;   /* algorithmic FLOP of those calls, when count_evals: the per-term
                        tally of SURVEY.md 8(d) over the terms evaluated (exact early
                        exits skip Menger folds and scene O's primitives)          */
    uint64_t skipped; /* when count_evals: of `evals`, the ray-steps the uninstrumented
                        kernels do not execute (exact early exits whose results equal
                        the reference's: settled soft shadows, the soft shadows of
                        points facing away from the light, scene T's reflection march
                        past depth 3); executed = evals - skipped -
                        the counts rm_certified_steps() and rm_reflection_cleared_steps() return */
    int32_t dispatch; /* RM_DISPATCH_*: the tile order this launch ran (ABI 3)           */
    int32_t lat_tiles; /* scene T: workgroups that rendered with the latency-optimized
                         fold tests (the costliest tiles at the head of an ordered
                         launch of at most 98304 tiles); 0 otherwise
                         (ABI 3)                                                        */
    float gather_ms;   /* rm_render_sharded*: device time of the RGB8 pack and the gather
                         on this rank's stream (rank 0: until every wire has arrived,
                         so it includes waiting for the slowest rank); 0 elsewhere (ABI 3) */
    float deinterleave_ms; /* rm_render_sharded*, rank 0: the de-interleave kernel (ABI 3) */
} rm_stats;

/* RM_ABI_VERSION of the library (compare with the header's). */
int rm_abi_version(void);

/* Create a context on HIP device `device`.  Scene unset, params default. */
rm_status rm_create(rm_ctx **out, int device);
/* Waits for the work this context enqueued (its own events, not the device),
 * then frees it.  The stream it is bound to must still exist (rm_set_stream).
 * If recording on that stream reports an error, it waits for the whole device
 * instead. */
rm_status rm_destroy(rm_ctx *ctx);

/* Replaces ShaderLoader::loadFromFile (source/shader_loader.cpp:8-20).
 * If `file_name` exists it is preprocessed with the reference's #include
 * semantics (source/shader_loader.cpp:22-81; missing include -> RM_ERR_FILE).
 * The scene is chosen by the file's base name: "output_shader.frag"
 * (scene O), "template.frag" (scene T, repaired as SURVEY.md App. A),
 * "sphere" (scene S0), "output_shader_glass" (test scene OG).  A registered
 * name needs no file on disk (the GPU host has no shader tree).  When the
 * file exists its text decides (the reference's reload recompiles the edited
 * shader): output_shader.frag whose lighting/render/main code and included
 * common.frag are the reference's (whitespace-insensitive fingerprints) loads
 * the compiled-in scene O if its scene part (materials, floorMat, sceneSDF) is
 * the reference's too, and otherwise compiles that scene part with hiprtc as
 * a scene plugin into output_shader.frag's pipeline; other edits (pipeline,
 * common.frag, template.frag's text) return RM_ERR_SCENE.  Any other
 * existing file named "*.hip" is a scene plugin: a source defining
 * `SdResult sceneSDF(vec3 p)` with the reference's scene library
 * (common.frag:37-679; raymarching_amd/csrc/rm_sdf_lib.h), compiled here with
 * hiprtc into output_shader.frag's pass around that scene (the reference's
 * "Reload scene shader", main.cpp:134-139).  A compile error prints the log
 * and returns RM_ERR_SCENE, keeping the previous scene.  Unknown name and no
 * file -> RM_ERR_FILE; another existing file -> RM_ERR_SCENE.
 *
 * A scene plugin (a .hip file or an edited scene part) may declare uniforms
 * of its own beside the pass's, at file scope (outside braces, parentheses,
 * comments, string literals and preprocessor lines):
 *     uniform <type> <name>;           type: float vec2 vec3 vec4 int bool
 *     uniform <type> <name> = <init>;  a signed literal, true/false, or
 *                                      vecN(literals) with 1 or N arguments
 *     uniform <ftype> <name>[N];       ftype: float vec2 vec3 vec4; N = 1..64
 * Without an initialiser, and for arrays, the value starts at zero.  The scene
 * reads a uniform as an rvalue of its type and an array element as name[i]
 * with any int i; writing to one does not compile.  Anything else (an
 * expression initialiser, several names in one declaration, sampler2D, an
 * int or bool array, N outside 1..64, a name of the pass such as u_time, a
 * name longer than 63 characters, more than 64 slots of 16 bytes -- one per
 * uniform, one per array element) is RM_ERR_SCENE with a file:line: message.
 * The declarations are matched in the text, before the compiler's
 * preprocessor runs: one inside an inactive #if region still creates the
 * uniform.  A successful load sets every uniform to its declaration's
 * default, also when the same file is loaded again; a failed load keeps the
 * previous scene, its uniforms and their values.  A built-in scene declares
 * none. */
rm_status rm_load_scene(rm_ctx *ctx, const char *file_name);

/* Compile a scene file as rm_load_scene would, without loading it (no GPU
 * needed), as a GL driver compiles a shader: RM_OK, RM_ERR_FILE (missing file
 * or #include) or RM_ERR_SCENE (compile errors, or an edit rm_load_scene
 * refuses).  The compiler's log, or "compiled-in scene O|T" when no compile is
 * needed (NUL-terminated, truncated to log_size), goes to `log` when it is not
 * NULL. */
rm_status rm_compile_scene(const char *file_name, char *log, size_t log_size);

/* sceneSDF(p) of the loaded scene at n points: points = n xyz float triples,
 * dist = n floats, material = n x 16 floats of struct Material
 * (common.frag:20-35, declaration order) or NULL.  Device or host pointers;
 * returns when the results are written.  Uniforms (u_time ...) are the ctx's. */
rm_status rm_scene_eval(rm_ctx *ctx, const float *points, int64_t n, float *dist, float *material);

/* The same in one of the forms a scene distance has.  RM_FORM_EXACT is
 * rm_scene_eval's kernel: the reference's arithmetic, the form of marches and
 * normals.  RM_FORM_PROBE is the form of the ambient-occlusion, soft-shadow and
 * thickness probes and of all of scene T's marches: fused and reciprocal
 * arithmetic, within ~1e-5 of the exact form, not its bits (a plugin's: its
 * sceneSDF over the scene library's probe instance).  RM_FORM_PROBE_NB1 is the
 * probe form with one fold exit test instead of three, which scene T's latency
 * tiles run; the same kernel as RM_FORM_PROBE for every other scene.
 * material (NULL or n x 16): as rm_scene_eval's; a plugin's comes from the
 * instance of the scene library that `form` names.  aux (NULL or n floats):
 * for the compiled-in scene O (and its glass variant) the probe form's slack
 * at the point, which certifies that the scene is its floor plane within that
 * distance (the renderer replaces ray spans and probe sets by the plane where
 * it is large enough); 0 for every other scene.  A form outside the enum:
 * RM_ERR_INVALID_ARGUMENT. */
typedef enum rm_form { RM_FORM_EXACT = 0, RM_FORM_PROBE = 1, RM_FORM_PROBE_NB1 = 2 } rm_form;
rm_status rm_scene_eval_form(rm_ctx *ctx, const float *points, int64_t n, int form, float *dist, float *material,
                             float *aux);

/* Ray queries: castRayD (common.frag:879-901; castRayDI, :903-925, when
 * inside != 0) of the loaded scene along n caller-supplied rays, the march the
 * render kernels run first for every pixel, on its own: picking, camera
 * collision, placing things on a surface, depth and normal buffers.
 * origins: n xyz float triples, or one triple for all rays when shared_origin
 * != 0; directions: n triples, used as given (not normalised: t is in units
 * of |direction|).  The loop is the reference's over rm_params.max_steps with
 * ZNEAR 0.02 and ZFAR 50 (max_steps = 0: t = 0, RM_RAY_EXHAUSTED, 0 steps), in
 * the reference's arithmetic (every scene's exact form, as rm_scene_eval's
 * distances).  Uniforms (u_time, a plugin's own) are the ctx's, read at the
 * call.
 * rm_ray_hits: every pointer may be NULL (not written) except t.  All buffers
 * of a call, inputs included, are device pointers or all are host pointers; a
 * mix is RM_ERR_INVALID_ARGUMENT.  Device: asynchronous on the ctx stream
 * unless `stats` is given; then the call waits and fills kernel_ms, pixels = n,
 * evals = the sum of `steps`, scene.  Host: staged, returns when the results
 * are written.  n < 0, n > 2^30, or a NULL origins / directions / out / out->t
 * with n > 0: RM_ERR_INVALID_ARGUMENT; no scene: RM_ERR_NO_SCENE; n = 0: RM_OK,
 * nothing launched (all checked before any pointer is used). */
enum { RM_RAY_MISS = 0, RM_RAY_HIT = 1, RM_RAY_EXHAUSTED = 2 };
typedef struct rm_ray_hits {
    float *t;         /* n: castRayD's dist: the depth on a hit, -1 past ZFAR, the last sceneSDF value
                         when max_steps ran out                                                   */
    int32_t *status;  /* n: RM_RAY_*                                                             */
    uint32_t *steps;  /* n: sceneSDF calls of the march                                          */
    float *position;  /* n x 3: origin + direction * t where t > 0 (the point render() shades,
                         output_shader.frag:351-355), else 0                                     */
    float *normal;    /* n x 3: getNormalFast(position) (common.frag:697-708) where t > 0, else 0 */
    float *material;  /* n x 16: the Material of the SdResult castRayD returns (sceneSDF at the last
                         point evaluated; the origin without steps), in the order of
                         rm_scene_eval's; scene O's floor colour in the CPU restatement's
                         arithmetic (C library sin and pow), within 6e-6 of a frame's           */
} rm_ray_hits;
rm_status rm_cast_rays(rm_ctx *ctx, const float *origins, int shared_origin, const float *directions, int64_t n,
                       int inside, const rm_ray_hits *out, rm_stats *stats);

/* The rays main() builds for a W x H frame (output_shader.frag:388-405,
 * template.frag:78-88) from u_resolution, u_pos and u_mouse: u_pos into
 * origin3 (3 floats), one direction per pixel into directions (W*H*3 floats,
 * row 0 first, pixel centres, no jitter), in the arithmetic of the loaded
 * scene's render kernel.  Each buffer device (asynchronous on the ctx stream)
 * or host.  rm_cast_rays of these rays with shared_origin = 1 gives the
 * frame's depth / normal / material buffers.  W*H <= 2^30. */
rm_status rm_camera_rays(rm_ctx *ctx, int W, int H, float *origin3, float *directions);

/* Shade caller-supplied rays: the pass's colour, render(ro, rd) of
 * output_shader.frag:348-385 / template.frag:45-76 (light, AO, soft shadow,
 * SSS probes, the mirror bounce, refraction, fog), along n rays the caller
 * built: a fisheye camera, a cube map or panorama, a stereo pair, lens rays,
 * or a frame's own rays (rm_camera_rays) for its colour before the tonemap.
 * The rays run the loaded scene's render kernel code, so rm_camera_rays' rays
 * with the shared origin u_pos, width = W and vignette = 1 give rm_render's /
 * rm_render_rgba8's frame in every bit.
 * directions: n xyz triples, used as given; they must be unit vectors (the
 * render kernels' exact shortcuts rest on that).  origins: with shared_origin
 * != 0 a HOST pointer to one triple, read during the call, which is the
 * launch's u_pos (the context's own is not changed); otherwise n triples of
 * the buffers' kind.  Exactly one of out_rgba (n x 4 floats, alpha 1) and
 * out_rgba8 (n words in the scene's own pack, as rm_render_rgba8's;
 * RM_SHADE_DISPLAY only) is non-NULL; ray i goes to out[i], which for a ray
 * image is out[y * width + x].
 * A ray whose origin or direction has a non-finite component, or whose
 * |direction|^2 differs from 1 by more than 1e-4, is not shaded: its output is
 * (0, 0, 0, 0) or the word 0 (alpha 0 marks it; every shaded ray has alpha 1 /
 * 255), and it enters no march.
 * All buffers are device pointers or all are host pointers (the shared origin
 * aside); a mix is RM_ERR_INVALID_ARGUMENT.  Device: asynchronous on the ctx
 * stream unless `stats` is given; then the call waits and fills kernel_ms,
 * pixels = n and scene (evals = 0).  Host: staged, returns when the results
 * are written.  RM_ERR_INVALID_ARGUMENT: n < 0, n > 2^30; a NULL params,
 * origins or directions with n > 0; both or neither output; RM_SHADE_LINEAR
 * with out_rgba8; width < 0 or n % width != 0; vignette = 1 with width = 0 or
 * with RM_SHADE_LINEAR; an enum value out of range.  No scene:
 * RM_ERR_NO_SCENE; a scene plugin without render kernels
 * (RM_PLUGIN_EVAL_ONLY): RM_ERR_SCENE; n = 0: RM_OK, nothing launched (all
 * checked before any pointer is used).  Uniforms (u_time, a plugin's own),
 * rm_params.max_steps and shadow_max_steps are the ctx's, read at the call.
 * Not here: count_evals and step maps, the adaptive tile order and
 * rm_set_tile_order (the tiles of a ray image run row-major), bands, shards
 * and the wire, accumulation, bench.py. */
enum { RM_SHADE_LINEAR = 0, RM_SHADE_DISPLAY = 1 };
typedef struct rm_shade_params {
    int32_t width;    /* 0: rays are a list (64 consecutive rays per wave);
                         > 0: rays are a width x (n / width) image, row 0 first
                         (n % width == 0), shaded in 8x8 tiles as a frame is   */
    int32_t output;   /* RM_SHADE_LINEAR: render()'s colour (float target only);
                         RM_SHADE_DISPLAY: main()'s tonemap -> contrast
                         (-> vignette) of it, as a frame's pixels               */
    int32_t vignette; /* DISPLAY only. 0: factor 1 (the factor at texcoord
                         (0.5, 0.5), which is exactly 1); 1: the ray image's own
                         (needs width > 0): pixel (x, y)'s texcoord as the
                         loaded scene's render kernel computes it for a
                         width x n/width frame                                  */
} rm_shade_params;
rm_status rm_shade_rays(rm_ctx *ctx, const float *origins, int shared_origin, const float *directions, int64_t n,
                        const rm_shade_params *params, float *out_rgba, uint32_t *out_rgba8, rm_stats *stats);

/* Replace sf::Shader::setUniform (include/SFML/Graphics/Shader.hpp:297,306,315)
 * for the names main.cpp sets: u_resolution (2f), u_pos (3f), u_mouse (2f),
 * u_time (1f), u_sample_part (1f), u_seed1/u_seed2 (2f).  The last three are
 * declared but unused by the reference's scenes (common.frag:8-11): the plain
 * renders ignore them and rm_render_accumulate* reads them.  Other names warn
 * once on stderr and are ignored, as SFML does for uniforms the GLSL compiler
 * removed.  Wrong arity -> RM_ERR_INVALID_ARGUMENT.
 *
 * They also set what the loaded scene declares itself (rm_load_scene), as
 * setUniform sets any uniform of the loaded shader: 1f..4f a float / vec2 /
 * vec3 / vec4, 1i an int or a bool (non-zero: true), fv the elements
 * [0, count) of an array of `components`-float elements from tightly packed
 * host floats (count = 1 also sets a non-array uniform of that many
 * components).  A declared name set with another arity or type -- a float
 * setter on an int, fv with more elements than declared -- or a name longer
 * than 63 characters is RM_ERR_INVALID_ARGUMENT, with the declared type in
 * rm_last_error.  The values are read by the next render or rm_scene_eval
 * call and travel in that launch's kernel arguments: setting one afterwards
 * does not reach work already enqueued. */
rm_status rm_set_uniform1f(rm_ctx *ctx, const char *name, float x);
rm_status rm_set_uniform2f(rm_ctx *ctx, const char *name, float x, float y);
rm_status rm_set_uniform3f(rm_ctx *ctx, const char *name, float x, float y, float z);
rm_status rm_set_uniform4f(rm_ctx *ctx, const char *name, float x, float y, float z, float w);
rm_status rm_set_uniform1i(rm_ctx *ctx, const char *name, int32_t v);
rm_status rm_set_uniformfv(rm_ctx *ctx, const char *name, int components, const float *v, int count);

/* The uniforms the loaded scene declares, in declaration order (none for a
 * built-in scene), and their current values.  rm_get_uniformfv writes a
 * float-typed uniform's components (an array's elements tightly packed) into
 * v[0, capacity) and their number into *written (may be NULL);
 * rm_get_uniform1i reads an int or a bool.  An undeclared name, the other
 * type or too small a capacity is RM_ERR_INVALID_ARGUMENT. */
typedef enum rm_uniform_type { RM_UNIFORM_FLOAT = 0, RM_UNIFORM_INT = 1, RM_UNIFORM_BOOL = 2 } rm_uniform_type;
typedef struct rm_uniform_info {
    char name[64];   /* NUL-terminated                      */
    int32_t type;    /* rm_uniform_type                     */
    int32_t components; /* 1..4 (int, bool: 1)              */
    int32_t count;   /* array length; 0: not an array       */
} rm_uniform_info;
rm_status rm_uniform_count(rm_ctx *ctx, int *n);
rm_status rm_uniform_info_at(rm_ctx *ctx, int index, rm_uniform_info *out);
rm_status rm_get_uniformfv(rm_ctx *ctx, const char *name, float *v, int capacity, int *written);
rm_status rm_get_uniform1i(rm_ctx *ctx, const char *name, int32_t *v);

rm_status rm_set_params(rm_ctx *ctx, const rm_params *params);
rm_status rm_get_params(rm_ctx *ctx, rm_params *params);

/* Stream the ctx launches on (a hipStream_t; NULL = the null stream).
 * Lifetime: a stream must outlive its binding.  Before destroying a stream the
 * context is bound to, bind another one (e.g. rm_set_stream(ctx, NULL)): that
 * records the context's completion marker (one event, only when the context
 * enqueued work there since it was bound) on the old stream while it exists.
 * Streams the context has left may be destroyed at any time.  Destroying the
 * bound stream first is undefined behaviour: the HIP runtime does not validate
 * stream handles, and a later rm_* call (rm_destroy included) that records on
 * the freed stream crashed the process in a test (SIGSEGV inside libamdhip64). */
rm_status rm_set_stream(rm_ctx *ctx, void *hip_stream);
/* rm_set_stream, with the caller's promise that the stream stays alive until
 * rm_destroy (e.g. a stream of PyTorch's pool, which is never destroyed).
 * Leaving a kept stream then records nothing on it; the context marks its work
 * there only when something waits for it (rm_destroy, or reusing a schedule
 * buffer), on the stream itself.  A frame loop that alternates between two
 * kept streams saves one marker per frame (~4 us each on MI355X, DESIGN.md
 * 2.14).  (No counterpart in the reference, which draws on one GL context.) */
rm_status rm_set_stream_kept(rm_ctx *ctx, void *hip_stream);
rm_status rm_synchronize(rm_ctx *ctx);

/* Replaces renderTexture.draw(sprite, &shader) (main.cpp:199,205): run the
 * pass over a W x H target into `out` (W*H*4 float).  Device `out`: the call
 * is asynchronous on the ctx stream unless `stats` is non-NULL (then it
 * waits and fills stats).  Host `out`: rendered through a device staging
 * buffer and copied back before returning. */
rm_status rm_render(rm_ctx *ctx, int W, int H, float *out, rm_stats *stats);

/* rm_render through the instrumented kernel, which also writes the number of
 * sceneSDF calls (ray-steps) each pixel made into evals_map (W*H uint32, row 0
 * first; the same count as rm_stats.evals, per pixel).  Device or host
 * buffers.  The parity tests compare it with the reference GLSL's counts. */
rm_status rm_render_step_map(rm_ctx *ctx, int W, int H, float *out, uint32_t *evals_map, rm_stats *stats);

/* Same pass over one shard of a W x H frame: frame row y belongs to shard
 * (y / band) % nshards; the shard's rows are packed into `out` in increasing
 * y (rm_shard_rows() rows of W float4).  Used by row-sharded multi-GPU frames. */
rm_status rm_render_band(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, float *out,
                         rm_stats *stats);

/* A sub-range of rm_render_band: the shard's packed rows [row_begin,
 * row_begin + row_count) into `out` (row_count rows of W float4).  Lets a
 * caller pipeline a shard in chunks (render chunk k+1 while chunk k is
 * gathered). */
rm_status rm_render_rows(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, int row_begin, int row_count,
                         float *out, rm_stats *stats);

/* Dispatch order of the render workgroups.  A render launch over W x rows
 * pixels is a grid of tiles_x x tiles_y tiles (rm_tile_grid: 8x8 pixels per
 * one-wave workgroup by default); with an order set, workgroup i renders tile
 * order[i] (tile = ty * tiles_x + tx), for launches whose grid has exactly n
 * tiles (others keep the identity order).  Pixels are unchanged; only the
 * time at which each tile starts moves -- e.g. the costliest tiles of the
 * previous frame first, so that the longest per-pixel chains (grazing soft
 * shadows) do not start last.  order: host or device, a permutation of
 * [0, n); n = 0 clears it. */
rm_status rm_set_tile_order(rm_ctx *ctx, const uint32_t *order, int64_t n);
rm_status rm_tile_grid(const rm_params *params, int W, int rows, int *tiles_x, int *tiles_y);

/* Number of frame rows shard `shard` owns. */
rm_status rm_shard_rows(int H, int band, int nshards, int shard, int *nrows);

/* Root side of a row-sharded frame: `gathered` holds nshards consecutive
 * blocks of rows_per_shard packed rows (rows_per_shard >= every shard's row
 * count); writes the W x H frame into `out`.  Device pointers, ctx stream. */
rm_status rm_deinterleave(rm_ctx *ctx, int W, int H, int band, int nshards, int rows_per_shard,
                          const float *gathered, float *out);

/* rm_deinterleave for RGBA8 frames (uint32 per pixel). */
rm_status rm_deinterleave_rgba8(rm_ctx *ctx, int W, int H, int band, int nshards, int rows_per_shard,
                                const uint32_t *gathered, uint32_t *out);

/* The 3 B/px wire of a row-sharded RGBA8 frame (the gather is
 * the only exchange, so its bytes bound multi-GPU scaling).  The pass writes
 * alpha 1 (vec4(col, 1.0), output_shader.frag:419, template.frag:98), so the
 * wire carries RGB only: rm_pack_rgb8 drops the alpha byte of npixels RGBA8
 * words; rm_deinterleave_rgb8 is rm_deinterleave_rgba8 over gathered rows of
 * 3*W bytes, restoring alpha 255.  Device pointers, ctx stream. */
rm_status rm_pack_rgb8(rm_ctx *ctx, int64_t npixels, const uint32_t *in, uint8_t *out);
rm_status rm_deinterleave_rgb8(rm_ctx *ctx, int W, int H, int band, int nshards, int rows_per_shard,
                               const uint8_t *gathered, uint32_t *out);

/* float RGBA -> RGBA8 unorm (round to nearest, clamped), device pointers. */
rm_status rm_pack_rgba8(rm_ctx *ctx, int64_t npixels, const float *in, uint32_t *out);

/* rm_render into a W*H RGBA8 target (device or host): the kernel packs each
 * pixel as rm_pack_rgba8 does (bit-identical to rm_render + rm_pack_rgba8),
 * writing 4 B/px instead of 16. */
rm_status rm_render_rgba8(rm_ctx *ctx, int W, int H, uint32_t *out, rm_stats *stats);

/* Progressive accumulation: the reference's ping-pong plumbing (main.cpp:192-207:
 * u_sample = the previous output texture, u_sample_part = 1/framesStill, fresh
 * u_seed1/u_seed2 per frame; common.frag:8-11), which its shaders declare but
 * never read, as a pass that reads it.  `accum` (W*H float4, or RGBA8 words for
 * the _rgba8 call; device or host) holds u_sample, the previous frame, and
 * receives mix(u_sample, colour, u_sample_part) per pixel, where the colour is
 * the pass's with the fragment moved by the sub-pixel offset fract(u_seed1) -
 * 0.5 (GLSL fract): with main.cpp's uniforms, accum is the running mean of the
 * jittered frames since the camera stopped (progressive supersampling).
 * u_sample_part >= 1 stores the colour (accum needs no clearing); with
 * u_seed1 = (0.5, 0.5) and u_sample_part = 1 the result is rm_render's /
 * rm_render_rgba8's, bit for bit. */
rm_status rm_render_accumulate(rm_ctx *ctx, int W, int H, float *accum, rm_stats *stats);
rm_status rm_render_accumulate_rgba8(rm_ctx *ctx, int W, int H, uint32_t *accum, rm_stats *stats);

/* Adaptive supersampling: one antialiased RGBA8 frame from one call (no
 * counterpart in the reference, whose main() is labelled "NO AA").  The edge
 * pixels of a frame are found on its RGBA8 words and only those are rendered
 * again, `samples` times each, in one launch sequence on the ctx stream with
 * no host round trip.
 *   Edge rule (integer, exact): pixel (x, y) is an edge pixel iff for some
 * channel of R, G, B the largest byte over the pixel's 3x3 neighbourhood minus
 * the smallest is >= threshold (0..255); neighbour coordinates are clamped to
 * the frame, alpha is ignored.  Threshold 0: every pixel.
 *   Samples: K = 2, 4 or 8 offsets from the pixel centre, in pixels (K = 4 a
 * rotated grid; rm_aa_offsets lists them).  Every offset o and o + 0.5 is exact
 * in f32, so u_seed1 = o + 0.5 makes rm_render_accumulate render that sample.
 *   A refined pixel is the scene's RGBA8 pack of the mean of its K samples,
 * each the pass's final colour with the fragment moved by the offset exactly
 * as rm_render_accumulate moves it, summed as a pairwise tree in sample order
 * ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) and multiplied by 1 / K in
 * f32: byte for byte what blending rm_render_accumulate's K jittered float
 * frames on the host gives.  Every other pixel keeps its bytes.
 * rm_aa_offsets: the 2 * samples floats x0, y0, x1, y1, ... (host only).
 * rm_aa_edge_mask: the edge rule on a host frame into mask (W*H bytes, 1 = edge
 * pixel); host pointers, no GPU.
 * rm_refine_rgba8: replaces the edge pixels of `frame`, any RGBA8 frame of the
 * context's current uniforms (normally rm_render_rgba8's), by their K-sample
 * colour, in place; mask (W*H bytes, 1 = refined) may be NULL.
 * rm_render_aa_rgba8: rm_render_rgba8 into `out`, then rm_refine_rgba8 of it.
 * Both: frame and mask are both device pointers (asynchronous on the ctx
 * stream unless `stats` is given; then the call waits and fills it) or both
 * host pointers (staged; returns when the results are written).  W, H <= 0,
 * W*H >= 2^30, a NULL params or frame, samples not 2, 4 or 8, a threshold
 * outside 0..255 or mixed pointers: RM_ERR_INVALID_ARGUMENT; no scene:
 * RM_ERR_NO_SCENE; a scene plugin: RM_ERR_SCENE ("adaptive supersampling:
 * built-in scenes only"), the frame untouched -- all checked before any
 * pointer is used.  The queue of edge pixels is a scratch buffer of the
 * context (a word per pixel) with the life and stream rule of rm_bloom's.
 * Out of scope: float targets, banded / sharded / wire renders
 * and count_evals of the refine (rm_params.count_evals counts the base frame
 * only).  Scene plugins: rm_refine_ex_rgba8 / rm_render_aa_ex_rgba8 below.
 *
 * rm_refine_ex_rgba8 and rm_render_aa_ex_rgba8 take any scene, a scene plugin
 * included.  For a built-in scene they are rm_refine_rgba8 and
 * rm_render_aa_rgba8: the same path and the same bytes.  For a plugin the
 * contract above holds with the plugin's frame in place of the frame: a refined
 * pixel is, byte for byte, the RGBA8 pack of the tree mean of
 * rm_render_accumulate's K float frames at u_seed1 = o + 0.5, u_sample_part = 1;
 * every other pixel keeps its bytes; mask and rm_aa_stats.refined follow the
 * edge rule on the frame's words.  The uniforms are the context's at the call,
 * the pass's and the scene's own (rm_set_uniform*).  (rm_refine_rgba8 and
 * rm_render_aa_rgba8 themselves keep refusing a scene plugin.)
 *   A plugin's refine kernel is a third code object of the scene (the detect
 * kernel is compiled in), compiled on the first _ex call after the scene was
 * loaded and cached by its text, as rm_render_batch_ex's is, so that a scene
 * never antialiased pays nothing; a call that must compile blocks for that
 * long.  rm_aa_prepare compiles and loads it now: RM_OK at once for a built-in
 * scene or when it is loaded already, RM_ERR_NO_SCENE without a scene,
 * RM_ERR_SCENE for a plugin built with RM_PLUGIN_EVAL_ONLY.
 * rm_compile_scene_aa is rm_compile_scene for that code object (no GPU needed;
 * a built-in scene: RM_OK with the compiled-in log; an RM_PLUGIN_EVAL_ONLY
 * scene: RM_ERR_SCENE).
 *   A plugin's refine has the lane = (queue entry, sample) layout only: the
 * environment variable RM_AA_LAYOUT, which selects the other one for the
 * built-in scenes' measurements, does not apply to a plugin.
 *   Errors, in the order above: sizes, NULL, samples and threshold; no scene;
 * then RM_ERR_SCENE for a plugin built with RM_PLUGIN_EVAL_ONLY; mixed
 * pointers; then RM_ERR_SCENE if the refine kernel fails to compile, its log in
 * rm_last_error.  In every case the frame is untouched.
 *   Out of scope: float targets,
 * RM_AA_LAYOUT=pixel for plugins, count_evals of the refine, banded / sharded /
 * wire renders.  (Supersampling of a plugin batch: rm_render_batch_aa_ex_rgba8
 * below.) */
typedef struct rm_aa_params {
    int32_t samples;   /* K: 2, 4 or 8 */
    int32_t threshold; /* 0..255       */
} rm_aa_params;
typedef struct rm_aa_stats {
    int64_t refined;  /* pixels refined (the mask's ones)                                 */
    float base_ms;    /* rm_render_aa_rgba8: the base frame's kernel (rm_stats.kernel_ms) */
    float detect_ms;  /* the detect kernel                                                */
    float refine_ms;  /* the refine kernel                                                */
} rm_aa_stats;
rm_status rm_aa_offsets(int samples, float *xy);
rm_status rm_aa_edge_mask(int W, int H, int threshold, const uint32_t *frame, uint8_t *mask);
rm_status rm_refine_rgba8(rm_ctx *ctx, int W, int H, const rm_aa_params *params, uint32_t *frame, uint8_t *mask,
                          rm_aa_stats *stats);
rm_status rm_render_aa_rgba8(rm_ctx *ctx, int W, int H, const rm_aa_params *params, uint32_t *out, uint8_t *mask,
                             rm_aa_stats *stats);
rm_status rm_refine_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_aa_params *params, uint32_t *frame, uint8_t *mask,
                             rm_aa_stats *stats);
rm_status rm_render_aa_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_aa_params *params, uint32_t *out, uint8_t *mask,
                                rm_aa_stats *stats);
rm_status rm_aa_prepare(rm_ctx *ctx);
rm_status rm_compile_scene_aa(const char *file_name, char *log, size_t log_size);

/* View batches: n poses of the loaded scene rendered by one launch over views x
 * tiles (no counterpart in the reference, whose frame loop draws one pose per
 * frame).  View v's frame is at out + v * W * H elements --
 * float4 for rm_render_batch, RGBA8 words for rm_render_batch_rgba8 -- tightly
 * packed, row 0 first, and every byte of it is what rm_render / rm_render_rgba8
 * writes after u_pos, u_mouse and u_time are set to the view's values; with a
 * non-zero `offset`, what rm_render_accumulate[_rgba8] stores for
 * u_sample_part = 1 and u_seed1 = offset + 0.5.  u_resolution (set or
 * defaulted), rm_params.max_steps and shadow_max_steps are the context's, read
 * at the call; the call neither reads nor changes the context's own u_pos,
 * u_mouse, u_time or u_seed1.
 *   `views` is a host pointer, read during the call (the caller may reuse it on
 * return).  `out` is a device pointer (asynchronous on the ctx stream unless
 * `stats` is given) or a host pointer (staged through the context's staging
 * buffer; the call returns when the frames are written).  With `stats` the call
 * waits and fills it: kernel_ms the one launch's time, pixels = n * W * H, scene
 * the loaded scene, dispatch = RM_DISPATCH_ROW_MAJOR, everything else 0.  The
 * counts behind rm_certified_steps / rm_reflection_cleared_steps are reset to
 * 0, as by every render launch.
 *   The batch always runs the timed kernels in one-wave 8x8 tiles, row-major
 * per view.  These do not apply to it: rm_params.kernel, schedule and
 * count_evals; rm_set_tile_order; step maps, accumulation into the target,
 * bands, shards and the wire.
 *   Size rule, checked before any pointer is used (rm_batch_bytes applies the
 * same rule): W, H > 0; 0 <= n <= 65535; ceil(H / 8) <= 65535; n * W * H <= 2^31.
 * rm_batch_bytes (host only, no GPU): the bytes of one view's frame and of the
 * whole target (rgba8 != 0: RGBA8 words, else float4); either pointer may be
 * NULL.
 *   Errors: the size rule broken, `views` or `out` NULL with n > 0, or an
 * offset component outside [-0.5, 0.5) or not finite: RM_ERR_INVALID_ARGUMENT;
 * no scene: RM_ERR_NO_SCENE; a scene plugin: RM_ERR_SCENE ("view batches:
 * built-in scenes only"), the target untouched; n = 0: RM_OK, nothing launched.
 * The device copy of the per-view constants is a scratch buffer of the context
 * (80 bytes per view for scenes S0 and T, 584 for O and OG; a scene plugin
 * through rm_render_batch_ex below: 592 + 16 * slots, the slots its uniforms
 * take, one each and one per array element) with the life and
 * stream rule of rm_bloom's; several batches may be in flight on a stream at
 * once.
 *   Out of scope: count_evals and
 * step maps per view; an adaptive or costliest-first order across views; views
 * of different sizes in one batch; device-resident view arrays; multi-GPU
 * batches.  (Adaptive supersampling of batched frames: rm_render_batch_aa_rgba8
 * below.) */
typedef struct rm_view {
    float pos[3];    /* u_pos   */
    float mouse[2];  /* u_mouse */
    float time;      /* u_time  */
    float offset[2]; /* sub-pixel offset of the fragment in pixels, each in [-0.5, 0.5); (0, 0): pixel centres.
                        The fragment moves exactly as rm_render_accumulate moves it for u_seed1 = offset + 0.5 */
} rm_view;
rm_status rm_batch_bytes(int W, int H, int n, int rgba8, int64_t *frame_bytes, int64_t *total_bytes);
rm_status rm_render_batch(rm_ctx *ctx, int W, int H, const rm_view *views, int n, float *out, rm_stats *stats);
rm_status rm_render_batch_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n, uint32_t *out,
                                rm_stats *stats);

/* View batches of any scene, scene plugins included, with the scene's own
 * uniforms set per view.  View v's frame is, byte for byte,
 * what rm_render / rm_render_rgba8 writes after u_pos, u_mouse and u_time are
 * set to the view's values and each uniform of the list is set to view v's
 * values by the matching rm_set_uniform* call (rm_set_uniform{1..4}f,
 * rm_set_uniformfv for the leading `count` elements of an array,
 * rm_set_uniform1i for an int or a bool); every unlisted uniform has the
 * context's current value, read at the call.  A non-zero `offset` means what it
 * means for rm_render_batch.  The call neither reads the context's pose nor
 * changes any of its uniform values: rm_get_uniformfv and rm_get_uniform1i answer
 * after it what they answered before.  `uniforms` and every `values` are host
 * pointers read during the call.  Target, staging, stats, stream, size rule and
 * the rule for batches in flight are rm_render_batch's.
 *   A built-in scene declares no uniforms: with n_uniforms == 0 the call is
 * rm_render_batch[_rgba8]; with n_uniforms > 0 it returns
 * RM_ERR_INVALID_ARGUMENT.  (rm_render_batch[_rgba8] and
 * rm_render_batch_aa_rgba8 themselves keep refusing a scene plugin.)
 *   A plugin's batch kernel is a second code object of the scene, compiled on
 * the first batch call after the scene was loaded (cached by its text, as
 * rm_load_scene caches), so that a scene never batched pays nothing; a call
 * that must compile blocks for that long.  rm_batch_prepare compiles and loads
 * it now: RM_OK at once for a built-in scene or when it is loaded already,
 * RM_ERR_NO_SCENE without a scene, RM_ERR_SCENE for a plugin built with
 * RM_PLUGIN_EVAL_ONLY.  rm_compile_scene_batch is rm_compile_scene for that
 * code object (no GPU needed; a built-in scene: RM_OK with the compiled-in
 * log; an RM_PLUGIN_EVAL_ONLY scene: RM_ERR_SCENE).
 *   Errors, checked before any pointer is used, in this order, the target
 * untouched: rm_render_batch's size rule and NULL `views` or `out`;
 * n_uniforms < 0 or a NULL `uniforms` with n_uniforms > 0
 * (RM_ERR_INVALID_ARGUMENT); no scene (RM_ERR_NO_SCENE); a plugin built with
 * RM_PLUGIN_EVAL_ONLY (RM_ERR_SCENE); a built-in scene with n_uniforms > 0; an
 * offset outside [-0.5, 0.5); then, per entry of the list, a NULL name, NULL
 * values with n > 0, a uniform of the pass (u_time, ...), a name the scene does
 * not declare, a name listed twice, components other than the declared type's
 * (rm_last_error names the declared type), count < 1, count > 1 for a
 * non-array, count above the declared length (all RM_ERR_INVALID_ARGUMENT).
 * n = 0: RM_OK, nothing launched.
 *   Out of scope: per-view max_steps or
 * resolution; device-resident view or uniform arrays; count_evals and step maps
 * per view; a dispatch order across views; multi-GPU batches.  (Supersampling
 * of a plugin batch: rm_render_batch_aa_ex_rgba8 below.) */
typedef struct rm_view_uniform {
    const char *name;    /* a uniform the loaded scene declares                        */
    int32_t components;  /* 1..4, the declared type's (int, bool: 1)                   */
    int32_t count;       /* elements given per view: 1 for a non-array; 1..N, the leading
                            elements, for an array of N                                */
    const void *values;  /* host; n * count * components 4-byte values, view-major:
                            floats for a float-typed uniform, int32 for int and bool
                            (non-zero: true)                                           */
} rm_view_uniform;
rm_status rm_render_batch_ex(rm_ctx *ctx, int W, int H, const rm_view *views, int n, const rm_view_uniform *uniforms,
                             int n_uniforms, float *out, rm_stats *stats);
rm_status rm_render_batch_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n,
                                   const rm_view_uniform *uniforms, int n_uniforms, uint32_t *out, rm_stats *stats);
rm_status rm_batch_prepare(rm_ctx *ctx);
rm_status rm_compile_scene_batch(const char *file_name, char *log, size_t log_size);

/* Adaptive supersampling of a view batch: n antialiased RGBA8 frames from one
 * call -- the batch launch, then detect, plan and refine launches over all the
 * views, with no host round trip.  View v's frame is at
 * out + v * W * H words, and every byte of it is what rm_render_aa_rgba8 writes
 * after u_pos, u_mouse and u_time are set to the view's values, with the same
 * rm_aa_params (edge rule, samples and sum: see rm_render_aa_rgba8 above).
 *   mask: NULL or n * W * H bytes; view v's part is the single call's mask.
 * refined: NULL or n words; word v is the single call's rm_aa_stats.refined for
 * view v.
 * rm_refine_batch_rgba8: the same relation to rm_refine_rgba8 -- it replaces the
 * edge pixels of the n given frames in place and reads nothing else from them.
 * rm_render_batch_aa_rgba8: rm_render_batch_rgba8 into `out`, then
 * rm_refine_batch_rgba8 of it.
 *   As for a view batch: `views` is a host pointer read during the call;
 * u_resolution, rm_params.max_steps and shadow_max_steps are the context's; the
 * context's own u_pos, u_mouse, u_time and u_seed1 are neither read nor changed.
 * frames / out, mask and refined are all device pointers (asynchronous on the
 * ctx stream unless `stats` is given) or all host pointers (staged; the call
 * returns when the results are written).  With `stats` the call waits and fills
 * it: refined the sum over the views, base_ms the batch launch, detect_ms the
 * detect and plan launches, refine_ms the refine launch.
 *   Size rule, checked by all three calls before any pointer is used: the view
 * batch's rule (W, H > 0; 0 <= n <= 65535; ceil(H / 8) <= 65535; n * W * H <= 2^31)
 * and W * H < 2^30.
 *   Errors, in this order: the size rule broken, a NULL params, a NULL views or
 * frames with n > 0, samples not 2, 4 or 8, a threshold outside 0..255, or a
 * view whose offset is not exactly (0, 0) (the samples' offsets take the place
 * of the fragment offset, and a sum of the two is not exact in f32):
 * RM_ERR_INVALID_ARGUMENT; no scene: RM_ERR_NO_SCENE; a scene plugin:
 * RM_ERR_SCENE ("batch supersampling: built-in scenes only"), the target
 * untouched; n = 0: RM_OK, nothing launched, stats zeroed; mixed host and
 * device pointers: RM_ERR_INVALID_ARGUMENT.
 *   The counters, the plan and the queue are one scratch buffer of the context
 * with the life and stream rule of rm_bloom's.  rm_batch_aa_scratch_bytes (host
 * only, no GPU) returns its size under the same size rule:
 *     4 * (32 * n + roundup32(n + 2) + n * W * H) bytes
 * -- a 128-byte line per view for its counter, the plan's n + 2 words (the
 * exclusive prefix of the views' group counts, the groups' total, the counts'
 * total) rounded up to a line, and a queue word per pixel; `bytes` may be NULL.
 * The view records are the view batch's own scratch.
 *   Out of scope: float targets, a threshold or sample count per
 * view, views of different sizes, multi-GPU batches and count_evals of the
 * refine.  (Scene plugins: the _ex calls below.)
 *
 * rm_refine_batch_ex_rgba8 and rm_render_batch_aa_ex_rgba8 take any scene, a
 * scene plugin included, with the scene's own uniforms set per view (DESIGN.md
 * 2.32).  View v's frame, mask part and refined[v] are, byte for byte, what
 * rm_render_aa_ex_rgba8 gives, with the same rm_aa_params, after u_pos, u_mouse
 * and u_time are set to the view's values and each uniform of the list is set to
 * view v's values by the matching rm_set_uniform* call (the list is
 * rm_render_batch_ex's); every unlisted uniform has the context's value at the
 * call.  rm_refine_batch_ex_rgba8 relates to rm_refine_ex_rgba8 the same way.
 * The context's pose, seed and uniform values are neither read nor changed: the
 * getters answer after the call what they answered before.  Pointer kinds, the
 * staging of host buffers, the stats fields, asynchrony, the size rule and
 * rm_batch_aa_scratch_bytes are rm_render_batch_aa_rgba8's; batches in flight
 * follow rm_render_batch_ex's rule.
 *   For a built-in scene with n_uniforms == 0 the calls are
 * rm_refine_batch_rgba8 / rm_render_batch_aa_rgba8, the same path and the same
 * bytes; with n_uniforms > 0 they return RM_ERR_INVALID_ARGUMENT.
 * (rm_refine_batch_rgba8 and rm_render_batch_aa_rgba8 themselves keep refusing a
 * scene plugin.)
 *   A plugin's batch refine kernel is a fourth code object of the scene (detect
 * and plan are compiled in), compiled on the first of these calls after the
 * scene was loaded and cached by its text, as the batch and AA forms are; a call
 * that must compile blocks for that long.  rm_batch_aa_prepare compiles and
 * loads what rm_render_batch_aa_ex_rgba8 needs, the batch form and this one, now:
 * RM_OK at once for a built-in scene or when both are loaded, RM_ERR_NO_SCENE
 * without a scene, RM_ERR_SCENE for a plugin built with RM_PLUGIN_EVAL_ONLY.
 * rm_compile_scene_batch_aa is rm_compile_scene for the new code object (no GPU
 * needed; a built-in scene: RM_OK with the compiled-in log; an
 * RM_PLUGIN_EVAL_ONLY scene: RM_ERR_SCENE).
 *   The refine runs G one-wave workgroups per view (DESIGN.md 2.32 has the rule
 * for G); the environment variable RM_PLUGIN_BATCH_AA_COLUMNS=<G>, read at every
 * call, overrides it for measurements.  Any G gives the same bytes.
 *   Errors, all checked before any pointer is used or anything is written, in
 * this order:
 *    1. the size rule above broken (RM_ERR_INVALID_ARGUMENT);
 *    2. a NULL params, or a NULL views or frames with n > 0;
 *    3. samples not 2, 4 or 8, or a threshold outside 0..255;
 *    4. a view whose offset is not exactly (0, 0);
 *    5. n_uniforms < 0, or a NULL `uniforms` with n_uniforms > 0;
 *    6. no scene (RM_ERR_NO_SCENE);
 *    7. a plugin built with RM_PLUGIN_EVAL_ONLY (RM_ERR_SCENE);
 *    8. a built-in scene with n_uniforms > 0 (RM_ERR_INVALID_ARGUMENT);
 *    9. per entry of the list, rm_render_batch_ex's faults, the message in
 *       rm_last_error (RM_ERR_INVALID_ARGUMENT);
 *   10. n = 0: RM_OK, stats zeroed, nothing launched;
 *   11. mixed host and device pointers (RM_ERR_INVALID_ARGUMENT);
 *   12. RM_ERR_SCENE, with the log in rm_last_error, if a form of the plugin
 *       fails to compile.
 *   Out of scope: float targets, a threshold or sample count per view, views of
 * different sizes, device-resident view or uniform arrays, count_evals of the
 * refine, RM_AA_LAYOUT=pixel, an order of the base frames' tiles across views
 * and multi-GPU batches. */
rm_status rm_batch_aa_scratch_bytes(int W, int H, int n, int64_t *bytes);
rm_status rm_refine_batch_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n, const rm_aa_params *params,
                                uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats);
rm_status rm_render_batch_aa_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n, const rm_aa_params *params,
                                   uint32_t *out, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats);
rm_status rm_refine_batch_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n,
                                   const rm_view_uniform *uniforms, int n_uniforms, const rm_aa_params *params,
                                   uint32_t *frames, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats);
rm_status rm_render_batch_aa_ex_rgba8(rm_ctx *ctx, int W, int H, const rm_view *views, int n,
                                      const rm_view_uniform *uniforms, int n_uniforms, const rm_aa_params *params,
                                      uint32_t *out, uint8_t *mask, uint32_t *refined, rm_aa_stats *stats);
rm_status rm_batch_aa_prepare(rm_ctx *ctx);
rm_status rm_compile_scene_batch_aa(const char *file_name, char *log, size_t log_size);

/* rm_render_band / rm_render_rows into RGBA8 rows (W uint32 per row). */
rm_status rm_render_band_rgba8(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, uint32_t *out,
                               rm_stats *stats);
rm_status rm_render_rows_rgba8(rm_ctx *ctx, int W, int H, int band, int nshards, int shard, int row_begin,
                               int row_count, uint32_t *out, rm_stats *stats);

/* The reference's FXAA post pass (post.frag:16-61, :135-144) over an RGBA8
 * frame: in/out W*H RGBA8 words (device, distinct), sampled as the reference's
 * RenderTexture is (nearest, clamp to edge), u_resolution = (W, H).  Like
 * post.frag, the output is the input flipped vertically.  W*H < 2^30. */
rm_status rm_fxaa(rm_ctx *ctx, int W, int H, const uint32_t *in, uint32_t *out);

/* The reference's bloom post pass (shaders/post/bloom.frag:14-43, applied by
 * PostBloom::apply, source/post_bloom.cpp:9-13, main.cpp:212-214) over an
 * RGBA8 frame: the mip levels bloom.frag's textureLod reads are built on the
 * device (glGenerateMipmap semantics, kept in a context scratch buffer), then
 * the 25-tap trilinear bloom is added to the frame; RGBA8 out, alpha 1.  As in
 * the shader, the output is flipped vertically (uv = (tc.x, 1 - tc.y)).
 * in/out: W x H device buffers, row 0 first, in != out.  Asynchronous on the
 * context's stream.  The scratch buffer also keeps the size's run tables
 *  between calls; they are rebuilt when W x H or the context's
 * stream changes.  The buffer is one per context: a bloom on another stream
 * than the last one first waits (on the device) for that one, marked when the
 * context left its stream. */
rm_status rm_bloom(rm_ctx *ctx, int W, int H, const uint32_t *in, uint32_t *out);

/* The reference's two post passes of a frame, chained as main.cpp:209-214 runs
 * them: FXAA of `in` into `mid` (post_shader into postTexture), then bloom of
 * `mid` into `out` (postTexture.generateMipmap, post_bloom.apply): the same
 * bits as rm_fxaa(in -> mid) followed by rm_bloom(mid -> out), in one call.
 * Device buffers of W x H RGBA8 words, pairwise distinct, W*H < 2^30;
 * asynchronous on the context's stream; bloom's scratch as rm_bloom's. */
rm_status rm_post_chain(rm_ctx *ctx, int W, int H, const uint32_t *in, uint32_t *mid, uint32_t *out);

/* post.frag's main() (:135-144) with the choices a user of the reference makes
 * by editing its one statement (the menu of post.frag:63-131):
 *   uv    = (tc.x, 1 - tc.y)                    the output is the input flipped vertically
 *   color = fxaa(tex, uv, res)                                         RM_POST_SAMPLE_FXAA
 *         | texture(tex, uv)                                           RM_POST_SAMPLE_TEXEL
 *         | vec4(chromaticAberration(tex, uv), texture(tex, uv).a)     RM_POST_SAMPLE_CHROMATIC
 *   color.rgb = tonemap_X(color.rgb)            X: rm_tonemap (NONE: no statement)
 *   gl_FragColor = color                        one RGBA8 store
 * Sampler and contract as rm_fxaa: nearest, clamp to edge, u_resolution = (W,
 * H); in/out W*H RGBA8 words (device, distinct), W*H < 2^30; asynchronous on
 * the context's stream.  (FXAA, NONE) is rm_fxaa, byte for byte.  A sample or
 * tonemap value outside its enum -> RM_ERR_INVALID_ARGUMENT. */
typedef enum rm_post_sample {
    RM_POST_SAMPLE_FXAA = 0,
    RM_POST_SAMPLE_TEXEL = 1,
    RM_POST_SAMPLE_CHROMATIC = 2
} rm_post_sample;

typedef enum rm_tonemap {
    RM_TONEMAP_NONE = 0,
    RM_TONEMAP_ACES = 1,           /* tonemapACES, post.frag:67-75 */
    RM_TONEMAP_REINHARD = 2,       /* tonemapReinhard, :77-80 */
    RM_TONEMAP_REINHARD_JODIE = 3, /* tonemapReinhardJodie, :82-88 */
    RM_TONEMAP_UNCHARTED2 = 4      /* tonemapUncharted2Filmic, :90-109 */
} rm_tonemap;

rm_status rm_post_frag(rm_ctx *ctx, int W, int H, int sample, int tonemap, const uint32_t *in, uint32_t *out);

/* rm_post_chain with that pass in FXAA's place: rm_post_frag(in -> mid), then
 * rm_bloom(mid -> out), in one call; (FXAA, NONE) gives rm_post_chain's bytes. */
rm_status rm_post_chain_ex(rm_ctx *ctx, int W, int H, int sample, int tonemap, const uint32_t *in, uint32_t *mid,
                           uint32_t *out);

/* The post passes over a batch: n equally sized RGBA8 frames packed as a view
 * batch packs them (view v's frame at p + v * W * H words), every view
 * processed by the same few launches -- their number does not grow with n,
 * apart from the groups below.  Every byte of view v is what
 * the single-frame call writes for that frame:
 *   rm_post_frag_batch   view v = rm_post_frag(in_v -> out_v) with the same
 *                        sample and tonemap; (FXAA, NONE) = rm_fxaa
 *   rm_bloom_batch       view v = rm_bloom(in_v -> out_v)
 *   rm_post_chain_batch  rm_post_frag_batch(in -> mid), then
 *                        rm_bloom_batch(mid -> out): view v = rm_post_chain_ex,
 *                        and with (FXAA, NONE) rm_post_chain
 * u_resolution = (W, H) for every view, and every view is flipped vertically
 * by itself, as the single call flips its frame.  All buffers are device
 * pointers; the calls are asynchronous on the context's stream.  No scene
 * needs to be loaded.
 *   Size rule, checked before any pointer is used: W, H > 0; 0 <= n <= 65535;
 * n * W * H <= 2^31; W * H < 2^30.  Then: a sample or tonemap value outside its
 * enum; n = 0: RM_OK, nothing launched; a NULL buffer; buffers whose ranges
 * [p, p + n * W * H) are not pairwise disjoint; a host pointer -- each
 * RM_ERR_INVALID_ARGUMENT with nothing written.
 *   Scratch: bloom's per-frame scratch is large for small frames (at 64 x 64
 * about 390 KB per view against a 16 KB frame), so the views go through the
 * context's bloom buffer (rm_bloom's, with its life and stream rule) in groups.
 * With P = bloom's single-frame layout for W x H,
 *     shared_bytes   = the bytes of P: what rm_bloom itself keeps for W x H.
 *                      A batch uses its run tables, which depend on W x H only,
 *                      are built once for all views and are kept for the next
 *                      batch or single bloom of this size on this stream;
 *     per_view_bytes = 4 * (roundup4(texels of mip levels 1..d2)
 *                           + 12 * (runs_x(d1) * runs_y(d1) + runs_x(d2) * runs_y(d2)))
 *                      -- the view's mip levels and the run-pair polynomials of
 *                      the two levels bloom.frag reads, runs(axis) = min(pixels
 *                      along it, 5 * the level's size along it + 1); 0 for
 *                      H <= 20, where bloom reads the frame alone;
 *     group_views    = max(1, min(n, (limit - shared_bytes) / per_view_bytes))
 *                      (n where per_view_bytes is 0);
 *     groups         = ceil(n / group_views);
 *     scratch_bytes  = shared_bytes + group_views * per_view_bytes: what the
 *                      call makes sure the buffer holds (0 for n = 0);
 *     launches       = groups * (1 + the launches of one bloom: a mip launch per
 *                      level or one pyramid launch, then two) + 1 for the run
 *                      tables: the kernel launches of one rm_post_chain_batch on
 *                      a context that has not bloomed this size (0 for n = 0).
 * rm_post_batch_plan (host only, no GPU) returns these under the size rule;
 * limit_bytes 0 means the default, RM_POST_BATCH_SCRATCH_DEFAULT; negative:
 * RM_ERR_INVALID_ARGUMENT; `out` may be NULL.
 * rm_set_post_batch_scratch_limit sets the context's limit (0 restores the
 * default); a view that alone exceeds it is still processed, in a group of 1.
 *   Out of scope: host pointers, views of different sizes, a sample or tonemap
 * per view, multi-GPU batches, float targets, a fused render + post launch. */
#define RM_POST_BATCH_SCRATCH_DEFAULT ((int64_t)512 << 20) /* 512 MiB */
struct rm_post_batch_plan {
    int64_t per_view_bytes;
    int64_t shared_bytes;
    int32_t group_views;
    int32_t groups;
    int64_t scratch_bytes;
    int32_t launches;
    int32_t reserved; /* 0 */
};
rm_status rm_post_batch_plan(int W, int H, int n, int64_t limit_bytes, struct rm_post_batch_plan *out);
rm_status rm_set_post_batch_scratch_limit(rm_ctx *ctx, int64_t bytes);
rm_status rm_post_frag_batch(rm_ctx *ctx, int W, int H, int n, int sample, int tonemap, const uint32_t *in,
                             uint32_t *out);
rm_status rm_bloom_batch(rm_ctx *ctx, int W, int H, int n, const uint32_t *in, uint32_t *out);
rm_status rm_post_chain_batch(rm_ctx *ctx, int W, int H, int n, int sample, int tonemap, const uint32_t *in,
                              uint32_t *mid, uint32_t *out);

/* Scenes S0/T keep the device's reciprocals of the frame size and of
 * u_resolution.y per resolution (W, H, u_resolution.y) in a small cache of the
 * context: the first render of a new resolution runs a one-thread kernel on the
 * context's stream and waits for it (so it must not fall inside a stream
 * capture); later frames of that resolution, whatever their pose and time, do
 * not.  entries: resolutions held now; capacity: the most it holds (the least
 * recently used one is replaced).  Either pointer may be NULL. */
rm_status rm_resolution_cache_info(rm_ctx *ctx, int *entries, int *capacity);

/* The certified ray-steps of this context's last render launch, if it filled an rm_stats with count_evals
 * on (every render launch resets the count, so a launch without an rm_stats or without counting leaves 0,
 * never an earlier launch's value): of its `evals`, and none of them in its `skipped`, the soft-shadow ray-steps of lit points whose
 * shadow ray passes scene T's certificate (csrc/rm_shadow_clear.h).  The march is proved
 * to return 1 and the uninstrumented kernels do not take it, so they execute evals - skipped - *steps.
 * 0 for every other scene and for uncounted renders.  (A call of its own, not an rm_stats member:
 * rm_stats keeps its layout and RM_ABI_VERSION its value.) */
rm_status rm_certified_steps(rm_ctx *ctx, uint64_t *steps);

/* The reflection ray-steps scene T's reflection certificate proves away, of this context's last render launch
 * (counted and reset as rm_certified_steps' count is): of its `evals`, and none of them in its `skipped` or in
 * rm_certified_steps' count, the steps begun at a depth < 3 of the reflection marches of lanes that hit the
 * sponge and whose reflection ray passes the certificate (csrc/rm_refl_clear.h), outside far-sky
 * waves.  With max_steps >= 28 the march is proved to meet nothing and to pass depth 3, where its factor is 1,
 * and the uninstrumented kernels do not take it; under a smaller step cap they march and the count is 0.  (A
 * sky lane of a mixed wave may pass the test as well; its one or two steps are not in the count.)  0 for every
 * other scene and for uncounted renders.  A call of its own, as rm_certified_steps: rm_stats keeps its layout. */
rm_status rm_reflection_cleared_steps(rm_ctx *ctx, uint64_t *steps);

/* The ray-steps scene T's near-sky ladder proves away, of this context's last render launch (counted and reset as
 * rm_certified_steps' count is): of its `evals`, and none of them in its `skipped` or in the two counts above, the
 * primary-march steps, and the reflection-march steps begun at a depth < 3, of the waves whose 64 rays all miss
 * the sponge's cube inflated by the margin m that max_steps admits (csrc/rm_far_sky.h, DESIGN.md 2.27: m = 0.25
 * from 39 steps, 0.1 from 63, 0.05 from 98, 0.02 from 205) and end 3.1 beyond it, but do not all miss the cube
 * inflated by 0.25 with max_steps >= 208 -- those waves' steps are in `skipped`, as before.  Each such march is
 * proved to return ZFAR, and the reflection factor 1, and the uninstrumented kernels take neither.  0 under a
 * step cap below 39, for every other scene and for uncounted renders.  The uninstrumented kernels execute
 * evals - skipped - certified - reflection_cleared - near_sky steps.  A call of its own, as rm_certified_steps:
 * rm_stats keeps its layout and RM_ABI_VERSION its value. */
rm_status rm_near_sky_steps(rm_ctx *ctx, uint64_t *steps);

/* The render kernels' code objects by content (16 hex digits of a SHA-256 of
 * the translation units that hold them): rocprofv3 counters of a render launch
 * (profiles/pmc_counters.json) name the build they counted, and bench.py
 * prices a launch with them only when this hash matches. */
const char *rm_render_code_hash(void);

/* ---- Weighted row parts: frame row y belongs to a part iff (y mod cycle) - offset
 * lies in [0, run).  Round-robin bands are the special case run = band,
 * cycle = band * nshards, offset = band * shard; parts with different runs give
 * ranks different shares of every cycle (bench.py's balanced multi-GPU split:
 * the root, which receives the others' rows, renders a longer run).
 * rm_cycle_rows: the number of frame rows of a part.  rm_render_cycle_rows[_rgba8]:
 * the part's packed rows [row_begin, row_begin + row_count) in increasing y,
 * as rm_render_rows[_rgba8].  rm_deinterleave_cycle_rgb8: the root side, the
 * W x H RGBA8 frame (alpha 255) from nparts parts that tile [0, cycle) in
 * order (offsets[i + 1] = offsets[i] + runs[i]), part i's packed 3 B/px rows
 * starting at byte part_bytes[i] of `gathered` (device pointers, ctx stream;
 * nparts <= 64). */
rm_status rm_cycle_rows(int H, int cycle, int offset, int run, int *nrows);
rm_status rm_render_cycle_rows(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int row_begin,
                               int row_count, float *out, rm_stats *stats);
rm_status rm_render_cycle_rows_rgba8(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int row_begin,
                                     int row_count, uint32_t *out, rm_stats *stats);
rm_status rm_deinterleave_cycle_rgb8(rm_ctx *ctx, int W, int H, int cycle, int nparts, const int *offsets,
                                     const int *runs, const int64_t *part_bytes, const uint8_t *gathered,
                                     uint32_t *out);

/* ---- Compressed wire of RGBA8 row parts ----
 * A lossless code per 8x8-pixel tile of a part's packed rows: the first
 * pixel, then per channel the differences to the left neighbour (to the one
 * above in the tile's first column) as bit planes of their zig-zagged bytes;
 * alpha is not sent (the root stores 255).  rm_wire_encode: nrows packed
 * RGBA8 rows -> msg (at most rm_wire_capacity bytes), using a caller-owned
 * device workspace of rm_wire_workspace_bytes; the message size (also its
 * first 8 bytes) is written to the device int64 *size_out when non-null
 * (asynchronous, ctx stream).  rm_wire_decode: a message of nrows rows of the
 * cyclic part (cycle, offset, run) into those rows of the W x H RGBA8 frame.
 * rm_scatter_part_rgba8: a part's packed RGBA8 rows into their frame rows
 * (the root's own part).
 * One size rule for a part of nrows rows of W pixels, T = ceil(W / 8) *
 * ceil(nrows / 8) tiles: 0 < W <= 2^18, 0 <= nrows <= 65535 and 25 T < 2^27
 * (a tile is at most 25 words, and a table entry holds a tile's word offset in
 * 27 bits; about 5.37 M tiles).  A part outside it is refused by every call of
 * this section and by rm_render_cycle_rows_wire (on row_count), before any
 * pointer is used: capacity and workspace return -1, the others
 * RM_ERR_INVALID_ARGUMENT (rm_wire_decode_parts for any of its parts). */
int64_t rm_wire_capacity(int W, int nrows);
int64_t rm_wire_workspace_bytes(int W, int nrows);
rm_status rm_wire_encode(rm_ctx *ctx, int W, int nrows, const uint32_t *rows, uint8_t *msg, void *workspace,
                         int64_t *size_out);
rm_status rm_wire_decode(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int nrows, const uint8_t *msg,
                         uint32_t *frame);
rm_status rm_scatter_part_rgba8(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int nrows,
                                const uint32_t *rows, uint32_t *frame);
/* rm_wire_decode for nparts (<= 64) messages in one launch: part i holds
 * nrows[i] rows of (cycle, offsets[i], runs[i]); msgs is a host array of
 * device pointers. */
rm_status rm_wire_decode_parts(rm_ctx *ctx, int W, int H, int cycle, int nparts, const int *offsets, const int *runs,
                               const int *nrows, const uint8_t *const *msgs, uint32_t *frame);

/* rm_render_cycle_rows_rgba8 and rm_wire_encode in one: the render kernel
 * encodes each of its 8x8-pixel tiles for the wire from registers (its own
 * epilogue: the rows are never written), then the tiles' words are scanned
 * and compacted into msg; msg, workspace and *size_out as rm_wire_encode's for
 * row_count rows, and the message is byte for byte rm_wire_encode's of the
 * rows rm_render_cycle_rows_rgba8 renders.  Built-in scenes (a plugin part:
 * the two calls).  The non-root ranks of a sharded frame call this instead of
 * rendering rows they only send. */
rm_status rm_render_cycle_rows_wire(rm_ctx *ctx, int W, int H, int cycle, int offset, int run, int row_begin,
                                    int row_count, uint8_t *msg, void *workspace, int64_t *size_out, rm_stats *stats);

/* ---- Multi-GPU: row-sharded frames over RCCL ----
 * The reference renders one frame on one GPU (main.cpp:196-207); here a frame's
 * rows are dealt to nranks GPUs in bands of `band` rows, round robin (rank r
 * owns frame row y iff (y / band) % nranks == r).  Each rank renders its rows
 * (rm_render_band_rgba8), packs them to the 3 B/px RGB8 wire (rm_pack_rgb8),
 * one ncclGather moves every wire to rank 0 over xGMI, and rank 0 writes the
 * W x H RGBA8 frame (rm_deinterleave_rgb8).  RCCL (librccl.so.1) is opened at
 * run time.  A communicator binds a context (its device, stream, scene and
 * uniforms: set the same uniforms on every rank's context).
 *
 * One process per GPU: rank 0 calls rm_comm_get_id and sends the id to the
 * others out of band (ncclGetUniqueId semantics), then every rank calls
 * rm_comm_init_rank (collective) and rm_render_sharded per frame (collective;
 * `frame` is a W*H RGBA8 device buffer on rank 0, ignored elsewhere).
 * One process driving n GPUs: rm_comm_init_all over n contexts on distinct
 * devices (ncclCommInitAll; comms[i] is rank i), then rm_render_sharded_all.
 * Calls are asynchronous on the contexts' streams unless `stats` is given
 * (then they wait; stats[i].kernel_ms is rank i's render time, gather_ms its
 * pack + gather and, on rank 0, deinterleave_ms the de-interleave kernel). */
typedef struct rm_comm rm_comm;
typedef struct rm_comm_id {
    char internal[128]; /* an ncclUniqueId */
} rm_comm_id;
/* The layout rm_render_sharded uses (host-only, no GPU): rank `rank` owns
 * rows_mine frame rows; every rank sends rows_per_shard rows of 3*W bytes
 * (wire_bytes; rows past rows_mine are padding); rank 0 receives nranks wires
 * back to back (gathered_bytes), rank r's at offset r * wire_bytes. */
typedef struct rm_shard_layout {
    int32_t rows_mine, rows_per_shard;
    int64_t wire_bytes, gathered_bytes;
} rm_shard_layout;
rm_status rm_sharded_layout(int W, int H, int band, int nranks, int rank, rm_shard_layout *out);
rm_status rm_comm_get_id(rm_comm_id *id);
rm_status rm_comm_init_rank(rm_comm **comm, rm_ctx *ctx, int nranks, const rm_comm_id *id, int rank);
rm_status rm_comm_init_all(rm_comm **comms, rm_ctx *const *ctxs, int n);
rm_status rm_comm_destroy(rm_comm *comm);
/* uses_rccl = 1 when the communicator runs RCCL (always for nranks > 1; a
 * one-rank communicator too whenever librccl loads, else a local copy). */
rm_status rm_comm_info(const rm_comm *comm, int *nranks, int *rank, int *uses_rccl);
rm_status rm_render_sharded(rm_comm *comm, int W, int H, int band, uint32_t *frame, rm_stats *stats);
rm_status rm_render_sharded_all(rm_comm *const *comms, int n, int W, int H, int band, uint32_t *frame,
                                rm_stats *stats);
/* The same with weighted parts instead of bands: runs[r] >= 1 rows of every
 * cycle of sum(runs) rows go to rank r, in rank order (rm_cycle_rows); the
 * parts cross the wire unpadded (grouped ncclSend/ncclRecv) and rank 0
 * rebuilds the frame with rm_deinterleave_cycle_rgb8.  Every rank passes the
 * same runs (nranks entries). */
rm_status rm_render_sharded_runs(rm_comm *comm, int W, int H, const int *runs, uint32_t *frame, rm_stats *stats);
rm_status rm_render_sharded_runs_all(rm_comm *const *comms, int n, int W, int H, const int *runs, uint32_t *frame,
                                     rm_stats *stats);

/* Message of the last failing call on ctx ("" if none). */
const char *rm_last_error(rm_ctx *ctx);
const char *rm_status_string(rm_status status);

#ifdef __cplusplus
}
#endif

#endif /* RM_H_ */
