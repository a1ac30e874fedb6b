// host_logic_test.cpp -- the HIP-free host logic of librm.so on the CPU: row
// parts (csrc/rm_rows.h) and scene-file text handling (csrc/rm_scene_file.cpp).
// Stand-alone: tests/test_host_logic.py builds it with the host compiler under
// the address and undefined-behaviour sanitizers and runs it in an empty
// directory (the loader resolves #include names against the working directory).
// Exits non-zero at the first failed check, naming it.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "../../raymarching_amd/csrc/rm_rows.h"
#include "../../raymarching_amd/csrc/rm_scene_file.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAILED %s (line %d): %s\n", __func__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static bool has(const std::string &s, const char *part) { return s.find(part) != std::string::npos; }

static void write(const char *name, const std::string &text) {
    std::ofstream f(name, std::ios::binary);
    f << text;
    CHECK(f.good());
}

static int brute_rows(int H, int cycle, int offset, int run) {
    int n = 0;
    for (int y = 0; y < H; y++) n += y % cycle - offset >= 0 && y % cycle - offset < run;
    return n;
}

static void row_parts_count_their_rows() {
    for (int cycle = 1; cycle <= 12; cycle++)
        for (int offset = -1; offset <= 13; offset++)
            for (int run = -1; run <= 13; run++) {
                rm::RowPart p{-1, -1, -1};
                const bool ok = rm::cycle_part(cycle, offset, run, p);
                CHECK(ok == (offset >= 0 && run > 0 && offset + run <= cycle));
                if (!ok) continue;
                CHECK(p.cycle == cycle && p.offset == offset && p.run == run);
                for (int H = 1; H <= 64; H++) CHECK(rm::rows_of_part(H, p) == brute_rows(H, cycle, offset, run));
            }
}

// every split of [0, cycle) into consecutive runs (bit i of `cuts`: a part ends after row i)
static void row_parts_of_a_cycle_sum_to_the_frame() {
    for (int cycle = 1; cycle <= 12; cycle++)
        for (unsigned cuts = 0; cuts < 1u << (cycle - 1); cuts++)
            for (int H = 1; H <= 64; H++) {
                int sum = 0, offset = 0;
                for (int i = 0; i < cycle; i++)
                    if (i == cycle - 1 || (cuts >> i & 1)) {
                        rm::RowPart p;
                        CHECK(rm::cycle_part(cycle, offset, i + 1 - offset, p));
                        sum += rm::rows_of_part(H, p);
                        offset = i + 1;
                    }
                CHECK(sum == H);
            }
}

static void cycle_part_refuses() {
    rm::RowPart p;
    CHECK(!rm::cycle_part(0, 0, 1, p));
    CHECK(!rm::cycle_part(-4, 0, 1, p));
    CHECK(!rm::cycle_part(4, -1, 1, p));
    CHECK(!rm::cycle_part(4, 0, 0, p));
    CHECK(!rm::cycle_part(4, 0, -1, p));
    CHECK(!rm::cycle_part(4, 3, 2, p));
    CHECK(!rm::cycle_part(4, 4, 1, p));
    CHECK(!rm::cycle_part(INT_MAX, INT_MAX, 1, p));  // offset + run past int
    CHECK(!rm::cycle_part(8, INT_MAX, 1, p));
    CHECK(rm::cycle_part(INT_MAX, INT_MAX - 1, 1, p));
    CHECK(rm::cycle_part(4, 3, 1, p));  // offset + run == cycle
    CHECK(rm::rows_of_part(8, p) == 2 && rm::rows_of_part(7, p) == 1 && rm::rows_of_part(3, p) == 0);
}

static void band_part_checks() {
    rm::RowPart p;
    CHECK(!rm::band_part(0, 2, 0, p));
    CHECK(!rm::band_part(-8, 2, 0, p));
    CHECK(!rm::band_part(8, 0, 0, p));
    CHECK(!rm::band_part(8, -1, 0, p));
    CHECK(!rm::band_part(8, 2, -1, p));
    CHECK(!rm::band_part(8, 2, 2, p));
    CHECK(!rm::band_part(65536, 32768, 0, p));  // band * nshards = 2^31
    CHECK(rm::band_part(65536, 32767, 32766, p));
    CHECK(p.cycle == 0x7fff0000 && p.offset == 65536 * 32766 && p.run == 65536);
    CHECK(rm::rows_of_part(INT_MAX, p) == 65536 && rm::rows_of_part(p.offset + 5, p) == 5);
    CHECK(rm::band_part(8, 3, 1, p));
    CHECK(p.cycle == 24 && p.offset == 8 && p.run == 8);
    for (int H = 1; H <= 64; H++) {
        int sum = 0;
        for (int s = 0; s < 3; s++) {
            CHECK(rm::band_part(8, 3, s, p));
            CHECK(rm::rows_of_part(H, p) == brute_rows(H, 24, 8 * s, 8));
            sum += rm::rows_of_part(H, p);
        }
        CHECK(sum == H);
    }
}

static void fingerprints() {
    using rmscene::fingerprint;
    CHECK(fingerprint("") == 0xcbf29ce484222325ULL);
    CHECK(fingerprint("a") == 0xaf63dc4c8601ec8cULL);  // the published FNV-1a 64 vector
    CHECK(fingerprint("foobar") == 0x85944171f73967e8ULL);
    CHECK(fingerprint(" f\to\ro\nb\va\fr ") == fingerprint("foobar"));
    CHECK(fingerprint("foo bar") != fingerprint("foo_bar"));
    const std::string a = "vec3 light() {\n", b = "  return vec3(1.0);\n}\n";
    CHECK(fingerprint(b, fingerprint(a)) == fingerprint(a + b));
}

static void names() {
    using namespace rmscene;
    CHECK(base_name("a/b\\c.frag") == "c.frag" && base_name("c.frag") == "c.frag" && base_name("dir/") == "");
    CHECK(scene_of("output_shader.frag") == kSceneO && scene_of("O") == kSceneO);
    CHECK(scene_of("template.frag") == kSceneT && scene_of("T") == kSceneT);
    CHECK(scene_of("sphere") == kSceneS0 && scene_of("sphere.frag") == kSceneS0 && scene_of("S0") == kSceneS0);
    CHECK(scene_of("output_shader_glass") == kSceneOG && scene_of("OG") == kSceneOG);
    CHECK(scene_of("scene.hip") == -1 && scene_of("") == -1);
    CHECK(is_plugin_source("scene.hip") && !is_plugin_source(".hip") && !is_plugin_source("scene.frag"));
}

static void preprocess_follows_includes() {
    using rmscene::preprocess;
    write("inc_a.frag", "float a;\n");
    write("inc_b.frag", "float b;\n#include \"inc_a.frag\"\n");
    // (the trailing comment after a <name>: a closing '"' re-opens the name, as in the reference's loader)
    const std::string body = "#version 130\n"
                             "#include <inc_a.frag> // the library\n"
                             "  #include <inc_b.frag>\n"
                             "// #include \"missing.frag\"\n"
                             "int x; // see #include \"missing.frag\"\n"
                             "void main() {}\n";
    const std::string want = "#version 130\n"
                             "float a;\n"
                             "float b;\nfloat a;\n"
                             "// #include \"missing.frag\"\n"
                             "int x; // see #include \"missing.frag\"\n"
                             "void main() {}\n";
    write("main_lf.frag", body);
    std::string crlf;
    for (char c : body) crlf += c == '\n' ? std::string("\r\n") : std::string(1, c);
    write("main_crlf.frag", crlf);
    std::string out, err;
    CHECK(preprocess("main_lf.frag", out, err));
    CHECK(out == want && err.empty());
    std::string out2;
    CHECK(preprocess("main_crlf.frag", out2, err));  // (an include name with '\r' would not open)
    CHECK(out2 == want);
    CHECK(!has(out2, "\r"));
}

static void preprocess_fails() {
    using rmscene::preprocess;
    std::string out, err;
    write("self.frag", "int before;\n#include \"self.frag\"\n");
    CHECK(!preprocess("self.frag", out, err));
    CHECK(err == "ShaderLoader: #include nesting too deep at \"self.frag\"");
    write("wants_nope.frag", "#include \"nope.frag\"\n");
    out.clear(), err.clear();
    CHECK(!preprocess("wants_nope.frag", out, err));
    CHECK(err == "ShaderLoader: can't load file \"nope.frag\"");
    err.clear();
    CHECK(!preprocess("absent.frag", out, err));
    CHECK(err == "ShaderLoader: can't load file \"absent.frag\"");
}

// an output_shader.frag-shaped text that is not the reference's
static const std::string kPrelude = "#version 130\nconst int STEPS = 4;\n#include \"lib.frag\"\n";
static const std::string kScene = "Material floorMat() { return Material(1.0); }\n"
                                  "SdResult sceneSDF(vec3 p)\n{\n"
                                  "  if (p.x > 0.0) { for (int i = 0; i < 2; i++) { p.x -= 1.0; } }\n"
                                  "  return SdResult(p.x);\n}";
static const std::string kPipeline = "\nvec3 light() { return vec3(1.0); }\nvoid main() { light(); }\n";

static void split_scene_parts() {
    using rmscene::split_scene;
    std::string pre, scene, pipe, inc;
    CHECK(split_scene(kPrelude + kScene + kPipeline, pre, scene, pipe, inc));
    CHECK(pre == kPrelude && scene == kScene && pipe == kPipeline);
    CHECK(inc == "lib.frag");
    CHECK(split_scene("#include <lib.frag>\nsceneSDF(){}", pre, scene, pipe, inc));
    CHECK(inc == "lib.frag" && pre == "#include <lib.frag>\n" && scene == "sceneSDF(){}" && pipe.empty());
    CHECK(!split_scene("#version 130\n" + kScene + kPipeline, pre, scene, pipe, inc));          // no #include
    CHECK(!split_scene(kPrelude + "Material floorMat() { }\n" + kPipeline, pre, scene, pipe, inc));  // no sceneSDF(
    CHECK(!split_scene(kPrelude + "SdResult sceneSDF(vec3 p) { if (p.x > 0.0) { return r; }\n", pre, scene, pipe, inc));
    CHECK(!split_scene(kPrelude + "SdResult sceneSDF(vec3 p);\n", pre, scene, pipe, inc));  // no body
    // the closing quote lies beyond the include's line
    CHECK(!split_scene("#include \"lib.frag\nint x; \"\n" + kScene + kPipeline, pre, scene, pipe, inc));
    CHECK(!split_scene("#include lib.frag\n" + kScene + kPipeline, pre, scene, pipe, inc));
}

static void classify() {
    using namespace rmscene;
    std::string src, err;
    int sc = -1;
    CHECK(classify_scene_file("dir/my_scene.frag", sc, src, err) == RM_ERR_SCENE);
    CHECK(err == "no HIP scene plugin for \"dir/my_scene.frag\"" && sc == -1);
    CHECK(classify_scene_file("dir/my_scene.hip", sc, src, err) == RM_OK);  // (by name: the file is not read)
    CHECK(sc == kScenePlugin);

    write("template.frag", "void main() { gl_FragColor = vec4(1.0); }\n");
    sc = scene_of(base_name("./template.frag"));
    err.clear();
    CHECK(classify_scene_file("./template.frag", sc, src, err) == RM_ERR_SCENE);
    CHECK(has(err, "is not the reference's template.frag") && sc == kSceneT);

    write("lib.frag", "float lib;\n");
    write("output_shader.frag", kPrelude + kScene + kPipeline);
    sc = kSceneO, err.clear();
    CHECK(classify_scene_file("output_shader.frag", sc, src, err) == RM_ERR_SCENE);
    CHECK(has(err, "only the scene part of output_shader.frag") && sc == kSceneO && src.empty());
    write("output_shader.frag", "no include, no scene\n");
    err.clear();
    CHECK(classify_scene_file("output_shader.frag", sc, src, err) == RM_ERR_SCENE);
    CHECK(has(err, "only the scene part of output_shader.frag"));

    // the build's own names: any text
    for (const char *name : {"S0", "OG"}) {
        write(name, "anything\n");
        const int want = sc = scene_of(name);
        err.clear();
        CHECK(want == kSceneS0 || want == kSceneOG);
        CHECK(classify_scene_file(name, sc, src, err) == RM_OK);
        CHECK(sc == want && err.empty() && src.empty());
    }
    sc = kSceneOG, err.clear();
    CHECK(classify_scene_file("output_shader_glass.frag", sc, src, err) == RM_ERR_FILE);  // a registered name, no file
    CHECK(err == "ShaderLoader: can't load file \"output_shader_glass.frag\"");
}

// the sequence rm_load_scene and rm_compile_scene share
static void load_scene_file_sequence() {
    using namespace rmscene;
    std::string src, err;
    int sc = 99;
    CHECK(load_scene_file("absent.hip", sc, src, err) == RM_ERR_FILE);
    CHECK(err == "ShaderLoader: can't load file \"absent.hip\"");
    write("plugin.hip", "#include \"inc_a.frag\"\nSdResult sceneSDF(vec3 p) { return r; }\n");
    src.clear(), err.clear();
    CHECK(load_scene_file("plugin.hip", sc, src, err) == RM_OK);
    CHECK(sc == kScenePlugin && src == "float a;\nSdResult sceneSDF(vec3 p) { return r; }\n");
    src.clear();
    CHECK(load_scene_file("S0", sc, src, err) == RM_OK);
    CHECK(sc == kSceneS0 && src == "anything\n");
    CHECK(load_scene_file("main_lf.frag", sc, src, err) == RM_ERR_SCENE);
    CHECK(sc == -1 && has(err, "no HIP scene plugin"));
}

int main() {
    row_parts_count_their_rows();
    row_parts_of_a_cycle_sum_to_the_frame();
    cycle_part_refuses();
    band_part_checks();
    fingerprints();
    names();
    preprocess_follows_includes();
    preprocess_fails();
    split_scene_parts();
    classify();
    load_scene_file_sequence();
    std::puts("host logic: all checks passed");
    return 0;
}
