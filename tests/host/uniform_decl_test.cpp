// uniform_decl_test.cpp -- the parser of a scene's `uniform` declarations
// (csrc/rm_uniform_decl.cpp) on the CPU.  Stand-alone:
// tests/test_uniform_decl_host.py builds it with the host compiler under the
// address and undefined-behaviour sanitizers, linked with rm_uniform_decl.cpp
// only.  Exits non-zero at the first failed check, naming it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../raymarching_amd/csrc/rm_uniform_decl.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "FAILED %s (line %d): %s\n", __func__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

using rmuniform::Decl;
using rmuniform::Table;

static bool has(const std::string &s, const std::string &part) { return s.find(part) != std::string::npos; }
static long lines(const std::string &s) { return std::count(s.begin(), s.end(), '\n'); }
static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

struct Parsed {
    bool ok;
    Table t;
    std::string blanked, err;
};
static Parsed parse(const std::string &src) {
    Parsed p;
    p.ok = rmuniform::parse(src, "scene.hip", p.t, p.blanked, p.err);
    // blanking never changes the length or a line break, parsed or refused
    CHECK(p.blanked.size() == src.size());
    CHECK(lines(p.blanked) == lines(src));
    for (size_t i = 0; i < src.size(); i++) CHECK((src[i] == '\n') == (p.blanked[i] == '\n'));
    if (!p.ok) {
        CHECK(p.t.decls.empty() && p.t.slots == 0 && p.blanked == src);
        CHECK(has(p.err, "scene.hip:") && has(p.err, "error"));
    } else {
        CHECK(p.err.empty());
    }
    return p;
}
// refused, at that line
static void refused(const std::string &src, int line, const char *word = nullptr) {
    Parsed p = parse(src);
    CHECK(!p.ok);
    CHECK(has(p.err, "scene.hip:" + std::to_string(line) + ":"));
    if (word) CHECK(has(p.err, word));
}

static void well_formed_tables() {
    const std::string src =
        "// a scene\n"
        "uniform float u_a = 2.5;\n"
        "uniform vec2 u_b = vec2(1.5, -2.0);\n"
        "uniform vec3 u_c = vec3(0.25);\n"
        "uniform vec4 u_d =\n    vec4(3.0, 2.0, 3.0, 1.0);\n"
        "uniform int u_e = -7;\n"
        "uniform bool u_f = true;\n"
        "uniform vec4 u_g[8];\n"
        "uniform float u_h[3];\n"
        "uniform float u_i;\n"
        "uniform int u_j = 0x10;\n"
        "uniform float u_k = 3;\n"
        "uniform float u_l = 1e-3f;\n"
        "SdResult sceneSDF(vec3 p)\n{\n    return SdResult(u_a, Material());\n}\n";
    Parsed p = parse(src);
    CHECK(p.ok);
    const Table &t = p.t;
    CHECK(t.decls.size() == 12);
    const char *names[] = {"u_a", "u_b", "u_c", "u_d", "u_e", "u_f", "u_g", "u_h", "u_i", "u_j", "u_k", "u_l"};
    const int types[] = {0, 0, 0, 0, 1, 2, 0, 0, 0, 1, 0, 0};
    const int comps[] = {1, 2, 3, 4, 1, 1, 4, 1, 1, 1, 1, 1};
    const int counts[] = {0, 0, 0, 0, 0, 0, 8, 3, 0, 0, 0, 0};
    const int slots[] = {0, 1, 2, 3, 4, 5, 6, 14, 17, 18, 19, 20};
    const int at[] = {2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14};
    for (int i = 0; i < 12; i++) {
        const Decl &d = t.decls[i];
        CHECK(d.name == names[i] && d.type == types[i] && d.components == comps[i] && d.count == counts[i]);
        CHECK(d.slot == slots[i] && d.line == at[i]);
        CHECK(t.find(names[i]) == &d);
    }
    CHECK(t.slots == 21);
    CHECK(!t.find("u_z") && !t.find("u_"));
    CHECK(t.decls[0].def[0] == bits(2.5f));
    CHECK(t.decls[1].def[0] == bits(1.5f) && t.decls[1].def[1] == bits(-2.0f));
    CHECK(t.decls[2].def[0] == bits(0.25f) && t.decls[2].def[2] == bits(0.25f) && t.decls[2].def[3] == 0);
    CHECK(t.decls[3].def[0] == bits(3.0f) && t.decls[3].def[3] == bits(1.0f));
    CHECK(t.decls[4].def[0] == (uint32_t)-7 && t.decls[5].def[0] == 1u);
    CHECK(t.decls[9].def[0] == 16u && t.decls[10].def[0] == bits(3.0f) && t.decls[11].def[0] == bits(1e-3f));
    uint32_t block[rmuniform::kBlockWords];
    t.defaults(block);
    CHECK(block[0] == bits(2.5f) && block[4] == bits(1.5f) && block[5] == bits(-2.0f) && block[16] == (uint32_t)-7);
    for (int w = 4 * 6; w < 4 * 18; w++) CHECK(block[w] == 0);  // arrays and u_i start at zero
    for (int w = 4 * 21; w < rmuniform::kBlockWords; w++) CHECK(block[w] == 0);
    // the declarations are gone from the text, the rest is untouched
    CHECK(!has(p.blanked, "uniform") && has(p.blanked, "// a scene\n"));
    CHECK(has(p.blanked, "SdResult sceneSDF(vec3 p)\n{\n    return SdResult(u_a, Material());\n}\n"));
    CHECK(rmuniform::type_name(t.decls[6]) == "vec4[8]" && rmuniform::type_name(t.decls[4]) == "int");
    std::string defs, undefs;
    rmuniform::device_text(t, defs, undefs);
    CHECK(lines(defs) == 12 && has(defs, "#define u_g ") && has(undefs, "#undef u_l\n"));
    CHECK(has(undefs, "RM_UNIFORM_PRELOAD()"));
}

static void not_declarations() {
    const std::string src =
        "// uniform float in_a_comment;\n"
        "/* uniform float in_a_block;\n uniform vec2 still; */\n"
        "const float uniformity = 1.0; float my_uniform = 2.0;\n"
        "#define DECL uniform float in_a_macro; \\\n    uniform float continued;\n"
        "const char* s = \"uniform float in_a_string;\";\n"
        "void f()\n{\n    uniform float in_a_body;\n}\n"
        "void g(uniform float in_parens);\n";
    Parsed p = parse(src);
    CHECK(p.ok && p.t.decls.empty() && p.t.slots == 0 && p.blanked == src);
    // an inactive #if region still declares: matching is textual
    Parsed q = parse("#if 0\nuniform float u_off;\n#endif\n");
    CHECK(q.ok && q.t.decls.size() == 1 && q.t.decls[0].line == 2);
}

static void refusals() {
    refused("\nuniform float u_a = 1.0 + 2.0;\n", 2, "initialiser");
    refused("uniform float u_a = sin(1.0);\n", 1, "initialiser");
    refused("uniform float u_a, u_b;\n", 1, "one name");
    refused("uniform sampler2D u_tex;\n", 1, "sampler2D");
    refused("uniform int u_n[4];\n", 1, "int or bool");
    refused("uniform bool u_n[4];\n", 1, "int or bool");
    refused("uniform float u_a[0];\n", 1, "1..64");
    refused("uniform float u_a[65];\n", 1, "1..64");
    refused("uniform float u_a[N];\n", 1, "decimal");
    refused("uniform float u_a[2] = 1.0;\n", 1, "initialiser");
    refused("uniform vec3 u_a = vec3(1.0, 2.0);\n", 1, "1 or 3");
    refused("uniform vec3 u_a = vec2(1.0, 2.0);\n", 1);
    refused("uniform int u_a = 1.5;\n", 1);
    refused("uniform int u_a = 4294967296;\n", 1);
    refused("uniform bool u_a = 1;\n", 1);
    refused("uniform float;\n", 1);
    refused("uniform float u_a;\n\nuniform vec2 u_a;\n", 3, "twice");
    for (const char *n : {"u_resolution", "u_pos", "u_mouse", "u_time", "u_sample", "u_sample_part", "u_seed1",
                          "u_seed2"})
        refused(std::string("\n\nuniform vec2 ") + n + ";\n", 3, "pass");
    // 64 slots fit, 65 do not (an array takes one per element)
    CHECK(parse("uniform vec4 u_a[64];\n").ok);
    CHECK(parse("uniform vec4 u_a[63];\nuniform float u_b;\n").t.slots == 64);
    refused("uniform vec4 u_a[63];\nuniform float u_b;\nuniform float u_c;\n", 3, "64");
    refused("uniform vec4 u_a[40];\nuniform vec4 u_b[25];\n", 2, "64");
}

static void adversarial() {
    refused("SdResult f();\nuniform float u_a", 2, "`;`");   // no ';' at end of file
    refused("uniform float u_a = ", 1);
    refused("uniform", 1);
    refused("uniform float u_a[;\n", 1);                      // '[' without ']'
    refused("uniform float u_a[3;\n", 1);
    refused("uniform float u_a[\n", 1);
    refused("uniform float u_a[12345678901234567890];\n", 1, "1..64");  // N of 20 digits
    refused("uniform float u_a[99999999999999999999999999999999999999999];\n", 1, "1..64");
    refused("uniform float " + std::string(200, 'n') + ";\n", 1, "200");  // a 200-character name
    CHECK(parse("uniform float " + std::string(63, 'n') + ";\n").ok);
    refused("uniform float " + std::string(64, 'n') + ";\n", 1);
    std::string many;  // 10^4 declarations: refused at the 65th
    for (int i = 0; i < 10000; i++) many += "uniform float u_" + std::to_string(i) + ";\n";
    refused(many, 65, "64");
    Parsed e = parse("");  // an empty file
    CHECK(e.ok && e.t.decls.empty() && e.blanked.empty());
    CHECK(parse("\n").ok && parse("/*").ok && parse("\"").ok && parse("#").ok && parse("//").ok && parse("'").ok);
    CHECK(parse("}}}}))))").ok);
    refused("uniform float u_a = 1e999999999999;\n", 1 + 0) ;
    refused(std::string("uniform float u_a = ") + std::string(5000, '-') + "1.0;\n", 1);
    refused("uniform float u_a = 1.0.0;\n", 1);
}

int main() {
    well_formed_tables();
    not_declarations();
    refusals();
    adversarial();
    std::printf("all checks passed\n");
    return 0;
}
