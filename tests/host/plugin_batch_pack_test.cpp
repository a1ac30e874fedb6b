// plugin_batch_pack_test.cpp -- raymarching_amd/csrc/rm_plugin_batch_pack.h
// with rm_uniform_decl.cpp, on the host: the per-view uniform blocks of
// rm_render_batch_ex from a scene's declarations, a current block and a list of
// per-view uniforms, and every fault of such a list by its message.  Built by
// tests/test_plugin_batch_host.py with the host compiler under
// -fsanitize=address,undefined; nothing of it is loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../raymarching_amd/csrc/rm_plugin_batch_pack.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof(u));
    return u;
}

// slots: u_f 0, u_v 1, u_arr 2..9, u_n 10, u_on 11, u_keep 12
static const char* kScene =
    "uniform float u_f = 1.5;\n"
    "uniform vec4 u_v = vec4(1.0, 2.0, 3.0, 4.0);\n"
    "uniform vec4 u_arr[8];\n"
    "uniform int u_n = 7;\n"
    "uniform bool u_on = true;\n"
    "uniform vec3 u_keep = vec3(0.25, 0.5, 0.75);\n"
    "SdResult sceneSDF(vec3 p) { return x; }\n";

static rm_view_uniform entry(const char* name, int components, int count, const void* values) {
    rm_view_uniform u;
    u.name = name;
    u.components = components;
    u.count = count;
    u.values = values;
    return u;
}

int main() {
    rmuniform::Table t;
    std::string blanked, err;
    CHECK(rmuniform::parse(kScene, "scene.hip", t, blanked, err));
    CHECK(t.slots == 13 && rmpack::block_words(t) == 52);
    // the current block: the defaults, then every word of the array and the unused words of the slots marked
    uint32_t current[rmuniform::kBlockWords];
    t.defaults(current);
    for (int i = 0; i < 8; i++)
        for (int c = 0; c < 4; c++) current[4 * (2 + i) + c] = bits(100.0f + 4 * i + c);
    current[4 * 0 + 1] = 0xAAAA0001u;  // (beyond u_f's one component)
    current[4 * 12 + 3] = 0xAAAA0002u; // (beyond u_keep's three)
    const size_t W = rmpack::block_words(t);
    std::vector<uint32_t> blocks;

    // ---- no list: every view's block is the current block
    CHECK(rmpack::pack_view_uniforms(t, current, nullptr, 0, 3, blocks).empty());
    CHECK(blocks.size() == 3 * W);
    for (int v = 0; v < 3; v++) CHECK(std::memcmp(blocks.data() + v * W, current, W * 4) == 0);
    // n = 0: nothing to pack, the list still checked
    CHECK(rmpack::pack_view_uniforms(t, current, nullptr, 0, 0, blocks).empty() && blocks.empty());

    // ---- a float, a vec4, the leading 2 of the array, an int and a bool, three views
    const int n = 3;
    const float f[n] = {-1.0f, 0.0f, 9.5f};
    float v4[n][4], arr[n][2][4];
    for (int v = 0; v < n; v++)
        for (int c = 0; c < 4; c++) {
            v4[v][c] = 10.0f * v + c;
            arr[v][0][c] = 1000.0f + 10 * v + c;
            arr[v][1][c] = 2000.0f + 10 * v + c;
        }
    const int32_t cnt[n] = {0, -3, 8};
    const int32_t on[n] = {0, 5, -1};
    const rm_view_uniform list[] = {entry("u_f", 1, 1, f), entry("u_v", 4, 1, v4), entry("u_arr", 4, 2, arr),
                                    entry("u_n", 1, 1, cnt), entry("u_on", 1, 1, on)};
    CHECK(rmpack::pack_view_uniforms(t, current, list, 5, n, blocks).empty());
    CHECK(blocks.size() == n * W);
    for (int v = 0; v < n && blocks.size() == n * W; v++) {
        const uint32_t* b = blocks.data() + v * W;
        CHECK(b[0] == bits(f[v]) && b[1] == 0xAAAA0001u && b[2] == current[2] && b[3] == current[3]);
        for (int c = 0; c < 4; c++) {
            CHECK(b[4 + c] == bits(v4[v][c]));
            CHECK(b[8 + c] == bits(arr[v][0][c]) && b[12 + c] == bits(arr[v][1][c]));
        }
        // the array's elements 2..7 keep the current values
        CHECK(std::memcmp(b + 16, current + 16, 6 * 16) == 0);
        CHECK(b[40] == (uint32_t)cnt[v]);
        CHECK(b[44] == (on[v] != 0 ? 1u : 0u));
        // the unlisted u_keep, its unused word included, is the current block's
        CHECK(std::memcmp(b + 48, current + 48, 16) == 0);
    }
    // a listed uniform alone: every other slot is copied
    const rm_view_uniform only[] = {entry("u_n", 1, 1, cnt)};
    CHECK(rmpack::pack_view_uniforms(t, current, only, 1, n, blocks).empty());
    for (int v = 0; v < n; v++) {
        std::vector<uint32_t> want(current, current + W);
        want[40] = (uint32_t)cnt[v];
        CHECK(std::memcmp(blocks.data() + v * W, want.data(), W * 4) == 0);
    }
    // values at an odd address are read byte-wise
    std::vector<char> odd(1 + sizeof(f));
    std::memcpy(odd.data() + 1, f, sizeof(f));
    const rm_view_uniform unaligned[] = {entry("u_f", 1, 1, odd.data() + 1)};
    CHECK(rmpack::pack_view_uniforms(t, current, unaligned, 1, n, blocks).empty());
    CHECK(blocks[2 * W] == bits(f[2]));
    // the whole array
    std::vector<float> whole((size_t)n * 8 * 4, 3.0f);
    const rm_view_uniform all8[] = {entry("u_arr", 4, 8, whole.data())};
    CHECK(rmpack::pack_view_uniforms(t, current, all8, 1, n, blocks).empty());
    CHECK(blocks[W + 8] == bits(3.0f) && blocks[W + 39] == bits(3.0f) && blocks[W + 40] == current[40]);

    // ---- a scene without uniforms: no blocks, an empty list is fine, any name is undeclared
    rmuniform::Table none;
    CHECK(rmuniform::parse("SdResult sceneSDF(vec3 p) { return x; }\n", "plain.hip", none, blanked, err));
    CHECK(rmpack::pack_view_uniforms(none, current, nullptr, 0, n, blocks).empty() && blocks.empty());
    CHECK(rmpack::pack_view_uniforms(none, current, only, 1, n, blocks) == "the loaded scene declares no uniform \"u_n\"");

    // ---- every fault of the list, by message; nothing is packed
    auto fault = [&](const rm_view_uniform* u, int k, int views) {
        blocks.assign(7, 1u);
        const std::string m = rmpack::pack_view_uniforms(t, current, u, k, views, blocks);
        CHECK(blocks.empty());
        return m;
    };
    CHECK(fault(list, -1, n) == "view uniforms: n_uniforms < 0");
    CHECK(fault(nullptr, 2, n) == "view uniforms: a null list with n_uniforms > 0");
    const rm_view_uniform noname[] = {entry("u_f", 1, 1, f), entry(nullptr, 1, 1, f)};
    CHECK(fault(noname, 2, n) == "view uniform 1: null name");
    const rm_view_uniform novalues[] = {entry("u_f", 1, 1, nullptr)};
    CHECK(fault(novalues, 1, n) == "view uniform \"u_f\": null values");
    CHECK(fault(novalues, 1, 0).empty());  // (no view reads them)
    const rm_view_uniform unknown[] = {entry("u_nope", 1, 1, f)};
    CHECK(fault(unknown, 1, n) == "the loaded scene declares no uniform \"u_nope\"");
    for (const char* pass : {"u_time", "u_pos", "u_mouse", "u_resolution", "u_seed1", "u_sample_part"}) {
        const rm_view_uniform p[] = {entry(pass, 1, 1, f)};
        CHECK(fault(p, 1, n) ==
              "uniform \"" + std::string(pass) + "\" is the pass's own: a view sets u_pos, u_mouse and u_time itself");
    }
    const rm_view_uniform twice[] = {entry("u_f", 1, 1, f), entry("u_n", 1, 1, cnt), entry("u_f", 1, 1, f)};
    CHECK(fault(twice, 3, n) == "view uniform \"u_f\" is listed twice");
    // components that are not the declared type's: the message names the declared type
    const rm_view_uniform c3[] = {entry("u_v", 3, 1, v4)};
    CHECK(fault(c3, 1, n) == "uniform \"u_v\" is declared vec4, got 3 components");
    const rm_view_uniform c1[] = {entry("u_keep", 1, 1, f)};
    CHECK(fault(c1, 1, n) == "uniform \"u_keep\" is declared vec3, got 1 component");
    const rm_view_uniform i2[] = {entry("u_n", 2, 1, cnt)};
    CHECK(fault(i2, 1, n) == "uniform \"u_n\" is declared int, got 2 components");
    const rm_view_uniform b4[] = {entry("u_on", 4, 1, on)};
    CHECK(fault(b4, 1, n) == "uniform \"u_on\" is declared bool, got 4 components");
    const rm_view_uniform a2[] = {entry("u_arr", 2, 2, arr)};
    CHECK(fault(a2, 1, n) == "uniform \"u_arr\" is declared vec4[8], got 2 components");
    const rm_view_uniform c0[] = {entry("u_f", 0, 1, f)};
    CHECK(fault(c0, 1, n) == "uniform \"u_f\" is declared float, got 0 components");
    // counts
    const rm_view_uniform k0[] = {entry("u_f", 1, 0, f)};
    CHECK(fault(k0, 1, n) == "view uniform \"u_f\": count 0 < 1");
    const rm_view_uniform kneg[] = {entry("u_arr", 4, -2, arr)};
    CHECK(fault(kneg, 1, n) == "view uniform \"u_arr\": count -2 < 1");
    const rm_view_uniform k2[] = {entry("u_v", 4, 2, arr)};
    CHECK(fault(k2, 1, n) == "uniform \"u_v\" is declared vec4, not an array: count 2");
    const rm_view_uniform k9[] = {entry("u_arr", 4, 9, arr)};
    CHECK(fault(k9, 1, n) == "uniform \"u_arr\" is declared vec4[8]: count 9 is above its length");
    // the first fault in the list's order is the one reported
    const rm_view_uniform two[] = {entry("u_v", 3, 1, v4), entry("u_nope", 1, 1, f)};
    CHECK(fault(two, 2, n) == "uniform \"u_v\" is declared vec4, got 3 components");

    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
